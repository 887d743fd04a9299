"""Time the soft-Dice and the LGA-weighted voxel losses, forward + backward, at the workload's size: coarse logits
(1,20,128,128,16) -> labels 256 x 256 x 32 (synthetic, ~10 % ignored).  The fused HIP paths and the tensor forms
(upsample_trilinear + ``dice_tensor`` / ``SSBEV_LGA=0``: upsample_trilinear + ``pal_tensor``) on the same card: warm-up, then HIP
events around windows of back-to-back steps, the two forms' windows in alternation, median of 7 windows.

What the figures are.  ``lga_fused``: ssbev_lga_weights + ssbev_occ_lga_fwd + _bwd, host-driven.  ``dice_fused``: the Dice term on
its own, i.e. the fused epilogue's sums (a pass the default step runs anyway) + ssbev_occ_dice_tail + ssbev_occ_loss_bwd;
``head3`` / ``head3_dice``: the three default terms of ``occ_losses_fused`` without and with the Dice term, whose difference is
what Dice adds to a step.  The tensor forms are ONE formulation in ATen ops, not a bound on what ATen could do.

Also prints, per fixture case of tests/golden/dice_lga.npz, the largest fused-vs-float64 loss and gradient errors.

Run:  python tools/dice_lga_probe.py [--small] [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402
from stereoscene_amd.plugin import losses as L  # noqa: E402


def window(fn, steps):
    """ms per step of one timed window of ``steps`` back-to-back steps (HIP events around the whole window)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def alternated(fns, steps, windows=7, warmup=5):
    """Median and minimum ms per step of each function, their windows taken in ALTERNATION (a, b, a, b, ...)."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(windows):
        for i, (fn, n) in enumerate(zip(fns, steps)):
            ms[i].append(window(fn, n))
    return [(statistics.median(m), min(m)) for m in ms]


def fixture_errors():
    """{case: {kind: (loss error, largest gradient error / max|float64 gradient|)}} of the fused paths against float64."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "dice_lga.npz")))
    cw = L.semkitti_class_weights().cuda()
    out = {}
    for name in ("A", "B", "G", "K", "L", "N", "Z"):
        x, lab = S.dice_lga_case(name)
        out[name] = {}
        for kind in ("dice", "lga"):
            xg = x.cuda().requires_grad_(True)
            if kind == "dice":
                loss = L.occ_losses_fused(xg, lab.cuda(), cw, w_ce=0.0, w_sem=0.0, w_geo=0.0, w_dice=1.0)["loss_voxel_dice_0"]
            else:
                loss = F.occ_lga_loss(xg, lab.cuda(), cw)
            loss.backward()
            g64 = g[f"{name}_{kind}_f64_grad"]
            out[name][kind] = (abs(float(loss.detach()) - float(g[f"{name}_{kind}_f64_loss"])),
                               float(np.abs(xg.grad.cpu().numpy() - g64).max() / np.abs(g64).max()))
    return out


def main():
    coarse = (1, 20, 16, 16, 8) if "--small" in sys.argv else (1, 20, 128, 128, 16)
    fine = (coarse[0],) + tuple(2 * v for v in coarse[2:])
    x = S.hash_normal("dice_lga_probe_x", coarse, 2.0).cuda().requires_grad_(True)
    lab = S.lovasz_labels("dice_lga_probe", fine).cuda()
    cw = L.semkitti_class_weights().cuda()

    def lga(fused):
        F.LGA = fused
        x.grad = None
        loss = L.occ_lga_loss(x, lab, cw)
        loss.backward()
        return loss.detach()

    def dice(fused):
        x.grad = None
        if fused:
            loss = F.occ_dice_tail(*F.occ_loss_sums(x, lab, cw))
        else:
            loss = L.dice_tensor(F.upsample_trilinear(x, fine[1:]), lab)
        loss.backward()
        return loss.detach()

    def head3(w_dice):
        x.grad = None
        out = L.occ_losses_fused(x, lab, cw, w_dice=w_dice)
        sum(out.values()).backward()

    res = dict(coarse=coarse, fine=fine, labelled=int((lab != 255).sum()),
               loss_lga_fused=float(lga(True)), loss_lga_tensor=float(lga(False)),
               loss_dice_fused=float(dice(True)), loss_dice_tensor=float(dice(False)))
    up64 = torch.nn.functional.interpolate(x.detach().double(), size=fine[1:], mode="trilinear", align_corners=False)
    res["loss_lga_float64"] = float(L.pal_tensor(up64, lab, cw.double()))
    res["loss_dice_float64"] = float(L.dice_tensor(up64, lab))
    del up64
    names = ("lga_fused", "lga_tensor", "dice_fused", "dice_tensor", "head3", "head3_dice")
    fns = [lambda: lga(True), lambda: lga(False), lambda: dice(True), lambda: dice(False), lambda: head3(0.0), lambda: head3(1.0)]
    # windows of 0.03 s and more
    for n, (med, mn) in zip(names, alternated(fns, [100, 20, 100, 20, 100, 100])):
        res[n + "_ms_median"], res[n + "_ms_min"] = med, mn
    F.LGA = True
    (med, mn), = alternated([lambda: F.lga_weights(lab)], [200])
    res["lga_weights_ms_median"], res["lga_weights_ms_min"] = med, mn
    res["fixture_errors_loss_abs_grad_rel"] = fixture_errors()
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
