"""Time the OHEM cross-entropy voxel loss, forward + backward, at the workload's size: coarse logits (1,20,128,128,16) -> labels
256 x 256 x 32 (synthetic, ~10 % ignored), top_k = 0.25.  The fused HIP path (``functional.ohem_ce_loss``) and the tensor form
(``SSBEV_OHEM=0``: upsample_trilinear + cross_entropy volume + one stable sort per sample) on the same card: warm-up, HIP events,
median of 20.  Also prints the workspace of the fused path and its largest per-voxel loss error against float64 (the selection
depends on it: tests/test_gpu_ohem.py holds it below 1/8 of the fixtures' gap at the threshold).

Run:  python tools/ohem_probe.py [--small] [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import capi, functional as F, synthetic as S  # noqa: E402
from stereoscene_amd.plugin import losses as L  # noqa: E402

TOP_K = 0.25


def timed(fn, warmup=3, reps=20):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms)


def main():
    coarse = (1, 20, 16, 16, 8) if "--small" in sys.argv else (1, 20, 128, 128, 16)
    fine = (coarse[0],) + tuple(2 * v for v in coarse[2:])
    x = S.hash_normal("ohem_probe_x", coarse, 2.0).cuda().requires_grad_(True)
    lab = S.lovasz_labels("ohem_probe", fine).cuda()
    cw = L.semkitti_class_weights().cuda()

    def step(fused):
        F.OHEM = fused
        x.grad = None
        loss = L.ohem_ce_loss(x, lab, cw, TOP_K)
        loss.backward()
        return loss.detach()

    lf, lt = float(step(True)), float(step(False))
    fused_ms, fused_min = timed(lambda: step(True))
    tensor_ms, tensor_min = timed(lambda: step(False))
    F.OHEM = True
    # per-voxel loss error of the fused path against float64 (up-sampled and evaluated in float64 on the card)
    l, mask = F.ohem_voxel_losses(x.detach(), lab, cw, TOP_K)
    up64 = torch.nn.functional.interpolate(x.detach().double(), size=fine[1:], mode="trilinear", align_corners=False)
    l64 = torch.nn.functional.cross_entropy(up64, lab.long(), weight=cw.double(), ignore_index=255, reduction="none")
    valid = lab != 255
    err = float((l.double() - l64)[valid].abs().max())
    srt = torch.sort(l64[valid], descending=True).values
    k = int(int(valid.sum()) * TOP_K)
    lib = capi.load()
    d = capi.OhemDims(*coarse[:1], *coarse[2:], 20, 255, 1, TOP_K)
    out = dict(coarse=coarse, fine=fine, labelled=int(valid.sum()), kept=int(mask.sum()), kept_expected=k, top_k=TOP_K,
               loss_fused=lf, loss_tensor=lt, fused_ms_median=fused_ms, fused_ms_min=fused_min, tensor_ms_median=tensor_ms,
               tensor_ms_min=tensor_min, voxel_loss_max_err_vs_f64=err, f64_gap_at_threshold=float(srt[k - 1] - srt[k]),
               workspace_fwd_bytes=int(lib.ssbev_ohem_ce_workspace(C.byref(d))),
               workspace_bwd_bytes=int(lib.ssbev_ohem_ce_bwd_workspace(C.byref(d))), kept_for_backward_bytes=lab.numel() + 4)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
