"""Time the image-view segmentation loss, forward + backward, at the model's size: logits (BN, 20, 24, 80) against labels
(BN, 384, 1280), ~5 % of the pixels labelled, for BN = 1 (case E of tests/golden/imgseg.npz) and BN = 2.  The fused HIP path
(ssbev_imgseg_ce_fwd + _bwd) and the tensor form (``SSBEV_IMGSEG=0``: F.interpolate + cross_entropy, the reference's lines) on the
same card: warm-up, then HIP events around windows of back-to-back steps, the two forms' windows in alternation, median and
minimum of 7 windows.  The tensor form is ONE formulation in ATen ops, not a bound on what ATen could do.

Also prints the bytes each form moves at least (counted, not measured) and, per fixture case, the fused-vs-float64 errors.

  fused        labels once (4 BN H W) + logits in forward and backward + the gradient (3 x 4 BN K h w) + the workspace written
               and read (per cell 16 B of partials and 4 K B of counts, each twice)
  tensor form  labels to int64 (4 + 8 + 8 BN H W), and the [BN, K, H, W] fp32 tensor at least five times: written by interpolate,
               read and log-softmax written forward, gradient written and read back by the interpolate backward

Run:  python tools/imgseg_probe.py [--small] [--out FILE]"""
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402
from stereoscene_amd.plugin.losses import semkitti_class_weights  # noqa: E402


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


def fixture_errors(cw):
    """{case: (|fused loss - float64 loss|, largest |fused gradient - float64 gradient| / max|float64 gradient|)}."""
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "imgseg.npz")))
    out = {}
    for name in ("A", "B", "D", "E"):
        logits, lab = S.imgseg_case(name)
        x = logits.cuda().requires_grad_(True)
        loss = F.imgseg_loss(x, lab.cuda(), cw)
        loss.backward()
        g64 = g[f"{name}_f64_grad"]
        out[name] = (abs(float(loss.detach()) - float(g[f"{name}_f64_loss"])),
                     float(np.abs(x.grad.cpu().numpy() - g64).max() / np.abs(g64).max()))
    return out


def bytes_moved(BN, K, h, w, H, W):
    cells, pixels = BN * h * w, BN * H * W
    fused = 4 * pixels + 3 * 4 * K * cells + 2 * cells * (16 + 4 * K)
    tensor = (4 + 8 + 8) * pixels + 5 * 4 * K * pixels
    return fused, tensor


def main():
    (h, w), (H, W) = ((6, 20), (96, 320)) if "--small" in sys.argv else ((24, 80), (384, 1280))
    K = S.IMGSEG_CLASSES
    cw = semkitti_class_weights().cuda()
    res = dict(K=K, logits_hw=(h, w), labels_hw=(H, W))
    for BN in (1, 2):
        x = S.hash_normal(f"imgseg_probe_x{BN}", (BN, K, h, w), 2.0).cuda().requires_grad_(True)
        cls = S.hash_uniform(f"imgseg_probe_cls{BN}", (BN, H, W), 1.0, float(K)).floor().clamp_(1, K - 1)
        lab = torch.where(S.hash_uniform(f"imgseg_probe_mask{BN}", (BN, H, W), 0.0, 1.0) < 0.05, cls, torch.zeros_like(cls)).cuda()

        def step(fused):
            F.IMGSEG = fused
            x.grad = None
            loss = F.imgseg_loss(x, lab, cw)
            loss.backward()
            return loss.detach()

        r = dict(valid=int((lab > 0).sum()), loss_fused=float(step(True)), loss_tensor=float(step(False)),
                 loss_float64=float(F.imgseg_loss_tensor(x.detach().double(), lab, cw)))
        (fm, fn), (tm, tn) = alternated([lambda: step(True), lambda: step(False)], [200, 50])
        r.update(fused_ms_median=fm, fused_ms_min=fn, tensor_ms_median=tm, tensor_ms_min=tn)
        r["fused_bytes"], r["tensor_bytes"] = bytes_moved(BN, K, h, w, H, W)
        res[f"BN{BN}"] = r
    F.IMGSEG = True
    res["fixture_errors_loss_abs_grad_rel"] = fixture_errors(cw)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
