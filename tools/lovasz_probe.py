"""Time the Lovasz-softmax voxel loss, forward + backward, at the workload's size: coarse logits (1,20,128,128,16) -> labels
256 x 256 x 32 (synthetic, ~10 % ignored, classes 2, 3 and 8 absent).  The fused HIP path (``functional.lovasz_softmax``) and
the tensor form (``SSBEV_LOVASZ=0``: upsample_trilinear + softmax + one torch.sort per present class) on the same card: warm-up,
HIP events, median of 20.  Also prints the workspace of the fused path and the bytes its sort moves.

Run:  python tools/lovasz_probe.py [--small] [--out FILE]"""
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
    x = S.hash_normal("lovasz_probe_x", coarse, 2.0).cuda().requires_grad_(True)
    lab = S.lovasz_labels("lovasz_probe", fine).cuda()

    def step(fused):
        F.LOVASZ = fused
        x.grad = None
        loss = L.lovasz_softmax_loss(x, lab)
        loss.backward()
        return loss.detach()

    lf, lt = float(step(True)), float(step(False))
    fused_ms, fused_min = timed(lambda: step(True))
    tensor_ms, tensor_min = timed(lambda: step(False))
    F.LOVASZ = True
    lib = capi.load()
    d = capi.LovaszDims(*coarse[:1], *coarse[2:], 20, 255, 1)
    m = int((lab != 255).sum())
    present = int((torch.bincount(lab.flatten().long(), minlength=256)[:20] > 0).sum())
    n = lab.numel()
    # per 8-bit pass: the histogram reads the keys, the placement reads and writes (key, voxel) pairs; the first pass walks all
    # n slots of a present class (keys only), the other three its m labelled voxels
    sort_bytes = present * (2 * 4 * n + 8 * m + 3 * (4 * m + 16 * m))
    out = dict(coarse=coarse, fine=fine, labelled=m, present_classes=present, loss_fused=lf, loss_tensor=lt,
               fused_ms_median=fused_ms, fused_ms_min=fused_min, tensor_ms_median=tensor_ms, tensor_ms_min=tensor_min,
               workspace_fwd_bytes=int(lib.ssbev_lovasz_workspace(C.byref(d))),
               workspace_bwd_bytes=int(lib.ssbev_lovasz_bwd_workspace(C.byref(d))), kept_for_backward_bytes=4 * 20 * n + 4 * 22,
               sort_bytes=sort_bytes)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
