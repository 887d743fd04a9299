"""Time the frustum-proportion voxel loss, forward + backward, at the workload's size: coarse logits (1,20,128,128,16) -> frustum ids
256 x 256 x 32 (the loader kernel's own ids for the KITTI calibration, synthetic labels with ~10 % ignored).  The fused HIP path
(``functional.frustum_dist_loss``) and the tensor form (``SSBEV_FRUSTUM_DIST=0``: upsample_trilinear + softmax + one scatter-add) on
the same card, and the label kernel against its CPU form.  Warm-up, then HIP events around windows of 200 fused steps / 20
tensor-form steps (0.1 s and more per window), the two forms' windows in alternation, median of 7 windows; wall clock for the CPU
form.  What the fused figure is: a host-driven step of five launches plus autograd, so at this size it is mostly launch and Python
overhead, not kernel time.  What the tensor-form figure is: ONE formulation in ATen ops (a scatter-add of the softmax volume into
65 rows, which contends on atomics), not a bound on what ATen could do.

Run:  python tools/frustum_probe.py [--small] [--out FILE]"""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import capi, functional as F, synthetic as S  # noqa: E402
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
    """Median and minimum ms per step of each function, their windows taken in ALTERNATION (a, b, a, b, ...) so that clock and
    allocator drift hits both sides alike."""
    for fn in fns:
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    ms = [[] for _ in fns]
    for _ in range(windows):
        for i, fn in enumerate(fns):
            ms[i].append(window(fn, steps))
    return [(statistics.median(m), min(m)) for m in ms]


def main():
    cfg = S.CFG_T if "--small" in sys.argv else S.CFG_K112
    fine = tuple(cfg["occ_size"])
    coarse = (1, 20) + tuple(v // 2 for v in fine)
    x = S.hash_normal("frustum_probe_x", coarse, 2.0).cuda().requires_grad_(True)
    lab = S.lovasz_labels("frustum_probe", fine)
    view = S.frustum_view(cfg)
    labg = lab.cuda()
    ids, dists = F.frustum_labels(labg, view, cfg["pc_range"])
    ids, dists = ids[None], dists[None]

    def step(fused):
        F.FRUSTUM_DIST = fused
        x.grad = None
        loss = L.frustum_dist_loss(x, ids, dists)
        loss.backward()
        return loss.detach()

    lf, lt = float(step(True)), float(step(False))
    # windows of 200 fused / 20 tensor-form steps: 0.1 s and more each
    (fused_ms, fused_min), (tensor_ms, tensor_min) = alternated([lambda: [step(True) for _ in range(10)], lambda: step(False)], 20)
    fused_ms, fused_min = fused_ms / 10, fused_min / 10
    F.FRUSTUM_DIST = True
    up64 = torch.nn.functional.interpolate(x.detach().double(), size=fine, mode="trilinear", align_corners=False)
    l64 = float(L.frustum_dist_tensor(up64, ids, dists.double()))
    (label_ms, label_min), = alternated([lambda: F.frustum_labels(labg, view, cfg["pc_range"])], 200)
    cpu = []
    for _ in range(3):
        t0 = time.perf_counter()
        cpu_ids, cpu_counts = F.frustum_labels(lab, view, cfg["pc_range"])
        cpu.append(1e3 * (time.perf_counter() - t0))
    lib = capi.load()
    d = capi.FrustumDims(1, *coarse[2:], 20, 64, 1)
    out = dict(coarse=coarse, fine=fine, in_a_frustum=int((ids != 255).sum()), loss_fused=lf, loss_tensor=lt, loss_float64=l64,
               fused_ms_median=fused_ms, fused_ms_min=fused_min, tensor_ms_median=tensor_ms, tensor_ms_min=tensor_min,
               label_kernel_ms_median=label_ms, label_kernel_ms_min=label_min, label_cpu_ms_median=statistics.median(cpu),
               label_ids_differ=int((cpu_ids != ids[0].cpu()).sum()),
               workspace_fwd_bytes=int(lib.ssbev_frustum_dist_workspace(C.byref(d))),
               workspace_bwd_bytes=int(lib.ssbev_frustum_dist_bwd_workspace(C.byref(d))), kept_for_backward_bytes=64 * 20 * 4)
    line = json.dumps(out)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
