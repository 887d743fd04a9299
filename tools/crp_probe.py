"""Per-step time of the relation gather and the relation loss, fused against tensor form, at the model's shape (B = 1, 512
features: N = 32 x 32 x 4 = 4096 row voxels, Mc = 512 mega voxels, C2 = 1024 context channels, 4 relations).  Forward + backward
of each operator, HIP events around ``--iters`` repetitions after ``--warmup``, the median of ``--rounds`` rounds.

Run:  python tools/crp_probe.py [--iters 20] [--warmup 5] [--rounds 5]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from stereoscene_amd import functional as F  # noqa: E402
from stereoscene_amd import synthetic as S  # noqa: E402


def timed(fn, iters, warmup, rounds):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters)
    return statistics.median(out), min(out), max(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    dev = "cuda"
    B, R, X, Y, Z, feat = 1, 4, 32, 32, 4, 512
    N, Mc, C2 = X * Y * Z, X * Y * Z // 8, 2 * feat
    # the layout the model hands over: P_logits is a view of the channels-last convolution result [B, N, R, Mc]
    pcl = S.hash_normal("crp_probe_p", (B, N, R, Mc), 2.0).to(dev)
    ctx = S.hash_normal("crp_probe_c", (B, Mc, C2)).to(dev).requires_grad_(True)
    x = S.hash_normal("crp_probe_x", (B, N, feat)).to(dev).permute(0, 2, 1).requires_grad_(True)
    g = S.hash_normal("crp_probe_g", (B, N, feat + R * C2)).to(dev).permute(0, 2, 1)
    lab = torch.tensor([0, 0, 0, 5, 9, 13], dtype=torch.uint8)[(S.hash_uniform("crp_probe_l", (B, X, Y, Z), 0.0, 6.0)).long().clamp_(0, 5)].to(dev)
    dense = F.relation_matrix(lab)

    def gather():
        p = pcl.permute(0, 2, 3, 1).detach().requires_grad_(True)
        F.relation_gather(p, ctx, x).backward(g)

    def loss():
        p = pcl.permute(0, 2, 3, 1).detach().requires_grad_(True)
        F.relation_loss(p, lab).backward()

    def loss_dense():
        p = pcl.permute(0, 2, 3, 1).detach().requires_grad_(True)
        F.relation_loss(p, matrices=dense).backward()

    print(f"shape: B {B} N {N} Mc {Mc} C2 {C2} R {R} Cin {feat}; {a.rounds} rounds of {a.iters} iterations, median (min .. max) ms")
    for crp in (True, False):
        F.CRP = crp
        name = "fused      " if crp else "tensor form"
        for what, fn in (("gather fwd+bwd", gather), ("loss   fwd+bwd", loss)):
            med, lo, hi = timed(fn, a.iters, a.warmup, a.rounds)
            print(f"{name} {what}: {med:8.3f} ({lo:.3f} .. {hi:.3f})")
    med, lo, hi = timed(loss_dense, a.iters, a.warmup, a.rounds)
    print(f"tensor form loss   fwd+bwd, dense matrix given (no expansion from the labels): {med:8.3f} ({lo:.3f} .. {hi:.3f})")


if __name__ == "__main__":
    main()
