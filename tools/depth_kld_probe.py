"""Time the Gaussian KL depth loss (``loss_depth_type="kld"``), forward + backward, at the workload's size: gt_depths
[B, 1, 384, 1280], depth_pred [B, D, 48, 160] for the kitti_d112 and kitti_d192 depth ranges (synthetic, ~5 % of the pixels
carry a LiDAR return).  The fused HIP path (``functional.depth_kld_loss``) and the tensor form (``SSBEV_DEPTH_KLD=0``) on the same
card in the same process: warm-up, then 5 alternating rounds of 100 steps each, one pair of HIP events around every round;
reported: the median over the rounds of the time per step.

Run:  python tools/depth_kld_probe.py [--small] [--out FILE]"""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402


def round_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / steps


def main():
    small = "--small" in sys.argv
    steps, rounds = (5, 2) if small else (100, 5)
    lines = []
    for cfg, B in ((S.CFG_K112, 1), (S.CFG_K192, 2)):
        ds, db = cfg["downsample"], cfg["dbound"]
        H, W = (32, 64) if small else cfg["input_size"]
        D = int(round((db[1] - db[0]) / db[2]))
        u = S.hash_uniform("depth_kld_probe/mask", (B, 1, H, W), 0.0, 1.0)
        d = S.hash_uniform("depth_kld_probe/val", (B, 1, H, W), db[0], db[1] - 6.0)
        gt = torch.where(u < 0.05, d, torch.zeros_like(d)).cuda()
        pred = torch.softmax(S.hash_normal("depth_kld_probe/pred", (B, D, H // ds, W // ds), 2.0), 1).cuda().requires_grad_(True)

        def step(fused):
            F.DEPTH_KLD = fused
            pred.grad = None
            loss = F.depth_kld_loss(gt, pred, ds, db, 1.0)
            loss.backward()
            return loss.detach()

        lf, lt = float(step(True)), float(step(False))
        for fused in (True, False):
            round_ms(lambda: step(fused), steps)                       # warm-up
        torch.cuda.synchronize()
        ms = {True: [], False: []}
        for _ in range(rounds):
            for fused in (True, False):
                ms[fused].append(round_ms(lambda: step(fused), steps))
        F.DEPTH_KLD = True
        lines.append(json.dumps(dict(grid=cfg["name"], B=B, D=D, pixels=B * (H // ds) * (W // ds), steps_per_round=steps,
                                     rounds=rounds, loss_fused=lf, loss_tensor=lt,
                                     fused_ms_median=statistics.median(ms[True]), fused_ms_rounds=ms[True],
                                     tensor_ms_median=statistics.median(ms[False]), tensor_ms_rounds=ms[False])))
        print(lines[-1])
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
