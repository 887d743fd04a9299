"""Forward + backward time of the head's point-level branch at the workload shape, fused and with the tensor forms
(``SSBEV_POINT_HEAD=0``) in the same run: B = 1, one level [384, 128, 128, 16], image features [1, 640, 48, 160], 40 000 synthetic
points (a stand-in for a labelled LiDAR sweep), soft weights and image sampling on as in the reference config.

Run:  python tools/point_head_bench.py [--iters 20] [--out profiles/point_head_times.txt]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402
from stereoscene_amd.plugin.voxel_encoder import OccHead  # noqa: E402

RANGE = (0.0, -25.6, -2.0, 51.2, 25.6, 4.4)


def step(head, feats, img, pts, uv):
    head.zero_grad(set_to_none=True)
    feats.grad = None
    logits = torch.cat(head.forward_points(pts, [feats], img, uv), 0)
    losses = head.loss_point_single(logits, pts[0])
    (losses["loss_point_ce_"] + losses["loss_point_lovasz_"]).backward()


def measure(fused, head, feats, img, pts, uv, iters):
    F.POINT_HEAD = fused
    for _ in range(3):
        step(head, feats, img, pts, uv)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(head, feats, img, pts, uv)
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], torch.cuda.max_memory_allocated() / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--points", type=int, default=40000)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = "cuda"
    head = OccHead(in_channels=[384], out_channel=20, semantic_kitti=True, num_level=1, supervise_points=True, soft_weights=True,
                   sampling_img_feats=True, in_img_channels=640, point_cloud_range=list(RANGE))
    S.fill_state_dict_(head, prefix="point_head_bench/")
    head = head.to(dev).train()
    n = args.points
    lo = torch.tensor(RANGE[:3])
    rng = torch.tensor(RANGE[3:]) - lo
    xyz = lo + S.hash_uniform("point_head_bench/xyz", (n, 3), 0.0, 1.0) * rng
    lab = (S.hash_uniform("point_head_bench/lab", (n, 1), 0.0, 1.0) * 20).floor().clamp_(0, 19)
    pts = [torch.cat((xyz, lab), 1).to(dev)]
    uv = [torch.cat((S.hash_uniform("point_head_bench/uv", (n, 1, 2), -1.05, 1.05),
                     S.hash_uniform("point_head_bench/d", (n, 1, 1), 0.5, 50.0)), -1).to(dev)]
    feats = S.hash_normal("point_head_bench/feat", (1, 384, 128, 128, 16)).to(dev).requires_grad_(True)
    img = S.hash_normal("point_head_bench/img", (1, 1, 640, 48, 160)).to(dev)          # the image branch is absent: no gradient
    lines = [f"point-level branch, forward + backward, B = 1, level [384, 128, 128, 16], image features [1, 640, 48, 160], "
             f"{n} points, {args.iters} iterations after 3 warm-up ({torch.cuda.get_device_name(0)})"]
    for fused in (True, False):
        med, best, mem = measure(fused, head, feats, img, pts, uv, args.iters)
        lines.append(f"{'fused (SSBEV_POINT_HEAD=1)' if fused else 'tensor forms (SSBEV_POINT_HEAD=0)':34s} median {med:8.3f} ms   best "
                     f"{best:8.3f} ms   peak memory {mem:8.1f} MiB")
    F.POINT_HEAD = True
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
