"""CreateDepthFromOccupancy of one view at the SemanticKITTI grid [256, 256, 32] into a 384 x 1280 image: the device form
(csrc/occ_depth.hip through ``functional.occupancy_depth_map``, labels resident on the card as
``LoadSemKittiAnnotation(device="cuda")`` leaves them) against the host form (``SSBEV_OCC_DEPTH=0``: the tensor form on the
host from the same device labels -- one download, elementwise fp32 ops, two scatter-min, one upload of the two maps).  Both forms
run from the same commit inside one process and are timed with HIP events after warm-up; median, min and max.

    python tools/occ_depth_bench.py [--out profiles/occ_depth_times.txt] [--runs 10]"""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import capi, functional as F, synthetic as S  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("occ_depth_bench.py measures on the GPU: none found")
    cfg = S.CFG_K112
    shape = tuple(cfg["occ_size"])                                   # the labels of synthetic.synthetic_sample: hashed classes, 10 % ignored
    c = S.hash_uniform("occ_depth_bench/gt_occ", shape, 0.0, 20.0).long().clamp_(0, 19)
    ig = S.hash_uniform("occ_depth_bench/gt_occ_ignore", shape, 0.0, 1.0) < 0.10
    labels = torch.where(ig, torch.full_like(c, 255), c).cuda()      # int64 [256,256,32] on the card
    view = [t[0] for t in S.frustum_view(cfg)]
    rng = cfg["pc_range"]
    rows = []
    for mode, down in (("reference", False), ("occupied", False), ("reference", True)):
        times = {}
        for device_form in (True, False):
            F.SSBEV_OCC_DEPTH = device_form
            for _ in range(2):
                out = F.occupancy_depth_map(labels, view, rng, mode, down)
            ts = []
            for _ in range(a.runs if device_form else max(3, a.runs // 3)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                out = F.occupancy_depth_map(labels, view, rng, mode, down)
                e1.record()
                torch.cuda.synchronize()
                ts.append(e0.elapsed_time(e1))
            times[device_form] = (ts, out)
        F.SSBEV_OCC_DEPTH = True
        assert all(torch.equal(x, y) for x, y in zip(times[True][1], times[False][1])), (mode, down)   # faster must not mean different
        rows.append((mode, down, times[True][0], times[False][0], int((times[True][1][0] != 0).sum())))

    def fmt(ts):
        return f"{statistics.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"
    lines = [f"CreateDepthFromOccupancy, one view, grid [256, 256, 32] (int64 labels on the card) -> depth and label maps 384 x 1280, "
             f"ssbev_version() {capi.load().ssbev_version()}, one MI355X, torch {torch.__version__}, HIP events after warm-up"]
    for mode, down, td, th, npix in rows:
        tag = f"seg_occluders={mode}{', downsample' if down else ''} ({npix} depth pixels)"
        lines.append(f"device form  {tag:58s} {fmt(td)}")
        lines.append(f"host form    {tag:58s} {fmt(th)}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
