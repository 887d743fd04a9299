"""BEV label augmentation of one sample at the SemanticKITTI grid [256, 256, 32]: the host form (``pipelines.bev_transform`` as
it has always run: scipy in place on one thread, flips, widening to int64, then the 16 MB upload ``collate`` does from pinned
memory) against the device form (2 MB uint8 upload + csrc/bev_augment.hip), both from the same uint8 host tensor to int64 labels
resident on the card.  Host clock around each call, ending in a device synchronise; the two forms alternate inside one process;
median, min and max of the timed runs after warm-up.  The kernels alone (labels already on the card) are timed with HIP events.

    python tools/bev_augment_bench.py [--out profiles/bev_augment_times.txt] [--runs 20] [--angle 3.75]"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import capi, functional as F, pipelines as P  # noqa: E402

SHAPE = (256, 256, 32)
CENTER = torch.tensor([25.6, 0.0, 1.2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--angle", type=float, default=3.75)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bev_augment_bench.py measures on the GPU: none found")
    dev = "cuda"
    rng = np.random.RandomState(0)
    lab = rng.randint(0, 20, size=SHAPE).astype(np.uint8)
    lab[rng.rand(*SHAPE) < 0.1] = 255
    labels = torch.from_numpy(lab)

    def host(mode="reference"):
        v, _ = P.bev_transform(labels.clone(), a.angle, 1.0, False, True, CENTER, rotate_mode=mode)
        out = v.pin_memory().to(dev, non_blocking=True)              # what pipelines.collate does with a host gt_occ
        torch.cuda.synchronize()
        return out

    def device(mode="reference"):
        out, _ = P.bev_transform(labels.clone(), a.angle, 1.0, False, True, CENTER, device=dev, rotate_mode=mode)
        torch.cuda.synchronize()
        return out

    for mode in ("reference", "exact"):                              # warm-up, and faster must not mean different
        assert torch.equal(host(mode), device(mode)), mode
    th, td = [], []
    for _ in range(a.runs):
        for f, ts in ((host, th), (device, td)):
            t0 = time.perf_counter()
            f()
            ts.append((time.perf_counter() - t0) * 1e3)
    resident = labels.to(dev)
    coeffs = P.bev_rotate_coeffs(SHAPE[0], SHAPE[1], a.angle)
    tk = {}
    for inplace in (True, False):
        for _ in range(3):
            F.bev_label_transform(resident, coeffs, False, True, inplace=inplace)
        ts = []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            F.bev_label_transform(resident, coeffs, False, True, inplace=inplace)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        tk[inplace] = ts

    def fmt(ts):
        return f"{statistics.median(ts):9.3f} ms (min {min(ts):.3f}, max {max(ts):.3f})"
    lines = [f"BEV label augmentation, one sample [256, 256, 32], angle {a.angle}, flip_dy, rotate_mode reference, ssbev_version() "
             f"{capi.load().ssbev_version()}, one MI355X, scipy {__import__('scipy').__version__}, median of {a.runs} alternating runs",
             f"host form    uint8 host labels -> int64 on the card (scipy in place + flips + int64 + 16 MB upload)  {fmt(th)}",
             f"device form  uint8 host labels -> int64 on the card (2 MB upload + kernels)                         {fmt(td)}",
             f"kernels alone, labels on the card, in-place chains (source map + 16 jump rounds + gather)          {fmt(tk[True])}",
             f"kernels alone, labels on the card, out-of-place (source map + gather)                              {fmt(tk[False])}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
