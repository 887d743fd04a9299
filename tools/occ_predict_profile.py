"""Kernel time of the inference epilogue at full size (B = 1, logits [1,20,128,128,16] -> labels [1,256,256,32]), both ways:
  --route fused    functional.occ_predict (ssbev_occ_predict + its reduce) + ssc_counts_from_confusion
  --route unfused  upsample_trilinear -> argmax(1) -> ssc_counts(recompute_mask=True)   (the fused=False route of evaluate)
Run each route under `rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o k -- python tools/occ_predict_profile.py
--route <r>`, then `python tools/occ_predict_profile.py --summarise <fused dir> <unfused dir>` prints, per route, the launches per
call, the median duration of every kernel and their sum (every call launches the same kernels, so the trace splits evenly)."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ITERS = 30


def run(route):
    import torch
    from stereoscene_amd import functional as F, synthetic as S
    from stereoscene_amd.plugin import losses as L
    x = S.hash_uniform("occ_predict_profile/logits", (1, 20, 128, 128, 16), -8.0, 8.0).cuda()
    c = S.hash_uniform("occ_predict_profile/gt", (1, 256, 256, 32), 0.0, 20.0).long().clamp_(0, 19)
    gt = torch.where(S.hash_uniform("occ_predict_profile/ignore", (1, 256, 256, 32), 0.0, 1.0) < 0.1, torch.full_like(c, 255), c).cuda()
    torch.cuda.synchronize()
    with torch.no_grad():
        for _ in range(ITERS):
            if route == "fused":
                pred, _raw, conf, nign = F.occ_predict(x, gt)
                counts = L.ssc_counts_from_confusion(conf, nign)
            else:
                pred = F.upsample_trilinear(x, (256, 256, 32)).argmax(dim=1)
                counts = L.ssc_counts(pred, gt, 20, recompute_mask=True)
            torch.cuda.synchronize()
    print(route, [int(v) if v.dim() == 0 else int(v.sum()) for v in counts])


def summarise(label, folder):
    path = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    per = len(rows) // ITERS
    # a few one-off kernels (set-up copies in front, the final print behind) surround the ITERS identical calls: take the
    # offset at which every slot of the period holds one kernel name
    for off in range(len(rows) - per * ITERS + 1):
        slots = [[] for _ in range(per)]
        for i, r in enumerate(rows[off:off + per * ITERS]):
            slots[i % per].append((r["Kernel_Name"], (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
        if all(len({n for n, _ in s}) == 1 for s in slots):
            break
    total = 0.0
    print(f"{label}: {per} kernel launches per call, median over {ITERS} calls")
    for s in slots:
        names = {n for n, _ in s}
        assert len(names) == 1, names
        med = statistics.median(d for _, d in s)
        total += med
        print(f"  {med:9.1f} us  {s[0][0][:120]}")
    print(f"  {total:9.1f} us  sum of the medians ({label})")
    return total, per


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=["fused", "unfused"])
    ap.add_argument("--summarise", nargs=2, metavar=("FUSED_DIR", "UNFUSED_DIR"))
    a = ap.parse_args()
    if a.summarise:
        f, nf = summarise("fused", a.summarise[0])
        u, nu = summarise("unfused", a.summarise[1])
        print(f"fused {f:.1f} us in {nf} launches  vs  unfused {u:.1f} us in {nu} launches  ({u / f:.1f}x)")
    else:
        run(a.route)
