"""Position encoder (``point_xyz_channel``) at the benchmark geometry: B = 1, 112 x 48 x 160 = 860 160 lifted points, 128 x 128 x 16
grid, Cxyz = 128, modes "cat" and "add" -- the xyz part (encoder + pooling + the join with a given lifted volume), fused HIP path
against the tensor form on the same card: forward and forward+backward time (median of timed runs after warm-up, HIP events) and
peak memory above the resident inputs.

    python tools/point_xyz_bench.py [--out profiles/point_xyz_times.txt] [--runs 20]

Every (form, mode) measurement is a fresh child process under its own time limit; the driver stops at the first child that fails."""
import argparse
import os
import statistics
import subprocess
import sys
from types import SimpleNamespace

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import functional as F, synthetic as S  # noqa: E402

CHILD_LIMIT = 240          # seconds


def one(form, mode, runs):
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT, gen_dx_bx
    cfg, Cx, dev = S.CFG_K112, 128, "cuda"
    grid = S.grid_config(cfg)
    ns = SimpleNamespace(data_config=dict(input_size=tuple(cfg["input_size"])), grid_config=grid, downsample=cfg["downsample"],
                         _apply3x3=VT._apply3x3)
    ns.frustum = VT.create_frustum(ns)
    geom = VT.get_geometry(ns, *S.frustum_view(cfg)[1:]).to(dev)
    dx, bx, nx = gen_dx_bx(grid["xbound"], grid["ybound"], grid["zbound"])
    gh = ((bx - dx / 2.0).tolist(), dx.tolist(), [int(v) for v in nx.tolist()])
    n = gh[2]
    tables = F.lift_splat_tables(geom, None, None, None, grid_host=gh)
    M = Cx // 2
    p = [S.hash_uniform(f"xyz_bench/{k}", s, lo, hi).to(dev).requires_grad_(True) for k, s, lo, hi in
         (("w1", (M, 3), -1, 1), ("b1", (M,), -.5, .5), ("gamma", (M,), .5, 1.5), ("beta", (M,), -.5, .5), ("w2", (Cx, M), -.3, .3),
          ("b2", (Cx,), -.1, .1))]
    rm, rv, nbt = torch.zeros(M, device=dev), torch.ones(M, device=dev), torch.zeros((), dtype=torch.long, device=dev)
    bev = F.from_cl(torch.randn(1, n[0], n[1], n[2], Cx, device=dev)).requires_grad_(True)
    gout = F.from_cl(torch.randn(1, n[0], n[1], n[2], Cx * (2 if mode == "cat" else 1), device=dev))
    F.POINT_XYZ = form == "fused"
    moments = F.point_xyz_moments(geom, tables[0], cfg["pc_range"], n) if F.POINT_XYZ else None      # calibration-only: cached

    def fwd():
        P = F.point_xyz_pool(geom, tables, cfg["pc_range"], n, *p, rm, rv, nbt, training=True, moments=moments)
        return torch.cat((bev, P), 1) if mode == "cat" else bev + P

    def step():
        for t in p + [bev]:
            t.grad = None
        fwd().backward(gout)

    def timed(f):
        for _ in range(3):
            f()
        ts = []
        for _ in range(runs):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return statistics.median(ts), min(ts), max(ts)

    with torch.no_grad():
        tf = timed(fwd)
    ts = timed(step)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
    kept = int((tables[0] >= 0).sum())
    print(f"{form:6s} {mode:3s}  forward {tf[0]:8.3f} ms (min {tf[1]:.3f}, max {tf[2]:.3f})   forward+backward {ts[0]:8.3f} ms "
          f"(min {ts[1]:.3f}, max {ts[2]:.3f})   peak above inputs {peak:8.1f} MiB   [{kept} of {tables[0].numel()} points kept, "
          f"median of {runs}]", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--runs", type=int, default=20)
    ap.add_argument("--one", nargs=2, metavar=("FORM", "MODE"), default=None)
    a = ap.parse_args()
    if a.one:
        return one(a.one[0], a.one[1], a.runs)
    lines = [f"Position encoder, xyz part + join, B = 1, 860 160 points, 128 x 128 x 16 grid, Cxyz = 128, ssbev_version() "
             f"{__import__('stereoscene_amd.capi', fromlist=['x']).load().ssbev_version()}, one MI355X"]
    for form in ("fused", "tensor"):
        for mode in ("cat", "add"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", form, mode, "--runs", str(a.runs)],
                               capture_output=True, text=True, timeout=CHILD_LIMIT)
            if r.returncode != 0:
                print(r.stdout, r.stderr, sep="\n")
                raise SystemExit(f"{form} {mode}: exit status {r.returncode}; nothing further is started")
            lines.append(r.stdout.strip().splitlines()[-1])
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
