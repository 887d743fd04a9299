"""Generate tests/golden/point_xyz.npz: the lifted-point position encoder (``point_xyz_channel`` of the reference's
``voxel_pooling``, occupancy/image2bev/ViewTransformerLSSVoxel.py:432-476) on the cases of
``stereoscene_amd.synthetic.POINT_XYZ_CASES``: the computation in the reference's order in fp32 next to a float64 restatement.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_point_xyz.py

What the reference computes, in this project's terms: the kept points (voxel index inside the grid, all samples together) get
u = ((g - lo) / (hi - lo) - 0.5) * 2 from their ego position g and the point-cloud range; the [n_kept, 3] matrix goes through
``Sequential(Linear(3, M), BatchNorm1d(M), ReLU, Linear(M, Cxyz))``, M = Cxyz // 2; the rows are summed per voxel.

  ``reference_order`` makes these calls as torch modules on the CPU in fp32 (training mode: batch statistics, running
  statistics updated; F: eval mode) and sums the rows with ``index_add_``; gradients are autograd's.
  ``restated`` is the float64 yardstick, written from the definition with explicit means and variances:
      h = u W1^T + b1;  mu = mean_p h;  var = mean_p (h - mu)^2;  z = gamma (h - mu) / sqrt(var + eps) + beta
      P[v] = sum_{p in v} (relu(z_p) W2^T + b2);  running_mean' = 0.9 rm + 0.1 mu;  running_var' = 0.9 rv + 0.1 var n / (n - 1)
  and it shares nothing with the module calls but u's fp32 inputs.

The scalar is sum(P * G) with the hashed G of the case.  Inputs are not stored: the tests rebuild them from
``synthetic.point_xyz_case(name)``; ``X_geom_crc`` pins the points.  Stored per case X and quantity q in (P, g0w, g0b, g1w, g1b,
g3w, g3b = the gradients of the six parameters, rm, rv = the running statistics after the step): ``X_ref_q`` (fp32),
``X_f64_q`` (float64) and ``X_spread_q`` = max |ref - f64| / max |f64| (g0b, whose true value is 0, is measured against
max |f64 g0w|).  P is stored for the occupied voxels only (``X_occ``: their linear indices; every other voxel is exactly 0).
F (eval mode) stores P only; G (no kept point) stores nothing but its counts.

Two conditions on the INPUTS make the ReLU masks and the voxel assignment of every fp32 evaluation agree (on failure bump
``synthetic.POINT_XYZ_SEED`` of the case, never the thresholds):
  * float64 min |z| >= 1e-4 max |z| over all kept points and channels;
  * no point that is kept, or within half a voxel of the grid, lies within 1e-4 voxel of a voxel face."""
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402

EPS, MOM = 1e-5, 0.1
NAMES = {"0.weight": "g0w", "0.bias": "g0b", "1.weight": "g1w", "1.bias": "g1b", "3.weight": "g3w", "3.bias": "g3b"}


def voxels_of(case):
    """(vox int64 [B P] with -1 for dropped points, fractional voxel coordinates float64 [B P, 3])."""
    origin, dx, n = case["grid_host"]
    g = case["geom"].reshape(-1, 3)
    f32 = (g - torch.tensor(origin)) / torch.tensor(dx)                      # the reference's fp32 sequence
    vox = F.voxel_index_tensor(case["geom"], origin, dx, n).long()
    return vox, f32.double()


def reference_order(case, vox):
    B, Cx, st = case["B"], case["Cxyz"], case["state"]
    n = case["grid_host"][2]
    M = Cx // 2
    enc = nn.Sequential(nn.Linear(3, M), nn.BatchNorm1d(M), nn.ReLU(inplace=True), nn.Linear(M, Cx))
    enc.load_state_dict(st, strict=True)
    enc.train(case["training"])
    kept = vox >= 0
    r = torch.tensor(case["cfg"]["pc_range"], dtype=torch.float32)
    u = ((case["geom"].reshape(-1, 3)[kept] - r[:3]) / (r[3:] - r[:3]) - 0.5) * 2
    f = enc(u)
    P = torch.zeros(B * n[0] * n[1] * n[2], Cx).index_add_(0, vox[kept], f)
    P = P.view(B, n[0], n[1], n[2], Cx).permute(0, 4, 1, 2, 3)
    out = {"P": P.detach()}
    if case["training"]:
        (P * case["G"]).sum().backward()
        for k, q in NAMES.items():
            out[q] = dict(enc.named_parameters())[k].grad
        out["rm"], out["rv"] = enc[1].running_mean.clone(), enc[1].running_var.clone()
    return out


def restated(case, vox):
    B, Cx, st = case["B"], case["Cxyz"], case["state"]
    n = case["grid_host"][2]
    p = {k: st[k].double().requires_grad_(True) for k in NAMES}
    kept = vox >= 0
    r = torch.tensor(case["cfg"]["pc_range"], dtype=torch.float32).double()
    u = ((case["geom"].reshape(-1, 3)[kept].double() - r[:3]) / (r[3:] - r[:3]) - 0.5) * 2
    h = u @ p["0.weight"].t() + p["0.bias"]
    out = {}
    if case["training"]:
        cnt = h.shape[0]
        mu = h.sum(0) / cnt
        var = ((h - mu) ** 2).sum(0) / cnt
        out["rm"] = ((1 - MOM) * st["1.running_mean"].double() + MOM * mu).detach()
        out["rv"] = ((1 - MOM) * st["1.running_var"].double() + MOM * var * cnt / (cnt - 1)).detach()
    else:
        mu, var = st["1.running_mean"].double(), st["1.running_var"].double()
    z = p["1.weight"] * (h - mu) / torch.sqrt(var + EPS) + p["1.bias"]
    f = torch.clamp(z, min=0.0) @ p["3.weight"].t() + p["3.bias"]
    P = torch.zeros(B * n[0] * n[1] * n[2], Cx, dtype=torch.float64).index_add(0, vox[kept], f)
    P = P.view(B, n[0], n[1], n[2], Cx).permute(0, 4, 1, 2, 3)
    out["P"] = P.detach()
    if case["training"]:
        (P * case["G"].double()).sum().backward()
        for k, q in NAMES.items():
            out[q] = p[k].grad
    return out, z.detach()


def main():
    torch.set_num_threads(1)
    out = {}
    for name in S.POINT_XYZ_CASES:
        case = S.point_xyz_case(name)
        B, Cx = case["B"], case["Cxyz"]
        nx, ny, nz = case["grid_host"][2]
        vox, fr = voxels_of(case)
        kept = vox >= 0
        n_kept = int(kept.sum())
        counts = torch.bincount(vox[kept], minlength=B * nx * ny * nz)
        out[f"{name}_geom_crc"] = np.int64(zlib.crc32(case["geom"].numpy().tobytes()))
        out[f"{name}_n_kept"] = np.int64(n_kept)
        out[f"{name}_max_list"] = np.int64(int(counts.max()))
        line = (f"case {name}: B={B} Cxyz={Cx} grid={nx}x{ny}x{nz} kept {n_kept} / {vox.numel()}, lists: max {int(counts.max())}, "
                f"{int((counts == 0).sum())} empty, {int((counts > 32).sum())} > 32, {int((counts > 256).sum())} > 256")
        # condition 2: no point near a voxel face
        near_grid = ((fr > -0.5) & (fr < torch.tensor([nx, ny, nz]) + 0.5)).all(1) | kept
        dist = (fr - fr.round()).abs()[near_grid]
        assert dist.numel() == 0 or float(dist.min()) >= 1e-4, (name, float(dist.min()))
        if name == "G":
            assert n_kept == 0
            print(line)
            continue
        assert n_kept >= 2
        if name == "B":
            per = [int((vox[i * (vox.numel() // B):(i + 1) * (vox.numel() // B)] >= 0).sum()) for i in range(B)]
            assert min(per) > 0 and not torch.equal(case["geom"][0], case["geom"][1]), per
        if name == "E":
            assert int((counts > 256).sum()) >= 1 and int(((counts > 32) & (counts <= 256)).sum()) >= 1 and int((counts == 0).sum()) >= 1
            assert n_kept < vox.numel() // 2
        ref = reference_order(case, vox)
        f64, z = restated(case, vox)
        # condition 1: no pre-activation near the ReLU's kink
        zr = float(z.abs().min() / z.abs().max())
        assert zr >= 1e-4, (name, zr)
        occ = torch.nonzero(counts > 0).flatten()
        out[f"{name}_occ"] = occ.numpy().astype(np.int32)
        spreads = []
        for q in f64:
            a, b = ref[q].double(), f64[q]
            scale = float(f64["g0w"].abs().max()) if q == "g0b" else float(b.abs().max())
            spread = float((a - b).abs().max()) / scale
            if q == "P":
                rows = lambda t: t.permute(0, 2, 3, 4, 1).reshape(-1, Cx)          # noqa: E731
                assert not rows(b)[counts == 0].any() and not rows(a)[counts == 0].any()
                a, b = rows(a)[occ], rows(b)[occ]
            out[f"{name}_ref_{q}"] = a.numpy().astype(np.float32)
            out[f"{name}_f64_{q}"] = b.numpy()
            out[f"{name}_spread_{q}"] = np.float64(spread)
            spreads.append(f"{q} {spread:.1e}")
        print(line + f" | min|z|/max|z| {zr:.1e} | spreads: " + ", ".join(spreads))
    path = os.path.join(ROOT, "tests", "golden", "point_xyz.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
