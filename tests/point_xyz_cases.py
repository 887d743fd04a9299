"""Shared by tests/test_point_xyz.py and tests/test_gpu_point_xyz.py: the fixture tests/golden/point_xyz.npz
(tools/make_golden_point_xyz.py), the cases rebuilt from ``synthetic.point_xyz_case`` and the bounds.

Bounds, the rule of tests/test_imgseg.py: K = 8 times the case's recorded reference-fp32-vs-float64 spread of the quantity, floored
at the fp32 unit roundoff 2^-23, times the quantity's largest float64 magnitude, on EVERY element.  ``g0b`` (the first Linear's
bias gradient, exactly 0 in exact arithmetic: BatchNorm removes the mean) is scaled by max |float64 g0w| as its spread was."""
import functools
import os

import numpy as np
import torch

from conftest import ROOT
from stereoscene_amd import functional as F, synthetic as S

GOLDEN = os.path.join(ROOT, "tests", "golden", "point_xyz.npz")
K = 8.0
EPS = 2.0 ** -23
TRAINED = ("A", "B", "C", "D", "E")
GRADS = {"0.weight": "g0w", "0.bias": "g0b", "1.weight": "g1w", "1.bias": "g1b", "3.weight": "g3w", "3.bias": "g3b"}


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs: rebuilt from the hash generator, shared and never modified."""
    return S.point_xyz_case(name)


@functools.lru_cache(maxsize=None)
def vox_of(name):
    c = case(name)
    return F.voxel_index_tensor(c["geom"], *c["grid_host"])


def tol(name, q):
    g = golden()
    scale = np.abs(g[f"{name}_f64_{'g0w' if q == 'g0b' else q}"]).max()
    return K * max(float(g[f"{name}_spread_{q}"]), EPS) * float(scale)


def rows(name, P):
    """[B, Cxyz, X, Y, Z] -> float64 numpy ([occupied voxels, Cxyz], [empty voxels, Cxyz])."""
    Cx = P.shape[1]
    r = P.detach().permute(0, 2, 3, 4, 1).reshape(-1, Cx).double().cpu()
    occ = torch.from_numpy(golden()[f"{name}_occ"].astype(np.int64))
    empty = torch.ones(r.shape[0], dtype=torch.bool)
    empty[occ] = False
    return r[occ].numpy(), r[empty].numpy()


def params_of(name, device):
    st = case(name)["state"]
    p = {k: st[k].clone().to(device).requires_grad_(k in GRADS) for k in st}
    return p


def run(name, device, fused, scale=1.0, moments=None, tables=None):
    """One forward (+ backward for the training cases) of the xyz part: dict P [B,Cxyz,X,Y,Z], g0w .. g3b, rm, rv, nbt (CPU)."""
    c = case(name)
    p = params_of(name, device)
    geom = c["geom"].to(device)
    n = c["grid_host"][2]
    args = (p["0.weight"], p["0.bias"], p["1.weight"], p["1.bias"], p["3.weight"], p["3.bias"], p["1.running_mean"],
            p["1.running_var"], p["1.num_batches_tracked"])
    if fused:
        if tables is None:
            tables = F.lift_splat_tables(geom, None, None, None, grid_host=c["grid_host"])
        P = F.point_xyz_pool(geom, tables, c["cfg"]["pc_range"], n, *args, training=c["training"], moments=moments)
    else:
        P = F.point_xyz_pool_tensor(geom, vox_of(name).to(device), c["cfg"]["pc_range"], n, *args, training=c["training"])
    out = {"P": P.detach().cpu()}
    if c["training"]:
        (P * (scale * c["G"].to(device))).sum().backward()
        for k, q in GRADS.items():
            out[q] = p[k].grad.cpu()
    out["rm"], out["rv"], out["nbt"] = p["1.running_mean"].cpu(), p["1.running_var"].cpu(), int(p["1.num_batches_tracked"])
    return out


def check(name, got, what, scale=1.0):
    g = golden()
    c = case(name)
    occ, empty = rows(name, got["P"])
    assert not empty.any(), f"{name} {what}: an empty voxel is not exactly 0"
    qs = ["P"] + (list(GRADS.values()) + ["rm", "rv"] if c["training"] else [])
    for q in qs:
        have = occ if q == "P" else got[q].double().numpy()
        if q in GRADS.values():
            have = have / scale
        bound = tol(name, q)
        e_ref = float(np.abs(have - g[f"{name}_ref_{q}"].astype(np.float64)).max())
        e_f64 = float(np.abs(have - g[f"{name}_f64_{q}"]).max())
        print(name, what, q, "error against reference fp32", e_ref, "against float64", e_f64, "bound", bound)
        assert np.isfinite(have).all() and e_ref <= bound and e_f64 <= bound, (name, what, q, e_ref, e_f64, bound)
