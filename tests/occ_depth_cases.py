"""Shared by tests/test_occ_depth.py, tests/test_gpu_occ_depth.py and tools/make_golden_occ_depth.py: the cases of
tests/golden/occ_depth.npz (inputs and the reference's own outputs, arrays only), a float32 NumPy brute-force model of the
nearest-voxel maps, a float64 model of the projection, and the rule that says which pixels may differ from the fixture.

The rule (the only allowance of these tests): the reference's broadcast matmul may round a product chain differently from the
explicit operation order, so a pixel may differ from the fixture only where the float64 projection puts a voxel within
``EPS`` = 2^-10 px of a rounding boundary (x.5) or of the frame (0, W-1, H-1) and that voxel can reach the pixel, or -- for the
label map -- where two differently labelled voxels of the pixel share the minimal fp32 depth exactly.  Over the whole fixture such
pixels may be at most ``CAP`` = 0.05 % of all fixture pixels."""
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "occ_depth.npz")
EPS = 2.0 ** -10
CAP = 0.0005
DS = 16
VIEW_KEYS = ("rots", "trans", "intrins", "post_rots", "post_trans", "bda")


def make_view(H, W, mats):
    """One view of ``img_inputs`` (ten slots) from the six camera arrays; slot 0 is a stride-0 all-zero image [1,3,H,W]."""
    return [torch.zeros(1).expand(1, 3, H, W)] + [torch.from_numpy(np.asarray(mats[k], dtype=np.float32).copy()) for k in VIEW_KEYS] + \
        [torch.zeros(1, H, W), torch.zeros(1), torch.zeros(())]


def load_cases():
    g = np.load(GOLDEN)
    cases = []
    for name in [str(n) for n in g["names"]]:
        H, W = (int(v) for v in g[f"{name}_hw"])
        depth = np.zeros(H * W, dtype=np.float32)
        depth[g[f"{name}_depth_idx"].astype(np.int64)] = g[f"{name}_depth_val"]
        mats = {k: g[f"{name}_{k}"] for k in VIEW_KEYS}
        cases.append(dict(name=name, labels=g[f"{name}_labels"], pc_range=[float(v) for v in g[f"{name}_pc_range"]], H=H, W=W,
                          mats=mats, view=make_view(H, W, mats), depth=depth.reshape(H, W),
                          seg=g[f"{name}_seg"].astype(np.float32), pooled=g[f"{name}_pooled"].astype(np.float32),
                          occlusion=bool(g[f"{name}_occlusion"])))
    return cases


def tie_case():
    """A grid placed so that several voxels share a pixel at exactly equal fp32 depth (see test_depth_ties_go_to_the_lowest_index)."""
    X, Y, Z = 8, 8, 6
    lab = (1 + (np.arange(X * Y * Z) * 7) % 19).astype(np.uint8).reshape(X, Y, Z)
    H, W = 16, 24
    K = np.eye(4, dtype=np.float32)
    K[0, 0] = K[1, 1] = 80.0
    K[0, 2], K[1, 2] = 12.0, 8.0
    mats = dict(rots=np.eye(3, dtype=np.float32)[None], trans=np.array([[0.125, 0.125, -40.0]], dtype=np.float32), intrins=K[None],
                post_rots=np.eye(3, dtype=np.float32)[None], post_trans=np.zeros((1, 3), dtype=np.float32),
                bda=np.eye(3, dtype=np.float32))
    return dict(name="ties", labels=lab, pc_range=[-1.0, -1.0, 0.0, 1.0, 1.0, 6.0], H=H, W=W, mats=mats, view=make_view(H, W, mats))


def centres(case, dtype):
    """Voxel centres [N,3] in grid order from the fp32 tables the step itself uses (the reference's torch.arange)."""
    from stereoscene_amd import functional as F
    X, Y, Z = case["labels"].shape
    t = F.occ_voxel_tables(case["pc_range"], (X, Y, Z)).numpy()
    xs, ys, zs = np.meshgrid(t[:X], t[X:X + Y], t[X + Y:], indexing="ij")
    return np.stack([xs, ys, zs], axis=-1).reshape(-1, 3).astype(dtype)


def _inverses(case):
    m = case["mats"]
    n = m["bda"].shape[-1]
    inv_bda = torch.inverse(torch.from_numpy(m["bda"].astype(np.float32).reshape(n, n))).numpy()
    inv_rot = torch.inverse(torch.from_numpy(m["rots"].astype(np.float32).reshape(3, 3))).numpy()
    return n, inv_bda, inv_rot


def project(case, dtype):
    """(u, v, d) of every voxel centre in ``dtype`` (np.float32: one rounding per operation in project_points' order; np.float64: the
    model the allowance is judged by).  The fp32 inverses are the inputs of both."""
    m = case["mats"]
    n, A, R = _inverses(case)
    A, R = A.astype(dtype), R.astype(dtype)
    t = m["trans"].reshape(-1)[:3].astype(dtype)
    K = m["intrins"].reshape(4, 4).astype(dtype)
    pr = m["post_rots"].reshape(3, 3)[:2, :2].astype(dtype)
    pt = m["post_trans"].reshape(-1)[:2].astype(dtype)
    p = centres(case, dtype)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        l3 = [(A[i, 0] * px + A[i, 1] * py) + A[i, 2] * pz for i in range(3)]
        if n == 4:
            l3 = [l3[i] + A[i, 3] for i in range(3)]
        x, y, z = (l3[i] - t[i] for i in range(3))
        c = [(R[i, 0] * x + R[i, 1] * y) + R[i, 2] * z for i in range(3)]
        q = [((K[i, 0] * c[0] + K[i, 1] * c[1]) + K[i, 2] * c[2]) + K[i, 3] for i in range(3)]
        u0, v0, d = q[0] / q[2], q[1] / q[2], q[2]
        u = (pr[0, 0] * u0 + pr[0, 1] * v0) + pt[0]
        v = (pr[1, 0] * u0 + pr[1, 1] * v0) + pt[1]
    return u, v, d


def brute_force(case, occupied_only):
    """float32 NumPy model: per pixel the nearest competing voxel centre (lowest index among equal depths).  Returns
    (depth [H,W], seg [H,W], tie [H,W] bool: the label map's winner shares its depth with a differently labelled voxel,
    hidden int: pixels where an empty / ignored voxel lies in front of an occupied one)."""
    H, W = case["H"], case["W"]
    u, v, d = project(case, np.float32)
    lab = case["labels"].reshape(-1)
    with np.errstate(all="ignore"):
        ok = (u >= 0) & (v >= 0) & (u <= np.float32(W - 1)) & (v <= np.float32(H - 1)) & (d > 0)
    occ = (lab != 0) & (lab != 255)
    depth = np.zeros((H, W), dtype=np.float32)
    seg = np.full((H, W), 255.0, dtype=np.float32)
    tie = np.zeros((H, W), dtype=bool)
    best_occ, best_any = {}, {}
    for i in np.nonzero(ok)[0]:
        pix = (int(np.rint(v[i])), int(np.rint(u[i])))
        for table, competes in ((best_occ, occ[i]), (best_any, True)):
            if competes:
                table.setdefault(pix, []).append((d[i], int(i)))
    for pix, lst in best_occ.items():
        depth[pix] = min(lst)[0]
    for pix, lst in (best_occ if occupied_only else best_any).items():
        dmin, imin = min(lst)
        seg[pix] = lab[imin]
        tie[pix] = any(dd == dmin and lab[j] != lab[imin] for dd, j in lst)
    hidden = sum(1 for pix, lst in best_occ.items() if not occ[min(best_any[pix])[1]])
    return depth, seg, tie, hidden


def borderline(case):
    """bool [H,W]: pixels a voxel can reach whose float64 projection lies within EPS of a rounding or frame boundary."""
    H, W = case["H"], case["W"]
    u, v, d = project(case, np.float64)
    with np.errstate(all="ignore"):
        fin = np.isfinite(u) & np.isfinite(v) & (d > 0)
        near = (np.abs(u - np.floor(u) - 0.5) <= EPS) | (np.abs(v - np.floor(v) - 0.5) <= EPS) | (np.abs(u) <= EPS) | \
            (np.abs(v) <= EPS) | (np.abs(u - (W - 1)) <= EPS) | (np.abs(v - (H - 1)) <= EPS)
    mask = np.zeros((H, W), dtype=bool)
    for i in np.nonzero(fin & near)[0]:
        for du in (-EPS, EPS):
            for dv in (-EPS, EPS):
                r, c = int(np.rint(v[i] + dv)), int(np.rint(u[i] + du))
                if 0 <= r < H and 0 <= c < W:
                    mask[r, c] = True
    return mask


def compare(case, depth, seg, pooled, tie=None):
    """Maps (arrays) against the fixture's: returns (differing pixels over the three maps, those the rule does not excuse)."""
    if tie is None:
        tie = brute_force(case, False)[2]
    dd, ds = depth != case["depth"], seg != case["seg"]
    n_diff = int(dd.sum()) + int(ds.sum())
    bad = 0
    if n_diff:
        edge = borderline(case)
        bad = int((dd & ~edge).sum()) + int((ds & ~edge & ~tie).sum())
    dp = pooled != case["pooled"]
    for i, j in zip(*np.nonzero(dp)):
        n_diff += 1
        bad += 0 if ds[i * DS:(i + 1) * DS, j * DS:(j + 1) * DS].any() else 1
    return n_diff, bad


def total_pixels(cases):
    return sum(c["H"] * c["W"] for c in cases)


def pool_model(seg, ds=DS):
    """NumPy histogram model of the pooling rule."""
    H, W = seg.shape
    out = np.zeros((H // ds, W // ds), dtype=np.float32)
    for i in range(H // ds):
        for j in range(W // ds):
            hist = np.bincount(seg[i * ds:(i + 1) * ds, j * ds:(j + 1) * ds].astype(np.int64).reshape(-1), minlength=256)
            if np.float32(hist[0] + hist[255]) > np.float32(0.95 * ds * ds):
                out[i, j] = 0 if hist[0] > hist[255] else 255
            else:
                out[i, j] = 1 + int(np.argmax(hist[1:255]))          # argmax: the first (lowest) of equal counts
    return out
