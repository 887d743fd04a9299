"""Generate tests/golden/frustum.npz: the reference's own frustum-proportion loss
(``compute_frustum_dist_loss``, utils/semkitti.py:218-244) in fp32 on the cases of ``stereoscene_amd.synthetic.FRUSTUM_CASES``,
called as the head calls it (on ``up`` = trilinear, align_corners=False, with the dense bool masks), and the reference's loader
step (``CreateRelationLabels.project_points`` / ``compute_local_frustums``, datasets/pipelines/voxel_labels.py:201-248) on the
cases of ``synthetic.FRUSTUM_LABEL_CASES``, each next to a float64 restatement.  Build container only (needs the reference
checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_frustum.py [--ref /path/to/reference]

The reference modules are loaded BY FILE PATH.  utils/semkitti.py imports only torch and numpy.  voxel_labels.py imports trimesh,
mmcv, numba and mmdet, none of which its frustum code uses: empty stand-in modules take their names in ``sys.modules`` for the
load (``numba.jit`` and ``PIPELINES.register_module`` as decorators that return their argument).  The inputs are not stored:
the tests rebuild them from ``synthetic.frustum_case`` / ``frustum_label_case`` (hash-generated, exactly reproducible).

Per loss case X: ``X_f64_loss`` and ``X_f64_grad`` (the float64 restatement ``frustum_restated``: a plain loop over
the frusta with the reference's two ``if``s; the gradient stored as fp32; not stored for D, where it is zero);
``X_counted`` (frusta that count); ``X_ref_loss`` (reference, fp32; not for D, where the reference divides 0 / 0 and raises
ZeroDivisionError -- asserted here); for the cases in ``WITH_DELTA`` ``X_ref_delta`` (fp16) with the reference's fp32 gradient =
``ref_grad(npz, X)`` = f64_grad + ref_delta * max|f64_grad| / DELTA_SCALE (the packing of tests/golden/ohem.npz);
``X_spread`` = max |reference gradient - float64 gradient| / max |float64 gradient| and ``X_loss_spread`` = |reference loss -
float64 loss| / max(1, |float64 loss|); ``X_grad_max`` = max |float64 gradient|.  For G (``SCALARS_ONLY``) no gradient array
is stored.

Per loader case X: ``X_uv_q`` (int32 [X,Y,Z,2]: the pixel coordinates of every voxel centre from the float64 restatement of the
projection, rounded to 2^-20 pixel -- half a unit, 4.8e-7 pixel, is added to the comparison rule's margin -- which halves their
size and leaves room for the gradient records; -2^31 for a centre that lands more than one image size outside the image, which
no patch edge is near) and ``X_d`` (its depth, stored as fp32); ``X_ref_ids`` (uint8: the reference's masks as ids,
argmax over its 64 masks, 255 where none holds the voxel) and ``X_ref_counts`` (float32 [64,20]); ``X_uv_err`` = the largest
|fp32 reference - float64| pixel coordinate over the voxels that land inside the image with d > 0; ``X_left_out`` = the share of
the labelled voxels the comparison rule leaves out.  For a 4x4 BEV matrix (case Q) the reference's ``project_points`` cannot run
(it multiplies the 4x4 inverse with 3-vectors): it is given the centres already taken through the inverse BEV matrix (in fp32)
and a 3x3 identity, so its record covers the rest of its chain.

Comparison rule (``left_out``).  A voxel is left out of an id comparison only if its float64 u or v lies within
8 x ``X_uv_err`` + 2^-21 of a patch edge (the image border included), or |d| <= 8 x ``X_uv_err`` / max(H, W) x max|d| (the same margin,
relative).  At most 0.5 % of a case's labelled voxels may be left out; a fixture whose own reference record needs more, or where
the reference and the restatement disagree on a voxel that is not left out, is refused: bump ``synthetic.FRUSTUM_LABEL_SEED``."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import synthetic as S  # noqa: E402
from stereoscene_amd.plugin.losses import KITTI_CLASS_NAMES  # noqa: E402

DELTA_SCALE = 16384.0
WITH_DELTA = ("A", "C", "E")            # B and F: the file would pass the size limit of a committed file
SCALARS_ONLY = ("G",)              # 327 680 gradient elements: the tests take G's gradient yardstick from a float64 run of their own
UV_SCALE = float(1 << 20)          # X_uv_q: pixel coordinates in units of 2^-20 pixel
UV_FAR = -(1 << 31)
MARGIN = 8.0
MAX_LEFT_OUT = 0.005
FS = 8


def ref_grad(npz, name):
    """The reference's fp32 logit gradient of case ``name`` from the stored float64 gradient and the fp16 difference."""
    g = npz[f"{name}_f64_grad"].astype(np.float64)
    return (g + npz[f"{name}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def load_by_path(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference_loader(ref_root):
    """voxel_labels.py with empty stand-ins for the four packages its frustum code does not use."""
    def identity_decorator(*args, **kwargs):
        return lambda fn: fn
    names = ("trimesh", "mmcv", "numba", "mmdet", "mmdet.datasets", "mmdet.datasets.builder")
    saved = {n: sys.modules.get(n) for n in names}
    try:
        for n in names:
            sys.modules[n] = types.ModuleType(n)
        sys.modules["numba"].jit = identity_decorator
        sys.modules["mmdet.datasets.builder"].PIPELINES = types.SimpleNamespace(register_module=identity_decorator)
        return load_by_path("ref_voxel_labels", os.path.join(ref_root, "projects", "mmdet3d_plugin", "datasets", "pipelines",
                                                             "voxel_labels.py"))
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m


def upsampled(x, grid):
    return x if tuple(x.shape[-3:]) == tuple(grid) else TF.interpolate(x, size=tuple(grid), mode="trilinear", align_corners=False)


def dense_masks(ids, F):
    """uint8 ids [B,X,Y,Z] -> the reference's bool masks [B,F,X,Y,Z]."""
    return ids.unsqueeze(1) == torch.arange(F, dtype=torch.uint8).view(1, F, 1, 1, 1)


def frustum_restated(up, ids, dists):
    """The loss in up's dtype, frustum by frustum; (loss, counted frusta).  0 when no frustum counts."""
    p = torch.softmax(up, dim=1)
    cnt = dists.to(up.dtype).sum(0)
    total, counted = up.sum() * 0.0, 0
    for f in range(dists.shape[1]):
        m = (ids == f).unsqueeze(1).to(up.dtype)
        cum = (p * m).sum(dim=(0, 2, 3, 4))
        if float(cum.detach().sum()) > 0 and float(cnt[f].sum()) > 0:
            t = cnt[f] / cnt[f].sum()
            q = cum / cum.sum()
            nz = t != 0
            total = total + (t[nz] * (torch.log(t[nz]) - torch.log(q[nz]))).sum()
            counted += 1
    return (total / counted if counted else total), counted


def loss_cases(ref, out):
    ref_grads = {}
    for name, (_, grid, F) in S.FRUSTUM_CASES.items():
        x, ids, dists = S.frustum_case(name)
        assert dists.shape[1] == F and tuple(ids.shape) == tuple(grid)
        x64 = x.double().requires_grad_(True)
        loss64, counted = frustum_restated(upsampled(x64, grid[1:]), ids, dists)
        loss64.backward()
        g64 = x64.grad
        out[f"{name}_f64_loss"] = np.float64(loss64.item())
        out[f"{name}_counted"] = np.int64(counted)
        line = f"case {name}: counted {counted} of {F} f64 loss {loss64.item():.9f}"
        x32 = x.clone().requires_grad_(True)
        if name == "D":
            assert counted == 0 and loss64.item() == 0.0 and not g64.any()
            try:
                ref.compute_frustum_dist_loss(upsampled(x32, grid[1:]), dense_masks(ids, F), dists)
                raise AssertionError("the reference was expected to divide 0 / 0")
            except ZeroDivisionError:
                line += " | the reference raises ZeroDivisionError"
            print(line)
            continue
        loss32 = ref.compute_frustum_dist_loss(upsampled(x32, grid[1:]), dense_masks(ids, F), dists)
        loss32.backward()
        g = g64.numpy().astype(np.float32)
        spread = ((x32.grad.double() - g64).abs().max() / g64.abs().max()).item()
        lspread = abs(loss32.item() - loss64.item()) / max(1.0, abs(loss64.item()))
        out[f"{name}_ref_loss"] = np.float32(loss32.item())
        out[f"{name}_grad_max"] = np.float64(g64.abs().max().item())
        if name not in SCALARS_ONLY:
            out[f"{name}_f64_grad"] = g
        out[f"{name}_spread"] = np.float64(spread)
        out[f"{name}_loss_spread"] = np.float64(lspread)
        if name in WITH_DELTA:
            ref_grads[name] = x32.grad.numpy().copy()
            out[f"{name}_ref_delta"] = ((ref_grads[name].astype(np.float64) - g) * (DELTA_SCALE / np.abs(g).max())).astype(np.float16)
        print(line + f" | fp32 loss {loss32.item():.9f} grad spread {spread:.2e} loss spread {lspread:.2e} max|grad| {np.abs(g).max():.3e}")
    return ref_grads


def view_tensors(view):
    """The single-view ``img_inputs`` the reference step was written for: a camera axis of 1 on every entry."""
    imgs, rots, trans, intrins, post_rots, post_trans, bda = view
    return imgs[0], rots[0], trans[0], intrins[0], post_rots[0], post_trans[0], bda[0]


def project_f64(view, pc_range, grid):
    """float64 (u, v, d) [X,Y,Z,3] of the voxel centres: the chain of ``project_points`` on exact centres."""
    imgs, rots, trans, intrins, post_rots, post_trans, bda = (t.double() for t in view_tensors(view))
    r = torch.tensor(pc_range, dtype=torch.float64)
    size = (r[3:] - r[:3]) / torch.tensor(grid, dtype=torch.float64)
    axes = [r[i] + size[i] / 2 + torch.arange(grid[i], dtype=torch.float64) * size[i] for i in range(3)]
    pts = torch.stack(torch.meshgrid(*axes, indexing="ij"), dim=-1).reshape(-1, 3)
    inv = torch.inverse(bda)
    pts = pts @ inv[:3, :3].T + (inv[:3, 3] if inv.shape[-1] == 4 else 0.0)
    pts = (pts - trans.reshape(1, 3)) @ torch.inverse(rots[0]).T
    cam = pts @ intrins[0][:3, :3].T + intrins[0][:3, 3]
    d = cam[:, 2:3]
    uv = (cam[:, :2] / d) @ post_rots[0][:2, :2].T + post_trans[0][:2]
    return torch.cat([uv, d], dim=1).reshape(*grid, 3)


def ids_from_uvd(uvd, labels, img_size):
    """The reference's patch rule on float64 coordinates -> uint8 ids."""
    H, W = img_size
    u, v, d = uvd[..., 0], uvd[..., 1], uvd[..., 2]
    ids = torch.full(labels.shape, 255, dtype=torch.uint8)
    for py in range(FS):
        for px in range(FS):
            m = ((u >= px / FS * W) & (u < (px + 1) / FS * W) & (v >= py / FS * H) & (v < (py + 1) / FS * H) & (d > 0)
                 & (labels != 255))
            ids[m] = py * FS + px
    return ids


def decode_uv(q):
    """int32 ``X_uv_q`` -> float64 pixel coordinates, NaN for a far-outside centre."""
    return np.where(q == UV_FAR, np.nan, q.astype(np.float64) / UV_SCALE)


def left_out(uv, d, uv_err, img_size):
    """bool [X,Y,Z]: the voxels the comparison rule leaves out (see the module docstring)."""
    H, W = img_size
    tol = MARGIN * float(uv_err) + 0.5 / UV_SCALE
    out = np.zeros(uv.shape[:-1], dtype=bool)
    for axis, size in ((0, W), (1, H)):
        for i in range(FS + 1):
            out |= np.abs(uv[..., axis] - i / FS * size) <= tol      # (a NaN coordinate is far outside: never near an edge)
    out |= np.abs(d) <= tol / max(H, W) * np.abs(d).max()
    return out


def loader_cases(refmod, out):
    for name in S.FRUSTUM_LABEL_CASES:
        labels, view, pc_range = S.frustum_label_case(name)
        grid = tuple(labels.shape)
        imgs, rots, trans, intrins, post_rots, post_trans, bda = view_tensors(view)
        img_size = tuple(imgs.shape[-2:])
        step = refmod.CreateRelationLabels(pc_range, grid, list(KITTI_CLASS_NAMES))
        centres = step.voxel_centers.view(-1, 3)
        if bda.shape[-1] == 4:
            inv = bda.inverse()
            centres, bda = centres @ inv[:3, :3].T + inv[:3, 3], torch.eye(3)
        uvd32 = step.project_points(centres, rots, trans, intrins, post_rots, post_trans, bda)[:, 0]
        masks, counts = step.compute_local_frustums(uvd32, labels, img_size=img_size)
        assert int(masks.sum(0).max()) <= 1                          # disjoint: one byte per voxel holds them
        ref_ids = torch.where(masks.any(0), masks.to(torch.uint8).argmax(0).to(torch.uint8), torch.tensor(255, dtype=torch.uint8))
        uvd64 = project_f64(view, pc_range, grid)
        ids64 = ids_from_uvd(uvd64, labels, img_size)
        H, W = img_size
        inside = ((uvd64[..., 0] >= 0) & (uvd64[..., 0] < W) & (uvd64[..., 1] >= 0) & (uvd64[..., 1] < H) & (uvd64[..., 2] > 0))
        uv_err = float((uvd32.reshape(*grid, 3)[..., :2].double() - uvd64[..., :2])[inside].abs().max())
        uv = uvd64[..., :2]
        far = ~((uv[..., 0] > -W) & (uv[..., 0] < 2 * W) & (uv[..., 1] > -H) & (uv[..., 1] < 2 * H))
        q = torch.round(uv * UV_SCALE)
        assert float(q[~far].abs().max()) < 2.0 ** 31 and not (far & (ids64 != 255)).any()
        q[far] = UV_FAR
        q = q.numpy().astype(np.int32)
        d32 = uvd64[..., 2].numpy().astype(np.float32)
        out_mask = torch.from_numpy(left_out(decode_uv(q), d32.astype(np.float64), uv_err, img_size))     # on the stored record
        labelled = labels != 255
        share = float((out_mask & labelled).sum()) / float(labelled.sum())
        differ = int(((ref_ids != ids64) & ~out_mask).sum())
        print(f"loader case {name}: uv_err {uv_err:.3e} left out {share:.4%} of {int(labelled.sum())} labelled voxels, "
              f"{int((ids64 != 255).sum())} in a frustum, {int(inside.sum())} centres inside the image, reference / float64 ids differ on "
              f"{int((ref_ids != ids64).sum())} voxels ({differ} of them kept)")
        assert share <= MAX_LEFT_OUT, (name, share, "bump synthetic.FRUSTUM_LABEL_SEED")
        assert differ == 0, (name, differ, "bump synthetic.FRUSTUM_LABEL_SEED")
        out[f"{name}_uv_q"] = q
        out[f"{name}_d"] = d32
        out[f"{name}_ref_ids"] = ref_ids.numpy()
        out[f"{name}_ref_counts"] = counts.numpy().astype(np.float32)
        out[f"{name}_uv_err"] = np.float64(uv_err)
        out[f"{name}_left_out"] = np.float64(share)


def main():
    torch.set_num_threads(1)
    if "--ref" in sys.argv:
        ref_root = sys.argv[sys.argv.index("--ref") + 1]
    else:
        from oracle import make_golden as MG
        ref_root = MG.REF
    ref = load_by_path("ref_semkitti", os.path.join(ref_root, "projects", "mmdet3d_plugin", "utils", "semkitti.py"))
    out = {}
    ref_grads = loss_cases(ref, out)
    loader_cases(load_reference_loader(ref_root), out)
    path = os.path.join(ROOT, "tests", "golden", "frustum.npz")
    np.savez_compressed(path, **out)
    back = np.load(path)
    for name, g32 in ref_grads.items():
        err = np.abs(ref_grad(back, name) - g32).max() / np.abs(back[f"{name}_f64_grad"]).max()
        assert err < 2e-7, (name, err)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
