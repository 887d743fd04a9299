"""Generate tests/golden/occ_depth.npz: the reference's own CreateDepthFromOccupancy (occ_to_depth.py:15-153) on small grids.
Build container only (needs the reference checkout; no GPU).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_occ_depth.py

The class is imported from the reference checkout under the stand-ins of tools/make_golden_augment.py for the absent third-party
imports (mmcv, mmdet, trimesh, numba; none takes part in its arithmetic).  Per case its ``__call__`` runs as it stands on a
nine-element view (the length its unpack at :143 accepts) and float labels (its index_put at :140 refuses an integer source for
the float map): that executes ``project_points`` and the two z-buffer blocks
(:96-140).  The label map is ``results['img_seg']``; the depth map, which the step computes and then drops (:144 assigns into a
temporary list), is the tensor its ``torch.zeros((img_h, img_w))`` returned, filled in place at :127 -- recorded by wrapping
``torch.zeros`` for the duration of the call.  ``_downsample_label`` is then called on the label map.  Stored: inputs and outputs
as arrays only (labels uint8, the six camera matrices, depth as sparse index / value pairs, label maps as uint8), plus one
hand-built label image with the reference's pooled result (``pool_in`` / ``pool_out``).

Cases: grids (16,16,4), (32,32,8), (24,40,6) x cameras a (KITTI-like Tr / P2 scaled to the image), b (a, with a post_rots that
carries a flip and a rotation), c (a 3x3 bda_rot with rotation, scale and both flips; its grid lies at negative x of the
augmented frame so that the inverse puts it in front of the camera), the image size rotating through 32x96, 48x160, 37x101;
``nothing`` (a camera that sees nothing of the grid), ``no_occupied`` (labels 0 / 255 only), ``only255``.  Labels: hashed
classes (stereoscene_amd.synthetic.hash_uniform), ~35 % occupied, ~5 % ignored, the quarter of the grid nearest the camera and
everything else empty -- empty voxels in front of surfaces, which take pixels in the reference's label map.

Header record (this container's CPU, torch 2.10): pixels where the reference differs from the explicit fp32 operation order
(the tensor form of functional.occupancy_depth_map): 0 of 57 956 fixture pixels, cap 28 (0.05 %); pixels the float64 model
calls borderline (a voxel within 2^-10 px of a rounding or frame boundary): 155 over the twelve cases, printed per case; pixels
whose nearest voxels tie exactly in fp32 depth with different labels: 0."""
import importlib
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import occ_depth_cases as OC  # noqa: E402
from stereoscene_amd import functional as F, synthetic as S  # noqa: E402

GRIDS = ((16, 16, 4), (32, 32, 8), (24, 40, 6))
RANGES = ([0, -6.4, -2, 12.8, 6.4, 1.2], [0, -12.8, -2, 25.6, 12.8, 4.4], [0, -20, -2, 24, 20, 4])
IMAGES = ((32, 96), (48, 160), (37, 101))


def labels_for(tag, shape, kind="scene"):
    if kind == "only255":
        return np.full(shape, 255, dtype=np.uint8)
    cls = S.hash_uniform(f"occ_depth/{tag}/cls", shape, 1.0, 20.0).floor().clamp_(1, 19).numpy().astype(np.uint8)
    u = S.hash_uniform(f"occ_depth/{tag}/occ", shape, 0.0, 1.0).numpy()
    lab = np.where(u < 0.35, cls, np.where(u > 0.95, 255, 0)).astype(np.uint8)
    near = np.abs(np.arange(shape[0]) - (0 if kind != "flipped" else shape[0] - 1)) < shape[0] // 4
    lab[near] = 0                                             # empty space between the camera and the surfaces
    if kind == "no_occupied":
        lab = np.where(u > 0.5, 255, 0).astype(np.uint8)
    return lab


def camera(W, H, form):
    rots, trans, intr, post_rots, post_trans, bda, _ = S.kitti_calibration(1, W)
    m = dict(rots=rots[0].numpy(), trans=trans[0].numpy(), intrins=intr[0].numpy(), post_rots=post_rots[0].numpy().copy(),
             post_trans=post_trans[0].numpy().copy(), bda=bda[0].numpy().copy())
    if form == "b":                                           # mirror about the width, then rotate about the image centre
        a = math.radians(4.0)
        rot = np.array([[math.cos(a), math.sin(a)], [-math.sin(a), math.cos(a)]])
        flip, fb = np.array([[-1.0, 0.0], [0.0, 1.0]]), np.array([W - 1.0, 0.0])
        ctr = np.array([(W - 1) / 2.0, (H - 1) / 2.0])
        m["post_rots"][0, :2, :2] = (rot @ flip).astype(np.float32)
        m["post_trans"][0, :2] = (rot @ (fb - ctr) + ctr).astype(np.float32)
    if form == "c":                                           # rotation, scale and both flips
        a = math.radians(10.0)
        rot = np.array([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1]])
        m["bda"] = (np.diag([-1.0, -1.0, 1.0]) @ (1.03 * rot)).astype(np.float32)
    if form == "nothing":                                     # the grid behind the camera
        m["bda"] = np.diag([-1.0, -1.0, 1.0]).astype(np.float32)
    return m


def case_list():
    out = []
    for gi, grid in enumerate(GRIDS):
        for ci, form in enumerate("abc"):
            r = list(RANGES[gi])
            if form == "c":
                r[0], r[3] = -r[3], -r[0]
            out.append((f"g{gi}{form}", grid, r, IMAGES[(gi + ci) % 3], form, "flipped" if form == "c" else "scene", True))
    out.append(("nothing", GRIDS[0], RANGES[0], IMAGES[0], "nothing", "scene", False))
    out.append(("no_occupied", GRIDS[1], RANGES[1], IMAGES[2], "a", "no_occupied", False))
    out.append(("only255", GRIDS[0], RANGES[0], IMAGES[1], "a", "only255", False))
    return out


def pool_image():
    """32 x 64 (eight 16 x 16 patches) + 5 trailing rows / 3 trailing columns that the rule drops.  0.95 * 256 = 243.2."""
    img = np.zeros((37, 67), dtype=np.uint8)
    def patch(i, j, counts):
        flat = np.concatenate([np.full(n, v, dtype=np.uint8) for v, n in counts])
        assert flat.size == 256
        perm = np.argsort(S.hash_uniform(f"occ_depth/pool/{i}{j}", (256,), 0.0, 1.0).numpy(), kind="stable")
        img[i * 16:(i + 1) * 16, j * 16:(j + 1) * 16] = flat[perm].reshape(16, 16)
    patch(0, 0, [(0, 200), (255, 44), (7, 12)])               # 244 empty > 243.2: zeros win -> 0
    patch(0, 1, [(0, 100), (255, 143), (7, 13)])              # 243 empty: not above the threshold -> the class, 7
    patch(0, 2, [(0, 122), (255, 122), (3, 12)])              # 244 empty, zeros == 255s -> 255
    patch(0, 3, [(0, 100), (9, 60), (4, 60), (255, 36)])      # a two-way class tie -> the lower id, 4
    patch(1, 0, [(255, 256)])                                 # all ignored -> 255
    patch(1, 1, [(0, 256)])                                   # all empty -> 0
    patch(1, 2, [(254, 50), (1, 50), (0, 156)])               # the ends of the class range tie -> 1
    patch(1, 3, [(12, 256)])
    img[32:, :] = 5
    img[:, 64:] = 6
    return img


def main():
    torch.set_num_threads(1)
    import make_golden_augment as MGA
    MGA.install_stand_ins()
    O2D = importlib.import_module("projects.mmdet3d_plugin.datasets.pipelines.occ_to_depth")
    out, names, cases = {}, [], []
    for name, grid, pc_range, (H, W), form, kind, occlusion in case_list():
        lab = labels_for(name, grid, kind)
        mats = camera(W, H, form)
        view = OC.make_view(H, W, mats)
        step = O2D.CreateDepthFromOccupancy(point_cloud_range=pc_range, grid_size=list(grid), downsample=False)
        made = []
        zeros = torch.zeros
        torch.zeros = lambda *a, **k: made.append(zeros(*a, **k)) or made[-1]
        try:
            res = step(dict(gt_occ=torch.from_numpy(lab.copy()).float(), img_inputs=[view[:9]]))
        finally:
            torch.zeros = zeros
        depth = next(t for t in made if tuple(t.shape) == (H, W))
        seg = res["img_seg"]
        pooled = step._downsample_label(seg)
        assert float(seg.min()) >= 0 and float(seg.max()) <= 255 and torch.equal(seg, seg.round())
        names.append(name)
        idx = torch.nonzero(depth.reshape(-1)).reshape(-1)
        out[f"{name}_labels"], out[f"{name}_pc_range"] = lab, np.asarray(pc_range, dtype=np.float64)
        out[f"{name}_hw"] = np.array([H, W], dtype=np.int32)
        for k in OC.VIEW_KEYS:
            out[f"{name}_{k}"] = np.asarray(mats[k], dtype=np.float32)
        out[f"{name}_depth_idx"], out[f"{name}_depth_val"] = idx.to(torch.int32).numpy(), depth.reshape(-1)[idx].numpy()
        out[f"{name}_seg"], out[f"{name}_pooled"] = seg.numpy().astype(np.uint8), pooled.numpy().astype(np.uint8)
        out[f"{name}_occlusion"] = np.uint8(occlusion)
        case = dict(name=name, labels=lab, pc_range=list(pc_range), H=H, W=W, mats=mats, view=view, depth=depth.numpy(),
                    seg=seg.numpy(), pooled=pooled.numpy(), occlusion=occlusion)
        cases.append(case)
        # the reference against the explicit operation order, judged by the float64 model
        d2, s2 = F.occupancy_depth_map(torch.from_numpy(lab.copy()), view, pc_range)
        p2 = F.label_map_downsample(s2)
        _, _, tie, hidden = OC.brute_force(case, False)
        n_diff, bad = OC.compare(case, d2.numpy(), s2.numpy(), p2.numpy(), tie)
        case["n_diff"], case["bad"] = n_diff, bad
        print(f"{name}: grid {grid} image {H}x{W}: depth pixels {idx.numel()}, label pixels {int((seg != 255).sum())}, hidden "
              f"surfaces {hidden}, borderline pixels {int(OC.borderline(case).sum())}, exact ties with different labels "
              f"{int(tie.sum())}; reference vs explicit order: {n_diff} pixels differ, {bad} outside the rule")
        assert hidden > 0 or not occlusion, name
    img = pool_image()
    out["pool_in"] = img
    out["pool_out"] = O2D.CreateDepthFromOccupancy(RANGES[0], list(GRIDS[0]))._downsample_label(torch.from_numpy(img).float()).numpy().astype(np.uint8)
    print("pool_out", out["pool_out"].tolist())
    out["names"] = np.array(names)
    total, diff = OC.total_pixels(cases), sum(c["n_diff"] for c in cases)
    print(f"total: {diff} differing pixels of {total}, cap {int(OC.CAP * total)}; outside the rule {sum(c['bad'] for c in cases)}")
    assert diff <= OC.CAP * total and not any(c["bad"] for c in cases)
    np.savez_compressed(OC.GOLDEN, **out)
    print("wrote", OC.GOLDEN, os.path.getsize(OC.GOLDEN) / 1e3, "kB")
    assert os.path.getsize(OC.GOLDEN) < 1 << 20


if __name__ == "__main__":
    main()
