"""Generate tests/golden/image_augment.npz: the reference's own LoadMultiViewImageFromFiles_SemanticKitti
(loading_semkitti.py:76-302) in train mode with the image-view augmentation its config ships commented out
(stereoscene.py:34-36: resize (-0.06, 0.11), rot (-5.4, 5.4), flip True), and its CreateDepthFromLiDAR
(occ_to_depth.py:189-412) on one such rotated sample.  Build container only (needs the reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_augment.py

Inputs are those of oracle/make_golden_data.py (stereo_images, stereo_meta, scene), under the same stand-ins for the absent
third-party imports; none of them takes part in the arithmetic of these classes.  Stored per seed: the drawn
(resize, crop, flip, rotate) and per view img / post_rot / post_tran; for the LiDAR sample the depth and segmentation maps in
the sparse layout of lidar_depth.npz."""
import importlib
import os
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import make_golden as MG  # noqa: E402
from oracle import make_golden_data as MGD  # noqa: E402

AUG_CONFIG = {"input_size": MGD.IN_SIZE, "resize": (-0.06, 0.11), "rot": (-5.4, 5.4), "flip": True, "crop_h": (0.0, 0.0),
              "resize_test": 0.0}
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)
SEEDS = (0, 2, 4, 5)               # both flip states, both angle signs, a crop above the image (checked below)
LIDAR_SEED = 0


def install_stand_ins():
    """The stand-ins of oracle/make_golden_data.py (main + loader_fixtures) for the imports of loading_semkitti.py and
    occ_to_depth.py."""
    from PIL import Image
    MG.install_shims()
    for name in ("trimesh", "numba"):
        MG._mod(name, jit=lambda *a, **k: (lambda f: f))
    MG._pkg("mmdet.datasets")
    MG._mod("mmdet.datasets.builder", PIPELINES=MG._Registry("pipelines"))
    sys.modules["mmcv"].__dict__.setdefault("__version__", "1.4.0")
    MG._pkg("projects.mmdet3d_plugin.datasets", os.path.join(MG.REF, "projects", "mmdet3d_plugin", "datasets"))
    MG._pkg("projects.mmdet3d_plugin.datasets.pipelines",
            os.path.join(MG.REF, "projects", "mmdet3d_plugin", "datasets", "pipelines"))

    def imread(path, flag="unchanged"):                       # mmcv.imread: cv2 order (BGR)
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"))[..., ::-1].copy()

    def imnormalize(img, mean, std, to_rgb=True):             # mmcv.image.photometric.imnormalize (published formula)
        img = img.copy().astype(np.float32)
        mean64 = np.float64(mean.reshape(1, -1))
        stdinv = 1 / np.float64(std.reshape(1, -1))
        if to_rgb:
            img = img[..., ::-1]
        return ((img - mean64.astype(np.float32)) * stdinv.astype(np.float32)).astype(np.float32)

    sys.modules["mmcv"].imread = imread
    MG._pkg("mmcv.image")
    MG._mod("mmcv.image.photometric", imnormalize=imnormalize)
    MG._mod("torchvision")
    MG._mod("pyquaternion", Quaternion=object)
    MG._pkg("mmdet3d.core")
    MG._mod("mmdet3d.core.points", BasePoints=object, get_points_type=None)
    MG._mod("mmdet3d.core.bbox", LiDARInstance3DBoxes=object)
    MG._mod("mmdet.datasets.pipelines", LoadAnnotations=object, LoadImageFromFile=object)
    import scipy.ndimage
    if not hasattr(scipy.ndimage, "interpolation"):
        scipy.ndimage.interpolation = types.SimpleNamespace(rotate=scipy.ndimage.rotate)


def main():
    torch.set_num_threads(1)                 # DataLoader-worker configuration (see oracle/make_golden_data.py: main)
    install_stand_ins()
    from PIL import Image
    LS = importlib.import_module("projects.mmdet3d_plugin.datasets.pipelines.loading_semkitti")
    O2D = importlib.import_module("projects.mmdet3d_plugin.datasets.pipelines.occ_to_depth")
    imgs, meta = MGD.stereo_images(), MGD.stereo_meta()
    pts, raw = MGD.scene()
    out = dict(seeds=np.asarray(SEEDS, dtype=np.int64))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:
        names = []
        for im, cam in zip(imgs, ("image_2", "image_3")):
            d = os.path.join(tmp, "sequences", "00", cam)
            os.makedirs(d)
            Image.fromarray(im).save(os.path.join(d, "000123.png"))
            names.append(os.path.join(d, "000123.png"))
        os.makedirs(os.path.join(tmp, "data/lidar/velodyne/dataset/sequences/00/velodyne"))
        os.makedirs(os.path.join(tmp, "data/lidar/lidarseg/dataset/sequences/00/labels"))
        pts.tofile(os.path.join(tmp, "data/lidar/velodyne/dataset/sequences/00/velodyne/000123.bin"))
        raw.tofile(os.path.join(tmp, "data/lidar/lidarseg/dataset/sequences/00/labels/000123.label"))
        for seed in SEEDS:
            step = LS.LoadMultiViewImageFromFiles_SemanticKitti(data_config=AUG_CONFIG, is_train=True, colorjitter=False,
                                                                img_norm_cfg=NORM)
            drawn = []
            draw = step.sample_augmentation
            step.sample_augmentation = lambda *a, **k: drawn.append(draw(*a, **k)) or drawn[-1]
            np.random.seed(seed)
            results = step(dict(img_filename=names, gt_occ=np.zeros((4, 4, 2), dtype=np.uint8), **meta))
            resize, dims, crop, flip, rotate = drawn[0]
            out[f"s{seed}_resize"] = np.float64(resize)
            out[f"s{seed}_resize_dims"] = np.asarray(dims, dtype=np.int64)
            out[f"s{seed}_crop"] = np.asarray(crop, dtype=np.int64)
            out[f"s{seed}_flip"] = np.int64(bool(flip))
            out[f"s{seed}_rotate"] = np.float64(rotate)
            for k, name in enumerate(("left", "right")):
                v = results["img_inputs"][k]
                for j, key in ((0, "img"), (4, "post_rot"), (5, "post_tran")):
                    out[f"s{seed}_{name}_{key}"] = np.asarray(v[j])
            print("seed", seed, "resize", round(resize, 4), "dims", dims, "crop", crop, "flip", bool(flip), "rotate", round(rotate, 3))
            if seed == LIDAR_SEED:
                ann = LS.LoadSemKittiAnnotation(bda_aug_conf=dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5,
                                                                  flip_dy_ratio=0.5), is_train=True)
                results = ann(results)
                results["img_inputs"] = [list(v) for v in results["img_inputs"]]
                os.chdir(tmp)
                try:
                    lid = O2D.CreateDepthFromLiDAR(point_cloud_range=[0, -25.6, -2, 51.2, 25.6, 4.4], grid_size=[256, 256, 32],
                                                   label_mapping=os.path.join(MG.REF, "semantickitti.yaml"))
                    lid(results)
                finally:
                    os.chdir(cwd)
                for k, name in enumerate(("left", "right")):
                    d = results["img_inputs"][k][7][0]
                    idx = torch.nonzero(d.reshape(-1)).reshape(-1)
                    out[f"depth_idx_{name}"] = idx.to(torch.int32).numpy()
                    out[f"depth_val_{name}"] = d.reshape(-1)[idx].numpy()
                    print(name, "depth pixels", idx.numel())
                seg = results["img_seg"]
                sidx = torch.nonzero(seg.reshape(-1)).reshape(-1)
                out["seg_idx_right"] = sidx.to(torch.int32).numpy()
                out["seg_val_right"] = seg.reshape(-1)[sidx].numpy()
                out["points_occ"] = results["points_occ"].numpy()
                out["points_uv"] = results["points_uv"].numpy()
                print("seg pixels", sidx.numel(), "points_occ", out["points_occ"].shape)
    flips = {int(out[f"s{s}_flip"]) for s in SEEDS}
    signs = {bool(out[f"s{s}_rotate"] > 0) for s in SEEDS}
    assert flips == {0, 1} and signs == {False, True}, (flips, signs)
    path = os.path.join(ROOT, "tests", "golden", "image_augment.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
