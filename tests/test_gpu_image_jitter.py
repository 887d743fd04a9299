"""Colour jitter on the GPU (-m gpu): the fused crop + flip + rotate + jitter + normalise kernel against the numpy statement
of the upstream (tests/test_image_jitter.py) over a grid of steps, modes, permutations and geometries, the registered loader
with colorjitter=True end to end from PNG files against the reference loader (tests/golden/image_jitter.npz) including the RNG
stream it leaves behind, the unchanged paths with the jitter off or in evaluation, and a files -> losses -> backward pass with
the jitter on."""
import itertools

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.make_golden_data import stereo_images, stereo_meta
from stereoscene_amd import pipelines as P
from test_gpu_image_augment import _write_pair
from test_image_jitter import jitter_rgb, normalize, photometric, rotate_gather
from test_image_rotate import AUG_CONFIG, NORM, augment_reference

pytestmark = pytest.mark.gpu

OFF = dict(delta=None, mode=0, alpha=None, saturation=None, hue=None, perm=None)

GEOMETRIES = [
    # raw (H, W), resize dims (W, H), crop (x0, y0, x1, y1), flip, angle
    ((47, 155), (165, 50), (3, 2, 163, 50), True, 3.75),
    ((47, 155), (156, 47), (0, -1, 160, 47), False, -5.178),           # crop above and right of the image: crop fill
    ((62, 155), (150, 60), (-4, 5, 140, 70), True, -22.5),              # crop fill on three sides and rotate fill
    ((47, 155), (160, 48), (0, 0, 160, 48), False, 0.0),                # angle 0: the identity map
]
BIG = ((370, 1220), (1344, 408), (32, 24, 1312, 408), True, -4.9)      # a 384 x 1280 view


def _jitters():
    """Each step alone (on / off), both modes, every permutation, the extremes of the upstream's ranges (hue wrap and the
    uint8 wrap on both sides), and draws of the loader's own sampler."""
    out = [dict(OFF), dict(OFF, mode=1)]                                 # the HSV round trip alone
    out += [dict(OFF, delta=31.9), dict(OFF, delta=-31.9), dict(OFF, alpha=1.5), dict(OFF, mode=1, alpha=0.5),
            dict(OFF, saturation=1.5), dict(OFF, saturation=0.5), dict(OFF, hue=18.0), dict(OFF, hue=-18.0)]
    for k, perm in enumerate(itertools.permutations(range(3))):
        out.append(dict(delta=7.25, mode=k % 2, alpha=1.25, saturation=1.3, hue=-9.5 if k % 2 else 9.5, perm=perm))
    out += [dict(delta=32.0, mode=0, alpha=1.5, saturation=1.5, hue=18.0, perm=(2, 1, 0)),
            dict(delta=-32.0, mode=1, alpha=1.5, saturation=1.5, hue=-18.0, perm=(1, 2, 0)),
            dict(delta=-32.0, mode=0, alpha=0.5, saturation=0.5, hue=17.99, perm=None)]
    step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=AUG_CONFIG, is_train=True,
                                  colorjitter=True))
    state = np.random.get_state()
    np.random.seed(1234)
    out += [step.sample_jitter() for _ in range(12)]
    np.random.set_state(state)
    return out


def _geometry_from_resized(resized, crop, flip, rotate):
    """crop (zero padded) + mirror + Pillow's fixed-point rotate of the GPU-resized bytes, in numpy."""
    x0, y0, x1, y1 = (int(v) for v in crop)
    c = np.zeros((y1 - y0, x1 - x0, 3), dtype=np.uint8)
    ys, xs = slice(max(y0, 0), min(y1, resized.shape[0])), slice(max(x0, 0), min(x1, resized.shape[1]))
    c[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = resized[ys, xs]
    if flip:
        c = c[:, ::-1]
    return rotate_gather(np.ascontiguousarray(c), P.pil_rotate_fixed(c.shape[1], c.shape[0], rotate))


def _run(case, jitters, mean=NORM["mean"], std=NORM["std"], swap_rb=False):
    (H, W), dims, crop, flip, angle = case
    raw = np.random.default_rng(abs(hash(case)) % 2**32).integers(0, 256, (H, W, 3), dtype=np.uint8)
    resized = P.resize_u8(torch.from_numpy(raw).cuda(), dims)
    geo = _geometry_from_resized(resized.cpu().numpy(), crop, flip, angle)
    wraps = set()
    for j in jitters:
        got = P.crop_rotate_jitter_normalize(resized, crop, flip, angle, j, mean, std, swap_rb=swap_rb).cpu().numpy()
        rgb = geo[..., ::-1] if swap_rb else geo                     # swap_rb: the source holds BGR
        want = normalize(jitter_rgb(rgb, j), mean, std)
        assert got.shape == want.shape and np.abs(got - want).max() == 0.0, (case, j, int((got != want).sum()))
        x = photometric(rgb[..., ::-1], j)
        wraps |= ({"below0"} if (x < 0).any() else set()) | ({"above255"} if (x >= 256).any() else set())
    return wraps


@pytest.mark.parametrize("case", GEOMETRIES)
def test_crop_rotate_jitter_normalize_kernel_is_bit_exact_with_the_numpy_statement(case):
    wraps = _run(case, _jitters())
    assert wraps == {"below0", "above255"}
    # a source held in BGR and an unnormalised read
    _run(case, [dict(delta=-12.5, mode=1, alpha=1.4, saturation=1.45, hue=-17.0, perm=(0, 2, 1))], [1.0, 2.0, 3.0],
         [2.0, 4.0, 8.0], swap_rb=True)


def test_crop_rotate_jitter_normalize_kernel_on_a_kitti_sized_view():
    js = _jitters()
    _run(BIG, js[:1] + js[10:19] + js[-3:])                           # round trip, permutations, extremes, draws


def test_jitter_loader_on_hip_matches_reference(tmp_path):
    g = load_golden("image_jitter")
    names, meta = _write_pair(tmp_path), stereo_meta()
    step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=AUG_CONFIG, is_train=True,
                                  colorjitter=True, img_norm_cfg=NORM))
    for seed in g["seeds"].tolist():
        np.random.seed(seed)
        res = step(dict(img_filename=names, **meta))
        assert np.random.uniform() == float(g[f"s{seed}_next"]), seed           # the same number of values consumed
        for k, name in enumerate(("left", "right")):
            v = res["img_inputs"][k]
            img = v[0].cpu().numpy()
            want = g[f"s{seed}_{name}_img"]
            assert np.array_equal(img, want), (seed, name, int((img != want).sum()))


def test_jitter_off_and_evaluation_are_unchanged(tmp_path):
    """colorjitter=False in training: today's pixels (tests/golden/image_augment.npz) and today's RNG stream; evaluation: the
    unjittered pixel path and no value drawn at all, and colorjitter=True stays refused there (the upstream ignores it)."""
    ga = load_golden("image_augment")
    names, meta = _write_pair(tmp_path), stereo_meta()
    Hs, Ws = stereo_images()[1].shape[:2]

    def build(**kw):
        return P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=AUG_CONFIG, img_norm_cfg=NORM,
                                      **kw))
    off = build(is_train=True, colorjitter=False)
    for seed in ga["seeds"].tolist():
        np.random.seed(seed)
        off.sample_augmentation(H=Hs, W=Ws)
        want_next = np.random.uniform()
        np.random.seed(seed)
        res = off(dict(img_filename=names, **meta))
        assert np.random.uniform() == want_next, seed
        for k, name in enumerate(("left", "right")):
            assert np.array_equal(res["img_inputs"][k][0].cpu().numpy(), ga[f"s{seed}_{name}_img"]), (seed, name)
    ev = build(is_train=False, colorjitter=False)
    np.random.seed(5)
    state = np.random.get_state()
    res = ev(dict(img_filename=names, **meta))
    after = np.random.get_state()
    assert np.array_equal(state[1], after[1]) and state[2:] == after[2:]
    resize, dims, crop, flip, rotate = ev.sample_augmentation(H=Hs, W=Ws)
    for k, raw in enumerate(stereo_images()):
        want = augment_reference(raw, dims, crop, flip, rotate, NORM["mean"], NORM["std"])
        assert np.array_equal(res["img_inputs"][k][0][0].cpu().numpy(), want), k
    with pytest.raises(NotImplementedError, match="training only"):
        build(is_train=False, colorjitter=True)


def test_files_to_losses_with_colour_jitter(tmp_path):
    """test_files_to_losses_with_image_view_augmentation with colorjitter=True."""
    from stereoscene_amd import model_zoo, plugin, synthetic as S  # noqa: F401  (plugin fills the registries)
    from stereoscene_amd.registry import DETECTORS
    from test_pipelines import _write_mini_kitti
    cfg = S.CFG_T
    _write_mini_kitti(str(tmp_path), 2, (62, 155), cfg["occ_size"])
    data_config = {"input_size": cfg["input_size"], "resize": (-0.06, 0.11), "rot": (-5.4, 5.4), "flip": True,
                   "crop_h": (0.0, 0.0), "resize_test": 0.0}
    pipeline = [
        dict(type="LoadMultiViewImageFromFiles_SemanticKitti", is_train=True, colorjitter=True, data_config=data_config,
             img_norm_cfg=NORM),
        dict(type="LoadSemKittiAnnotation", bda_aug_conf=dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5,
                                                              flip_dy_ratio=0.5), is_train=True),
        dict(type="CreateDepthFromLiDAR", point_cloud_range=list(cfg["pc_range"]), grid_size=list(cfg["occ_size"]),
             lidar_root=str(tmp_path / "velodyne"), lidarseg_root=str(tmp_path / "lidarseg")),
    ]
    ds = P.DATASETS.build(dict(type="CustomSemanticKITTILssDataset", data_root=str(tmp_path / "kitti"),
                               ann_file=str(tmp_path / "labels"), pipeline=pipeline, split="train", occ_size=cfg["occ_size"],
                               pc_range=cfg["pc_range"]))
    np.random.seed(1)
    batch = P.collate([ds[0], ds[1]])
    left, right = batch["img_inputs"]
    assert left[0].shape == (2, 1, 3) + tuple(cfg["input_size"]) and torch.isfinite(left[0]).all()
    assert not torch.equal(left[0], right[0])
    mc = model_zoo.model_cfg(cfg, image_branch=True)
    model = DETECTORS.build(mc)
    S.fill_state_dict_(model)
    model = model.cuda().train()
    losses = model.forward_train(img_inputs=batch["img_inputs"], gt_occ=batch["gt_occ"])
    total = sum(v for k, v in losses.items() if k.startswith("loss"))
    total.backward()
    assert torch.isfinite(total) and float(losses["loss_depth"].detach()) > 0
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
