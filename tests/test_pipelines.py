"""Data side: file formats and CreateDepthFromLiDAR.  CPU part: the oracle (oracle/data_ref.py) against
outputs of the reference's own pipeline class (tests/golden/lidar_depth.npz), and the host-side parsers.  GPU part
(-m gpu): the registered pipeline step on the HIP kernel against the same fixture."""
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import data_ref as DR
from oracle.make_golden_data import H, W, cameras, scene
from stereoscene_amd import pipelines as P


def _dense(idx, val):
    d = torch.zeros(H * W)
    d[torch.from_numpy(idx.astype(np.int64))] = torch.from_numpy(val)
    return d.view(H, W)


def test_oracle_matches_reference_pipeline_outputs():
    g = load_golden("lidar_depth")
    pts, raw = scene()
    lm = dict(zip(g["learning_map_keys"].tolist(), g["learning_map_vals"].tolist()))
    assert lm == P.LEARNING_MAP
    seg = torch.tensor([lm[int(v) & 0xFFFF] for v in raw], dtype=torch.float32)
    points = torch.from_numpy(pts[:, :3].copy())
    views = cameras()
    for k, name in enumerate(("left", "right")):
        v = views[k]
        out = DR.create_depth_view(points, seg, v[1], v[2], v[3], v[4], v[5], views[0][6], H, W)
        want = _dense(g[f"depth_idx_{name}"], g[f"depth_val_{name}"])
        # bit-identical on the CPU that generated the fixture; another host's BLAS may round the 3x3 products
        # differently in the last bit, which can move a point across a .5 pixel boundary
        diff = out["depth"] != want
        assert diff.sum().item() <= 6
        assert (out["depth"][~diff] - want[~diff]).abs().max().item() < 1e-5
    assert (out["img_seg"] != _dense(g["seg_idx_right"], g["seg_val_right"])).sum().item() <= 6
    ref_occ, ref_uv = torch.from_numpy(g["points_occ"]), torch.from_numpy(g["points_uv"])
    assert abs(out["points_occ"].shape[0] - ref_occ.shape[0]) <= 2
    if out["points_occ"].shape == ref_occ.shape:
        assert (out["points_occ"] - ref_occ).abs().max().item() < 1e-4 and (out["points_uv"] - ref_uv).abs().max().item() < 1e-4


def test_file_format_parsers(tmp_path):
    calib = tmp_path / "calib.txt"
    rows = {k: np.arange(12, dtype=np.float64) * (i + 1) + 0.5 for i, k in enumerate(("P0", "P1", "P2", "P3", "Tr"))}
    calib.write_text("".join(f"{k}: " + " ".join(repr(float(v)) for v in r) + "\n" for k, r in rows.items()))
    c = P.read_calib(str(calib))
    assert set(c) == {"P2", "P3", "Tr"} and c["P2"].shape == (4, 4)
    assert np.array_equal(c["P3"][:3], rows["P3"].reshape(3, 4)) and np.array_equal(c["Tr"][3], [0, 0, 0, 1])
    pts, raw = scene()
    (tmp_path / "a.bin").write_bytes(pts.tobytes())
    (tmp_path / "a.label").write_bytes(raw.tobytes())
    assert np.array_equal(P.load_velodyne(str(tmp_path / "a.bin")), pts)
    ids = P.load_lidarseg(str(tmp_path / "a.label"))
    assert ids.dtype == np.int32 and ids.min() >= 0 and ids.max() == 19
    assert np.array_equal(ids, np.array([P.LEARNING_MAP[int(v) & 0xFFFF] for v in raw], dtype=np.int32))
    (tmp_path / "bad.label").write_bytes(np.array([7], dtype=np.uint32).tobytes())        # id 7 is not in the map
    with pytest.raises(KeyError):
        P.load_lidarseg(str(tmp_path / "bad.label"))
    vox = (np.arange(256 * 256 * 32) % 21).astype(np.uint8).reshape(256, 256, 32)
    np.save(tmp_path / "000000_1_1.npy", vox)
    assert np.array_equal(P.load_voxel_labels(str(tmp_path / "000000_1_1.npy")), vox)
    np.save(tmp_path / "f.npy", vox.astype(np.float32))
    with pytest.raises(TypeError):
        P.load_voxel_labels(str(tmp_path / "f.npy"))
    assert "CreateDepthFromLiDAR" in P.PIPELINES


@pytest.mark.gpu
def test_create_depth_from_lidar_on_hip_matches_reference(tmp_path):
    g = load_golden("lidar_depth")
    pts, raw = scene()
    vel = tmp_path / "velodyne/00/velodyne"
    lab = tmp_path / "lidarseg/00/labels"
    os.makedirs(vel), os.makedirs(lab)
    pts.tofile(str(vel / "000123.bin"))
    raw.tofile(str(lab / "000123.label"))
    step = P.PIPELINES.build(dict(type="CreateDepthFromLiDAR", point_cloud_range=[0, -25.6, -2, 51.2, 25.6, 4.4],
                                  grid_size=[256, 256, 32], lidar_root=str(tmp_path / "velodyne"),
                                  lidarseg_root=str(tmp_path / "lidarseg")))
    results = dict(img_filename=["x/sequences/00/image_2/000123.png", "x/sequences/00/image_3/000123.png"],
                   img_inputs=[list(v) for v in cameras()])
    step(results)
    for k, name in enumerate(("left", "right")):
        got = results["img_inputs"][k][7][0].cpu()
        want = _dense(g[f"depth_idx_{name}"], g[f"depth_val_{name}"])
        diff = (got != want)
        # the device projection rounds like the CPU one up to the last bit: a handful of points may land on the other
        # side of a .5 pixel boundary / the image border
        assert diff.sum().item() <= 6, (name, diff.sum().item())
        same = ~diff
        assert torch.equal(got[same], want[same])
    seg = results["img_seg"].cpu()
    assert (seg != _dense(g["seg_idx_right"], g["seg_val_right"])).sum().item() <= 6
    occ, uv = results["points_occ"].cpu(), results["points_uv"].cpu()
    ref_occ, ref_uv = torch.from_numpy(g["points_occ"]), torch.from_numpy(g["points_uv"])
    assert abs(occ.shape[0] - ref_occ.shape[0]) <= 2
    if occ.shape == ref_occ.shape:
        assert (occ - ref_occ).abs().max().item() < 1e-4 and (uv - ref_uv).abs().max().item() < 1e-4
    # empty scan: all-zero maps, no launch on zero points
    uvd, valid, depth, s2 = P.lidar_depth_map(torch.zeros(0, 3, device="cuda"), None, *cameras()[0][1:6], H, W)
    assert uvd.shape == (0, 3) and depth.abs().sum().item() == 0 and s2 is None


# ---------------------------------------------------------------------------------------------------------------------
# image loading / annotation loading
# ---------------------------------------------------------------------------------------------------------------------
from oracle.make_golden_data import DATA_CONFIG, stereo_images, stereo_meta  # noqa: E402


def test_pillow_resize_restatements_are_byte_exact():
    """Both restatements of libImaging's fixed-point bicubic resize (the oracle's scalar one and the product's table
    builder, emulated here with integer numpy) against Pillow itself, up- and down-scaling."""
    from PIL import Image
    rng = np.random.default_rng(1)
    for (Hs, Ws, Hd, Wd) in [(37, 124, 39, 128), (60, 200, 30, 77), (50, 80, 50, 96), (64, 64, 100, 64), (47, 155, 48, 160)]:
        img = rng.integers(0, 256, (Hs, Ws, 3), dtype=np.uint8)
        ref = np.asarray(Image.fromarray(img).resize((Wd, Hd)))
        assert np.array_equal(DR.pil_resize_u8(img, (Wd, Hd)), ref)
        cur = img.astype(np.int64)
        for axis, (n_in, n_out) in ((1, (Ws, Wd)), (0, (Hs, Hd))):
            if n_in == n_out:
                continue
            kk, bounds, ksize = P.pil_resample_tables(n_in, n_out)
            src = np.moveaxis(cur, axis, 0)
            out = np.stack([np.clip(((1 << 21) + np.tensordot(kk[o, :bounds[o, 1]].astype(np.int64),
                                                               src[bounds[o, 0]:bounds[o, 0] + bounds[o, 1]], axes=(0, 0))) >> 22,
                                    0, 255) for o in range(n_out)])
            cur = np.moveaxis(out, 0, axis)
        assert np.array_equal(cur.astype(np.uint8), ref)


def test_oracle_image_loading_matches_reference_loader():
    g = load_golden("image_loading")
    imgs, meta = stereo_images(), stereo_meta()
    for mode, is_train in (("test", False), ("train", True)):
        for k, name in enumerate(("left", "right")):
            img, rot, tran, post_rot, post_tran = DR.load_view(imgs[k], meta["lidar2cam"][k], meta["cam_intrinsic"][k], DATA_CONFIG,
                                                               is_train)
            pre = f"load_{mode}_{name}_"
            assert np.abs(img.numpy() - g[pre + "img"][0]).max() < 1e-5
            assert np.abs(rot.numpy() - g[pre + "rot"][0]).max() < 1e-6 and np.abs(tran.numpy() - g[pre + "tran"][0]).max() < 1e-6
            assert np.abs(post_rot.numpy() - g[pre + "post_rot"][0]).max() < 1e-6
            assert np.abs(post_tran.numpy() - g[pre + "post_tran"][0]).max() < 1e-5
            assert np.array_equal(g[pre + "bda"], np.eye(3, dtype=np.float32))          # apply_bda=False: identity in slot 6


def test_image_augmentation_draw_and_pixel_map_match_reference_loader():
    """Host side of the product's image loader (no GPU): the augmentation draw (RNG order, integer truncations) and the 2x3
    pixel map against what the reference's loader produced for the same seed (tests/golden/image_loading.npz)."""
    g = load_golden("image_loading")
    Hs, Ws = stereo_images()[1].shape[:2]
    for mode, is_train in (("test", False), ("train", True)):
        step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=DATA_CONFIG, is_train=is_train,
                                      device="cpu"))
        np.random.seed(0)
        resize, dims, crop, flip, rotate = step.sample_augmentation(H=Hs, W=Ws)
        assert rotate == 0 and dims == (int(Ws * resize), int(Hs * resize))
        assert (crop[2] - crop[0], crop[3] - crop[1]) == tuple(DATA_CONFIG["input_size"][::-1])
        rot2, tran2 = step.pixel_map(torch.eye(2), torch.zeros(2), resize, crop, flip)
        for name in ("left", "right"):                                       # one draw per sample, shared by both views
            assert np.abs(rot2.numpy() - g[f"load_{mode}_{name}_post_rot"][0][:2, :2]).max() < 1e-6
            assert np.abs(tran2.numpy() - g[f"load_{mode}_{name}_post_tran"][0][:2]).max() < 1e-5
        with pytest.raises(ValueError):               # the reference never composes onto a non-zero translation
            step.pixel_map(torch.eye(2), torch.ones(2), resize, crop, flip)
    # flips off in the config: the RNG stream is not consumed for them (the crop after it would move otherwise)
    cfg = dict(DATA_CONFIG, flip=False)
    step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=cfg, is_train=True, device="cpu"))
    np.random.seed(3)
    a = step.sample_augmentation(H=Hs, W=Ws)
    np.random.seed(3)
    u = [np.random.uniform(*cfg["resize"]), np.random.uniform(*cfg["crop_h"])]
    assert a[3] is False and abs(a[0] - (cfg["input_size"][1] / Ws + u[0])) < 1e-12


def test_bev_transform_and_annotation_loader_host_logic():
    from stereoscene_amd import synthetic as S
    g = load_golden("image_loading")
    lab = (S.hash_uniform("bev/lab", (16, 16, 4), 0.0, 20.0).floor()).to(torch.uint8)
    center = torch.tensor([25.6, 0.0, 1.2])
    for tag, (rot, fx, fy) in dict(flipx=(0.0, True, False), flipxy=(0.0, True, True), rot=(30.0, False, True)).items():
        v, m = P.bev_transform(lab.clone(), rot, 1.0, fx, fy, center)
        assert np.array_equal(v.numpy().astype(np.uint8), g[f"bev_{tag}_labels"]) and v.dtype == torch.int64
        assert np.abs(m.numpy() - g[f"bev_{tag}_mat"]).max() < 1e-5
    step = P.PIPELINES.build(dict(type="LoadSemKittiAnnotation", bda_aug_conf=dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05),
                                                                                  flip_dx_ratio=0.5, flip_dy_ratio=0.5)))
    views = [[torch.zeros(1)] * 9, [torch.ones(1)] * 9]
    res = step(dict(gt_occ=np.zeros((4, 4, 2), dtype=np.uint8), img_inputs=views))
    assert len(res["img_inputs"]) == 2 and all(len(v) == 10 for v in res["img_inputs"])
    assert torch.equal(res["img_inputs"][0][6], torch.eye(3)) and res["gt_occ"].shape == (4, 4, 2)
    with pytest.raises(NotImplementedError):
        P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=DATA_CONFIG, colorjitter=True))


@pytest.mark.gpu
def test_image_loader_on_hip_matches_reference(tmp_path):
    from PIL import Image
    g = load_golden("image_loading")
    imgs, meta = stereo_images(), stereo_meta()
    names = []
    for im, cam in zip(imgs, ("image_2", "image_3")):
        d = tmp_path / "sequences" / "00" / cam
        os.makedirs(d)
        Image.fromarray(im).save(str(d / "000123.png"))
        names.append(str(d / "000123.png"))
    # the resize kernels alone: byte-exact with Pillow
    for (Wd, Hd) in [(160, 48), (77, 30), (155, 60), (200, 47)]:
        got = P.resize_u8(torch.from_numpy(imgs[0]).cuda(), (Wd, Hd)).cpu().numpy()
        assert np.array_equal(got, np.asarray(Image.fromarray(imgs[0]).resize((Wd, Hd)))), (Wd, Hd)
    for mode, is_train in (("test", False), ("train", True)):
        step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=DATA_CONFIG, is_train=is_train,
                                      img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)))
        np.random.seed(0)
        res = step(dict(img_filename=names, **meta))
        for k, name in enumerate(("left", "right")):
            v = res["img_inputs"][k]
            assert len(v) == 9
            for j, key in enumerate(("img", "rot", "tran", "intrin", "post_rot", "post_tran", "depth", "cam2lidar", "calib")):
                want = g[f"load_{mode}_{name}_{key}"]
                got = v[j].detach().cpu().numpy()
                assert got.shape == want.shape, (key, got.shape, want.shape)
                assert np.abs(got.astype(np.float64) - want.astype(np.float64)).max() < 1e-5, (mode, name, key)
    # flip path of crop_normalize against numpy
    r = P.resize_u8(torch.from_numpy(imgs[1]).cuda(), (160, 48))
    out = P.crop_normalize(r, (3, -2, 150, 40), True, [1.0, 2.0, 3.0], [2.0, 4.0, 8.0]).cpu().numpy()
    ref = np.zeros((42, 147, 3), dtype=np.float32)
    ref[2:] = r.cpu().numpy()[0:40, 3:150].astype(np.float32)
    ref = ((ref[:, ::-1] - np.array([1.0, 2.0, 3.0], dtype=np.float32)) * np.array([0.5, 0.25, 0.125], dtype=np.float32))
    assert np.abs(out - ref.transpose(2, 0, 1)).max() < 1e-6


def _write_mini_kitti(root, n_frames, img_hw, occ_size):
    """Synthetic SemanticKITTI-shaped tree: images, calib.txt, voxel ids, preprocessed labels, velodyne scans + labels."""
    from PIL import Image
    from stereoscene_amd import synthetic as S
    seq = os.path.join(root, "kitti", "dataset", "sequences", "00")
    for d in ("image_2", "image_3", "voxels"):
        os.makedirs(os.path.join(seq, d))
    os.makedirs(os.path.join(root, "labels", "00"))
    os.makedirs(os.path.join(root, "velodyne", "00", "velodyne"))
    os.makedirs(os.path.join(root, "lidarseg", "00", "labels"))
    Hh, Ww = img_hw
    fx = 707.0912 * Ww / 1241.0
    P2 = [fx, 0, 601.8873 * Ww / 1241.0, 4.5, 0, fx, 183.1104 * Ww / 1241.0, 0.2, 0, 0, 1, 0.003]
    P3 = list(P2)
    P3[3] = P2[3] - 0.54 * fx
    Tr = [0, -1, 0, 0.0, 0, 0, -1, -0.08, 1, 0, 0, -0.27]
    with open(os.path.join(seq, "calib.txt"), "w") as f:
        for k, v in (("P0", P2), ("P1", P2), ("P2", P2), ("P3", P3), ("Tr", Tr)):
            f.write(f"{k}: " + " ".join(repr(float(x)) for x in v) + "\n")
    pts, raw = scene()
    for i in range(n_frames):
        fid = f"{i:06d}"
        for cam in ("image_2", "image_3"):
            im = S.hash_uniform(f"mini/{cam}/{fid}", (Hh, Ww, 3), 0.0, 256.0).floor().clamp(0, 255).to(torch.uint8).numpy()
            Image.fromarray(im).save(os.path.join(seq, cam, fid + ".png"))
        open(os.path.join(seq, "voxels", fid + ".bin"), "wb").close()
        lab = (S.hash_uniform(f"mini/lab/{fid}", tuple(occ_size), 0.0, 20.0).floor()).to(torch.uint8).numpy()
        lab[::7, ::5] = 255
        np.save(os.path.join(root, "labels", "00", fid + "_1_1.npy"), lab)
        pts.tofile(os.path.join(root, "velodyne", "00", "velodyne", fid + ".bin"))
        raw.tofile(os.path.join(root, "lidarseg", "00", "labels", fid + ".label"))
    return fx, P2, P3


def test_dataset_index_and_sample_dict(tmp_path):
    fx, P2, P3 = _write_mini_kitti(str(tmp_path), 2, (62, 155), (32, 32, 8))
    ds = P.DATASETS.build(dict(type="CustomSemanticKITTILssDataset", data_root=str(tmp_path / "kitti"),
                               ann_file=str(tmp_path / "labels"), pipeline=None, split="train", occ_size=(32, 32, 8)))
    assert len(ds) == 2 and ds.data_infos[1]["frame_id"] == "000001"
    d = ds.get_data_info(0)
    assert [os.path.basename(os.path.dirname(p)) for p in d["img_filename"]] == ["image_2", "image_3"]
    assert d["cam_intrinsic"][1][0, 3] == P3[3] and d["lidar2cam"][0].shape == (4, 4) and d["gt_occ"].shape == (32, 32, 8)
    assert np.allclose(d["lidar2img"][0], d["cam_intrinsic"][0] @ d["lidar2cam"][0])
    base = P.dynamic_baseline(P.read_calib_file(ds.data_infos[0]["calib_path"]))
    assert abs(base - 0.54) < 1e-12 and abs(d["calib"] - fx * 0.54) < 1e-9           # P3[0,3]/(-fx) - P2[0,3]/(-fx)
    assert P.DATASETS.build(dict(type="CustomSemanticKITTILssDataset", data_root=str(tmp_path / "kitti"),
                                 ann_file=str(tmp_path / "labels"), pipeline=None, split="val")).__len__() == 0


@pytest.mark.gpu
def test_files_to_losses_end_to_end(tmp_path):
    """Disk -> dataset -> LoadMultiViewImage -> LoadSemKittiAnnotation -> CreateDepthFromLiDAR -> collate -> detector with
    the image branch -> losses -> backward: every data-side and model-side piece of the build in one pass."""
    from stereoscene_amd import model_zoo, plugin, synthetic as S  # noqa: F401  (plugin fills the registries)
    from stereoscene_amd.registry import DETECTORS
    cfg = S.CFG_T
    _write_mini_kitti(str(tmp_path), 2, (62, 155), cfg["occ_size"])
    data_config = {"input_size": cfg["input_size"], "resize": (0.0, 0.0), "rot": (0.0, 0.0), "flip": False, "crop_h": (0.0, 0.0),
                   "resize_test": 0.0}
    pipeline = [
        dict(type="LoadMultiViewImageFromFiles_SemanticKitti", is_train=True, colorjitter=False, data_config=data_config,
             img_norm_cfg=dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)),
        dict(type="LoadSemKittiAnnotation", bda_aug_conf=dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5,
                                                              flip_dy_ratio=0.5), is_train=True),
        dict(type="CreateDepthFromLiDAR", point_cloud_range=list(cfg["pc_range"]), grid_size=list(cfg["occ_size"]),
             lidar_root=str(tmp_path / "velodyne"), lidarseg_root=str(tmp_path / "lidarseg")),
    ]
    ds = P.DATASETS.build(dict(type="CustomSemanticKITTILssDataset", data_root=str(tmp_path / "kitti"),
                               ann_file=str(tmp_path / "labels"), pipeline=pipeline, split="train", occ_size=cfg["occ_size"],
                               pc_range=cfg["pc_range"]))
    batch = P.collate([ds[0], ds[1]])
    left, right = batch["img_inputs"]
    assert left[0].shape == (2, 1, 3) + tuple(cfg["input_size"]) and left[7].shape == (2, 1) + tuple(cfg["input_size"])
    assert left[9].shape == (2,) and (left[7] > 0).sum().item() > 100 and batch["gt_occ"].shape == (2,) + tuple(cfg["occ_size"])
    mc = model_zoo.model_cfg(cfg, image_branch=True)
    model = DETECTORS.build(mc)
    S.fill_state_dict_(model)
    model = model.cuda().train()
    losses = model.forward_train(img_inputs=batch["img_inputs"], gt_occ=batch["gt_occ"])
    total = sum(v for k, v in losses.items() if k.startswith("loss"))
    total.backward()
    assert torch.isfinite(total) and float(losses["loss_depth"].detach()) > 0
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)


@pytest.mark.gpu
def test_training_loop_from_files_with_runner(tmp_path):
    """The whole stack in one loop: files -> dataset -> DistributedGroupSampler -> pipeline steps (GPU resize / z-buffer) ->
    collate -> detector (hot path only, image-neck features synthesised from the loaded images by a fixed projection) ->
    fused AdamW + clip -> EpochBasedRunner hooks (step LR, checkpoint rotation, evaluation with save_best, resume)."""
    from stereoscene_amd import evaluate as E, model_zoo, plugin, runner as R, synthetic as S, train as T  # noqa: F401
    cfg = S.CFG_T
    _write_mini_kitti(str(tmp_path), 4, (62, 155), cfg["occ_size"])
    data_config = {"input_size": cfg["input_size"], "resize": (0.0, 0.0), "rot": (0.0, 0.0), "flip": False, "crop_h": (0.0, 0.0),
                   "resize_test": 0.0}
    pipeline = [
        dict(type="LoadMultiViewImageFromFiles_SemanticKitti", is_train=True, data_config=data_config),
        dict(type="LoadSemKittiAnnotation", bda_aug_conf=dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5,
                                                              flip_dy_ratio=0.5), is_train=True),
        dict(type="CreateDepthFromLiDAR", point_cloud_range=list(cfg["pc_range"]), grid_size=list(cfg["occ_size"]),
             lidar_root=str(tmp_path / "velodyne"), lidarseg_root=str(tmp_path / "lidarseg")),
    ]
    ds = P.DATASETS.build(dict(type="CustomSemanticKITTILssDataset", data_root=str(tmp_path / "kitti"),
                               ann_file=str(tmp_path / "labels"), pipeline=pipeline, split="train", occ_size=cfg["occ_size"],
                               pc_range=cfg["pc_range"]))
    assert len(ds) == 4
    model = model_zoo.build_detector(cfg).train()
    torch.manual_seed(0)
    proj = torch.randn(640, 3 * 8 * 8, device="cuda") * 0.2          # stand-in image branch: 8x8 patch embedding -> 640 ch

    def to_batch(indices):
        b = P.collate([ds[i] for i in indices])
        views = []
        for v in b["img_inputs"]:
            img = v[0][:, 0]                                                         # [B,3,H,W]
            patches = torch.nn.functional.unfold(img, 8, stride=8)                   # [B, 192, fH*fW]
            feat = torch.einsum("ck,bkn->bcn", proj, patches).reshape(img.shape[0], 1, 640, img.shape[2] // 8, img.shape[3] // 8)
            views.append((feat.contiguous(),) + tuple(v[1:]))
        return dict(img_inputs=tuple(views), gt_occ=b["gt_occ"])

    sampler = R.DistributedGroupSampler(ds, samples_per_gpu=2, num_replicas=1, rank=0, seed=0)

    class Loader:
        def __iter__(self):
            idx = list(iter(sampler))
            for i in range(0, len(idx), 2):
                yield to_batch(idx[i:i + 2])

    opt = R.optimizer_from_config(model, dict(optimizer=dict(type="AdamW", lr=2e-3, weight_decay=0.01),
                                              optimizer_config=dict(grad_clip=dict(max_norm=5, norm_type=2))))
    assert isinstance(opt, T.FlatAdamW) and opt.max_grad_norm == 5.0 and opt.wd == 0.01

    def step_fn(batch):
        return {k: float(v.detach()) for k, v in T.train_step(model, opt, batch["img_inputs"], batch["gt_occ"]).items()
                if k.startswith("loss")}

    def eval_fn():
        scores = E.evaluate(model, [to_batch([0, 1])])
        model.train()
        return scores

    def set_lr(lr):
        opt.lr = lr

    def make(max_epochs):
        return R.EpochBasedRunner(step_fn, set_lr, lambda: dict(state_dict=model.state_dict(), optimizer=opt.state_dict()),
                                  lambda ck: (model.load_state_dict(ck["state_dict"]), opt.load_state_dict(ck["optimizer"])),
                                  str(tmp_path / "work"), base_lr=2e-3, lr_step=(3, 5), max_epochs=max_epochs, eval_fn=eval_fn,
                                  eval_interval=2, log=lambda r: None)
    run = make(4)
    hist = run.run(Loader(), sampler)
    tot = [sum(v for k, v in h.items() if k.startswith("loss")) for h in hist]
    print("epoch loss totals:", [round(t, 3) for t in tot])
    assert len(hist) == 4 and all(np.isfinite(tot)) and tot[-1] < tot[0], tot
    assert abs(hist[3]["lr"] - 2e-4) < 1e-12 and "semkitti_combined_IoU" in hist[1]["eval"]
    files = sorted(os.listdir(tmp_path / "work"))
    assert "epoch_4.pth" in files and "epoch_3.pth" in files and "epoch_2.pth" not in files and any(f.startswith("best_") for f in files)
    run2 = make(5)
    meta = run2.resume()
    assert meta["epoch"] == 4 and opt.step_count == 8
    hist2 = run2.run(Loader(), sampler)
    assert [h["epoch"] for h in hist2] == [5] and np.isfinite(sum(v for k, v in hist2[0].items() if k.startswith("loss")))


def test_reference_config_pipelines_build_unchanged():
    """train_pipeline / test_pipeline / data.train of the reference's own config build from the registries as they are
    (host logic: no file is read, no kernel launched)."""
    from conftest import reference_config
    cfg = reference_config()
    train = P.Compose(cfg.train_pipeline)
    test = P.Compose(cfg.test_pipeline)
    assert [type(s).__name__ for s in train.steps] == ["LoadMultiViewImageFromFiles_SemanticKitti", "LoadSemKittiAnnotation",
                                                       "CreateDepthFromLiDAR", "OccDefaultFormatBundle3D", "Collect3D"]
    assert [type(s).__name__ for s in test.steps] == ["LoadMultiViewImageFromFiles_SemanticKitti", "LoadSemKittiAnnotation",
                                                      "OccDefaultFormatBundle3D", "Collect3D"]
    assert train.steps[0].is_train and not test.steps[0].is_train and train.steps[0].data_config["input_size"] == (384, 1280)
    out = train.steps[4](train.steps[3](dict(gt_occ=np.zeros((2, 2, 2), dtype=np.uint8), points_occ=np.zeros((3, 4)), img_inputs=1,
                                             pc_range=[0], sequence="00", other=5)))
    assert set(out) == {"img_metas", "img_inputs", "gt_occ", "points_occ"} and torch.is_tensor(out["gt_occ"])
    assert out["img_metas"] == {"pc_range": [0], "sequence": "00"}
    dcfg = dict(cfg.data.train)
    assert dcfg["type"] == "CustomSemanticKITTILssDataset"
    ds = P.DATASETS.build({**dcfg, "data_root": "/nonexistent", "ann_file": "/nonexistent"})
    assert len(ds) == 0 and [type(s).__name__ for s in ds.pipeline.steps][-1] == "Collect3D"
