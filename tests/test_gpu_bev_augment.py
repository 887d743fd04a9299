"""GPU: the BEV label augmentation kernels (csrc/bev_augment.hip through ``functional.bev_label_transform``) against
tests/golden/bev_augment.npz, byte for byte in both rotate modes (``reference`` = the upstream's in-place rotation as the host
``pipelines.bev_transform`` computes it, ``exact`` = out-of-place scipy), the reference-made case of image_loading.npz, the
loader step on the device against the host step, and one training step behind it.  There is no tolerance anywhere."""
import ctypes as C

import numpy as np
import pytest
import torch

import bev_augment_cases as B
from conftest import load_golden
from stereoscene_amd import capi, functional as F, pipelines as P, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
BDA_CONF = dict(rot_lim=(-22.5, 22.5), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5, flip_dy_ratio=0.5)


def run(case, mode, out_dtype=torch.int64, labels=None):
    lab = torch.from_numpy(case["labels"].copy()).to(DEV) if labels is None else labels
    out = F.bev_label_transform(lab, case["coeffs"], case["flip_dx"], case["flip_dy"], inplace=mode == "reference", out_dtype=out_dtype)
    assert out.is_cuda and out.dtype == out_dtype and tuple(out.shape) == case["shape"] and out.is_contiguous()
    return out.cpu().numpy()


def small_cases():
    return [c for c in B.load_cases() if not c["name"].startswith("big")]


@pytest.mark.parametrize("mode", ["reference", "exact"])
def test_small_cases_match_the_fixture(mode):
    cases = small_cases()
    assert {c["shape"] for c in cases} == set(B.SMALL_SHAPES) and len(cases) >= 60
    for case in cases:
        got = run(case, mode)
        assert np.array_equal(got, case[mode].astype(np.int64)), (case["name"], int((got != case[mode]).sum()))


@pytest.mark.parametrize("name", ["big_0.3", "big_3.75"])
def test_full_grid_matches_the_fixture_in_both_modes(name):
    case = next(c for c in B.load_cases() if c["name"] == name)
    assert case["shape"] == (256, 256, 32)
    lab = torch.from_numpy(case["labels"].copy()).to(DEV)
    for mode in ("reference", "exact"):
        got = run(case, mode, labels=lab)
        assert np.array_equal(got, case[mode].astype(np.int64)), (name, mode, int((got != case[mode]).sum()))
    assert np.array_equal(run(case, "reference", torch.uint8, labels=lab), case["reference"])
    assert not np.array_equal(case["reference"], case["exact"])


def test_byte_output_and_unaligned_grids():
    """The uint8 form on every small case, and grids whose first byte sits at an odd address (the scalar path at any Z)."""
    for case in small_cases():
        for mode in ("reference", "exact"):
            assert np.array_equal(run(case, mode, torch.uint8), case[mode]), (case["name"], mode)
    for case in [c for c in small_cases() if c["shape"] in ((16, 16, 4), (16, 16, 20))]:
        n = case["labels"].size
        buf = torch.zeros(n + 3, dtype=torch.uint8, device=DEV)
        for off in (1, 2):
            lab = buf[off:off + n].view(case["shape"])
            lab.copy_(torch.from_numpy(case["labels"].copy()))
            assert lab.data_ptr() % 4 == off and lab.is_contiguous()
            assert np.array_equal(run(case, "reference", labels=lab), case["reference"].astype(np.int64)), (case["name"], off)
            assert np.array_equal(run(case, "exact", torch.uint8, labels=lab), case["exact"]), (case["name"], off)


def test_reference_made_case_of_the_image_loading_fixture():
    """bev_rot_labels was written by the reference's own bev_transform (16 x 16 x 4, 30 degrees, flip_dy): the default mode
    reproduces the reference itself, not only this project's host copy.  The coefficients are spelled out so that the test needs
    no scipy: cos 30 = sqrt(3) / 2 and sin 30 = 1 / 2 are what cosdg / sindg return, and the offset is scipy's expression."""
    g = load_golden("image_loading")
    lab = (S.hash_uniform("bev/lab", (16, 16, 4), 0.0, 20.0).floor()).to(torch.uint8)
    c, s = 0.8660254037844387, 0.49999999999999994
    m = np.array([[c, s], [-s, c]])
    off = np.array([7.5, 7.5]) - m @ np.array([7.5, 7.5])
    rot30 = next(k for k in B.load_cases() if k["name"] == "flip2_rot")
    assert rot30["coeffs"] == (c, s, -s, c, float(off[0]), float(off[1]))           # ... and they are what scipy composed
    out = F.bev_label_transform(lab.to(DEV), rot30["coeffs"], False, True, inplace=True)
    assert np.array_equal(out.cpu().numpy().astype(np.uint8), g["bev_rot_labels"])
    exact = F.bev_label_transform(lab.to(DEV), rot30["coeffs"], False, True, inplace=False)
    assert not torch.equal(out, exact)
    for tag, (fx, fy) in dict(flipx=(True, False), flipxy=(True, True)).items():
        out = F.bev_label_transform(lab.to(DEV), None, fx, fy)
        assert np.array_equal(out.cpu().numpy().astype(np.uint8), g[f"bev_{tag}_labels"]), tag


def test_runs_repeat_bit_for_bit_in_the_workspace_the_query_names():
    lib = capi.load()
    assert lib.ssbev_version() >= 120
    case = next(c for c in B.load_cases() if c["name"] == "big_0.3")
    X, Y, Z = case["shape"]
    lab = torch.from_numpy(case["labels"].copy()).to(DEV)
    c6 = (C.c_double * 6)(*case["coeffs"])
    nbytes = lib.ssbev_bev_label_workspace(X, Y, 1, 1)
    assert nbytes == 2 * X * Y * 4
    guard = 4096
    outs = []
    for fill in (0x5A, 0xC3):                         # whatever the workspace held before, and nothing written past its end
        ws = torch.full((nbytes + guard,), fill, dtype=torch.uint8, device=DEV)
        out = torch.empty(X, Y, Z, dtype=torch.int64, device=DEV)
        capi.check(lib.ssbev_bev_label_transform(capi.ptr(lab), capi.ptr(out), X, Y, Z, c6, 1, 0, 1, 255, capi.ptr(ws), nbytes,
                                                 capi.stream()), "ssbev_bev_label_transform")
        assert bool((ws[nbytes:] == fill).all())
        outs.append(out)
    assert torch.equal(outs[0], outs[1])
    assert np.array_equal(outs[0].cpu().numpy(), case["reference"].astype(np.int64))
    # refusals, with real device pointers: nothing is launched
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    out = torch.empty(X, Y, Z, dtype=torch.int64, device=DEV)

    def call(src=lab, dst=out, x=X, y=Y, z=Z, c=c6, w=ws, n=nbytes):
        return lib.ssbev_bev_label_transform(capi.ptr(src), capi.ptr(dst), x, y, z, c, 1, 0, 0, 255, capi.ptr(w), n, capi.stream())
    assert call(src=None) == capi.EINVAL and call(dst=None) == capi.EINVAL and call(w=None) == capi.EINVAL
    assert call(x=0) == capi.EINVAL and call(y=-1) == capi.EINVAL and call(z=0) == capi.EINVAL
    assert call(x=65536, y=32768) == capi.EINVAL
    for bad in (float("nan"), float("inf")):
        assert call(c=(C.c_double * 6)(1, 0, bad, 1, 0, 0)) == capi.EINVAL
    assert call(n=nbytes - 1) == capi.EWORKSPACE
    assert lib.ssbev_bev_label_transform_u8(capi.ptr(lab), capi.ptr(lab), X, Y, Z, c6, 1, 0, 0, 255, capi.ptr(ws), nbytes,
                                            capi.stream()) == capi.EINVAL
    with pytest.raises(capi.SsbevError):
        F.bev_label_transform(lab.long(), None, False, False)
    torch.cuda.synchronize()                          # the stream is alive after the refusals


def annotation_step(seed, gt, device, **kw):
    step = P.PIPELINES.build(dict(type="LoadSemKittiAnnotation", bda_aug_conf=BDA_CONF, is_train=True, apply_bda=True, device=device, **kw))
    views = [[torch.zeros(1)] * 9, [torch.ones(1)] * 9]
    np.random.seed(seed)
    res = step(dict(gt_occ=gt.copy(), img_inputs=views))
    tail = np.random.uniform()                         # the draws and their order: the generator is left in the same state
    return res, tail


def test_annotation_loader_on_the_device_equals_the_host_step(monkeypatch):
    pytest.importorskip("scipy")
    gt = np.random.RandomState(3).randint(0, 20, size=(32, 32, 8)).astype(np.uint8)
    gt[np.random.RandomState(4).rand(32, 32, 8) < 0.1] = 255
    seen = set()
    for seed in range(6):
        for kw in (dict(), dict(bda_rotate="exact")):
            host, tail_h = annotation_step(seed, gt, None, **kw)
            dev, tail_d = annotation_step(seed, gt, DEV, **kw)
            monkeypatch.setattr(F, "SSBEV_BDA", False)
            off, tail_o = annotation_step(seed, gt, DEV, **kw)
            monkeypatch.setattr(F, "SSBEV_BDA", True)
            assert tail_h == tail_d == tail_o
            assert not host["gt_occ"].is_cuda and host["gt_occ"].dtype == torch.int64
            for res in (dev, off):
                assert res["gt_occ"].is_cuda and res["gt_occ"].dtype == torch.int64
                assert torch.equal(res["gt_occ"].cpu(), host["gt_occ"])
                for k in range(2):
                    m = res["img_inputs"][k][6]
                    assert not m.is_cuda and tuple(m.shape) == (4, 4) and torch.equal(m, host["img_inputs"][k][6])
                    assert len(res["img_inputs"][k]) == 10
            seen.add((float(host["img_inputs"][0][6][0, 0]) < 0, float(host["img_inputs"][0][6][1, 1]) < 0))
    assert len(seen) >= 3                              # the seeds draw different flip combinations
    ref, _ = annotation_step(0, gt, DEV)
    ex, _ = annotation_step(0, gt, DEV, bda_rotate="exact")
    assert not torch.equal(ref["gt_occ"], ex["gt_occ"])
    # eval and apply_bda=False never touch the device path
    for kw, n in ((dict(is_train=False, apply_bda=True), 4), (dict(apply_bda=False), 3)):
        step = P.PIPELINES.build(dict(type="LoadSemKittiAnnotation", bda_aug_conf=BDA_CONF, device=DEV, **kw))
        res = step(dict(gt_occ=gt.copy(), img_inputs=[[torch.zeros(1)] * 9, [torch.ones(1)] * 9]))
        assert not res["gt_occ"].is_cuda and torch.equal(res["img_inputs"][0][6], torch.eye(n))
        assert np.array_equal(res["gt_occ"].numpy(), gt)


def test_training_step_behind_the_augmented_labels():
    pytest.importorskip("scipy")
    from stereoscene_amd import model_zoo, plugin  # noqa: F401
    from stereoscene_amd.plugin import losses as L
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1, tag="bda_step")
    gt = smp["gt_occ"][0].numpy().astype(np.uint8)
    view = [t[0] for t in S.frustum_view(cfg)[:6]] + [torch.zeros(1)] * 3        # one sample of one view, before the BEV slot
    loader_kw = dict(type="LoadSemKittiAnnotation", bda_aug_conf=BDA_CONF, is_train=True, apply_bda=True,
                     point_cloud_range=cfg["pc_range"])
    rel_kw = dict(type="CreateRelationLabels", point_cloud_range=cfg["pc_range"], grid_size=list(cfg["occ_size"]),
                  class_names=L.KITTI_CLASS_NAMES)
    out = {}
    for tag, dev_load, dev_rel in (("device", DEV, None), ("host", None, DEV)):
        np.random.seed(1)
        res = P.PIPELINES.build(dict(loader_kw, device=dev_load))(dict(gt_occ=gt.copy(), img_inputs=[list(view), list(view)]))
        assert res["gt_occ"].is_cuda == (tag == "device")
        out[tag] = P.PIPELINES.build(dict(rel_kw, device=dev_rel))(res)
        assert out[tag]["frustums_ids"].is_cuda                                   # device=None: where gt_occ lives
    dev, host = out["device"], out["host"]
    assert torch.equal(dev["frustums_ids"], host["frustums_ids"]) and torch.equal(dev["frustums_class_dists"], host["frustums_class_dists"])
    assert torch.equal(dev["gt_occ"].cpu(), host["gt_occ"]) and int((dev["frustums_ids"] != 255).sum()) > 1000
    bda = dev["img_inputs"][0][6]
    assert tuple(bda.shape) == (4, 4) and not torch.equal(bda, torch.eye(4))
    batch = P.collate([dev], device=DEV)                                          # device tensors pass through
    assert batch["gt_occ"].is_cuda and tuple(batch["gt_occ"].shape) == (1, 32, 32, 8) and batch["gt_occ"].dtype == torch.int64
    assert torch.equal(batch["gt_occ"][0], dev["gt_occ"]) and torch.equal(batch["frustums_ids"][0], dev["frustums_ids"])
    # the tiny model keeps its own 3x3 BEV slot: a 4x4 matrix widens the SE input to 33 channels, which its GroupNorm(2) cannot take
    model = model_zoo.build_detector(cfg, frustum_dist=1.0).eval()
    losses = model.forward_train(img_inputs=model_zoo.img_inputs_from_sample(smp), gt_occ=batch["gt_occ"],
                                 frustums_ids=batch["frustums_ids"], frustums_class_dists=batch["frustums_class_dists"])
    total = sum(v for k, v in losses.items() if k.startswith("loss"))
    total.backward()
    assert "loss_voxel_fp_0" in losses and all(torch.isfinite(v).all() for v in losses.values())
    g = model.pts_bbox_head.occ_convs[0][0].weight.grad
    assert g is not None and torch.isfinite(g).all() and float(g.abs().max()) > 0
