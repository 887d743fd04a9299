"""CPU: the image-view segmentation loss (``imgseg=True``) in its tensor form (functional.imgseg_loss_tensor) against the
reference's own fp32 results and the float64 restatement recorded by tools/make_golden_imgseg.py (tests/golden/imgseg.npz), the
host version of the nearest index rule against ``F.interpolate``, the wiring into ``ViewTransformerLiftSplatShootVoxel``,
``collate`` and ``model_zoo``, and the host-side checks of the three C entry points.

Bounds, from the fixture as in tests/test_depth_kld.py: K x the case's recorded reference-fp32-vs-float64 spread, K = 8, floored
at the fp32 unit roundoff 2^-23 (a spread recorded below it measures luck: the results under test are fp32 numbers).  Loss:
K * max(X_loss_spread, eps) * max(1, |loss|); gradient: K * max(X_spread, eps) * max|float64 gradient| on EVERY element.  A, B, D, E
are held to the reference's fp32 values; C (nothing labelled, the reference gives NaN) to exact zeros."""
import ctypes as C
import functools
import os
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import ROOT
from stereoscene_amd import capi, functional as F, synthetic as S

GOLDEN = os.path.join(ROOT, "tests", "golden", "imgseg.npz")
K = 8.0
EPS = 2.0 ** -23
CHECKED = ("A", "B", "D", "E")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """(seg_logits, seg_labels) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.imgseg_case(name)


@functools.lru_cache(maxsize=None)
def class_weights():
    from stereoscene_amd.plugin.losses import semkitti_class_weights
    return semkitti_class_weights()


def want(name):
    return float(golden()[f"{name}_ref_loss"]), golden()[f"{name}_ref_grad"].astype(np.float64)


def loss_tol(name):
    return K * max(float(golden()[f"{name}_loss_spread"]), EPS) * max(1.0, abs(float(golden()[f"{name}_f64_loss"])))


def grad_tol(name):
    return K * max(float(golden()[f"{name}_spread"]), EPS) * float(np.abs(golden()[f"{name}_f64_grad"]).max())


@functools.lru_cache(maxsize=None)
def empty_cells(name):
    """Boolean [BN, h, w]: cells without a valid pixel."""
    logits, labels = case(name)
    BN, Kc, h, w = logits.shape
    H, W = labels.shape[1:]
    iy, ix = F.imgseg_nearest_index(h, H), F.imgseg_nearest_index(w, W)
    valid = (labels >= 1) & (labels < Kc)
    flat = (torch.arange(BN)[:, None, None] * h + iy[None, :, None]) * w + ix[None, None, :]
    counts = torch.bincount(flat[valid], minlength=BN * h * w)
    return (counts == 0).reshape(BN, h, w)


def check(name, loss, grad, what):
    wl, wg = want(name)
    got = float(loss)
    err = float(np.abs(grad.double().numpy() - wg).max())
    print(name, what, "loss", got, "want", wl, "bound", loss_tol(name), "| max gradient error", err, "bound", grad_tol(name))
    assert abs(got - wl) <= loss_tol(name)
    assert abs(got - float(golden()[f"{name}_f64_loss"])) <= loss_tol(name)
    assert torch.isfinite(grad).all() and err <= grad_tol(name)
    empty = empty_cells(name).unsqueeze(1).expand_as(grad)
    assert torch.equal(grad[empty], torch.zeros_like(grad[empty]))         # exactly 0 where no pixel is labelled


SIZES = sorted({(h, H) for _, (h, w), (H, W), _ in S.IMGSEG_CASES.values()} | {(w, W) for _, (h, w), (H, W), _ in S.IMGSEG_CASES.values()}
               | {(24, 384), (80, 1280), (7, 101), (5, 37), (1, 9), (7, 7), (24, 24)})


@pytest.mark.parametrize("n_in,n_out", SIZES)
def test_nearest_index_is_the_map_interpolate_applies(n_in, n_out):
    src = torch.arange(n_in, dtype=torch.float32)
    by_rows = TF.interpolate(src.view(1, 1, n_in, 1), size=(n_out, 1), mode="nearest").flatten().long()
    by_cols = TF.interpolate(src.view(1, 1, 1, n_in), size=(1, n_out), mode="nearest").flatten().long()
    idx = F.imgseg_nearest_index(n_in, n_out)
    assert idx.dtype == torch.int64 and torch.equal(idx, by_rows) and torch.equal(idx, by_cols)
    assert int(idx[0]) == 0 and int(idx.max()) <= n_in - 1 and bool((idx[1:] >= idx[:-1]).all())


def test_fixture_has_something_to_check():
    g = golden()
    for name in S.IMGSEG_CASES:
        logits, labels = case(name)
        assert int(g[f"{name}_logits_crc"]) == zlib.crc32(logits.numpy().tobytes()), name
        assert int(g[f"{name}_labels_crc"]) == zlib.crc32(labels.numpy().tobytes()), name
    for name in CHECKED:
        assert 0 < int(g[f"{name}_n_valid"]) and float(g[f"{name}_f64_loss"]) > 0 and np.abs(g[f"{name}_f64_grad"]).max() > 0
        assert float(g[f"{name}_spread"]) < 1e-6 and float(g[f"{name}_loss_spread"]) < 1e-6, name
    assert int(g["C_n_valid"]) == 0 and not case("C")[1].any()
    assert case("A")[0].shape == (2, 20, 3, 5) and case("A")[1].shape == (2, 48, 80)
    assert case("B")[0].shape == (2, 20, 5, 7) and case("B")[1].shape == (2, 37, 101)
    assert case("D")[0].shape == (1, 20, 2, 3) and case("E")[0].shape == (1, 20, 24, 80) and case("E")[1].shape == (1, 384, 1280)
    assert int(g["B_n_valid"]) == int((case("B")[1] > 0).sum()) and set(case("B")[1].unique().tolist()) == set(range(20))
    assert empty_cells("A").sum() == 1 and bool(empty_cells("A")[1, 2, 4])
    assert empty_cells("D")[0].tolist() == [[False, True, False], [False, False, False]]
    assert int(((case("D")[1][0, :16, :16] >= 1)).sum()) == 1 and float(case("D")[0].abs().max()) > 70
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", CHECKED)
def test_tensor_form_matches_the_fixture(name):
    logits, labels = case(name)
    x = logits.clone().requires_grad_(True)
    loss = F.imgseg_loss_tensor(x, labels, class_weights(), 1.0)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    check(name, loss.detach(), x.grad, "tensor form")


def test_no_valid_pixel_gives_zero_and_a_zero_gradient():
    logits, labels = case("C")
    x = logits.clone().requires_grad_(True)
    loss = F.imgseg_loss(x, labels, class_weights())
    assert loss.dim() == 0 and torch.isfinite(loss) and float(loss.detach()) == 0.0
    loss.backward()
    assert torch.equal(x.grad, torch.zeros_like(x))


def _loss_and_grad(logits, labels, weight=1.0):
    x = logits.clone().requires_grad_(True)
    loss = F.imgseg_loss(x, labels, class_weights(), weight)
    loss.backward()
    return loss.detach(), x.grad


def test_float_and_int64_labels_give_the_same_bits():
    logits, labels = case("B")
    lf, gf = _loss_and_grad(logits, labels)
    li, gi = _loss_and_grad(logits, labels.long())
    assert torch.equal(lf, li) and torch.equal(gf, gi)


def test_labels_outside_the_classes_are_ignored():
    logits, labels = case("A")
    l0, g0 = _loss_and_grad(logits, labels)
    bad = labels.clone()
    unl = (labels == 0)
    bad[unl & (S.hash_uniform("imgseg_bad", labels.shape, 0.0, 1.0) < 0.1)] = 20.0
    bad[0, 0, 0], bad[0, 0, 1], bad[1, 3, 3] = 255.0, -3.0, float("nan")
    assert unl[0, 0, 0] and unl[0, 0, 1] and unl[1, 3, 3] and int((bad == 20.0).sum()) > 100
    l1, g1 = _loss_and_grad(logits, bad)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    l2, g2 = _loss_and_grad(logits, torch.where(torch.isnan(bad), torch.zeros_like(bad), bad).long())
    assert torch.equal(l0, l2) and torch.equal(g0, g2)


def test_float64_and_bad_arguments():
    logits, labels = case("B")
    l64 = F.imgseg_loss(logits.double(), labels, class_weights(), 1.0)
    assert l64.dtype == torch.float64 and abs(float(l64) - float(golden()["B_f64_loss"])) <= 1e-12
    assert torch.equal(F.imgseg_loss(logits, labels, class_weights(), 0.5), F.imgseg_loss_tensor(logits, labels, class_weights(), 0.5))
    with pytest.raises(ValueError):
        F.imgseg_loss(logits, labels[:1], class_weights())
    with pytest.raises(ValueError):
        F.imgseg_loss(logits, labels, class_weights()[:19])
    with pytest.raises(ValueError):
        F.imgseg_nearest_index(0, 4)


def vt_kwargs(**kw):
    grid = S.grid_config(S.CFG_T)
    return dict(loss_depth_weight=1.0, grid_config=grid, data_config=dict(input_size=tuple(S.CFG_T["input_size"])), numC_input=32,
                numC_Trans=16, downsample=8, cam_channels=30, **kw)


def test_view_transformer_builds_the_head_with_the_reference_names():
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT
    plain = VT(**vt_kwargs())
    keys = list(plain.state_dict())
    assert plain.imgseg is False and not hasattr(plain, "img_seg_head") and not any("img_seg" in k for k in keys)
    assert keys == list(VT(imgseg=False, imgseg_class=19, loss_seg_weight=3.0, lift_with_imgseg=True, **vt_kwargs()).state_dict())
    vt = VT(imgseg=True, loss_seg_weight=0.5, **vt_kwargs())
    assert vt.imgseg is True and vt.imgseg_class == 20 and vt.loss_seg_weight == 0.5 and vt.lift_with_imgseg is False
    sd = vt.state_dict()
    head = [k for k in sd if k.startswith("img_seg_head.")]
    assert [k for k in sd if not k.startswith("img_seg_head.")] == keys            # nothing else moved
    blocks = [f"img_seg_head.{i}.{n}" for i in (0, 1) for n in
              ("conv1.weight", "bn1.weight", "bn1.bias", "bn1.running_mean", "bn1.running_var", "bn1.num_batches_tracked",
               "conv2.weight", "bn2.weight", "bn2.bias", "bn2.running_mean", "bn2.running_var", "bn2.num_batches_tracked")]
    assert sorted(head) == sorted(blocks + ["img_seg_head.2.weight", "img_seg_head.2.bias"])
    assert sd["img_seg_head.0.conv1.weight"].shape == (32, 32, 3, 3) and sd["img_seg_head.2.weight"].shape == (20, 32, 1, 1)
    assert sd["img_seg_head.2.bias"].shape == (20,)
    with pytest.raises(ValueError):
        VT(imgseg=True, imgseg_class=19, **vt_kwargs())
    for other in (dict(point_xyz_channel=3), dict(use_voxel_net=True), dict(vp_megvii=True)):
        with pytest.raises(NotImplementedError):
            VT(imgseg=True, **other, **vt_kwargs())


def test_get_seg_loss_weights_the_loss_of_the_stored_logits():
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT
    logits, labels = case("B")
    vt = VT(imgseg=True, loss_seg_weight=0.5, **vt_kwargs())
    with pytest.raises(RuntimeError):
        vt.get_seg_loss(labels)                                   # no forward pass yet
    vt.forward_dic["imgseg_logits"] = logits
    got = float(vt.get_seg_loss(labels))
    assert abs(got - 0.5 * want("B")[0]) <= 0.5 * loss_tol("B")
    assert float(vt.get_seg_loss(labels.long())) == got
    assert float(vt.get_seg_loss(labels.view(2, 1, 37, 101)[:, 0])) == got
    with pytest.raises(RuntimeError):
        VT(**vt_kwargs()).get_seg_loss(labels)


def test_model_cfg_and_detector_options():
    from stereoscene_amd import model_zoo, plugin  # noqa: F401
    from stereoscene_amd.plugin.detector import BEVDepthOccupancy
    base = model_zoo.model_cfg(S.CFG_T)
    assert "imgseg" not in base["img_view_transformer"] and "imgseg_labels" not in base
    assert base["img_bev_encoder_backbone"]["n_input_channels"] == 128
    mc = model_zoo.model_cfg(S.CFG_T, imgseg=True, loss_seg_weight=2.0, imgseg_labels="img_seg_left")
    vt = mc["img_view_transformer"]
    assert vt["imgseg"] is True and vt["imgseg_class"] == 20 and vt["loss_seg_weight"] == 2.0 and vt["lift_with_imgseg"] is False
    assert mc["imgseg_labels"] == "img_seg_left" and mc["img_bev_encoder_backbone"]["n_input_channels"] == 128
    assert model_zoo.model_cfg(S.CFG_T, imgseg=True)["imgseg_labels"] == "img_seg"
    lifted = model_zoo.model_cfg(S.CFG_T, numC_Trans=64, imgseg=True, lift_with_imgseg=True)
    assert lifted["img_view_transformer"]["lift_with_imgseg"] is True and lifted["img_view_transformer"]["numC_Trans"] == 64
    assert lifted["img_bev_encoder_backbone"]["n_input_channels"] == 84
    assert BEVDepthOccupancy.IMGSEG_LABELS == ("img_seg", "img_seg_left")
    with pytest.raises(ValueError):
        model_zoo.build_detector(S.CFG_T, device="cpu", fill=False, imgseg=True, imgseg_labels="img_seg_right")


def test_collate_stacks_the_label_maps():
    from stereoscene_amd import pipelines as P
    smp = S.synthetic_sample(S.CFG_T, B=2)
    assert smp["img_seg"].shape == (2,) + tuple(S.CFG_T["input_size"]) and smp["img_seg"].dtype == torch.float32
    assert 0 < int((smp["img_seg"] > 0).sum()) and set(smp["img_seg"].unique().tolist()) <= set(range(20))
    assert torch.equal(smp["img_seg"] > 0, smp["gt_depths"][:, 0] > 0)

    def sample(b, with_left=True):
        view = [torch.zeros(1, 3, 4, 4), torch.eye(3)[None], torch.zeros(1, 3), torch.eye(4)[None], torch.eye(3)[None], torch.zeros(1, 3),
                torch.eye(3), torch.zeros(1, 4, 4), torch.zeros(1, 4, 4), torch.tensor(0.5)]
        out = dict(img_inputs=[view, view], gt_occ=torch.zeros(2, 2, 2), img_seg=smp["img_seg"][b].numpy())
        if with_left:
            out["img_seg_left"] = smp["img_seg"][b].long()
        return out

    batch = P.collate([sample(0), sample(1)], device="cpu")
    for k in ("img_seg", "img_seg_left"):
        assert batch[k].dtype == torch.float32 and torch.equal(batch[k], smp["img_seg"])
    batch = P.collate([sample(0), sample(1, with_left=False)], device="cpu")
    assert "img_seg" in batch and "img_seg_left" not in batch
    view = sample(0)["img_inputs"][0]
    assert "img_seg" not in P.collate([dict(img_inputs=[view, view], gt_occ=torch.zeros(2, 2, 2))], device="cpu")


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 115
    for n in ("ssbev_imgseg_ce_workspace", "ssbev_imgseg_ce_fwd", "ssbev_imgseg_ce_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    BN, Kc, h, w, H, W = 2, 20, 24, 80, 384, 1280
    cells = BN * h * w
    ws = lib.ssbev_imgseg_ce_workspace(BN, h, w)
    assert cells * (16 + 4 * 20) <= ws <= cells * (16 + 4 * 32) + 64     # (num, den) partials and the class counts per cell
    for bad in ((0, h, w), (BN, -1, w), (BN, h, 0), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.ssbev_imgseg_ce_workspace(*bad) == 0

    def fwd(p=(fake, fake, fake), dims=(BN, Kc, h, w, H, W), out=fake, w_=fake, nbytes=ws):
        return lib.ssbev_imgseg_ce_fwd(*p, *dims, 1.0, out, w_, nbytes, None)

    def bwd(p=(fake, fake, fake, fake), dims=(BN, Kc, h, w, H, W), out=fake, w_=fake, nbytes=None):
        return lib.ssbev_imgseg_ce_bwd(*p, *dims, 1.0, out, w_, None)

    for call, n in ((fwd, 3), (bwd, 4)):
        for i in range(n):
            assert call(p=tuple(None if j == i else fake for j in range(n))) == capi.EINVAL
        assert call(out=None) == capi.EINVAL
        assert call(w_=None) == capi.EINVAL
        for dims in ((0, Kc, h, w, H, W), (BN, 1, h, w, H, W), (BN, 33, h, w, H, W), (BN, Kc, 0, w, H, W), (BN, Kc, h, -2, H, W),
                     (BN, Kc, h, w, 0, W), (BN, Kc, h, w, H, 0), (BN, Kc, H + 1, w, H, W), (BN, Kc, h, W + 1, H, W),
                     (1 << 15, Kc, 1 << 8, 1 << 8, 1 << 8, 1 << 8)):
            assert call(dims=dims) == capi.EINVAL, dims
    assert fwd(nbytes=ws - 1) == capi.EINVAL and fwd(nbytes=0) == capi.EINVAL
