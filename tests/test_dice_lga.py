"""CPU: the soft-Dice and the LGA-weighted voxel losses in their tensor forms (plugin/losses.py) against the reference's own results
recorded by tools/make_golden_dice_lga.py (tests/golden/dice_lga.npz), their wiring into ``occ_losses``, ``OccHead`` and
``model_zoo.model_cfg``, and the host-side checks of the new C entry points.

Bounds, from the fixture as in tests/test_ohem.py: K x the case's recorded fp32-vs-float64 spread, K = 8.  Loss:
K * max(X_loss_spread, eps) * max(1, |loss|) with eps = 2^-23, the fp32 unit roundoff.  Gradient: K * X_spread * max|float64
gradient| on EVERY element, no floor.  The LGA weights are integers (twice the reference's ``get_lga``) and are held bit-equal."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from stereoscene_amd import capi, synthetic as S
from stereoscene_amd.plugin import losses as L

GOLDEN = os.path.join(ROOT, "tests", "golden", "dice_lga.npz")
DELTA_SCALE = 16384.0              # tools/make_golden_dice_lga.py
K = 8.0
EPS = 2.0 ** -23
CASES = tuple(S.DICE_LGA_CASES)
WITH_GRAD = tuple(n for n in CASES if n != "E")
KINDS = ("dice", "lga")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, labels) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.dice_lga_case(name)


@functools.lru_cache(maxsize=None)
def class_weights():
    return L.semkitti_class_weights()


def ref_grad(name, kind):
    """The reference's fp32 gradient: stored as the float64 gradient plus an fp16 difference (see the generator)."""
    g = golden()[f"{name}_{kind}_f64_grad"].astype(np.float64)
    return (g + golden()[f"{name}_{kind}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def loss_tol(name, kind):
    g = golden()
    return K * max(float(g[f"{name}_{kind}_loss_spread"]), EPS) * max(1.0, abs(float(g[f"{name}_{kind}_f64_loss"])))


def grad_tol(name, kind):
    g = golden()
    return K * float(g[f"{name}_{kind}_spread"]) * float(np.abs(g[f"{name}_{kind}_f64_grad"]).max())


def upsampled(x, lab, device="cpu"):
    if tuple(x.shape[-3:]) == tuple(lab.shape[-3:]):
        return x
    if device != "cpu":
        from stereoscene_amd import functional as F
        return F.upsample_trilinear(x, lab.shape[-3:])
    return torch.nn.functional.interpolate(x, size=tuple(lab.shape[-3:]), mode="trilinear", align_corners=False)


def tensor_form(name, kind, device="cpu"):
    """(loss, logit gradient) of the tensor form on ``device``: ``dice_tensor`` of the up-sampled logits, or the dispatcher
    ``occ_lga_loss`` (which reaches ``pal_tensor`` on the CPU and with ``functional.LGA`` off)."""
    x, lab = case(name)
    x = x.clone().to(device).requires_grad_(True)
    lab = lab.to(device)
    if kind == "dice":
        loss = L.dice_tensor(upsampled(x, lab, device), lab)
    else:
        loss = L.occ_lga_loss(x, lab, class_weights().to(device))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.detach().cpu(), x.grad.detach().cpu()


def check(name, kind, loss, grad, what):
    want = float(golden()[f"{name}_{kind}_f64_loss"])
    err = float(np.abs(grad.numpy() - golden()[f"{name}_{kind}_f64_grad"]).max())
    print(name, kind, what, "loss", float(loss), "float64", want, "err", abs(float(loss) - want), "bound", loss_tol(name, kind),
          "| max gradient error", err, "bound", grad_tol(name, kind))
    assert abs(float(loss) - want) <= loss_tol(name, kind)
    assert torch.isfinite(grad).all() and err <= grad_tol(name, kind)


def test_fixture_conditions():
    g = golden()
    for name in WITH_GRAD:
        for kind in KINDS:
            assert 0.0 < float(g[f"{name}_{kind}_spread"]) <= 2e-6 and float(g[f"{name}_{kind}_loss_spread"]) <= 1e-6, (name, kind)
    _, k = case("K")
    assert (k[0, :2] == 255).all() and not (k[0, 2:] == 255).any() and not (k[1] == 255).any()
    assert not torch.equal(k[0, -1], k[1, 0])                                 # a read across the sample boundary shows
    # blocky, but with blocks of two every voxel has a neighbour in the next block: 9 % of the voxels have lga = 0, not most
    assert 0.05 < float((torch.from_numpy(g["K_lga2"]) == 0).float().mean()) < 0.5
    assert sorted(set(k.flatten().tolist())) == [0, 9, 15, 255]
    assert g["L_lga2"].shape == (1, 2, 2, 2) and g["L_lga2"].max() > 0
    _, e = case("E")
    assert (e == 255).all() and not g["E_lga2"].any()
    _, n = case("N")
    assert not (n == 0).any() and (n == 9).any()
    assert not case("Z")[0].any()
    assert case("C")[0].shape[-3:] == case("C")[1].shape[-3:]                 # the tensor-form route
    assert int(g["B_lga2"].max()) >= 8 and g["A_lga2"].dtype == np.uint8
    assert os.path.getsize(GOLDEN) < 1000000


@pytest.mark.parametrize("name", CASES)
def test_lga_weights_tensor_is_bit_equal_to_the_reference(name):
    _, lab = case(name)
    got = L.lga_weights_tensor(lab)
    assert got.dtype == torch.uint8 and torch.equal(got, torch.from_numpy(golden()[f"{name}_lga2"]))
    from stereoscene_amd import functional as F
    assert torch.equal(F.lga_weights(lab), got)                               # CPU labels: the same tensor ops


@pytest.mark.parametrize("shape", ((1, 1, 4, 4), (2, 4, 1, 4), (1, 4, 4, 1), (4, 4, 4)))
def test_lga_weights_refuse_an_axis_shorter_than_two(shape):
    from stereoscene_amd import functional as F
    lab = torch.zeros(shape, dtype=torch.uint8)
    with pytest.raises(ValueError):
        L.lga_weights_tensor(lab)
    with pytest.raises(ValueError):
        F.lga_weights(lab)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", WITH_GRAD)
def test_tensor_form_matches_float64_and_the_reference_fp32(name, kind):
    loss, grad = tensor_form(name, kind)
    check(name, kind, loss, grad, "tensor form")
    assert abs(float(loss) - float(golden()[f"{name}_{kind}_ref_loss"])) <= loss_tol(name, kind)
    if f"{name}_{kind}_ref_delta" in golden():
        assert float(np.abs(grad.numpy() - ref_grad(name, kind)).max()) <= grad_tol(name, kind)


def sums_by_tensor_ops(x, lab):
    """(diff [41], aux [2 + 20 + 400]) in the layout of ``functional.occ_loss_sums`` from float64 tensor ops (conf left zero)."""
    up = upsampled(x.double(), lab)
    p = torch.softmax(up, dim=1).permute(0, 2, 3, 4, 1)[lab != 255]
    t = lab[lab != 255].long()
    onehot = torch.nn.functional.one_hot(t, 20).double()
    cw = class_weights().double()
    ce_num = (cw[t] * -torch.log((p * onehot).sum(1))).sum().reshape(1)
    diff = torch.cat((ce_num, p.sum(0), (p * onehot).sum(0)))
    aux = torch.cat((cw[t].sum().reshape(1), torch.tensor([float(t.numel())], dtype=torch.float64), onehot.sum(0),
                     torch.zeros(400, dtype=torch.float64)))
    return diff, aux


@pytest.mark.parametrize("name", WITH_GRAD)
def test_dice_from_sums_equals_dice_tensor(name):
    x, lab = case(name)
    x = x.clone().requires_grad_(True)
    diff, aux = sums_by_tensor_ops(x, lab)
    loss = L.dice_from_sums(diff, aux).float()
    loss.backward()
    check(name, "dice", loss.detach(), x.grad, "from sums")
    tl, tg = tensor_form(name, "dice")
    assert abs(float(loss.detach()) - float(tl)) <= loss_tol(name, "dice")
    assert float((x.grad - tg).abs().max()) <= grad_tol(name, "dice")


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_labelled_gives_exact_zeros(kind):
    loss, grad = tensor_form("E", kind)
    assert float(loss) == 0.0 == float(golden()[f"E_{kind}_f64_loss"])
    assert torch.equal(grad, torch.zeros_like(grad))
    x, lab = case("E")
    diff, aux = sums_by_tensor_ops(x, lab)
    assert float(L.dice_from_sums(diff, aux)) == 0.0


def test_pal_tensor_alpha_beta():
    x, lab = case("C")
    cw = class_weights()
    plain = L.pal_tensor(x, lab, cw, alpha=1.0, beta=0.0)                     # alpha alone: the class-weighted CE
    assert abs(float(plain) - float(L.ce_ssc_loss(x, lab, cw))) <= 1e-4   # (sanity of the linearity: a few fp32 ulps at ~50)
    full = L.pal_tensor(x, lab, cw)
    assert abs(float(L.pal_tensor(x, lab, cw, alpha=0.0, beta=1.0)) - (float(full) - float(plain))) <= 1e-4
    assert abs(float(L.pal_tensor(x, lab, cw, alpha=2.0, beta=3.0)) - (3.0 * float(full) - float(plain))) <= 1e-4


def test_occ_losses_keys_order_and_weight():
    x, lab = case("C")                   # logits on the label grid: the x2 up-sampling of occ_losses is a HIP kernel
    cw = class_weights()
    base = L.occ_losses(x, lab, cw, w_lovasz=0.5)
    zero = L.occ_losses(x, lab, cw, w_lovasz=0.5, w_dice=0.0, w_lga=0.0)
    assert list(zero) == list(base) and all(torch.equal(zero[k], base[k]) for k in base)
    both = L.occ_losses(x, lab, cw, w_lovasz=0.5, w_dice=0.5, w_lga=2.0)
    assert list(both) == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0", "loss_voxel_lovasz_0",
                          "loss_voxel_dice_0", "loss_voxel_lga_0"]            # the reference's order (occhead.py:291-343)
    assert all(torch.equal(both[k], base[k]) for k in base)
    assert abs(float(both["loss_voxel_dice_0"]) - 0.5 * float(golden()["C_dice_ref_loss"])) <= loss_tol("C", "dice")
    assert abs(float(both["loss_voxel_lga_0"]) - 2.0 * float(golden()["C_lga_ref_loss"])) <= 2.0 * loss_tol("C", "lga")
    with_metric = L.occ_losses(x, lab, cw, compute_metric=True, w_dice=1.0, w_lga=1.0)
    assert list(with_metric)[3:5] == ["loss_voxel_dice_0", "loss_voxel_lga_0"] and "ssc_miou_0" in with_metric


def test_occ_head_flags_and_weights():
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    kw = dict(in_channels=[32], out_channel=20, semantic_kitti=True, norm_cfg=dict(type="GN", num_groups=8, requires_grad=True))
    x, lab = case("C")
    w = dict(voxel_ce=1, frustum_dist=1.0, voxel_dice=2.0, voxel_lga=0.5)
    head = OccHead(semkitti_loss_weight_cfg=w, use_frustum_loss=True, use_dice_loss=True, use_lga_loss=True, **kw)
    ids = torch.zeros(lab.shape, dtype=torch.uint8)
    dists = torch.ones(lab.shape[0], 1, 20)
    out = head.loss(output_voxels=[x], target_voxels=lab, frustums_ids=ids, frustums_class_dists=dists)
    assert [k for k in out if k.startswith("loss")] == ["loss_voxel_ce_0", "loss_voxel_fp_0", "loss_voxel_dice_0",
                                                        "loss_voxel_lga_0"]
    assert abs(float(out["loss_voxel_dice_0"]) - 2.0 * float(golden()["C_dice_ref_loss"])) <= 2.0 * loss_tol("C", "dice")
    assert abs(float(out["loss_voxel_lga_0"]) - 0.5 * float(golden()["C_lga_ref_loss"])) <= loss_tol("C", "lga")
    plain = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1), **kw).loss(output_voxels=[x], target_voxels=lab)
    assert torch.equal(plain["loss_voxel_ce_0"], out["loss_voxel_ce_0"])
    for k, flag in (("voxel_dice", "use_dice_loss"), ("voxel_lga", "use_lga_loss")):
        with pytest.raises(NotImplementedError, match=f"{flag}=True"):        # the weight alone does not switch it on
            OccHead(semkitti_loss_weight_cfg={"voxel_ce": 1, k: 1}, **kw)
        other = "use_lga_loss" if flag == "use_dice_loss" else "use_dice_loss"
        with pytest.raises(NotImplementedError, match=f"{flag}=True"):
            OccHead(semkitti_loss_weight_cfg={"voxel_ce": 1, k: 1}, **{other: True}, **kw)
        only = OccHead(semkitti_loss_weight_cfg={"voxel_ce": 1, k: 1}, **{flag: True}, **kw)
        got = only.loss(output_voxels=[x], target_voxels=lab)
        assert list(got)[:2] == ["loss_voxel_ce_0", f"loss_{k}_0"]
    flags_only = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_dice=0.0, voxel_lga=0.0), use_dice_loss=True,
                         use_lga_loss=True, **kw)
    out0 = flags_only.loss(output_voxels=[x], target_voxels=lab)
    assert list(out0) == list(plain) and all(torch.equal(out0[k], plain[k]) for k in plain)


def test_model_cfg_plumbing():
    from stereoscene_amd import model_zoo
    head = model_zoo.model_cfg(S.CFG_T)["pts_bbox_head"]
    assert "use_dice_loss" not in head and "use_lga_loss" not in head
    assert head["semkitti_loss_weight_cfg"].get("voxel_dice", 0.0) == 0.0 and head["semkitti_loss_weight_cfg"].get("voxel_lga", 0.0) == 0.0
    head = model_zoo.model_cfg(S.CFG_T, voxel_dice=0.5, voxel_lga=0.25)["pts_bbox_head"]
    assert head["semkitti_loss_weight_cfg"]["voxel_dice"] == 0.5 and head["use_dice_loss"] is True
    assert head["semkitti_loss_weight_cfg"]["voxel_lga"] == 0.25 and head["use_lga_loss"] is True
    one = model_zoo.model_cfg(S.CFG_T, voxel_lga=1.0)["pts_bbox_head"]
    assert "use_dice_loss" not in one and one["use_lga_loss"] is True
    from stereoscene_amd import plugin  # noqa: F401  (fills the registries)
    from stereoscene_amd.registry import HEADS
    built = HEADS.build(head)
    assert built.use_dice_loss and built.use_lga_loss
    assert built.semkitti_loss_weight_cfg["voxel_dice"] == 0.5 and built.semkitti_loss_weight_cfg["voxel_lga"] == 0.25


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 114
    for n in ("ssbev_occ_dice_tail", "ssbev_lga_weights", "ssbev_occ_lga_workspace", "ssbev_occ_lga_fwd",
              "ssbev_occ_lga_bwd_workspace", "ssbev_occ_lga_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    assert lib.ssbev_occ_dice_tail(None, 1.0, fake, fake, None) == capi.EINVAL
    assert lib.ssbev_occ_dice_tail(fake, 1.0, None, fake, None) == capi.EINVAL
    assert lib.ssbev_occ_dice_tail(fake, 1.0, fake, None, None) == capi.EINVAL
    assert lib.ssbev_lga_weights(None, fake, 1, 4, 4, 4, None) == capi.EINVAL
    assert lib.ssbev_lga_weights(fake, None, 1, 4, 4, 4, None) == capi.EINVAL
    for dims in ((0, 4, 4, 4), (1, 1, 4, 4), (1, 4, 1, 4), (1, 4, 4, 1), (64, 1024, 1024, 64)):      # the last: 2^32 voxels
        assert lib.ssbev_lga_weights(fake, fake, *dims, None) == capi.EINVAL
    good = capi.UpsampleDims(1, 16, 16, 8, 20)
    n_fine = 8 * 16 * 16 * 8
    ws = lib.ssbev_occ_lga_workspace(C.byref(good))
    assert 0 < ws <= 2048 * 2 * 8                                             # per-workgroup (num, den) partials
    assert lib.ssbev_occ_lga_bwd_workspace(C.byref(good)) == n_fine * 20 * 4  # the fine-resolution gradient
    for bad in (capi.UpsampleDims(0, 16, 16, 8, 20), capi.UpsampleDims(1, 16, 16, 8, 19), capi.UpsampleDims(1, 16, -1, 8, 20),
                capi.UpsampleDims(8, 512, 512, 64, 20)):                      # 20 x voxels past 2^31
        assert lib.ssbev_occ_lga_workspace(C.byref(bad)) == 0
        assert lib.ssbev_occ_lga_bwd_workspace(C.byref(bad)) == 0
        assert lib.ssbev_occ_lga_fwd(*[fake] * 4, 1.0, 1.0, fake, fake, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
        assert lib.ssbev_occ_lga_bwd(*[fake] * 4, 1.0, 1.0, fake, fake, fake, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
    assert lib.ssbev_occ_lga_fwd(*[None] * 4, 1.0, 1.0, None, None, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_occ_lga_fwd(*[fake] * 4, 1.0, 1.0, fake, fake, None, fake, ws, None) == capi.EINVAL
    assert lib.ssbev_occ_lga_bwd(*[None] * 4, 1.0, 1.0, None, None, None, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_occ_lga_fwd(*[fake] * 4, 1.0, 1.0, fake, fake, C.byref(good), fake, ws - 1, None) == capi.EWORKSPACE
    assert lib.ssbev_occ_lga_bwd(*[fake] * 4, 1.0, 1.0, fake, fake, fake, C.byref(good), fake, 16, None) == capi.EWORKSPACE


def test_unsupported_inputs_take_the_tensor_form():
    from stereoscene_amd import functional as F
    x, lab = case("G")
    assert not F.occ_lga_supported(x, lab)                                    # CPU tensor
    got = float(F.occ_lga_loss(x, lab, class_weights()))
    assert abs(got - float(golden()["G_lga_ref_loss"])) <= loss_tol("G", "lga")
