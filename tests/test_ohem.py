"""CPU: the OHEM cross-entropy voxel loss in its tensor form (plugin/losses.py) against the reference's own fp32 results and the
float64 restatement recorded by tools/make_golden_ohem.py (tests/golden/ohem.npz), its wiring into ``occ_losses``, ``OccHead`` and
``model_zoo.model_cfg``, and the host-side checks of the four C entry points.

Bounds, from the fixture as in tests/test_depth_kld.py: K x the case's recorded fp32-vs-float64 spread, K = 8.  Loss:
K * max(X_loss_spread, eps) * max(1, |loss|) with eps = 2^-23, the fp32 unit roundoff (every result under test is an fp32 number and
cannot resolve a smaller relative distance; B's recorded 4.2e-8 is below it).  Gradient: K * X_spread * max|float64 gradient| on
EVERY element, no floor.  A, B, C, G are held to the reference's fp32 values, D's value too; D's gradient and H to the float64
restatement with the lowest-index tie rule (``torch.topk``'s choice among ties is unspecified, so the reference's record is no
yardstick there).  The gap condition of the generator (every sample's float64 gap at the threshold >= 64 x the largest fp32
per-voxel loss error) makes the fp32 and float64 selections of A, B, C, G the same set, so no voxel is excluded anywhere."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from stereoscene_amd import capi, synthetic as S
from stereoscene_amd.plugin import losses as L

GOLDEN = os.path.join(ROOT, "tests", "golden", "ohem.npz")
DELTA_SCALE = 16384.0              # tools/make_golden_ohem.py
K = 8.0
EPS = 2.0 ** -23
GAP_CHECKED = ("A", "B", "C", "G")


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, labels, top_k) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.ohem_case(name)


@functools.lru_cache(maxsize=None)
def class_weights():
    return L.semkitti_class_weights()


def ref_grad(name):
    """The reference's fp32 gradient: stored as the float64 gradient plus an fp16 difference (see the generator)."""
    g = golden()[f"{name}_f64_grad"].astype(np.float64)
    return (g + golden()[f"{name}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def loss_tol(name):
    return K * max(float(golden()[f"{name}_loss_spread"]), EPS) * max(1.0, abs(float(golden()[f"{name}_f64_loss"])))


def grad_tol(name):
    return K * float(golden()[f"{name}_spread"]) * float(np.abs(golden()[f"{name}_f64_grad"]).max())


def tensor_form(name, device="cpu"):
    x, lab, top_k = case(name)
    x = x.clone().to(device).requires_grad_(True)
    loss = L.ohem_ce_loss(x, lab.to(device), class_weights().to(device), top_k)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.detach().cpu(), x.grad.detach().cpu()


def test_fixture_conditions():
    g = golden()
    for name in GAP_CHECKED:
        gap, err = g[f"{name}_gap"], float(g[f"{name}_l_err"])
        print(name, "gap", gap.tolist(), "largest fp32 per-voxel loss error", err)
        assert (gap >= 64.0 * err).all(), name
        assert 0.0 < float(g[f"{name}_spread"]) <= 1e-6 and float(g[f"{name}_loss_spread"]) <= 1e-6, name
    assert g["A_M"][0] != g["A_M"][1] and g["A_k"][0] != g["A_k"][1]          # two samples, two thresholds
    assert g["B_M"].tolist() == [14716] and g["B_k"].tolist() == [3679]        # eight tiles of the selection kernels
    assert g["E_M"].tolist() == [0, 0] and g["F_M"].tolist() == [1, 1] and g["F_k"].tolist() == [0, 0]
    assert g["G_M"][0] < 128
    assert (g["D_gap"] == 0.0).all() and float(g["H_gap"].max()) < 1e-12      # the threshold sits inside a tie group
    for name in S.OHEM_CASES:                                                 # the recorded counts are the inputs' own
        _, lab, top_k = case(name)
        m = (lab.flatten(1) != 255).sum(1).tolist()
        assert m == g[f"{name}_M"].tolist() and [int(v * top_k) for v in m] == g[f"{name}_k"].tolist(), name
    x, lab, _ = case("H")
    xc, _, _ = case("C")
    planted = (x != xc).flatten(2).any(1)                                     # [B, N]
    frac = float(planted.sum()) / float((lab != 255).sum())
    assert 0.15 < frac < 0.25 and not planted[lab.flatten(1) == 255].any()
    assert float((x - xc).max()) == 40.0
    assert os.path.getsize(GOLDEN) < 1000000


@pytest.mark.parametrize("name", GAP_CHECKED)
def test_tensor_form_matches_the_reference_fp32(name):
    loss, grad = tensor_form(name)
    want, got = float(golden()[f"{name}_ref_loss"]), float(loss)
    err = float(np.abs(grad.numpy() - ref_grad(name)).max())
    print(name, "loss", got, "reference", want, "bound", loss_tol(name), "| max gradient error", err, "bound", grad_tol(name))
    assert abs(got - want) <= loss_tol(name)
    assert abs(got - float(golden()[f"{name}_f64_loss"])) <= loss_tol(name)
    assert err <= grad_tol(name)
    assert float(np.abs(grad.numpy() - golden()[f"{name}_f64_grad"]).max()) <= grad_tol(name)


def test_ties_inside_one_class_give_the_reference_value_and_the_float64_gradient():
    loss, grad = tensor_form("D")
    assert abs(float(loss) - float(golden()["D_ref_loss"])) <= loss_tol("D")
    assert abs(float(loss) - float(golden()["D_f64_loss"])) <= loss_tol("D")
    err = float(np.abs(grad.numpy() - golden()["D_f64_grad"]).max())
    print("D max gradient error", err, "bound", grad_tol("D"))
    assert err <= grad_tol("D")


def test_zero_losses_inside_the_selection_go_to_the_lowest_index():
    loss, grad = tensor_form("H")
    assert abs(float(loss) - float(golden()["H_f64_loss"])) <= loss_tol("H")
    err = float(np.abs(grad.numpy() - golden()["H_f64_grad"]).max())
    print("H max gradient error", err, "bound", grad_tol("H"))
    assert err <= grad_tol("H")
    # the trap: a saturated voxel's cross entropy is -0.0 in torch, and the tensor form canonicalises it
    x, lab, _ = case("H")
    raw = torch.nn.functional.cross_entropy(x, lab.long(), weight=class_weights(), ignore_index=255, reduction="none")
    zero = (raw == 0) & (lab != 255)
    assert int(zero.sum()) > 400 and torch.signbit(raw[zero]).any()


@pytest.mark.parametrize("name", ("E", "F"))
def test_nothing_selected_gives_zero_and_a_zero_gradient(name):
    loss, grad = tensor_form(name)
    assert float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("top_k", (0.25, 0.9, 1.0, 1.0 / 3.0))
def test_kept_count_is_pythons_truncated_product(top_k):
    x, lab, _ = case("A")
    up = torch.nn.functional.interpolate(x, size=lab.shape[-3:], mode="trilinear", align_corners=False).detach().requires_grad_(True)
    L.ohem_ce_tensor(up, lab, class_weights(), top_k).backward()
    kept = (up.grad != 0).any(1).flatten(1).sum(1).tolist()                   # a kept voxel has a non-zero gradient row here
    m = (lab.flatten(1) != 255).sum(1).tolist()
    assert kept == [int(v * top_k) for v in m] == [L.ohem_k(v, top_k) for v in m]
    assert top_k == 1.0 or kept != m


def test_occ_losses_keys_order_and_weight():
    x, lab, _ = case("C")                # logits on the label grid: the x2 up-sampling of occ_losses is a HIP kernel
    cw = class_weights()
    base = L.occ_losses(x, lab, cw, w_lovasz=0.5)
    assert list(base) == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0", "loss_voxel_lovasz_0"]
    zero = L.occ_losses(x, lab, cw, w_lovasz=0.5, w_ohem=0.0, ohem_topk=0.9)
    assert list(zero) == list(base) and all(torch.equal(zero[k], base[k]) for k in base)
    half = L.occ_losses(x, lab, cw, w_lovasz=0.5, w_ohem=0.5, ohem_topk=0.9)
    assert list(half) == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0", "loss_voxel_sem_ohem_0",
                          "loss_voxel_lovasz_0"]                             # the reference's order (occhead.py:291-324)
    assert all(torch.equal(half[k], base[k]) for k in base)
    unweighted = float(L.ohem_ce_loss(x, lab, cw, 0.9))
    assert abs(float(half["loss_voxel_sem_ohem_0"]) - 0.5 * unweighted) <= 1e-6
    assert abs(unweighted - float(golden()["C_ref_loss"])) <= loss_tol("C")
    with_metric = L.occ_losses(x, lab, cw, compute_metric=True, w_ohem=0.5, ohem_topk=0.9)
    assert list(with_metric)[3] == "loss_voxel_sem_ohem_0" and "ssc_miou_0" in with_metric


def test_occ_head_flag_weight_and_fraction():
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    kw = dict(in_channels=[32], out_channel=20, semantic_kitti=True, norm_cfg=dict(type="GN", num_groups=8, requires_grad=True))
    x, lab, top_k = case("C")
    head = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_ohem=2.0), use_ohem_loss=True, ohem_topk=top_k, **kw)
    out = head.loss(output_voxels=[x], target_voxels=lab)
    assert list(out)[:2] == ["loss_voxel_ce_0", "loss_voxel_sem_ohem_0"]
    want = 2.0 * float(golden()["C_ref_loss"])
    assert abs(float(out["loss_voxel_sem_ohem_0"]) - want) <= 2.0 * loss_tol("C")
    plain = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1), **kw).loss(output_voxels=[x], target_voxels=lab)
    assert torch.equal(plain["loss_voxel_ce_0"], out["loss_voxel_ce_0"])
    with pytest.raises(NotImplementedError, match="use_ohem_loss=True"):     # the weight alone does not switch it on
        OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_ohem=1), **kw)
    flag_only = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_ohem=0.0), use_ohem_loss=True, **kw)
    out0 = flag_only.loss(output_voxels=[x], target_voxels=lab)
    assert list(out0) == list(plain) and all(torch.equal(out0[k], plain[k]) for k in plain)
    for bad in (0.0, -0.25, 1.5, float("nan")):
        with pytest.raises(ValueError):
            OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_ohem=1), use_ohem_loss=True, ohem_topk=bad, **kw)
    for k in ("frustum_dist", "voxel_dice", "voxel_lga"):
        with pytest.raises(NotImplementedError):
            OccHead(semkitti_loss_weight_cfg={"voxel_ce": 1, k: 1}, use_ohem_loss=True, **kw)


def test_model_cfg_plumbing():
    from stereoscene_amd import model_zoo
    head = model_zoo.model_cfg(S.CFG_T)["pts_bbox_head"]
    assert head["semkitti_loss_weight_cfg"]["voxel_ohem"] == 0.0 and "use_ohem_loss" not in head and "ohem_topk" not in head
    head = model_zoo.model_cfg(S.CFG_T, voxel_ohem=0.5, ohem_topk=0.3)["pts_bbox_head"]
    assert head["semkitti_loss_weight_cfg"]["voxel_ohem"] == 0.5 and head["use_ohem_loss"] is True and head["ohem_topk"] == 0.3
    from stereoscene_amd import plugin  # noqa: F401  (fills the registries)
    from stereoscene_amd.registry import HEADS
    built = HEADS.build(head)
    assert built.use_ohem_loss and built.ohem_topk == 0.3 and built.semkitti_loss_weight_cfg["voxel_ohem"] == 0.5


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 110
    for n in ("ssbev_ohem_ce_workspace", "ssbev_ohem_ce_fwd", "ssbev_ohem_ce_bwd_workspace", "ssbev_ohem_ce_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    good = capi.OhemDims(1, 16, 16, 8, 20, 255, 1, 0.25)
    n_fine = 8 * 16 * 16 * 8
    ws = lib.ssbev_ohem_ce_workspace(C.byref(good))
    assert 4 * n_fine <= ws < 5 * n_fine                              # the fp32 losses; histograms and tile partials are small
    assert lib.ssbev_ohem_ce_bwd_workspace(C.byref(good)) == n_fine * 20 * 4      # the fine-resolution gradient
    same_grid = capi.OhemDims(1, 16, 16, 8, 20, 255, 0, 1.0)
    assert 0 < lib.ssbev_ohem_ce_workspace(C.byref(same_grid)) < ws
    assert lib.ssbev_ohem_ce_bwd_workspace(C.byref(same_grid)) == 0
    for bad in (capi.OhemDims(0, 16, 16, 8, 20, 255, 1, 0.25), capi.OhemDims(1, 16, 16, 8, 19, 255, 1, 0.25),
                capi.OhemDims(1, 16, 16, 8, 20, 255, 2, 0.25), capi.OhemDims(1, 16, -1, 8, 20, 255, 0, 0.25),
                capi.OhemDims(1, 16, 16, 8, 20, 255, 1, 0.0), capi.OhemDims(1, 16, 16, 8, 20, 255, 1, 1.25),
                capi.OhemDims(1, 16, 16, 8, 20, 255, 1, float("nan")),
                capi.OhemDims(8, 512, 512, 64, 20, 255, 1, 0.25)):    # 20 x voxels past 2^31
        assert lib.ssbev_ohem_ce_workspace(C.byref(bad)) == 0
        assert lib.ssbev_ohem_ce_bwd_workspace(C.byref(bad)) == 0
        assert lib.ssbev_ohem_ce_fwd(*[fake] * 6, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
        assert lib.ssbev_ohem_ce_bwd(*[fake] * 7, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
    assert lib.ssbev_ohem_ce_fwd(*[None] * 6, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_ohem_ce_fwd(*[fake] * 6, None, fake, ws, None) == capi.EINVAL
    assert lib.ssbev_ohem_ce_bwd(*[None] * 7, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_ohem_ce_fwd(*[fake] * 6, C.byref(good), fake, ws - 1, None) == capi.EWORKSPACE
    assert lib.ssbev_ohem_ce_bwd(*[fake] * 7, C.byref(good), fake, 16, None) == capi.EWORKSPACE


def test_unsupported_inputs_take_the_tensor_form():
    from stereoscene_amd import functional as F
    x, lab, top_k = case("G")
    assert not F.ohem_supported(x, lab)                                # CPU tensor
    got = float(F.ohem_ce_loss(x, lab, class_weights(), top_k))
    assert abs(got - float(golden()["G_ref_loss"])) <= loss_tol("G")
