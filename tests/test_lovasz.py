"""CPU: the Lovasz-softmax voxel loss in its tensor form (plugin/losses.py) against the reference's own fp32 results and the
float64 restatement recorded by tools/make_golden_lovasz.py (tests/golden/lovasz.npz), its wiring into ``occ_losses`` and
``OccHead``, and the host-side checks of the three C entry points.

Bounds.  Loss: 2e-5 * max(1, |v|), the project's loss tolerance.  Gradient: max(2e-4, 8 x recorded spread) * max|grad| on EVERY
element, where the spread is the reference's own fp32-vs-float64 gradient difference on the fixture (nearly equal errors sort
differently in the two precisions; a swapped fg / non-fg pair moves two entries), recorded as a fraction of the largest entry."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from stereoscene_amd import capi, synthetic as S
from stereoscene_amd.plugin import losses as L

GOLDEN = os.path.join(ROOT, "tests", "golden", "lovasz.npz")
DELTA_SCALE = 16384.0              # tools/make_golden_lovasz.py
FULL = ("A", "B", "C", "F", "G")   # value and gradient; D is value only (ties), E is all ignored


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """(logits, labels) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.lovasz_case(name)


def ref_grad(name):
    """The reference's fp32 gradient: stored as the float64 gradient plus an fp16 difference (see the generator)."""
    g = golden()[f"{name}_f64_grad"].astype(np.float64)
    return (g + golden()[f"{name}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def loss_tol(v):
    return 2e-5 * max(1.0, abs(float(v)))


def grad_tol(name):
    return max(2e-4, 8.0 * float(golden()[f"{name}_spread"])) * float(np.abs(golden()[f"{name}_f64_grad"]).max())


def test_fixture_spread_is_within_the_limit_the_bound_assumes():
    for name in ("A", "B", "C", "G"):
        assert float(golden()[f"{name}_spread"]) <= 2.5e-5, name
        assert float(golden()[f"{name}_loss_spread"]) <= 2e-6, name
    x, lab = case("A")
    present = [set(torch.unique(lab[b]).tolist()) - {255} for b in range(2)]
    assert 19 in present[1] and 19 not in present[0]              # one class in sample 1 only
    assert not ({2, 3, 8} & (present[0] | present[1]))            # absent classes
    assert 0.05 < float((lab == 255).float().mean()) < 0.15
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", FULL)
def test_tensor_form_matches_the_reference_fp32(name):
    x, lab = case(name)
    x = x.clone().requires_grad_(True)
    loss = L.lovasz_softmax_loss(x, lab)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    want, got = float(golden()[f"{name}_ref_loss"]), float(loss.detach())
    print(name, "loss", got, "reference", want)
    assert abs(got - want) <= loss_tol(want)
    assert abs(got - float(golden()[f"{name}_f64_loss"])) <= loss_tol(want)
    loss.backward()
    err = float(np.abs(x.grad.numpy() - ref_grad(name)).max())
    print(name, "max gradient error", err, "bound", grad_tol(name))
    assert err <= grad_tol(name)


def test_ties_give_the_float64_value():
    x, lab = case("D")
    v = float(L.lovasz_softmax_loss(x, lab))
    want = float(golden()["D_f64_loss"])
    assert abs(v - want) <= loss_tol(want)


def test_no_labelled_voxel_gives_zero_and_a_zero_gradient():
    x, lab = case("E")
    x = x.clone().requires_grad_(True)
    loss = L.lovasz_softmax_loss(x, lab)
    assert loss.dim() == 0 and float(loss.detach()) == 0.0
    loss.backward()
    assert torch.equal(x.grad, torch.zeros_like(x))


def test_single_labelled_voxel_is_the_ordinary_value():
    """M = 1 (the reference's squeeze() breaks here): one voxel of class c gives J_0 = 1, so the loss is 1 - p_c."""
    x, _ = case("G")
    lab = torch.full(S.LOVASZ_CASES["G"][1], 255, dtype=torch.uint8)
    lab[0, 1, 2, 3] = 6
    up = torch.nn.functional.interpolate(x, size=lab.shape[-3:], mode="trilinear", align_corners=False)
    want = 1.0 - float(torch.softmax(up, 1)[0, 6, 1, 2, 3])
    assert abs(float(L.lovasz_softmax_loss(x, lab)) - want) <= loss_tol(want)


def test_occ_losses_keys_and_weight():
    x, lab = case("C")                   # logits on the label grid: the x2 up-sampling of occ_losses is a HIP kernel
    cw = L.semkitti_class_weights()
    base = L.occ_losses(x, lab, cw)
    assert list(base) == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0"]
    zero = L.occ_losses(x, lab, cw, w_lovasz=0.0)
    assert list(zero) == list(base) and all(torch.equal(zero[k], base[k]) for k in base)
    half = L.occ_losses(x, lab, cw, w_lovasz=0.5)
    assert list(half) == list(base) + ["loss_voxel_lovasz_0"]
    assert all(torch.equal(half[k], base[k]) for k in base)
    unweighted = float(L.lovasz_softmax_loss(x, lab))
    assert abs(float(half["loss_voxel_lovasz_0"]) - 0.5 * unweighted) <= 1e-7
    with_metric = L.occ_losses(x, lab, cw, compute_metric=True, w_lovasz=0.5)
    assert list(with_metric)[3] == "loss_voxel_lovasz_0" and "ssc_miou_0" in with_metric


def test_occ_head_accepts_voxel_lovasz_and_still_refuses_the_others():
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    kw = dict(in_channels=[32], out_channel=20, semantic_kitti=True, norm_cfg=dict(type="GN", num_groups=8, requires_grad=True))
    head = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_lovasz=1), **kw)
    x, lab = case("C")
    out = head.loss(output_voxels=[x], target_voxels=lab)
    assert list(out)[:2] == ["loss_voxel_ce_0", "loss_voxel_lovasz_0"]
    want = float(golden()["C_ref_loss"])
    assert abs(float(out["loss_voxel_lovasz_0"]) - want) <= loss_tol(want)
    for k in ("voxel_ohem", "frustum_dist", "voxel_dice", "voxel_lga"):
        with pytest.raises(NotImplementedError):
            OccHead(semkitti_loss_weight_cfg={"voxel_ce": 1, k: 1}, **kw)


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 104
    for n in ("ssbev_lovasz_workspace", "ssbev_lovasz_fwd", "ssbev_lovasz_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    good = capi.LovaszDims(1, 16, 16, 8, 20, 255, 1)
    n_fine = 8 * 16 * 16 * 8
    ws = lib.ssbev_lovasz_workspace(C.byref(good))
    assert ws >= 4 * 20 * n_fine * 4                              # two (key, voxel) buffers of 20 class segments
    assert lib.ssbev_lovasz_bwd_workspace(C.byref(good)) == n_fine * 20 * 4      # the fine-resolution gradient
    same_grid = capi.LovaszDims(1, 16, 16, 8, 20, 255, 0)
    assert 0 < lib.ssbev_lovasz_workspace(C.byref(same_grid)) < ws
    assert lib.ssbev_lovasz_bwd_workspace(C.byref(same_grid)) == 0
    assert lib.ssbev_lovasz_num_counts() >= 22
    for bad in (capi.LovaszDims(0, 16, 16, 8, 20, 255, 1), capi.LovaszDims(1, 16, 16, 8, 19, 255, 1),
                capi.LovaszDims(1, 16, 16, 8, 20, 255, 2), capi.LovaszDims(1, 16, -1, 8, 20, 255, 0),
                capi.LovaszDims(8, 512, 512, 64, 20, 255, 1)):     # 20 x voxels past 2^31
        assert lib.ssbev_lovasz_workspace(C.byref(bad)) == 0
        assert lib.ssbev_lovasz_bwd_workspace(C.byref(bad)) == 0
        assert lib.ssbev_lovasz_fwd(fake, fake, fake, fake, fake, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
        assert lib.ssbev_lovasz_bwd(fake, fake, fake, fake, fake, fake, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
    assert lib.ssbev_lovasz_fwd(None, None, None, None, None, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_lovasz_fwd(fake, fake, fake, fake, fake, None, fake, ws, None) == capi.EINVAL
    assert lib.ssbev_lovasz_bwd(None, None, None, None, None, None, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_lovasz_fwd(fake, fake, fake, fake, fake, C.byref(good), fake, ws - 1, None) == capi.EWORKSPACE
    assert lib.ssbev_lovasz_bwd(fake, fake, fake, fake, fake, fake, C.byref(good), fake, 16, None) == capi.EWORKSPACE


def test_unsupported_inputs_take_the_tensor_form():
    from stereoscene_amd import functional as F
    x, lab = case("G")
    assert not F.lovasz_supported(x, lab)                          # CPU tensor
    want = float(golden()["G_ref_loss"])
    assert abs(float(F.lovasz_softmax(x, lab)) - want) <= loss_tol(want)
