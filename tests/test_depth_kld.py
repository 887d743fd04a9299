"""CPU: the Gaussian KL depth loss (``loss_depth_type="kld"``) in its tensor form (functional.depth_kld_loss_tensor) against the
reference's own fp32 results and the float64 restatement recorded by tools/make_golden_depth_kld.py
(tests/golden/depth_kld.npz), its wiring into ``ViewTransformerLiftSplatShootVoxel`` and the host-side checks of the three C
entry points.

Bounds.  Both come from the fixture: K x the case's recorded reference-fp32-vs-float64 spread, K = 8, the factor that
tests/test_lovasz.py applies to its recorded spread (``grad_tol``; its ``loss_tol`` is a fixed project constant with no factor to
take, and no constant is introduced here).  Loss: K * max(X_loss_spread, eps) * max(1, |loss|); gradient: K * max(X_spread, eps) *
max|float64 gradient| on EVERY element.  eps = 2^-23 is the fp32 unit roundoff: the stored reference loss and every result under
test are fp32 numbers, which cannot resolve a smaller relative distance, so a spread recorded below it (case B's loss: 1.2e-9,
the reference's fp32 sum happened to round onto the float64 value) measures luck, not accuracy -- 8 x 1.2e-9 is a sixth of the
spacing of fp32 numbers at 0.8, and the fused kernel's loss of B on the MI355X is the neighbouring fp32 number, 6.0e-8 away.
The recorded gradient spreads (1.6e-7 .. 3.6e-7) are all above eps.  A, B, E are held to the reference's fp32 values, D (bin
units, which the reference does not have) to float64."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import ROOT
from stereoscene_amd import capi, functional as F, synthetic as S

GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_kld.npz")
K = 8.0
EPS = 2.0 ** -23
YARDSTICK = {"A": "ref", "B": "ref", "D": "f64", "E": "ref"}      # C: exact zeros


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """(gt_depths, depth_pred, ds, dbound, units) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.depth_kld_case(name)


def want(name):
    """(loss, gradient) the case is held to."""
    k = YARDSTICK[name]
    return float(golden()[f"{name}_{k}_loss"]), golden()[f"{name}_{k}_grad"].astype(np.float64)


def loss_tol(name):
    return K * max(float(golden()[f"{name}_loss_spread"]), EPS) * max(1.0, abs(float(golden()[f"{name}_f64_loss"])))


def grad_tol(name):
    return K * max(float(golden()[f"{name}_spread"]), EPS) * float(np.abs(golden()[f"{name}_f64_grad"]).max())


def background_rows(name):
    """Boolean [BN, fH, fW]: feature pixels whose float64 gradient row is entirely zero-by-mask (not foreground)."""
    gt, pred, ds, dbound, _ = case(name)
    B, N, H, W = gt.shape
    g = gt.reshape(B * N, H // ds, ds, W // ds, ds).permute(0, 1, 3, 2, 4).reshape(B * N, H // ds, W // ds, ds * ds)
    m = torch.where(g != 0, g, torch.full_like(g, 1e10)).min(dim=-1).values
    m = torch.where(m == 1e10, torch.zeros_like(m), m)
    return ~((m >= dbound[0]) & (m <= dbound[1] - dbound[2]))


def check(name, loss, grad, what):
    wl, wg = want(name)
    got = float(loss)
    err = float(np.abs(grad.double().numpy() - wg).max())
    print(name, what, "loss", got, "want", wl, "bound", loss_tol(name), "| max gradient error", err, "bound", grad_tol(name))
    assert abs(got - wl) <= loss_tol(name)
    assert torch.isfinite(grad).all() and err <= grad_tol(name)
    bg = background_rows(name).unsqueeze(1).expand_as(grad)
    assert bg.any() and not bg.all()
    assert torch.equal(grad[bg], torch.zeros_like(grad[bg]))              # exactly 0 off the foreground


def test_fixture_has_something_to_check():
    g = golden()
    for name in "ABDE":
        n_rows = case(name)[1][:, 0].numel()
        assert 0 < int(g[f"{name}_n_fg"]) < n_rows, name
        assert float(g[f"{name}_f64_loss"]) > 0 and np.abs(g[f"{name}_f64_grad"]).max() > 0
        assert float(g[f"{name}_spread"]) < 1e-6 and float(g[f"{name}_loss_spread"]) < 1e-6, name
    assert int(g["C_n_fg"]) == 0
    assert case("A")[1].shape == (2, 112, 3, 5) and case("B")[1].shape == (2, 13, 12, 23) and case("E")[1].shape == (1, 192, 2, 3)
    assert case("E")[3] == tuple(S.grid_config(S.CFG_K192)["dbound"])
    bg = background_rows("A")[0, 0]
    assert bg.tolist() == [False, False, True, True, False]              # d0, d1 - dd | next fp32 above, 1.9 | 33.6
    assert not np.any(g["A_ref_grad"][0, :, 0, 4]) and not np.any(g["A_f64_grad"][0, :, 0, 4])    # all-zero target row
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", ("A", "B", "D", "E"))
def test_tensor_form_matches_the_fixture(name):
    gt, pred, ds, dbound, units = case(name)
    p = pred.clone().requires_grad_(True)
    loss = F.depth_kld_loss_tensor(gt, p, ds, dbound, 1.0, 0.5, units)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    check(name, loss.detach(), p.grad, "tensor form")
    assert abs(float(loss.detach()) - float(golden()[f"{name}_f64_loss"])) <= loss_tol(name)


def test_no_foreground_row_gives_zero_and_a_zero_gradient():
    gt, pred, ds, dbound, units = case("C")
    assert not gt.any()
    p = pred.clone().requires_grad_(True)
    loss = F.depth_kld_loss(gt, p, ds, dbound, 1.0)
    assert loss.dim() == 0 and torch.isfinite(loss) and float(loss.detach()) == 0.0
    loss.backward()
    assert torch.equal(p.grad, torch.zeros_like(p))


def test_unsupported_inputs_take_the_tensor_form_and_bad_arguments_are_refused():
    gt, pred, ds, dbound, units = case("B")
    a = F.depth_kld_loss(gt, pred, ds, dbound, 0.5)                        # CPU tensors
    b = F.depth_kld_loss_tensor(gt, pred, ds, dbound, 0.5)
    assert torch.equal(a, b)
    l64 = F.depth_kld_loss(gt.double(), pred.double(), ds, dbound, 1.0)
    assert l64.dtype == torch.float64 and abs(float(l64) - float(golden()["B_f64_loss"])) <= 1e-12
    with pytest.raises(ValueError):
        F.depth_kld_loss(gt, pred, ds, dbound, 1.0, units="metres")
    with pytest.raises(ValueError):
        F.depth_kld_loss_tensor(gt, pred, ds, (2.0, 9.0, 0.5), 1.0)       # 15 edges for 13 bins


def vt_kwargs(name, **kw):
    gt, pred, ds, dbound, _ = case(name)
    grid = dict(S.grid_config(S.CFG_T), dbound=list(dbound))
    return dict(loss_depth_weight=3.0, grid_config=grid, data_config=dict(input_size=tuple(gt.shape[-2:])), numC_input=32,
                numC_Trans=16, downsample=ds, cam_channels=30, **kw)


def test_view_transformer_dispatches_on_loss_depth_type():
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT
    gt, pred, ds, dbound, _ = case("B")
    vt = VT(loss_depth_type="kld", **vt_kwargs("B"))
    assert vt.constant_std == 0.5 and vt.depth_kld_units == "reference" and vt.D == pred.shape[1]
    got = float(vt.get_depth_loss(gt, pred))
    assert abs(got - 3.0 * want("B")[0]) <= 3.0 * loss_tol("B")
    assert float(vt.get_klv_depth_loss(gt, pred)) == got
    bins = VT(loss_depth_type="kld", depth_kld_units="bins", **vt_kwargs("D"))
    assert abs(float(bins.get_depth_loss(gt, pred)) - 3.0 * want("D")[0]) <= 3.0 * loss_tol("D")
    with pytest.raises(ValueError):
        VT(loss_depth_type="kld", depth_kld_units="metres", **vt_kwargs("B"))
    with pytest.raises(NotImplementedError):
        VT(loss_depth_type="l1", **vt_kwargs("B")).get_depth_loss(gt, pred)
    bce = VT(**vt_kwargs("B"))
    assert bce.loss_depth_type == "bce" and torch.isfinite(bce.get_depth_loss(gt, pred))


def test_model_cfg_passes_loss_depth_type_through():
    from stereoscene_amd import model_zoo
    assert "loss_depth_type" not in model_zoo.model_cfg(S.CFG_T)["img_view_transformer"] or \
        model_zoo.model_cfg(S.CFG_T)["img_view_transformer"]["loss_depth_type"] == "bce"
    assert model_zoo.model_cfg(S.CFG_T, loss_depth_type="kld")["img_view_transformer"]["loss_depth_type"] == "kld"


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 109
    for n in ("ssbev_depth_kld_workspace", "ssbev_depth_kld_fwd", "ssbev_depth_kld_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    BN, D, fH, fW, ds = 2, 112, 48, 160, 8
    npix = BN * fH * fW
    ws = lib.ssbev_depth_kld_workspace(BN, fH, fW)
    assert ws >= npix * 8 + (npix // 256) * 8 * 16                      # m and the flag per pixel + (kl, count) partials
    for bad in ((0, fH, fW), (BN, -1, fW), (BN, fH, 0), (1 << 15, 1 << 8, 1 << 8)):
        assert lib.ssbev_depth_kld_workspace(*bad) == 0

    def fwd(p=(fake, fake, fake), dims=(BN, D, fH, fW, ds), db=(2.0, 58.0, 0.5), sigma=0.5, es=1.0, w=fake, nbytes=ws):
        return lib.ssbev_depth_kld_fwd(*p, *dims, *db, sigma, es, 1.0, w, nbytes, None)

    def bwd(p=(fake, fake, fake, fake), dims=(BN, D, fH, fW, ds), db=(2.0, 58.0, 0.5), sigma=0.5, es=1.0, w=fake, nbytes=ws):
        return lib.ssbev_depth_kld_bwd(*p, *dims, *db, sigma, es, 1.0, w, nbytes, None)

    for call, n in ((fwd, 3), (bwd, 4)):
        for i in range(n):
            assert call(p=tuple(None if j == i else fake for j in range(n))) == capi.EINVAL
        assert call(w=None) == capi.EINVAL
        assert call(dims=(0, D, fH, fW, ds)) == capi.EINVAL
        assert call(dims=(BN, D, fH, fW, 0)) == capi.EINVAL
        assert call(sigma=0.0) == capi.EINVAL
        assert call(db=(2.0, 58.0, 0.0)) == capi.EINVAL
        assert call(db=(2.0, 58.0, -0.5)) == capi.EINVAL
        assert call(es=0.0) == capi.EINVAL
        assert call(db=(2.0, float("nan"), 0.5)) == capi.EINVAL
        assert call(db=(2.0, 58.5, 0.5)) == capi.EINVAL                   # 114 edges for 112 bins
        assert call(dims=(BN, D + 1, fH, fW, ds)) == capi.EINVAL          # 113 edges for 113 bins
        assert call(db=(2.0, 98.0, 0.5)) == capi.EINVAL
        assert call(nbytes=ws - 1) == capi.EWORKSPACE
        assert call(nbytes=0) == capi.EWORKSPACE
    assert fwd(dims=(BN, 192, fH, fW, ds), db=(2.0, 98.0, 0.5), nbytes=ws - 1) == capi.EWORKSPACE      # valid dims reach the size check
