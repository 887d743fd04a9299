"""GPU: the fused Lovasz-softmax path (csrc/lovasz.hip through ``functional.lovasz_softmax``) against the float64 yardstick of
tests/golden/lovasz.npz and against the tensor form on the same card.  Bounds as in tests/test_lovasz.py: loss within
2e-5 * max(1, |v|); EVERY element of the logit gradient within max(2e-4, 8 x the reference's recorded fp32-vs-float64 spread) *
max|grad| (the factor of 8 covers another exp and another summation order on the device)."""
import numpy as np
import pytest
import torch

from stereoscene_amd import functional as F
from stereoscene_amd.plugin import losses as L
from test_lovasz import FULL, case, golden, grad_tol, loss_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"


def fused(name, scale=1.0):
    x, lab = case(name)
    xg = x.to(DEV).requires_grad_(True)
    assert F.LOVASZ and F.lovasz_supported(xg, lab.to(DEV))
    loss = F.lovasz_softmax(xg, lab.to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), xg.grad.detach().cpu()


def tensor_form(name, monkeypatch):
    monkeypatch.setattr(F, "LOVASZ", False)            # what SSBEV_LOVASZ=0 sets at import
    x, lab = case(name)
    xg = x.to(DEV).requires_grad_(True)
    loss = L.lovasz_softmax_loss(xg, lab.to(DEV))
    loss.backward()
    monkeypatch.setattr(F, "LOVASZ", True)
    return loss.detach().cpu(), xg.grad.detach().cpu()


@pytest.mark.parametrize("name", FULL)
def test_fused_matches_float64_and_the_tensor_form(name, monkeypatch):
    loss, grad = fused(name)
    want = float(golden()[f"{name}_f64_loss"])
    g64 = golden()[f"{name}_f64_grad"]
    err = float(np.abs(grad.numpy() - g64).max())
    print(name, "loss", float(loss), "float64", want, "max gradient error", err, "bound", grad_tol(name))
    assert abs(float(loss) - want) <= loss_tol(want)
    assert torch.isfinite(grad).all() and err <= grad_tol(name)
    tl, tg = tensor_form(name, monkeypatch)
    terr = float((grad - tg).abs().max())
    print(name, "tensor form loss", float(tl), "max gradient difference", terr)
    assert abs(float(loss) - float(tl)) <= loss_tol(want)
    assert abs(float(tl) - want) <= loss_tol(want)
    assert terr <= grad_tol(name)


def test_ties_give_the_float64_value():
    loss, grad = fused("D")
    want = float(golden()["D_f64_loss"])
    assert abs(float(loss) - want) <= loss_tol(want)
    assert torch.isfinite(grad).all()


def test_no_labelled_voxel_gives_exact_zeros():
    loss, grad = fused("E")
    assert float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


def test_single_labelled_voxel():
    x, _ = case("G")
    lab = torch.full((1, 6, 4, 4), 255, dtype=torch.uint8)
    lab[0, 1, 2, 3] = 6
    up = torch.nn.functional.interpolate(x.double(), size=lab.shape[-3:], mode="trilinear", align_corners=False)
    want = 1.0 - float(torch.softmax(up, 1)[0, 6, 1, 2, 3])
    got = F.lovasz_softmax(x.to(DEV), lab.to(DEV))
    assert abs(float(got) - want) <= loss_tol(want)


@pytest.mark.parametrize("name", ("A", "B"))
def test_two_runs_give_the_same_bits(name):
    l0, g0 = fused(name)
    l1, g1 = fused(name)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_incoming_gradient_scale_is_applied():
    _, g1 = fused("A")
    _, g3 = fused("A", scale=3.0)
    assert float((g3 - 3.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    assert float(np.abs(g3.numpy() / 3.0 - golden()["A_f64_grad"]).max()) <= grad_tol("A")


def test_occ_head_loss_with_all_four_terms():
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    kw = dict(in_channels=[32], out_channel=20, semantic_kitti=True, norm_cfg=dict(type="GN", num_groups=8, requires_grad=True))
    x, lab = case("A")
    four = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_sem_scal=1, voxel_geo_scal=1, voxel_lovasz=1), **kw).to(DEV)
    three = OccHead(semkitti_loss_weight_cfg=dict(voxel_ce=1, voxel_sem_scal=1, voxel_geo_scal=1), **kw).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = four.loss(output_voxels=[xg], target_voxels=lab.to(DEV))
    keys = [k for k in out if k.startswith("loss")]
    assert keys == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0", "loss_voxel_lovasz_0"]
    sum(out[k] for k in keys).backward()
    x3 = x.to(DEV).requires_grad_(True)
    out3 = three.loss(output_voxels=[x3], target_voxels=lab.to(DEV))
    assert [k for k in out3 if k.startswith("loss")] == keys[:3]
    for k in keys[:3]:
        assert torch.equal(out3[k], out[k])
    sum(out3[k] for k in keys[:3]).backward()
    want = float(golden()["A_f64_loss"])
    assert abs(float(out["loss_voxel_lovasz_0"].detach()) - want) <= loss_tol(want)
    # the three-term gradient is held to 2e-6 by test_fused_occ_loss_matches_unfused_and_oracle, the Lovasz one to grad_tol above
    parts = x3.grad.cpu().numpy() + golden()["A_f64_grad"]
    err = float(np.abs(xg.grad.cpu().numpy() - parts).max())
    print("four-term gradient error", err, "bound", 2e-6 + grad_tol("A"))
    assert err <= 2e-6 + grad_tol("A")
