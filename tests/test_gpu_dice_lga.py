"""GPU: the fused soft-Dice tail and the fused LGA-weighted cross entropy (csrc/occ_extra.hip through ``functional``) against the
float64 results of tests/golden/dice_lga.npz and against the tensor forms on the same card.  Bounds as in tests/test_dice_lga.py:
loss within 8 * max(recorded loss spread, 2^-23) * max(1, |loss|); EVERY element of the logit gradient within 8 x the recorded
fp32-vs-float64 gradient spread * max|grad|.  The LGA weights are integers and are held bit-equal to the reference's."""
import numpy as np
import pytest
import torch

from stereoscene_amd import functional as F, synthetic as S
from stereoscene_amd.plugin import losses as L
from test_dice_lga import KINDS, case, check, class_weights, golden, grad_tol, loss_tol, tensor_form

pytestmark = pytest.mark.gpu
DEV = "cuda"
FUSED_CASES = ("A", "B", "G", "K", "N", "Z")        # x2 cases with labelled voxels (C runs the tensor form, L is checked below)


def fused(name, kind, scale=1.0):
    """(loss, logit gradient) of the fused path: the Dice term of the fused epilogue (its tail follows ``F.OCC_TAIL``), or
    ``functional.occ_lga_loss``."""
    x, lab = case(name)
    xg = x.to(DEV).requires_grad_(True)
    lab = lab.to(DEV)
    if kind == "dice":
        loss = L.occ_losses_fused(xg, lab, class_weights().to(DEV), w_ce=0.0, w_sem=0.0, w_geo=0.0, w_dice=1.0)["loss_voxel_dice_0"]
    else:
        assert F.LGA and F.occ_lga_supported(xg, lab)
        loss = F.occ_lga_loss(xg, lab, class_weights().to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), xg.grad.detach().cpu()


@pytest.mark.parametrize("name", ("A", "B", "G", "K", "L"))
def test_lga_weights_are_bit_equal_to_the_reference(name):
    _, lab = case(name)
    got = F.lga_weights(lab.to(DEV))
    assert got.is_cuda and got.dtype == torch.uint8
    assert torch.equal(got.cpu(), torch.from_numpy(golden()[f"{name}_lga2"]))


def test_lga_weights_refuse_an_axis_shorter_than_two():
    with pytest.raises(ValueError):
        F.lga_weights(torch.zeros(1, 4, 1, 4, dtype=torch.uint8, device=DEV))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", FUSED_CASES + ("L",))
def test_fused_matches_float64_and_the_tensor_form(name, kind, monkeypatch):
    assert F.OCC_TAIL and F.LGA
    loss, grad = fused(name, kind)
    check(name, kind, loss, grad, "fused")
    monkeypatch.setattr(F, "LGA", False)                   # what SSBEV_LGA=0 sets at import
    tl, tg = tensor_form(name, kind, DEV)                  # dice_tensor of the up-sampled volume / pal_tensor
    check(name, kind, tl, tg, "tensor form")
    assert abs(float(loss) - float(tl)) <= loss_tol(name, kind)
    assert float((grad - tg).abs().max()) <= grad_tol(name, kind)
    if kind == "dice":
        monkeypatch.setattr(F, "OCC_TAIL", False)          # what SSBEV_OCC_TAIL=0 sets: dice_from_sums on the fused sums
        sl, sg = fused(name, kind)
        check(name, kind, sl, sg, "torch algebra on the fused sums")
        assert abs(float(loss) - float(sl)) <= loss_tol(name, kind)
        assert float((grad - sg).abs().max()) <= grad_tol(name, kind)


@pytest.mark.parametrize("kind", KINDS)
def test_nothing_labelled_gives_exact_zeros(kind, monkeypatch):
    loss, grad = fused("E", kind)
    assert float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))
    monkeypatch.setattr(F, "LGA", False)
    monkeypatch.setattr(F, "OCC_TAIL", False)
    loss, grad = fused("E", kind) if kind == "dice" else tensor_form("E", kind, DEV)
    assert float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", ("A", "B"))
def test_two_runs_give_the_same_bits(name, kind):
    l0, g0 = fused(name, kind)
    l1, g1 = fused(name, kind)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


@pytest.mark.parametrize("kind", KINDS)
def test_incoming_gradient_scale_is_applied(kind):
    _, g3 = fused("A", kind, scale=3.0)
    assert float(np.abs(g3.numpy() / 3.0 - golden()[f"A_{kind}_f64_grad"]).max()) <= grad_tol("A", kind)


def test_alpha_and_beta_reach_the_kernel(monkeypatch):
    x, lab = case("A")
    cw = class_weights().to(DEV)
    got = float(F.occ_lga_loss(x.to(DEV), lab.to(DEV), cw, alpha=2.0, beta=3.0))
    monkeypatch.setattr(F, "LGA", False)
    want = float(F.occ_lga_loss(x.to(DEV), lab.to(DEV), cw, alpha=2.0, beta=3.0))
    assert abs(got - want) <= 3.0 * loss_tol("A", "lga")   # the loss is at most 3 x the alpha = beta = 1 one


def test_occ_head_loss_with_all_eight_terms():
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    kw = dict(in_channels=[32], out_channel=20, semantic_kitti=True, norm_cfg=dict(type="GN", num_groups=8, requires_grad=True))
    x, lab = case("A")
    ids = (S.hash_uniform("dice_lga_head_ids", tuple(lab.shape), 0.0, 1.0) * 70).to(torch.uint8)   # 64..69: in no frustum
    ids[ids >= 64] = 255
    dists = (S.hash_uniform("dice_lga_head_dists", (lab.shape[0], 64, 20), 0.0, 1.0) * 50).floor()
    fr = dict(frustums_ids=ids.to(DEV), frustums_class_dists=dists.to(DEV))
    w6 = dict(voxel_ce=1, voxel_sem_scal=1, voxel_geo_scal=1, voxel_ohem=1, voxel_lovasz=1, frustum_dist=1)
    old_kw = dict(use_ohem_loss=True, use_frustum_loss=True, **kw)
    eight = OccHead(semkitti_loss_weight_cfg=dict(w6, voxel_dice=1, voxel_lga=1), use_dice_loss=True, use_lga_loss=True, **old_kw).to(DEV)
    six = OccHead(semkitti_loss_weight_cfg=w6, **old_kw).to(DEV)
    xg = x.to(DEV).requires_grad_(True)
    out = eight.loss(output_voxels=[xg], target_voxels=lab.to(DEV), **fr)
    keys = [k for k in out if k.startswith("loss")]
    assert keys == ["loss_voxel_ce_0", "loss_voxel_sem_scal_0", "loss_voxel_geo_scal_0", "loss_voxel_sem_ohem_0",
                    "loss_voxel_lovasz_0", "loss_voxel_fp_0", "loss_voxel_dice_0", "loss_voxel_lga_0"]
    sum(out[k] for k in keys).backward()
    x6 = x.to(DEV).requires_grad_(True)
    out6 = six.loss(output_voxels=[x6], target_voxels=lab.to(DEV), **fr)
    old = keys[:6]
    assert [k for k in out6 if k.startswith("loss")] == old
    for k in old:
        assert torch.equal(out6[k], out[k])
    sum(out6[k] for k in old).backward()
    for kind in KINDS:
        assert abs(float(out[f"loss_voxel_{kind}_0"].detach()) - float(golden()[f"A_{kind}_f64_loss"])) <= loss_tol("A", kind)
    # the head without the two terms on the same card gives the other six terms' gradient (bit-equal terms); 2e-6 is the existing
    # bound of a sum of the head's gradients (test_gpu_ohem.py: autograd accumulates the terms in another order)
    parts = x6.grad.cpu().numpy().astype(np.float64) + golden()["A_dice_f64_grad"] + golden()["A_lga_f64_grad"]
    err = float(np.abs(xg.grad.cpu().numpy() - parts).max())
    bound = 2e-6 + grad_tol("A", "dice") + grad_tol("A", "lga")
    print("eight-term gradient error", err, "bound", bound)
    assert err <= bound
