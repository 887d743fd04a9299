"""GPU: the fused Gaussian KL depth loss (csrc/lidar_depth.hip ``ssbev_depth_kld_*`` through ``functional.depth_kld_loss``)
against the reference's fp32 results / the float64 restatement of tests/golden/depth_kld.npz and against the tensor form on the
same card.  Bounds as in tests/test_depth_kld.py: 8 x the case's recorded reference-vs-float64 spread (never below the fp32 unit
roundoff) for the loss and for EVERY element of the gradient; the factor covers another erf / log and another summation order on
the device.  Background rows of the gradient are exactly 0."""
import numpy as np
import pytest
import torch

from stereoscene_amd import functional as F, synthetic as S
from test_depth_kld import case, check, golden, grad_tol, loss_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(name, scale=1.0, weight=1.0):
    gt, pred, ds, dbound, units = case(name)
    p = pred.to(DEV).requires_grad_(True)
    loss = F.depth_kld_loss(gt.to(DEV), p, ds, dbound, weight, 0.5, units)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), p.grad.detach().cpu()


@pytest.mark.parametrize("name", ("A", "B", "D", "E"))
def test_fused_matches_the_fixture_and_the_tensor_form(name, monkeypatch):
    assert F.DEPTH_KLD
    loss, grad = run(name)
    check(name, loss, grad, "fused")
    monkeypatch.setattr(F, "DEPTH_KLD", False)            # what SSBEV_DEPTH_KLD=0 sets at import
    tl, tg = run(name)
    check(name, tl, tg, "tensor form on the card")
    terr = float((grad - tg).abs().max())
    print(name, "fused vs tensor form: loss", float(loss) - float(tl), "gradient", terr)
    assert abs(float(loss) - float(tl)) <= loss_tol(name)
    assert terr <= grad_tol(name)


def test_no_foreground_row_gives_exact_zeros():
    loss, grad = run("C")
    assert torch.isfinite(loss) and float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


def test_two_runs_give_the_same_bits():
    l0, g0 = run("B")
    l1, g1 = run("B")
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_incoming_gradient_scale_and_weight_are_applied():
    l1, g1 = run("B")
    _, g3 = run("B", scale=3.0)
    assert float((g3 - 3.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    assert float(np.abs(g3.double().numpy() / 3.0 - golden()["B_ref_grad"]).max()) <= grad_tol("B")
    lw, gw = run("B", weight=0.25)                         # powers of two: exact
    assert float(lw) == 0.25 * float(l1) and torch.equal(gw, 0.25 * g1)


def test_one_training_step_with_the_kld_depth_loss():
    from stereoscene_amd import model_zoo
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1)
    keys = {}
    for kind in ("kld", "bce"):
        model = model_zoo.build_detector(cfg, loss_depth_type=kind)
        inputs = model_zoo.img_inputs_from_sample(smp)
        losses = model.forward_train(img_inputs=inputs, gt_occ=smp["gt_occ"].to(DEV))
        keys[kind] = list(losses)
        if kind == "bce":
            break
        assert model.img_view_transformer.loss_depth_type == "kld"
        ld = float(losses["loss_depth"].detach())
        assert np.isfinite(ld) and ld > 0.0
        sum(v for k, v in losses.items() if k.startswith("loss")).backward()
        grads = [p.grad for p in model.img_view_transformer.depth_net.parameters() if p.grad is not None]
        assert grads and all(torch.isfinite(g).all() for g in grads)
        assert any(float(g.abs().max()) > 0.0 for g in grads)
    assert keys["kld"] == keys["bce"]
