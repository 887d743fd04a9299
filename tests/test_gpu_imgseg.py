"""GPU: the fused image-view segmentation loss (csrc/imgseg.hip ``ssbev_imgseg_ce_*`` through ``functional.imgseg_loss``) against
the reference's fp32 results / the float64 restatement of tests/golden/imgseg.npz and against the tensor form on the same card,
and the ``imgseg=True`` training step.  Bounds as in tests/test_imgseg.py: 8 x the case's recorded reference-vs-float64 spread
(never below the fp32 unit roundoff) for the loss and for EVERY element of the gradient.  Gradient rows of cells without a valid
pixel are exactly 0."""
import numpy as np
import pytest
import torch

from stereoscene_amd import functional as F, synthetic as S
from test_imgseg import case, check, class_weights, empty_cells, golden, grad_tol, loss_tol

pytestmark = pytest.mark.gpu
DEV = "cuda"


def run(name, scale=1.0, weight=1.0, labels=None, channels_last=False):
    logits, lab = case(name)
    lab = (lab if labels is None else labels).to(DEV)
    x = logits.to(DEV)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
        assert not x.is_contiguous()
    x.requires_grad_(True)
    loss = F.imgseg_loss(x, lab, class_weights().to(DEV), weight)
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), x.grad.detach().cpu()


@pytest.mark.parametrize("name", ("A", "B", "D", "E"))
def test_fused_matches_the_fixture_and_the_tensor_form(name, monkeypatch):
    assert F.IMGSEG
    loss, grad = run(name)
    check(name, loss, grad, "fused")
    monkeypatch.setattr(F, "IMGSEG", False)               # what SSBEV_IMGSEG=0 sets at import
    tl, tg = run(name)
    check(name, tl, tg, "tensor form on the card")
    terr = float((grad - tg).abs().max())
    print(name, "fused vs tensor form: loss", float(loss) - float(tl), "gradient", terr)
    assert abs(float(loss) - float(tl)) <= loss_tol(name)
    assert terr <= grad_tol(name)


def test_cells_without_a_valid_pixel_get_exact_zeros():
    for name in ("A", "D"):
        _, grad = run(name)
        empty = empty_cells(name).unsqueeze(1).expand_as(grad)
        assert empty.any() and not empty.all()
        assert torch.equal(grad[empty], torch.zeros_like(grad[empty]))
        assert float(grad[~empty].abs().max()) > 0.0


def test_no_valid_pixel_gives_exact_zeros():
    loss, grad = run("C")
    assert torch.isfinite(loss) and float(loss) == 0.0
    assert torch.equal(grad, torch.zeros_like(grad))


def test_two_runs_give_the_same_bits():
    l0, g0 = run("B")
    l1, g1 = run("B")
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_channels_last_logits_and_int64_labels_give_the_same_bits():
    l0, g0 = run("B")
    l1, g1 = run("B", channels_last=True)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    l2, g2 = run("B", labels=case("B")[1].long())
    assert torch.equal(l0, l2) and torch.equal(g0, g2)


def test_labels_outside_the_classes_are_ignored():
    lab = case("A")[1]
    bad = lab.clone()
    unl = lab == 0
    bad[unl & (S.hash_uniform("imgseg_bad", lab.shape, 0.0, 1.0) < 0.1)] = 20.0
    bad[0, 0, 0], bad[0, 0, 1], bad[1, 3, 3], bad[1, 47, 79] = 255.0, -3.0, float("nan"), 1e30
    assert unl[0, 0, 0] and unl[0, 0, 1] and unl[1, 3, 3] and unl[1, 47, 79]
    l0, g0 = run("A")
    l1, g1 = run("A", labels=bad)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)
    ints = lab.long()
    ints[bad == 20.0] = 20
    ints[0, 0, 0], ints[0, 0, 1], ints[1, 3, 3], ints[1, 47, 79] = 255, -3, -(1 << 40), 1 << 40
    l2, g2 = run("A", labels=ints)
    assert torch.equal(l0, l2) and torch.equal(g0, g2)


def test_incoming_gradient_scale_and_weight_are_applied():
    l1, g1 = run("B")
    _, g3 = run("B", scale=3.0)
    assert float((g3 - 3.0 * g1).abs().max()) <= 1e-6 * float(g1.abs().max())
    assert float(np.abs(g3.double().numpy() / 3.0 - golden()["B_ref_grad"]).max()) <= grad_tol("B")
    lw, gw = run("B", weight=0.25)                         # powers of two: exact
    assert float(lw) == 0.25 * float(l1) and torch.equal(gw, 0.25 * g1)


def test_fused_path_never_holds_the_upsampled_logits(monkeypatch):
    logits, lab = case("E")
    BN, K, h, w = logits.shape
    H, W = lab.shape[1:]
    upsampled = BN * K * H * W * 4                         # the tensor the fused path exists to avoid
    x, lab, cw = logits.to(DEV).requires_grad_(True), lab.to(DEV), class_weights().to(DEV)

    def rise():
        x.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        F.imgseg_loss(x, lab, cw).backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    fused = rise()
    monkeypatch.setattr(F, "IMGSEG", False)
    tensor = rise()
    print("peak memory above the inputs: fused", fused, "tensor form", tensor, "up-sampled logits", upsampled)
    assert fused < upsampled
    assert tensor > upsampled


def _step(model, smp, **extra):
    from stereoscene_amd import model_zoo
    inputs = model_zoo.img_inputs_from_sample(smp)
    torch.manual_seed(0)                                   # ASPP's dropout draws from the global generator
    losses = model.forward_train(img_inputs=inputs, gt_occ=smp["gt_occ"].to(DEV), **extra)
    return inputs, losses


def test_one_training_step_with_the_segmentation_branch():
    from stereoscene_amd import model_zoo
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1)
    _, plain = _step(model_zoo.build_detector(cfg), smp)
    model = model_zoo.build_detector(cfg, imgseg=True, loss_seg_weight=0.5)
    vt = model.img_view_transformer
    assert vt.imgseg and model.imgseg_labels == "img_seg"
    with pytest.raises(KeyError, match="img_seg"):
        _step(model, smp)
    _, losses = _step(model, smp, img_seg=smp["img_seg"].to(DEV))
    keys = list(losses)
    assert keys[:2] == ["loss_depth", "loss_imgseg"] and [k for k in keys if k != "loss_imgseg"] == list(plain)
    fH, fW = (v // cfg["downsample"] for v in cfg["input_size"])
    assert vt.forward_dic["imgseg_logits"].shape == (1, 20, fH, fW)
    ls = float(losses["loss_imgseg"].detach())
    assert np.isfinite(ls) and ls > 0.0
    for k in plain:                                        # the branch leaves every other loss alone
        assert abs(float(losses[k].detach()) - float(plain[k].detach())) <= 1e-4 * max(1.0, abs(float(plain[k].detach()))), k
    sum(v for k, v in losses.items() if k.startswith("loss")).backward()
    params = dict(vt.img_seg_head.named_parameters())
    assert len(params) == 2 * 6 + 2
    for n, p in params.items():
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0.0, n
    left = model_zoo.build_detector(cfg, imgseg=True, imgseg_labels="img_seg_left")
    with pytest.raises(KeyError, match="img_seg_left"):
        _step(left, smp, img_seg=smp["img_seg"].to(DEV))
    _, ll = _step(left, smp, img_seg_left=smp["img_seg"].to(DEV))
    assert abs(float(ll["loss_imgseg"].detach()) - 2.0 * ls) <= 1e-5 * ls      # loss_seg_weight 1.0 against 0.5


def test_one_training_step_lifting_the_class_probabilities():
    from stereoscene_amd import model_zoo
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1)
    model = model_zoo.build_detector(cfg, numC_Trans=64, imgseg=True, lift_with_imgseg=True)
    vt = model.img_view_transformer
    seen = {}
    hooks = [vt.register_forward_hook(lambda m, i, o: seen.update(bev=o[0], depth=o[1])),
             vt.depth_net.register_forward_hook(lambda m, i, o: seen.update(y=o))]
    inputs, losses = _step(model, smp, img_seg=smp["img_seg"].to(DEV))
    for hk in hooks:
        hk.remove()
    total = sum(v for k, v in losses.items() if k.startswith("loss"))
    assert torch.isfinite(total)
    total.backward()
    assert all(torch.isfinite(p.grad).all() for p in model.parameters() if p.grad is not None)
    assert all(p.grad is not None and float(p.grad.abs().max()) > 0.0 for p in vt.img_seg_head.parameters())
    bev = seen["bev"].detach()
    assert bev.shape[1] == 84
    with torch.no_grad():                                  # the reference-shaped entry on the same inputs (VT:512-523)
        feat = torch.cat((seen["y"][:, vt.D:vt.D + 64].float(), torch.softmax(vt.forward_dic["imgseg_logits"].float(), dim=1)), dim=1)
        depth = seen["depth"]
        B, N = 1, 1
        volume = (depth.unsqueeze(1) * feat.unsqueeze(2)).view(B, N, 84, vt.D, *depth.shape[-2:]).permute(0, 1, 3, 4, 5, 2)
        want = vt.voxel_pooling(vt.get_geometry(*inputs[0][1:7]), volume.contiguous())
    err = float((bev - want).abs().max())
    print("lifted 84-channel BEV against voxel_pooling: max error", err, "max |ref|", float(want.abs().max()))
    assert want.shape == bev.shape and float(want[:, 64:].abs().max()) > 0.0
    assert err <= 2e-4 * max(1.0, float(want.abs().max()))
