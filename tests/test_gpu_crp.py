"""GPU: the 3-D context relation prior on its HIP kernels (csrc/crp.hip) against tests/golden/crp.npz: the label down-sampling
(byte-exact), the fused relation loss against float64 and against the tensor form on the same card, the relation gather (forward
and both gradients) against a float64 ``bmm`` restatement and against ``SSBEV_CRP=0``, the whole ``CPMegaVoxels`` block against
the reference's float64 record, and one training step of the tiny model with ``crp3d=True``.

Bounds.  Loss: as in tests/test_crp.py against float64; fused against tensor form within twice that (each side may use its whole
bound).  Gather: K * max(the case's recorded spread of the reference's own fp32 ops against float64, 2^-23) * max|float64 result| on
EVERY element of the output and of both gradients; fused against tensor form within twice that.  Block: K * max(recorded spread,
2^-23) * max|float64 record| on every element of x, P_logits and the input gradient."""
import numpy as np
import pytest
import torch

from stereoscene_amd import functional as F, synthetic as S
from test_crp import EPS, K, LOSS_CASES, check, down_case, golden, grad_tol, loss_case, loss_tol, tensor_form

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.mark.parametrize("name", tuple(S.CRP_DOWNSAMPLE_CASES))
def test_downsample_kernel_is_byte_equal_to_the_reference(name):
    lab, ds = down_case(name)
    out = F.label_downsample(lab.to(DEV), ds)
    assert out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), golden()[f"{name}_down"])


def fused_loss(name, scale=1.0):
    x, lab = loss_case(name)
    xg = x.to(DEV).requires_grad_(True)
    assert F.CRP and F.relation_loss_supported(xg, lab.to(DEV))
    loss = F.relation_loss(xg, lab.to(DEV))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    (scale * loss).backward()
    return loss.detach().cpu(), xg.grad.detach().cpu()


@pytest.mark.parametrize("name", LOSS_CASES)           # E: two 256-wide column chunks, 72 row chunks
def test_fused_loss_matches_float64_and_the_tensor_form(name, monkeypatch):
    calls = []
    real = F._RelationLoss.apply
    monkeypatch.setattr(F._RelationLoss, "apply", lambda *a: (calls.append(1), real(*a))[1])
    loss, grad = fused_loss(name)
    assert calls == [1]                                    # the native path ran
    check(name, loss, grad, "fused")
    monkeypatch.setattr(F, "CRP", False)                   # what SSBEV_CRP=0 sets at import
    tl, tg = tensor_form(name, DEV)
    monkeypatch.setattr(F, "CRP", True)
    assert calls == [1]
    check(name, tl, tg, "tensor form")
    assert abs(float(loss) - float(tl)) <= 2.0 * loss_tol(name)
    assert float((grad - tg).abs().max()) <= 2.0 * grad_tol(name)


@pytest.mark.parametrize("name", ("C", "E"))
def test_two_runs_of_the_loss_give_the_same_bits(name):
    l0, g0 = fused_loss(name)
    l1, g1 = fused_loss(name)
    assert torch.equal(l0, l1) and torch.equal(g0, g1)


def test_zero_positive_relation_is_finite_without_a_read_back():
    x, lab = loss_case("B")
    xg, lg = x.to(DEV).requires_grad_(True), lab.to(DEV)
    F.relation_loss(xg.detach(), lg)                       # lazy initialisation (library load) may synchronise once
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                # any host read-back of a device value raises
    try:
        loss = F.relation_loss(xg, lg)
        loss.backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.isfinite(loss) and torch.isfinite(xg.grad).all()
    check("B", loss.detach().cpu(), xg.grad.cpu(), "fused, no read-back")


def test_incoming_gradient_scale_is_applied():
    _, g3 = fused_loss("A", scale=3.0)
    assert float(np.abs(g3.numpy() / 3.0 - golden()["LA_f64_grad"]).max()) <= grad_tol("A")


def test_labels_on_the_host_are_moved_to_the_logits_device():
    x, lab = loss_case("A")
    l0, _ = fused_loss("A")
    assert torch.equal(F.relation_loss(x.to(DEV), lab).cpu(), l0)


# ---------------------------------------------------------------------------------------------------------------- gather
def gather_f64(name):
    """float64 restatement on the host: (out, dP, dctx, dx)."""
    P, ctx, x, g = S.crp_gather_case(name)
    p, c = P.double().requires_grad_(True), ctx.double().requires_grad_(True)
    xx = None if x is None else x.double().requires_grad_(True)
    B, R, Mc, N = P.shape
    rels = [torch.bmm(torch.sigmoid(p[:, r]).transpose(1, 2), c).transpose(1, 2) for r in range(R)]      # [B, C2, N] each
    out = torch.cat(([xx] if xx is not None else []) + rels, dim=1)
    (out * g.double()).sum().backward()
    return out.detach(), p.grad, c.grad, (None if xx is None else xx.grad)


def gather_run(name):
    P, ctx, x, g = S.crp_gather_case(name)
    p, c = P.to(DEV).requires_grad_(True), ctx.to(DEV).requires_grad_(True)
    xx = None if x is None else x.to(DEV).requires_grad_(True)
    out = F.relation_gather(p, c, xx)
    (out * g.to(DEV)).sum().backward()
    return out.detach().cpu(), p.grad.cpu(), c.grad.cpu(), (None if xx is None else xx.grad.cpu())


@pytest.mark.parametrize("name", tuple(S.CRP_GATHER_CASES))
def test_relation_gather_matches_float64_and_the_tensor_form(name, monkeypatch):
    calls = []
    real = F._RelationGather.apply
    monkeypatch.setattr(F._RelationGather, "apply", lambda *a: (calls.append(1), real(*a))[1])
    fused = gather_run(name)
    assert calls == [1]                                    # the native path ran
    monkeypatch.setattr(F, "CRP", False)
    plain = gather_run(name)
    monkeypatch.setattr(F, "CRP", True)
    assert calls == [1]
    want = gather_f64(name)
    Cin = S.CRP_GATHER_CASES[name][5]
    for k, tag in enumerate(("out", "dP", "dctx")):
        ref = want[k][:, Cin:] if tag == "out" else want[k]
        tol = K * max(float(golden()[f"G{name}_spread_{tag}"]), EPS) * float(ref.abs().max())
        for what, got in (("fused", fused[k]), ("tensor form", plain[k])):
            got = got[:, Cin:] if tag == "out" else got
            err = float((got.double() - ref).abs().max())
            print(name, tag, what, "max error", err, "bound", tol)
            assert torch.isfinite(got).all() and err <= tol, (name, tag, what)
        a, b = (fused[k][:, Cin:], plain[k][:, Cin:]) if tag == "out" else (fused[k], plain[k])
        assert float((a - b).abs().max()) <= 2.0 * tol
    if Cin:                                                # x passes through, and so does its gradient
        _, _, x, g = S.crp_gather_case(name)
        assert torch.equal(fused[0][:, :Cin], x) and torch.equal(fused[3], g[:, :Cin])


def test_two_runs_of_the_gather_give_the_same_bits():
    a, b = gather_run("X"), gather_run("X")
    assert all(torch.equal(u, v) for u, v in zip(a[:3], b[:3]))


# ---------------------------------------------------------------------------------------------------------------- block
def test_block_matches_the_reference_record():
    from stereoscene_amd.plugin.crp3d import CPMegaVoxels
    g = golden()
    blk = CPMegaVoxels(S.CRP_BLOCK["feature"], S.CRP_BLOCK["size"], bn_momentum=0.1)
    blk.load_state_dict({k[len("blk_sd/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("blk_sd/")}, strict=True)
    blk = blk.to(DEV).train()
    x, wx, wp = S.crp_block_case()
    xi = x.to(DEV).requires_grad_(True)
    out = blk(xi)
    assert tuple(out["P_logits"].shape) == (2, 4, 4, 32) and tuple(out["x"].shape) == tuple(x.shape)
    ((out["x"] * wx.to(DEV)).sum() + (out["P_logits"] * wp.to(DEV)).sum()).backward()
    for tag, got in (("x", out["x"]), ("P", out["P_logits"]), ("gin", xi.grad)):
        ref = torch.from_numpy(g[f"blk_f64_{tag}"])
        tol = K * max(float(g[f"blk_{tag}_spread"]), EPS) * float(ref.abs().max())
        err = float((got.detach().cpu().double() - ref).abs().max())
        print("block", tag, "max error", err, "bound", tol)
        assert err <= tol, tag
    sd = blk.state_dict()
    for k, v in g.items():                                 # running statistics after one training forward
        if k.startswith("blk_run/"):
            key = k[len("blk_run/"):]
            used = not any(s in key for s in ("downsample2", "downsample3", "downsample4"))
            before = torch.from_numpy(g["blk_sd/" + key])
            now = sd[key].cpu()
            assert torch.equal(now, before) != used, key
            assert float((now - torch.from_numpy(v)).abs().max()) <= 1e-4 * max(1.0, float(np.abs(v).max())), key
    assert int(sd["aspp.bn1.0.num_batches_tracked"]) == 1


def test_bf16_storage_is_refused():
    from stereoscene_amd.plugin.crp3d import CPMegaVoxels
    blk = CPMegaVoxels(8, (4, 4, 2)).to(DEV)
    with pytest.raises(NotImplementedError, match="fp32"):
        blk(torch.zeros(1, 8, 4, 4, 2, device=DEV, dtype=torch.bfloat16))


# ---------------------------------------------------------------------------------------------------------------- one step
def test_forward_train_step_of_the_tiny_model():
    from stereoscene_amd import model_zoo, pipelines as P
    from stereoscene_amd.plugin import losses as L
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1, tag="crp_step")
    gt = smp["gt_occ"].to(DEV)
    step = P.CreateRelationLabels(cfg["pc_range"], list(cfg["occ_size"]), L.KITTI_CLASS_NAMES, relations=True, relation_downscale=4)
    res = step(dict(gt_occ=gt[0].to(torch.uint8), img_inputs=[t[0] for t in S.frustum_view(cfg)]))
    labels = res["CP_mega_labels"]
    assert labels.is_cuda and tuple(labels.shape) == (8, 8, 2)
    assert torch.equal(labels.cpu(), F.label_downsample(gt[0].to(torch.uint8).cpu(), 4))
    model = model_zoo.build_detector(cfg, crp3d=True, crp_level=1).train()
    crp = model.img_bev_encoder_backbone.CP_mega_voxels

    def run():
        model.zero_grad()
        losses = model.forward_train(img_inputs=model_zoo.img_inputs_from_sample(smp), gt_occ=gt, CP_mega_labels=labels[None])
        sum(v for k, v in losses.items() if k.startswith("loss")).backward()
        return losses
    losses = run()
    assert "loss_rel_ce" in losses and torch.isfinite(losses["loss_rel_ce"]) and float(losses["loss_rel_ce"]) > 0
    unused = ("downsample2", "downsample3", "downsample4")
    for n, p in crp.named_parameters():
        if any(u in n for u in unused):                    # the stride != 1 shortcuts: parameters only
            assert p.grad is None, n
            continue
        assert p.grad is not None and torch.isfinite(p.grad).all() and float(p.grad.abs().max()) > 0, n
    again = run()
    assert torch.isfinite(again["loss_rel_ce"])
    with pytest.raises(KeyError, match="relations=True"):
        model.forward_train(img_inputs=model_zoo.img_inputs_from_sample(smp), gt_occ=gt)
