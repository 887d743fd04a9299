"""GPU: the lifted-point position encoder on its HIP kernels (csrc/point_xyz.hip through ``functional.point_xyz_pool``) against
tests/golden/point_xyz.npz and against the tensor form on the same card (``F.POINT_XYZ = False``, what SSBEV_POINT_XYZ=0 sets):
output, every parameter gradient and the running statistics of cases A-E, the eval-mode forward (F), exact zeros without a kept
point (G), bit reproducibility, the geometry cache, the bf16 refusal and one training step of the tiny model in both modes.
Bounds: tests/point_xyz_cases.py (the same for the fused path and the tensor form)."""
import numpy as np
import pytest
import torch

import point_xyz_cases as X
from stereoscene_amd import functional as F, synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
QS = ["P", "rm", "rv"] + list(X.GRADS.values())


def counted(monkeypatch):
    calls = []
    real = F._PointXyzSum.apply
    monkeypatch.setattr(F._PointXyzSum, "apply", lambda *a: (calls.append(1), real(*a))[1])
    return calls


@pytest.mark.parametrize("name", X.TRAINED + ("F",))
def test_fused_path_matches_the_fixture_and_the_tensor_form(name, monkeypatch):
    calls = counted(monkeypatch)
    got = X.run(name, DEV, fused=True)
    assert calls == [1]                                    # the native path ran
    X.check(name, got, "fused")
    monkeypatch.setattr(F, "POINT_XYZ", False)
    plain = X.run(name, DEV, fused=True)                   # the same call takes the tensor form
    monkeypatch.setattr(F, "POINT_XYZ", True)
    assert calls == [1]
    X.check(name, plain, "tensor form on the card")
    training = X.case(name)["training"]
    assert got["nbt"] == plain["nbt"] == (1 if training else 7)
    if training:
        assert not got["g0b"].any()                        # exactly 0: BatchNorm removes the mean
    else:
        st = X.case(name)["state"]
        assert torch.equal(got["rm"], st["1.running_mean"]) and torch.equal(got["rv"], st["1.running_var"])


def test_no_kept_point_gives_exact_zeros_without_a_read_back():
    X.run("G", DEV, fused=True)                            # lazy initialisation (library load) may synchronise once
    c = X.case("G")
    geom = c["geom"].to(DEV)
    tables = F.lift_splat_tables(geom, None, None, None, grid_host=c["grid_host"])
    p = X.params_of("G", DEV)
    Gd = c["G"].to(DEV)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")                # any host read-back of a device value raises
    try:
        P = F.point_xyz_pool(geom, tables, c["cfg"]["pc_range"], c["grid_host"][2], p["0.weight"], p["0.bias"], p["1.weight"],
                             p["1.bias"], p["3.weight"], p["3.bias"], p["1.running_mean"], p["1.running_var"],
                             p["1.num_batches_tracked"], training=True)
        (P * Gd).sum().backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert not P.any() and tuple(P.shape) == (1, 16, 16, 16, 4)
    for k in X.GRADS:
        assert p[k].grad is not None and not p[k].grad.any(), k
    assert int(p["1.num_batches_tracked"]) == 0 and not p["1.running_mean"].any() and torch.equal(p["1.running_var"].cpu(), torch.ones(8))


@pytest.mark.parametrize("name", ("B", "C", "E"))
def test_two_runs_give_the_same_bits(name):
    a, b = X.run(name, DEV, fused=True), X.run(name, DEV, fused=True)
    for q in QS:
        assert torch.equal(a[q], b[q]), q


def test_incoming_gradient_scale_is_applied():
    got = X.run("A", DEV, fused=True, scale=3.0)
    X.check("A", got, "fused, gradient x 3", scale=3.0)


def test_moments_kernel_matches_the_tensor_form_and_repeats():
    for name in ("B", "E", "G"):
        c = X.case(name)
        geom, vox = c["geom"].to(DEV), X.vox_of(name).to(DEV)
        m0 = F.point_xyz_moments(geom, vox, c["cfg"]["pc_range"], c["grid_host"][2])
        m1 = F.point_xyz_moments(geom, vox, c["cfg"]["pc_range"], c["grid_host"][2])
        want = F.point_xyz_moments_tensor(c["geom"], X.vox_of(name), c["cfg"]["pc_range"])
        assert m0.is_cuda and m0.dtype == torch.float64 and torch.equal(m0, m1)
        assert float(m0[0]) == float(want[0]) == float(X.golden()[f"{name}_n_kept"])
        assert float((m0.cpu() - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


def vt_kwargs(**kw):
    grid = S.grid_config(S.CFG_T)
    return dict(loss_depth_weight=1.0, grid_config=grid, data_config=dict(input_size=tuple(S.CFG_T["input_size"])), numC_input=32,
                numC_Trans=16, downsample=8, cam_channels=30, point_cloud_range=list(S.CFG_T["pc_range"]), **kw)


def test_geometry_cache_gives_the_same_bits_on_consecutive_calls():
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel as VT
    vt = VT(point_xyz_channel=16, **vt_kwargs()).to(DEV).train()
    vt.point_xyz_encoder.load_state_dict(X.case("A")["state"])
    calib = [t.to(DEV) for t in S.frustum_view(S.CFG_T)[1:]]

    def xyz():
        tables = vt._cached_tables(*calib)
        geom, moments = vt._xyz_geo
        return vt.point_xyz_pool(geom, tables, moments).detach().clone(), moments

    fresh, m_fresh = xyz()
    vt.geometry_cache = True
    first, m1 = xyz()
    second, m2 = xyz()
    assert m1 is m2 and m1 is not m_fresh and torch.equal(m1, m_fresh)          # kept with the cached tables
    assert torch.equal(fresh, first) and torch.equal(first, second)
    assert int(vt.point_xyz_encoder[1].num_batches_tracked) == 3
    got, empty = X.rows("A", fresh)
    assert not empty.any() and float(np.abs(got - X.golden()["A_f64_P"]).max()) <= X.tol("A", "P")


def test_bf16_storage_is_refused():
    c = X.case("A")
    geom = c["geom"].to(DEV)
    tables = F.lift_splat_tables(geom, None, None, None, grid_host=c["grid_host"])
    p = X.params_of("A", DEV)
    F.set_precision("bf16")
    try:
        with pytest.raises(NotImplementedError, match="fp32"):
            F.point_xyz_pool(geom, tables, c["cfg"]["pc_range"], c["grid_host"][2], p["0.weight"], p["0.bias"], p["1.weight"],
                             p["1.bias"], p["3.weight"], p["3.bias"], p["1.running_mean"], p["1.running_var"], None)
    finally:
        F.set_precision("fp32")


@pytest.mark.parametrize("mode", ("cat", "add"))
def test_forward_train_step_of_the_tiny_model(mode):
    from stereoscene_amd import model_zoo
    cfg = S.CFG_T
    smp = S.synthetic_sample(cfg, B=1, tag="point_xyz_step")
    gt = smp["gt_occ"].to(DEV)
    model = model_zoo.build_detector(cfg, point_xyz_channel=16, point_xyz_mode=mode).train()
    enc = model.img_view_transformer.point_xyz_encoder
    assert enc[3].out_features == (16 if mode == "cat" else 128)
    losses = model.forward_train(img_inputs=model_zoo.img_inputs_from_sample(smp), gt_occ=gt)
    sum(v for k, v in losses.items() if k.startswith("loss")).backward()
    assert all(torch.isfinite(v).all() for k, v in losses.items() if k.startswith("loss"))
    for n, p in enc.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        assert (float(p.grad.abs().max()) > 0) == (n != "0.bias"), n
    assert int(enc[1].num_batches_tracked) == 1
