"""CPU: the lifted-point position encoder (``point_xyz_channel``) in its tensor form (functional.point_xyz_pool_tensor) against
the reference-order fp32 results and the float64 restatement of tests/golden/point_xyz.npz, the moment identity the fused path
rests on, the constructor rules and state-dict names of ``ViewTransformerLiftSplatShootVoxel``, the ``model_zoo`` wiring, a CPU
forward, and the host-side checks of the C entry points.  Bounds: tests/point_xyz_cases.py."""
import ctypes as C
import os
import zlib

import numpy as np
import pytest
import torch

import point_xyz_cases as X
from stereoscene_amd import capi, functional as F, synthetic as S


def vt_kwargs(**kw):
    grid = S.grid_config(S.CFG_T)
    return dict(loss_depth_weight=1.0, grid_config=grid, data_config=dict(input_size=tuple(S.CFG_T["input_size"])), numC_input=32,
                numC_Trans=16, downsample=8, cam_channels=30, **kw)


def VT(**kw):
    from stereoscene_amd.plugin.view_transformer import ViewTransformerLiftSplatShootVoxel
    return ViewTransformerLiftSplatShootVoxel(**vt_kwargs(**kw))


RANGE = list(S.CFG_T["pc_range"])


def test_fixture_has_something_to_check():
    g = X.golden()
    for name in S.POINT_XYZ_CASES:
        assert int(g[f"{name}_geom_crc"]) == zlib.crc32(X.case(name)["geom"].numpy().tobytes()), name
        assert int(g[f"{name}_n_kept"]) == int((X.vox_of(name) >= 0).sum()), name
    for name in X.TRAINED:
        for q in ["P", "rm", "rv"] + list(X.GRADS.values()):
            assert float(g[f"{name}_spread_{q}"]) < 2e-5 and (q == "g0b" or np.abs(g[f"{name}_f64_{q}"]).max() > 0), (name, q)
    assert int(g["E_max_list"]) > 256 and int(g["A_max_list"]) <= 32 and int(g["B_max_list"]) > 32 and int(g["G_n_kept"]) == 0
    assert X.case("C")["Cxyz"] == 128 and X.case("D")["Cxyz"] == 8 and X.case("E")["Cxyz"] == 24 and X.case("B")["B"] == 2
    assert os.path.getsize(X.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", X.TRAINED + ("F",))
def test_tensor_form_matches_the_fixture(name):
    got = X.run(name, "cpu", fused=False)
    X.check(name, got, "tensor form")
    assert got["nbt"] == (1 if X.case(name)["training"] else 7)
    if not X.case(name)["training"]:
        st = X.case(name)["state"]
        assert torch.equal(got["rm"], st["1.running_mean"]) and torch.equal(got["rv"], st["1.running_var"])


def test_no_kept_point_gives_zeros_zero_gradients_and_untouched_statistics():
    got = X.run("G", "cpu", fused=False)
    assert not got["P"].any() and tuple(got["P"].shape) == (1, 16, 16, 16, 4)
    for q in X.GRADS.values():
        assert not got[q].any()
    assert got["nbt"] == 0 and not got["rm"].any() and torch.equal(got["rv"], torch.ones(8))


@pytest.mark.parametrize("name", ("A", "B", "E"))
def test_moments_give_the_batch_statistics(name):
    c = X.case(name)
    vox = X.vox_of(name)
    m = F.point_xyz_moments_tensor(c["geom"], vox, c["cfg"]["pc_range"])
    w1, b1 = c["state"]["0.weight"], c["state"]["0.bias"]
    n, ubar, cov, mu, var = F.point_xyz_stats(m, w1, b1)
    h = F.point_xyz_unit(c["geom"], c["cfg"]["pc_range"])[vox >= 0].double() @ w1.double().t() + b1.double()
    assert int(n) == h.shape[0] == int(X.golden()[f"{name}_n_kept"])
    assert float(((mu - h.mean(0)).abs() / h.abs().max(0).values).max()) <= 1e-12
    assert float(((var - h.var(0, unbiased=False)) / h.var(0, unbiased=False)).abs().max()) <= 1e-12


def test_voxel_index_tensor_is_the_truncating_rule():
    geom = torch.tensor([[[0.0, 0.0, 0.0], [-0.3, 0.0, 0.0], [-0.5, 0.0, 0.0], [1.99, 0.99, 0.5], [2.0, 0.0, 0.0], [float("nan"), 0, 0]],
                         [[1.5, 0.5, 0.25], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -0.49], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]]])
    vox = F.voxel_index_tensor(geom, [0.0, 0.0, 0.0], [0.5, 0.5, 0.5], [4, 2, 2])
    assert vox.dtype == torch.int32 and vox.tolist() == [0, 0, -1, 15, -1, -1, 16 + 12 + 2, -1, -1, 16, 16, 16]


def test_constructor_rules():
    assert VT().point_xyz_channel == 0 and not hasattr(VT(), "point_xyz_encoder")
    vt = VT(point_xyz_channel=24, point_cloud_range=RANGE)
    assert vt.point_xyz_channel == 24 and vt.point_xyz_mode == "cat" and vt.point_xyz_encoder[0].out_features == 12
    assert VT(point_xyz_channel=8, point_xyz_mode="add", point_cloud_range=RANGE).point_xyz_channel == 16      # numC_Trans
    assert VT(point_xyz_channel=3, point_xyz_mode="add", point_cloud_range=RANGE).point_xyz_channel == 16
    for bad in (3, 4, 12, 20, 520):
        with pytest.raises(NotImplementedError, match="multiple of 8"):
            VT(point_xyz_channel=bad, point_cloud_range=RANGE)
    with pytest.raises(NotImplementedError, match="multiple of 8"):
        VT(point_xyz_channel=3)                                      # the width rule comes first (tests/test_imgseg.py)
    for other in (dict(use_voxel_net=True), dict(vp_megvii=True)):
        with pytest.raises(NotImplementedError):
            VT(point_xyz_channel=16, point_cloud_range=RANGE, **other)
    with pytest.raises(ValueError, match="point_cloud_range"):
        VT(point_xyz_channel=16)
    with pytest.raises(ValueError, match="point_cloud_range"):
        VT(point_xyz_channel=16, point_cloud_range=RANGE[:3])
    with pytest.raises(ValueError, match="point_xyz_mode"):
        VT(point_xyz_channel=16, point_xyz_mode="mul", point_cloud_range=RANGE)
    with pytest.raises(ValueError, match="lift_with_imgseg"):
        VT(point_xyz_channel=16, point_xyz_mode="add", point_cloud_range=RANGE, imgseg=True, lift_with_imgseg=True)
    VT(point_xyz_channel=16, point_xyz_mode="cat", point_cloud_range=RANGE, imgseg=True, lift_with_imgseg=True)
    VT(point_xyz_channel=16, point_xyz_mode="add", point_cloud_range=RANGE, imgseg=True)


def test_state_dict_keys_are_the_reference_names():
    plain = list(VT().state_dict())
    assert not any("point_xyz" in k for k in plain)
    vt = VT(point_xyz_channel=16, point_cloud_range=RANGE)
    sd = vt.state_dict()
    assert [k for k in sd if not k.startswith("point_xyz_encoder.")] == plain
    assert [k for k in sd if k.startswith("point_xyz_encoder.")] == [
        "point_xyz_encoder." + k for k in ("0.weight", "0.bias", "1.weight", "1.bias", "1.running_mean", "1.running_var",
                                           "1.num_batches_tracked", "3.weight", "3.bias")]
    assert sd["point_xyz_encoder.0.weight"].shape == (8, 3) and sd["point_xyz_encoder.3.weight"].shape == (16, 8)
    ref = {"point_xyz_encoder." + k: v for k, v in X.case("A")["state"].items()}          # a checkpoint with the reference's keys
    vt.load_state_dict({**VT().state_dict(), **ref}, strict=True)
    assert torch.equal(vt.point_xyz_encoder[3].bias, ref["point_xyz_encoder.3.bias"])


def test_model_cfg_wiring():
    from stereoscene_amd import model_zoo
    base = model_zoo.model_cfg(S.CFG_T)
    assert "point_xyz_channel" not in base["img_view_transformer"] and "point_cloud_range" not in base["img_view_transformer"]
    cat = model_zoo.model_cfg(S.CFG_T, point_xyz_channel=16, point_xyz_mode="cat")
    vt = cat["img_view_transformer"]
    assert vt["point_xyz_channel"] == 16 and vt["point_xyz_mode"] == "cat" and vt["point_cloud_range"] == RANGE
    assert cat["img_bev_encoder_backbone"]["n_input_channels"] == 128 + 16
    add = model_zoo.model_cfg(S.CFG_T, point_xyz_channel=16, point_xyz_mode="add")
    assert add["img_view_transformer"]["point_xyz_mode"] == "add" and add["img_bev_encoder_backbone"]["n_input_channels"] == 128
    both = model_zoo.model_cfg(S.CFG_T, numC_Trans=64, imgseg=True, lift_with_imgseg=True, point_xyz_channel=8)
    assert both["img_bev_encoder_backbone"]["n_input_channels"] == 64 + 20 + 8


def _cpu_lift_splat(depth_prob, img_feat, geom, bx, dx, nx, grid_host=None, tables=None):
    """Stand-in for the HIP-only functional.lift_splat: outer product, then a sum per voxel."""
    n = grid_host[2]
    vox = tables[0].long()
    BN, D, H, W = depth_prob.shape
    x = (depth_prob[:, :, :, :, None] * img_feat.permute(0, 2, 3, 1)[:, None]).reshape(-1, img_feat.shape[1])
    B = BN                                               # one camera per sample
    out = torch.zeros(B * n[0] * n[1] * n[2], x.shape[1]).index_add_(0, vox[vox >= 0], x[vox >= 0])
    return out.view(B, n[0], n[1], n[2], -1).permute(0, 4, 1, 2, 3)


@pytest.mark.parametrize("mode", ("cat", "add"))
@torch.no_grad()
def test_cpu_forward_joins_the_encoding_and_voxel_pooling_agrees(mode, monkeypatch):
    vt = VT(point_xyz_channel=16, point_xyz_mode=mode, point_cloud_range=RANGE, ablation="bev_only").train()
    vt.point_xyz_encoder.load_state_dict(X.case("A")["state"])
    D = vt.D
    feat = S.hash_normal("point_xyz_fwd_y", (1, D + 16, 8, 20))

    class Net(torch.nn.Module):
        def forward(self, x, mlp_input):
            return feat

    vt.depth_net = Net()
    monkeypatch.setattr(F, "lift_splat", _cpu_lift_splat)
    view = S.frustum_view(S.CFG_T)
    x = torch.zeros(1, 1, 32, 8, 20)
    inputs = [x, *view[1:], None] + [None] * 9
    bev, depth = vt(inputs)
    assert tuple(bev.shape) == (1, 32 if mode == "cat" else 16, 16, 16, 4) and tuple(depth.shape) == (1, D, 8, 20)
    assert int(vt.point_xyz_encoder[1].num_batches_tracked) == 1
    geom = vt.get_geometry(*view[1:])
    lifted = (depth.view(1, 1, D, 8, 20, 1) * feat[:, D:].permute(0, 2, 3, 1).view(1, 1, 1, 8, 20, 16))
    pooled = vt.voxel_pooling(geom, lifted)
    assert tuple(pooled.shape) == tuple(bev.shape) and float((pooled - bev).abs().max()) <= 1e-5 * float(bev.abs().max())
    P = vt.point_xyz_pool(geom, (F.voxel_index_tensor(geom, *vt._grid_host()), None, None))
    plain = _cpu_lift_splat(depth, feat[:, D:], None, None, None, None, vt._grid_host(), (F.voxel_index_tensor(geom, *vt._grid_host()),))
    xyz = bev[:, 16:] if mode == "cat" else bev - plain
    assert float(P.abs().max()) > 0 and float((xyz - P).abs().max()) <= 1e-5 * float(bev.abs().max())
    assert int(vt.point_xyz_encoder[1].num_batches_tracked) == 3
    got, _ = X.rows("A", P)
    assert float(np.abs(got - X.golden()["A_f64_P"]).max()) <= X.tol("A", "P")


def test_running_statistics_after_a_step():
    got = X.run("B", "cpu", fused=False)
    g = X.golden()
    assert got["nbt"] == 1
    for q in ("rm", "rv"):
        assert float(np.abs(got[q].double().numpy() - g[f"B_f64_{q}"]).max()) <= X.tol("B", q)
    assert float(got["rm"].abs().max()) > 0 and not torch.equal(got["rv"], torch.ones(8))


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 118
    for n in ("ssbev_point_xyz_workspace", "ssbev_point_xyz_moments", "ssbev_point_xyz_fwd", "ssbev_point_xyz_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments

    def dims(**kw):
        v = dict(B=1, P=112 * 48 * 160, nx=128, ny=128, nz=16, M=64, lo=(0.0, -25.6, -2.0), hi=(51.2, 25.6, 4.4))
        v.update(kw)
        d = capi.PointXyzDims(v["B"], v["P"], v["nx"], v["ny"], v["nz"], v["M"])
        for i in range(3):
            d.lo[i], d.hi[i] = v["lo"][i], v["hi"][i]
        return d

    good = dims()
    ws = lib.ssbev_point_xyz_workspace(C.byref(good))
    assert 5 * 64 * 8 <= ws <= 1024 * 5 * 64 * 8 and ws >= 10 * 8           # per-workgroup partials of 5 M (or 10) doubles
    assert lib.ssbev_point_xyz_workspace(None) == 0
    bad_dims = [dims(B=0), dims(P=0), dims(nx=0), dims(ny=-1), dims(nz=0), dims(M=0), dims(M=6), dims(M=260), dims(M=-4),
                dims(hi=(0.0, 25.6, 4.4)), dims(lo=(0.0, 30.0, -2.0)), dims(hi=(float("nan"), 25.6, 4.4)),
                dims(lo=(float("-inf"), -25.6, -2.0)), dims(B=1 << 12, P=1 << 19), dims(B=64, nx=1 << 10, ny=1 << 10, nz=1 << 5)]
    for d in bad_dims:
        assert lib.ssbev_point_xyz_workspace(C.byref(d)) == 0

    def moments(p=(fake, fake, fake), d=good, w=fake, nbytes=ws):
        return lib.ssbev_point_xyz_moments(*p, C.byref(d) if d is not None else None, w, nbytes, None)

    def fwd(p=(fake, fake, fake, fake, fake, fake), d=good, w=None, nbytes=None):
        return lib.ssbev_point_xyz_fwd(*p, C.byref(d) if d is not None else None, None)

    def bwd(p=(fake, fake, fake, fake, fake, fake), d=good, w=fake, nbytes=ws):
        return lib.ssbev_point_xyz_bwd(*p, C.byref(d) if d is not None else None, w, nbytes, None)

    for call, n, optional in ((moments, 3, ()), (fwd, 6, (3,)), (bwd, 6, ())):
        for i in range(n):
            if i not in optional:                                        # (the long-voxel list of _fwd may be NULL)
                assert call(p=tuple(None if j == i else fake for j in range(n))) == capi.EINVAL, (call.__name__, i)
        assert call(d=None) == capi.EINVAL
        for d in bad_dims:
            assert call(d=d) == capi.EINVAL
    for call in (moments, bwd):
        assert call(w=None) == capi.EINVAL
        assert call(nbytes=ws - 1) == capi.EWORKSPACE and call(nbytes=0) == capi.EWORKSPACE
