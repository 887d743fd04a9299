"""CPU: the point-level branch of ``OccHead`` (``supervise_points=True``) -- modules with the reference's keys and shapes, the
tensor form against tests/golden/point_head.npz on every case, the detector's call, the KeyError without points, ``model_cfg``
and the host-side answers of the new entry points.  Bounds and cases: tests/point_head_cases.py."""
import ctypes as C

import pytest
import torch

import point_head_cases as X
from stereoscene_amd import capi, functional as F, model_zoo, synthetic as S
from stereoscene_amd.plugin.voxel_encoder import OccHead

HEAD_KW = dict(in_channels=[384], out_channel=20, semantic_kitti=True, num_level=1)


def test_constructor_builds_the_reference_modules():
    head = OccHead(supervise_points=True, sampling_img_feats=True, in_img_channels=640, soft_weights=True, **HEAD_KW)
    shapes = {k: tuple(v.shape) for k, v in head.state_dict().items() if not k.startswith("occ_convs")}
    assert shapes == {"img_feat_reduce.weight": (384, 640), "img_feat_reduce.bias": (384,),
                      "point_soft_weights.0.weight": (192, 384), "point_soft_weights.0.bias": (192,),
                      "point_soft_weights.2.weight": (2, 192), "point_soft_weights.2.bias": (2,),
                      "point_occ_mlp.fc1.weight": (384, 384), "point_occ_mlp.fc1.bias": (384,),
                      "point_occ_mlp.fc2.weight": (20, 384), "point_occ_mlp.fc2.bias": (20,)}
    assert head.loss_point_ce_weight == head.loss_point_lovasz_weight == 1.0 and head.point_axis_order == "reference"
    bare = OccHead(supervise_points=True, out_point_channel=7, loss_weight_cfg=dict(loss_point_ce_weight=0.5), **HEAD_KW)
    assert sorted(k for k in bare.state_dict() if not k.startswith("occ_convs")) == [
        "point_occ_mlp.fc1.bias", "point_occ_mlp.fc1.weight", "point_occ_mlp.fc2.bias", "point_occ_mlp.fc2.weight"]
    assert bare.point_occ_mlp.fc2.out_features == 7 and bare.loss_point_ce_weight == 0.5
    plain = OccHead(**HEAD_KW)
    assert all(k.startswith("occ_convs") for k in plain.state_dict()) and plain.supervise_points is False
    with pytest.raises(ValueError, match="point_axis_order"):
        OccHead(supervise_points=True, point_axis_order="zyx", **HEAD_KW)


def test_unsupported_combinations_still_raise():
    with pytest.raises(NotImplementedError):
        OccHead(supervise_points=True, **dict(HEAD_KW, semantic_kitti=False))
    with pytest.raises(NotImplementedError):
        OccHead(supervise_points=True, supervise_voxel=False, **HEAD_KW)


def test_grid_sample_walks_the_last_axis_with_the_first_coordinate():
    """The quirk ``point_axis_order`` names, seen with ``grid_sample`` itself on an X != Z map."""
    x, y, z = torch.arange(2.0).view(2, 1, 1), torch.arange(3.0).view(1, 3, 1), torch.arange(5.0).view(1, 1, 5)
    f = (100 * x + 10 * y + z).view(1, 1, 2, 3, 5)
    g = torch.tensor([[0.5, 0.0, -0.8]])                     # the centre of cell (x, y, z) = (1, 1, 0)
    as_given = F.point_sample_tensor([f], g, [1], "reference")
    flipped = F.point_sample_tensor([f], g, [1], "xyz")
    assert abs(float(as_given) - 9.275) < 1e-5 and float(flipped) == 110.0


@pytest.mark.parametrize("name", X.CASES)
def test_tensor_form_matches_the_fixture(name):
    X.check(name, X.run(name, "cpu"), "tensor form on the CPU")


def test_no_labelled_point_gives_exact_zeros():
    got = X.run("G", "cpu")
    assert float(got["ce"]) == 0.0 and float(got["lov"]) == 0.0
    assert all(not v.any() for k, v in got.items() if k.startswith("g"))


def test_forward_and_loss_of_the_head():
    c = X.case("E")
    head = X.build_head("E")
    head.forward_voxel = lambda feats: feats                 # (the voxel convolutions have no CPU form)
    out = head(voxel_feats=[c["feats"][0]], points=c["points"])
    assert [tuple(o.shape) for o in out["output_points"]] == [(0, 20), (1, 20)] and len(out["output_voxels"]) == 1
    with pytest.raises(KeyError, match="points_occ"):
        head(voxel_feats=[c["feats"][0]])
    both = X.build_head("C1")
    with pytest.raises(KeyError, match="points_occ.*points_uv"):
        both(voxel_feats=list(X.case("C1")["feats"]))
    head.eval()
    assert head(voxel_feats=[c["feats"][0]])["output_points"] is None
    losses = head.loss_point_single(torch.cat(out["output_points"]), torch.cat(c["points"]))
    assert list(losses) == ["loss_point_ce_", "loss_point_lovasz_"]


def test_detector_passes_the_point_inputs_to_a_points_head_only():
    from stereoscene_amd.plugin.detector import BEVDepthOccupancy
    seen = {}

    class Head(torch.nn.Module):
        supervise_points = True

        def forward(self, voxel_feats, points=None, img_metas=None, img_feats=None, points_uv=None):
            seen.update(points=points, img_feats=img_feats, points_uv=points_uv)
            return {"output_voxels": voxel_feats, "output_points": ["logits"]}

        def loss(self, **kw):
            seen["loss"] = sorted(kw)
            return {"loss_x": torch.zeros(())}

    class Stub(torch.nn.Module):
        def forward(self, voxel_feats, points=None, img_metas=None):
            return {"output_voxels": voxel_feats, "output_points": None}

        def loss(self, **kw):
            seen["loss"] = sorted(kw)
            return {"loss_x": torch.zeros(())}
    det = BEVDepthOccupancy.__new__(BEVDepthOccupancy)
    torch.nn.Module.__init__(det)
    det.pts_bbox_head, det.disable_loss_depth = Head(), True
    det.extract_feat = lambda points, img, img_metas=None: (["feats"], "img_feats", None)
    det.forward_train(img_inputs="views", gt_occ="gt", points_occ="pts", points_uv="uv")
    assert seen["points"] == "pts" and seen["img_feats"] == "img_feats" and seen["points_uv"] == "uv"
    assert seen["loss"] == ["img_metas", "output_points", "output_voxels", "target_points", "target_voxels"]
    det.pts_bbox_head = Stub()
    det.forward_train(img_inputs="views", gt_occ="gt", points_occ="pts", points_uv="uv")     # the three-argument call
    assert seen["loss"] == ["img_metas", "output_points", "output_voxels", "target_points", "target_voxels"]


def test_model_cfg_plumbing():
    base = model_zoo.model_cfg(S.CFG_T)
    assert base["pts_bbox_head"]["supervise_points"] is False and "point_axis_order" not in base["pts_bbox_head"]
    assert base["pts_bbox_head"]["sampling_img_feats"] is True and base["pts_bbox_head"]["soft_weights"] is True
    on = model_zoo.model_cfg(S.CFG_T, supervise_points=True, sampling_img_feats=False, soft_weights=False, point_axis_order="xyz")
    h = on["pts_bbox_head"]
    assert (h["supervise_points"], h["sampling_img_feats"], h["soft_weights"], h["point_axis_order"]) == (True, False, False, "xyz")
    rest = {k: v for k, v in h.items() if k not in ("supervise_points", "sampling_img_feats", "soft_weights", "point_axis_order")}
    assert rest == {k: v for k, v in base["pts_bbox_head"].items() if k in rest}
    assert {k: v for k, v in on.items() if k != "pts_bbox_head"} == {k: v for k, v in base.items() if k != "pts_bbox_head"}


def test_entry_points_answer_on_the_host():
    lib = capi.load()
    assert lib.ssbev_version() >= 119
    d = capi.PointHeadDims()
    d.B, d.N, d.C, d.L, d.axis_xyz, d.per_level = 1, 40000, 384, 1, 0, 0
    d.X[0], d.Y[0], d.Z[0] = 128, 128, 16
    assert lib.ssbev_point_sample_workspace(C.byref(d)) == 2 * 8 * 40000 * 4          # keys + weights, already 256-byte multiples
    fake = C.c_void_p(256)                                                              # never dereferenced
    assert lib.ssbev_point_sample_fwd(None, fake, fake, None, None, None, fake, C.byref(d), fake, 1 << 30, None) == capi.EINVAL
    assert lib.ssbev_point_sample_fwd(fake, fake, fake, None, None, None, fake, C.byref(d), fake, 16, None) == capi.EWORKSPACE
    assert lib.ssbev_point_sample_bwd(fake, fake, fake, fake, None, None, None, None, C.byref(d), None) == capi.EINVAL
    for field, bad in (("C", 6), ("N", 0), ("L", 5), ("B", 0), ("axis_xyz", 2)):
        e = capi.PointHeadDims.from_buffer_copy(d)
        setattr(e, field, bad)
        assert lib.ssbev_point_sample_workspace(C.byref(e)) == 0, field
        assert lib.ssbev_point_sample_fwd(fake, fake, fake, fake, fake, fake, fake, C.byref(e), fake, 1 << 30, None) == capi.EINVAL
    e = capi.PointHeadDims.from_buffer_copy(d)
    e.Z[0] = 0
    assert lib.ssbev_point_sample_workspace(C.byref(e)) == 0
    assert lib.ssbev_point_sample_workspace(None) == 0
    i = capi.PointImgDims(1, 40000, 1, 640, 48, 160)
    assert lib.ssbev_point_img_workspace(C.byref(i)) == 2 * 4 * 40000 * 4
    assert lib.ssbev_point_img_fwd(fake, None, fake, fake, C.byref(i), fake, 1 << 30, None) == capi.EINVAL
    assert lib.ssbev_point_img_bwd(fake, fake, fake, fake, None, C.byref(i), None) == capi.EINVAL
    for bad in (capi.PointImgDims(1, 40000, 1, 642, 48, 160), capi.PointImgDims(1, 40000, 0, 640, 48, 160),
                capi.PointImgDims(1, -1, 1, 640, 48, 160)):
        assert lib.ssbev_point_img_workspace(C.byref(bad)) == 0
        assert lib.ssbev_point_img_fwd(fake, fake, fake, fake, C.byref(bad), fake, 1 << 30, None) == capi.EINVAL
