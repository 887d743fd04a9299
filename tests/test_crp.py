"""CPU: the 3-D context relation prior against the reference's records and the float64 restatements of tools/make_golden_crp.py
(tests/golden/crp.npz): the label down-sampling in its CPU form (byte-exact), ``functional.relation_matrix`` (every element), the
relation loss in its tensor form, the state-dict layout of ``CustomResNet3D(crp3d=True)`` / ``CPMegaVoxels``, the wiring into the
loader, ``collate``, the detector and ``model_zoo.model_cfg``, and the host-side checks of the C entry points.

Bounds, as in tests/test_frustum.py: K x the case's recorded fp32-vs-float64 spread, K = 8, floored at the fp32 unit roundoff eps =
2^-23.  Loss: K * max(LX_loss_spread, eps) * max(1, |loss|).  Gradient: K * max(LX_spread, eps) * max|float64 gradient| on EVERY
element.  Case B (a relation without a positive) is finite here with pos_weight 1; the reference's record is NaN."""
import ctypes as C
import functools
import json
import os
import zlib

import numpy as np
import pytest
import torch

from conftest import ROOT
from stereoscene_amd import capi, functional as F, pipelines as P, synthetic as S
from stereoscene_amd.plugin import losses as L

GOLDEN = os.path.join(ROOT, "tests", "golden", "crp.npz")
K = 8.0
EPS = 2.0 ** -23
LOSS_CASES = tuple(S.CRP_LOSS_CASES)
BACKBONE_KW = dict(depth=18, block_inplanes=[8, 16, 32], num_stage=3, n_input_channels=4, out_indices=(0, 1, 2), crp3d=True,
                   crp_level=2, norm_cfg=dict(type="BN3d", requires_grad=True))      # tools/make_golden_crp.py


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def loss_case(name):
    """(P_logits, labels) of the case: rebuilt from the hash generator, shared and never modified."""
    return S.crp_loss_case(name)


@functools.lru_cache(maxsize=None)
def down_case(name):
    return S.crp_downsample_case(name)


def loss_tol(name):
    return K * max(float(golden()[f"L{name}_loss_spread"]), EPS) * max(1.0, abs(float(golden()[f"L{name}_f64_loss"])))


def grad_tol(name):
    return K * max(float(golden()[f"L{name}_spread"]), EPS) * float(golden()[f"L{name}_grad_max"])


@functools.lru_cache(maxsize=None)
def f64_grad(name):
    """The float64 logit gradient of a case: the fixture's record, or for E (2.6 M elements, not stored) the float64 run of the
    tensor form, whose loss and largest element are held to the generator's record here."""
    g = golden()
    if f"L{name}_f64_grad" in g:
        return g[f"L{name}_f64_grad"]
    x, lab = loss_case(name)
    x = x.double().requires_grad_(True)
    loss = F.relation_loss_tensor(x, F.relation_matrix(lab))
    loss.backward()
    assert abs(float(loss.detach()) - float(g[f"L{name}_f64_loss"])) <= 1e-12
    assert abs(float(x.grad.abs().max()) - float(g[f"L{name}_grad_max"])) <= 1e-12 * float(g[f"L{name}_grad_max"])
    return x.grad.numpy().astype(np.float32)


def tensor_form(name, device="cpu", dense=False):
    x, lab = loss_case(name)
    x = x.clone().to(device).requires_grad_(True)
    if dense:
        loss = F.relation_loss(x, matrices=F.relation_matrix(lab).to(device))
    else:
        loss = F.relation_loss(x, lab.to(device))
    assert loss.dim() == 0 and loss.dtype == torch.float32
    loss.backward()
    return loss.detach().cpu(), x.grad.detach().cpu()


def check(name, loss, grad, what):
    want = float(golden()[f"L{name}_f64_loss"])
    err = float(np.abs(grad.numpy() - f64_grad(name)).max())
    print(name, what, "loss", float(loss), "float64", want, "error", abs(float(loss) - want), "bound", loss_tol(name),
          "| max gradient error", err, "bound", grad_tol(name))
    assert np.isfinite(float(loss)) and abs(float(loss) - want) <= loss_tol(name)
    assert torch.isfinite(grad).all() and err <= grad_tol(name)


def matrix_record(key, m):
    """``m`` (uint8 numpy) against the fixture's record of the reference's matrix: every element, or its sums and CRC."""
    g = golden()
    if f"{key}_matrix" in g:
        assert m.shape == g[f"{key}_matrix"].shape and np.array_equal(m, g[f"{key}_matrix"])
    else:
        assert np.array_equal(m.reshape(4, -1).sum(1).astype(np.int64), g[f"{key}_matrix_sum"])
        assert zlib.crc32(np.ascontiguousarray(m).tobytes()) == int(g[f"{key}_matrix_crc"])


def test_fixture_conditions():
    g = golden()
    for name in LOSS_CASES:
        assert 0.0 < float(g[f"L{name}_spread"]) <= 1e-6 and float(g[f"L{name}_loss_spread"]) <= 1e-6, name
    assert all(int(v) > 0 for n in "ACDE" for v in g[f"L{n}_positives"]) and np.isfinite(g["LA_ref_loss"])
    assert int(g["LB_positives"][1]) == 0 and np.isnan(g["LB_ref_loss"]) and np.isfinite(g["LB_f64_loss"])
    assert bool((loss_case("C")[1] == 255).any()) and float(loss_case("C")[0].abs().max()) == 90.0
    x, lab = loss_case("D")
    assert lab.shape[0] == 2 and int((lab[1] != 0).sum()) == 1
    assert "LE_f64_grad" not in g and "LE_matrix" not in g and loss_case("E")[0].shape[2] > 256
    for name, (grid, ds) in S.CRP_DOWNSAMPLE_CASES.items():
        assert g[f"{name}_down"].shape == tuple(v // ds for v in grid) and g[f"{name}_down"].dtype == np.uint8
    d8, d2 = g["D8_down"].reshape(-1), g["D2_down"].reshape(-1)
    assert [int(d8[i]) for i in range(7)] == [11, 0, 255, 255, 3, 255, 0]          # 486 / 487 / 487 / tie / class tie / all 255 / all 0
    assert [int(d2[i]) for i in range(5)] == [4, 255, 0, 2, 255]
    lab8, _ = down_case("D8")
    blk = lambda i: lab8[(i // 4) * 8:(i // 4 + 1) * 8, ((i // 2) % 2) * 8:((i // 2) % 2 + 1) * 8, (i % 2) * 8:(i % 2 + 1) * 8]
    assert int(((blk(0) == 0) | (blk(0) == 255)).sum()) == 486 and int(((blk(1) == 0) | (blk(1) == 255)).sum()) == 487
    assert os.path.getsize(GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", tuple(S.CRP_DOWNSAMPLE_CASES))
def test_cpu_downsample_is_byte_equal_to_the_reference(name):
    lab, ds = down_case(name)
    out = F.label_downsample(lab, ds)
    assert out.dtype == torch.uint8 and np.array_equal(out.numpy(), golden()[f"{name}_down"])
    with pytest.raises(ValueError):
        F.label_downsample(lab, 5)


def test_relation_matrix_equals_the_reference_on_every_element():
    for name in ("D8", "D4"):
        matrix_record(name, F.relation_matrix(torch.from_numpy(golden()[f"{name}_down"])).numpy())
    for name in LOSS_CASES:
        m = F.relation_matrix(loss_case(name)[1])
        assert m.dtype == torch.uint8 and m.dim() == 4
        matrix_record(f"L{name}", m.numpy())
        assert np.array_equal(m.numpy().reshape(m.shape[0], 4, -1).sum((0, 2)), golden()[f"L{name}_positives"])
    single = F.relation_matrix(loss_case("A")[1][0])
    assert single.dim() == 3 and torch.equal(single, F.relation_matrix(loss_case("A")[1])[0])
    with pytest.raises(ValueError):
        F.relation_matrix(torch.zeros(4, 3, 2, dtype=torch.uint8))


@pytest.mark.parametrize("name", LOSS_CASES)
def test_tensor_form_matches_float64_and_the_reference(name):
    loss, grad = tensor_form(name)
    check(name, loss, grad, "tensor form")
    if name != "B":
        assert abs(float(loss) - float(golden()[f"L{name}_ref_loss"])) <= loss_tol(name)
    l2, g2 = tensor_form(name, dense=True)                                   # a caller's dense matrix: the same tensor form
    assert torch.equal(loss, l2) and torch.equal(grad, g2)


def test_counts_are_pooled_over_the_batch():
    x, lab = loss_case("D")
    per_sample = sum(float(F.relation_loss(x[b:b + 1], lab[b:b + 1])) for b in range(2)) / 2
    assert abs(per_sample - float(golden()["LD_f64_loss"])) > 100 * loss_tol("D")


def test_state_dict_layout_equals_the_reference():
    from stereoscene_amd.plugin.crp3d import CPMegaVoxels
    from stereoscene_amd.plugin.voxel_encoder import CustomResNet3D
    g = golden()
    keys, shapes = json.loads(str(g["bb_keys"])), json.loads(str(g["bb_shapes"]))
    m = CustomResNet3D(**BACKBONE_KW)
    sd = m.state_dict()
    assert list(sd.keys()) == keys
    assert [list(t.shape) for t in sd.values()] == shapes
    rec = {k: torch.zeros(s, dtype=sd[k].dtype) for k, s in zip(keys, shapes)}
    S.fill_state_dict_(rec)
    m.load_state_dict(rec, strict=True)
    assert torch.equal(m.CP_mega_voxels.context_prior_logits[3][0].weight, rec["CP_mega_voxels.context_prior_logits.3.0.weight"])
    assert m.CP_mega_voxels.size == (32, 32, 4) and m.CP_mega_voxels.flatten_context_size == 512
    blk = CPMegaVoxels(S.CRP_BLOCK["feature"], S.CRP_BLOCK["size"], bn_momentum=0.1)
    blk.load_state_dict({k[len("blk_sd/"):]: torch.from_numpy(v) for k, v in g.items() if k.startswith("blk_sd/")}, strict=True)
    small = CustomResNet3D(**dict(BACKBONE_KW, crp_size=(4, 4, 2), crp_level=1))
    assert small.CP_mega_voxels.feature == 16 and small.CP_mega_voxels.flatten_context_size == 4
    plain = CustomResNet3D(**dict(BACKBONE_KW, crp3d=False))
    assert not plain.crp3d and not any(k.startswith("CP_mega_voxels") for k in plain.state_dict())
    with pytest.raises(RuntimeError):
        m.crp_loss(CP_mega_labels=torch.zeros(1, 32, 32, 4, dtype=torch.uint8))     # no forward yet
    with pytest.raises(NotImplementedError):
        blk.resize[1].main[0].__class__(8, 2, torch.nn.BatchNorm3d, stride=2)(torch.zeros(1, 8, 2, 2, 2))


def test_model_cfg_plumbing():
    from stereoscene_amd import model_zoo
    base = model_zoo.model_cfg(S.CFG_T)
    assert "crp3d" not in base["img_bev_encoder_backbone"]
    assert repr(model_zoo.model_cfg(S.CFG_T, crp3d=False)) == repr(base)
    bb = model_zoo.model_cfg(S.CFG_K112, crp3d=True)["img_bev_encoder_backbone"]
    assert bb["crp3d"] is True and bb["crp_level"] == 2 and bb["crp_size"] == (32, 32, 4)      # the reference's hard-coded grid
    bb = model_zoo.model_cfg(S.CFG_T, crp3d=True, crp_level=1)["img_bev_encoder_backbone"]
    assert bb["crp_size"] == (8, 8, 2)
    with pytest.raises(ValueError):
        model_zoo.model_cfg(S.CFG_T, crp3d=True, crp_level=3)
    from stereoscene_amd import plugin  # noqa: F401  (fills the registries)
    from stereoscene_amd.registry import BACKBONES
    built = BACKBONES.build(dict(bb, block_inplanes=[8, 16, 32], norm_cfg=dict(type="BN3d", requires_grad=True)))
    assert built.crp3d and built.crp_level == 1 and built.CP_mega_voxels.size == (8, 8, 2)


def test_detector_asks_for_the_labels_and_adds_the_loss():
    from stereoscene_amd.plugin.detector import BEVDepthOccupancy
    seen = {}

    class Head(torch.nn.Module):
        def forward(self, voxel_feats, points=None, img_metas=None):
            return {"output_voxels": voxel_feats, "output_points": None}

        def loss(self, **kw):
            return {"loss_x": torch.zeros(())}

    class Backbone(torch.nn.Module):
        crp3d = True

        def crp_loss(self, CP_mega_matrices=None, CP_mega_labels=None):
            seen.update(matrices=CP_mega_matrices, labels=CP_mega_labels)
            return torch.ones(())
    det = BEVDepthOccupancy.__new__(BEVDepthOccupancy)
    torch.nn.Module.__init__(det)
    det.pts_bbox_head, det.disable_loss_depth, det.img_bev_encoder_backbone = Head(), True, Backbone()
    det.extract_feat = lambda points, img, img_metas: (["feats"], None, None)
    with pytest.raises(KeyError, match="relations=True"):
        det.forward_train(img_inputs="views", gt_occ="gt")
    out = det.forward_train(img_inputs="views", gt_occ="gt", CP_mega_labels="grid")
    assert list(out) == ["loss_rel_ce", "loss_x"] and seen == dict(matrices=None, labels="grid")
    det.forward_train(img_inputs="views", gt_occ="gt", CP_mega_matrix="dense")
    assert seen == dict(matrices="dense", labels=None)
    det.img_bev_encoder_backbone.crp3d = False
    assert list(det.forward_train(img_inputs="views", gt_occ="gt")) == ["loss_x"]


def test_pipeline_step_and_collate():
    from test_frustum import stereo_results
    labels, left, right, rng = stereo_results()
    kw = dict(type="CreateRelationLabels", point_cloud_range=rng, grid_size=list(labels.shape), class_names=L.KITTI_CLASS_NAMES)
    plain = P.PIPELINES.build(kw)(dict(gt_occ=labels, img_inputs=(left, right)))
    assert "CP_mega_labels" not in plain
    out = P.PIPELINES.build(dict(kw, relations=True, relation_downscale=4))(dict(gt_occ=labels, img_inputs=(left, right)))
    assert out["CP_mega_labels"].dtype == torch.uint8 and tuple(out["CP_mega_labels"].shape) == (8, 8, 2)
    assert torch.equal(out["CP_mega_labels"], F.label_downsample(labels, 4))
    assert torch.equal(out["frustums_ids"], plain["frustums_ids"])
    with pytest.raises(ValueError):
        P.PIPELINES.build(dict(kw, relations=True))                          # 8 x 2 does not divide Z = 8
    smp = S.synthetic_sample(S.CFG_T, B=1, C_in=8, tag="crp_collate")

    def sample(extra):
        views = []
        for x, geo in ((smp["x_l"], smp["geo_l"]), (smp["x_r"], smp["geo_r"])):
            rots, trans, intr, post_rots, post_trans, bda = (t[0] for t in geo)
            views.append([x[0], rots, trans, intr, post_rots, post_trans, bda, smp["gt_depths"][0], torch.zeros(1, 4, 4),
                          smp["calib"][0]])
        return dict(img_inputs=views, gt_occ=smp["gt_occ"][0], **extra)
    extra = {"CP_mega_labels": out["CP_mega_labels"]}
    full = P.collate([sample(extra), sample(extra)], device="cpu")
    assert tuple(full["CP_mega_labels"].shape) == (2, 8, 8, 2) and full["CP_mega_labels"].dtype == torch.uint8
    assert "CP_mega_labels" not in P.collate([sample(extra), sample({})], device="cpu")


def test_library_exports_the_entry_points_and_checks_arguments_on_host():
    import __graft_entry__ as ge
    ge.build()
    lib = capi.load()
    assert lib.ssbev_version() >= 117
    for n in ("ssbev_crp_loss_workspace", "ssbev_crp_loss_fwd", "ssbev_crp_loss_bwd", "ssbev_label_downsample",
              "ssbev_crp_gather_fwd", "ssbev_crp_gather_bwd_workspace", "ssbev_crp_gather_bwd"):
        assert hasattr(lib, n) and n in capi.SIGNATURES
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    good = capi.CrpDims(1, 32, 32, 4)
    ws = lib.ssbev_crp_loss_workspace(C.byref(good))
    assert 12 * 8 * 2 * 128 <= ws <= 12 * 8 * 2 * 128 + 256                     # twelve doubles per workgroup: 2 column x 128 row chunks
    assert lib.ssbev_crp_loss_fwd(*[fake] * 4, C.byref(good), fake, ws - 1, None) == capi.EWORKSPACE
    for bad in (capi.CrpDims(0, 32, 32, 4), capi.CrpDims(1, 32, 31, 4), capi.CrpDims(1, 32, 32, 0), capi.CrpDims(1, -2, 32, 4),
                capi.CrpDims(1, 512, 512, 64)):
        assert lib.ssbev_crp_loss_workspace(C.byref(bad)) == 0
        assert lib.ssbev_crp_loss_fwd(*[fake] * 4, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
        assert lib.ssbev_crp_loss_bwd(*[fake] * 5, C.byref(bad), None) == capi.EINVAL
    assert lib.ssbev_crp_loss_fwd(*[None] * 4, C.byref(good), None, 0, None) == capi.EINVAL
    assert lib.ssbev_crp_loss_fwd(*[fake] * 4, None, fake, ws, None) == capi.EINVAL
    assert lib.ssbev_crp_loss_bwd(*[None] * 5, C.byref(good), None) == capi.EINVAL
    assert lib.ssbev_label_downsample(None, fake, 32, 32, 8, 4, None) == capi.EINVAL
    for X, Y, Z, ds in ((0, 32, 8, 4), (32, 32, 8, 0), (32, 32, 8, 33), (32, 30, 8, 4), (2048, 2048, 512, 8)):
        assert lib.ssbev_label_downsample(fake, fake, X, Y, Z, ds, None) == capi.EINVAL
    gd = capi.CrpGatherDims(1, 4096, 512, 1024, 4, 4608)
    gws = lib.ssbev_crp_gather_bwd_workspace(C.byref(gd))
    assert gws == 4 * 8 * 512 * 1024 * 4                                        # (relation, 512-row slice) partials of the context gradient
    assert lib.ssbev_crp_gather_bwd(*[fake] * 5, C.byref(gd), fake, gws - 1, None) == capi.EWORKSPACE
    for bad in (capi.CrpGatherDims(0, 32, 4, 16, 4, 72), capi.CrpGatherDims(1, 32, 4, 16, 4, 63), capi.CrpGatherDims(1, 32, 0, 16, 4, 72),
                capi.CrpGatherDims(1, 32, 4, 16, 17, 512), capi.CrpGatherDims(1, 1 << 24, 4, 16, 4, 72)):
        assert lib.ssbev_crp_gather_bwd_workspace(C.byref(bad)) == 0
        assert lib.ssbev_crp_gather_fwd(*[fake] * 3, C.byref(bad), None) == capi.EINVAL
        assert lib.ssbev_crp_gather_bwd(*[fake] * 5, C.byref(bad), fake, 1 << 40, None) == capi.EINVAL
    assert lib.ssbev_crp_gather_fwd(*[None] * 3, C.byref(gd), None) == capi.EINVAL
    assert lib.ssbev_crp_gather_bwd(*[None] * 5, C.byref(gd), None, 0, None) == capi.EINVAL


def test_unsupported_inputs_take_the_tensor_form():
    x, lab = loss_case("A")
    assert not F.relation_loss_supported(x, lab.to(torch.uint8))                 # CPU tensors
    Pg, ctx, xin, _ = S.crp_gather_case("T")
    assert not F.relation_gather_supported(Pg, ctx, xin)
    out = F.relation_gather(Pg, ctx, xin)
    ref = torch.einsum("brmn,bmc->brcn", torch.sigmoid(Pg.double()), ctx.double()).reshape(1, -1, Pg.shape[3])
    assert tuple(out.shape) == (1, 8 + 4 * 16, 32) and torch.equal(out[:, :8], xin)
    assert float((out[:, 8:].double() - ref).abs().max()) <= K * EPS * float(ref.abs().max())
