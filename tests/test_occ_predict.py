"""CPU side of the fused inference epilogue (``ssbev_occ_predict``): the count algebra, the label-file writer, the argument
checks of the C entry point and the ``fused=True`` evaluation loop through ``predict``'s tensor-op route."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import path_ref as O
from stereoscene_amd import capi
from stereoscene_amd.evaluate import LEARNING_MAP_INV
from stereoscene_amd.plugin import losses as L
from stereoscene_amd.plugin.detector import BEVDepthOccupancy


def _volumes(seed, B=3, shape=(6, 5, 4)):
    """pred / gt with 255s; sample 1 is all ignored, sample 2 has no ignored voxel."""
    g = torch.Generator().manual_seed(seed)
    pred = torch.randint(0, 20, (B, *shape), generator=g)
    gt = torch.randint(0, 20, (B, *shape), generator=g)
    gt[torch.rand(gt.shape, generator=g) < 0.3] = 255
    gt[1] = 255
    gt[2] = torch.randint(0, 20, shape, generator=g)
    return pred, gt


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_counts_from_confusion_equal_ssc_counts(seed):
    pred, gt = _volumes(seed)
    conf, nign = L.confusion_counts(pred, gt)
    assert conf.dtype == torch.int64 and conf.shape == (3, 20, 20) and nign.tolist()[1:] == [gt[1].numel(), 0]
    assert int(conf[1].sum()) == 0 and int(conf.sum() + nign.sum()) == gt.numel()
    for sel in ([0], [1], [2], [0, 1, 2], [2, 0]):
        got = L.ssc_counts_from_confusion(conf[sel], nign[sel])
        want = L.ssc_counts(pred[sel], gt[sel], 20, recompute_mask=True)
        ora = O.ssc_counts(pred[sel].numpy(), gt[sel].numpy(), 20, recompute_mask=True)
        for a, b, c in zip(got, want, ora):
            assert a.dtype == torch.int64 and torch.equal(a, b), sel
            assert np.array_equal(a.numpy(), np.asarray(c).astype(np.int64).reshape(a.shape)), sel
    one = L.ssc_counts_from_confusion(conf[0], nign[0])                  # a single [20,20] matrix and a 0-dim count
    for a, b in zip(one, L.ssc_counts(pred[:1], gt[:1], 20, recompute_mask=True)):
        assert torch.equal(a, b)


def test_prediction_writer_matches_the_logits_writer(tmp_path):
    from stereoscene_amd.evaluate import save_output_semantic_kitti, save_prediction_semantic_kitti
    cls = (torch.arange(4 * 3 * 2).reshape(4, 3, 2) * 7) % 20
    logits = torch.zeros(20, 4, 3, 2).scatter_(0, cls[None], 1.0)
    want = open(save_output_semantic_kitti(logits, str(tmp_path / "a"), "11", "000007"), "rb").read()
    p8 = save_prediction_semantic_kitti(cls.to(torch.uint8), str(tmp_path / "b"), "11", "000007")
    raw = torch.from_numpy(LEARNING_MAP_INV[cls.numpy()].astype(np.uint16))
    p16 = save_prediction_semantic_kitti(raw, str(tmp_path / "c"), "11", "000007")
    p16n = save_prediction_semantic_kitti(raw.numpy(), str(tmp_path / "d"), "11", "000007")
    assert p8.endswith("sequences/11/predictions/000007.label")
    assert len(want) == 2 * cls.numel()
    for p in (p8, p16, p16n):
        assert open(p, "rb").read() == want
    with pytest.raises(TypeError):
        save_prediction_semantic_kitti(cls, str(tmp_path / "e"), "11", "000007")       # int64: neither raw nor training ids


def test_entry_point_refuses_bad_arguments_on_host():
    lib = capi.load()
    assert lib.ssbev_version() >= 103
    fake = C.c_void_p(256)                # never dereferenced: the calls are refused on their arguments
    tab = (C.c_uint16 * 20)(*[int(v) for v in LEARNING_MAP_INV])
    ok = capi.UpsampleDims(1, 4, 4, 2, 20)
    big = 1 << 30

    def call(d, logits=fake, label=fake, remap=tab, pred=fake, raw=fake, conf=fake, nign=fake, ws=fake):
        return lib.ssbev_occ_predict(logits, label, remap, pred, raw, conf, nign, None if d is None else C.byref(d), ws, big, None)

    assert call(ok, label=None) == capi.EINVAL                                     # conf without labels
    assert call(ok, label=None, conf=None) == capi.EINVAL                          # n_ignored without labels
    assert call(ok, pred=None, raw=None, conf=None, nign=None) == capi.EINVAL      # all outputs NULL
    assert call(ok, remap=None) == capi.EINVAL                                     # raw without its table
    assert call(ok, logits=None) == capi.EINVAL
    assert call(ok, ws=None) == capi.EINVAL                                        # counts need the workspace
    assert call(None) == capi.EINVAL
    for bad in ((1, 4, 4, 2, 19), (1, 4, 4, 2, 24), (0, 4, 4, 2, 20), (1, 0, 4, 2, 20), (1, 4, -1, 2, 20), (1, 4, 4, 0, 20),
                (1, 1024, 1024, 256, 20)):                                         # the last: 2^31 fine voxels in one sample
        d = capi.UpsampleDims(*bad)
        assert call(d) == capi.EINVAL, bad
        assert lib.ssbev_occ_predict_workspace(C.byref(d)) == 0, bad
    assert lib.ssbev_occ_predict(fake, fake, tab, fake, fake, fake, fake, C.byref(ok), fake, 16, None) == capi.EWORKSPACE
    # workspace: per-block int32 partials of the 400 + 1 counters, monotone in B
    last = 0
    for B in (1, 2, 3, 8):
        d = capi.UpsampleDims(B, 128, 128, 16, 20)
        ws = lib.ssbev_occ_predict_workspace(C.byref(d))
        assert ws >= B * 401 * 4 and ws > last
        last = ws
    assert lib.ssbev_occ_predict_workspace(C.byref(capi.UpsampleDims(1, 128, 128, 16, 20))) <= 8 << 20


def test_functional_refuses_cpu_tensors_and_bad_shapes():
    from stereoscene_amd import functional as F
    with pytest.raises(capi.SsbevError):
        F.occ_predict(torch.zeros(1, 20, 2, 2, 2))
    with pytest.raises(capi.SsbevError):
        F.occ_predict(torch.zeros(1, 20, 2, 2, 2), torch.zeros(1, 4, 4, 4, dtype=torch.uint8), LEARNING_MAP_INV)
    assert not F.occ_predict_supported(torch.zeros(1, 20, 2, 2, 2), (4, 4, 4))


class _FakeModel(nn.Module):
    """The real ``BEVDepthOccupancy.predict`` over a stand-in trunk: logits at the label grid's size that depend only on the
    sample (its gt shifted by the sample id), so the tensor-op route of ``predict`` runs on the CPU."""
    predict = BEVDepthOccupancy.predict

    def extract_feat(self, points, img, img_metas=None):
        return img, None, None

    def pts_bbox_head(self, voxel_feats, points=None, img_metas=None):
        sid, gt = voxel_feats
        pred = (gt.clamp(max=19) + sid.view(-1, 1, 1, 1)) % 20
        return {"output_voxels": [nn.functional.one_hot(pred.long(), 20).permute(0, 4, 1, 2, 3).float()]}

    def simple_test(self, img_metas, img_inputs, gt_occ=None):
        return {"output_voxels": self.pts_bbox_head(img_inputs)["output_voxels"][0]}


def _fake_batches(ids, batch):
    g = torch.Generator().manual_seed(0)
    vox = torch.randint(0, 21, (64, 4, 4, 2), generator=g)
    vox[vox == 20] = 255
    for i in range(0, len(ids), batch):
        sel = torch.tensor(ids[i:i + batch])
        yield {"img_inputs": (sel, vox[sel]), "gt_occ": vox[sel]}


def test_fused_evaluation_equals_the_unfused_loop_on_the_cpu():
    from stereoscene_amd.evaluate import evaluate, evaluate_counts
    from stereoscene_amd.runner import DistributedSampler
    model = _FakeModel()
    out = model.predict(None, next(_fake_batches([3, 4], 2))["img_inputs"], gt_occ=next(_fake_batches([3, 4], 2))["gt_occ"],
                        remap=LEARNING_MAP_INV)
    assert out["pred_voxels"].dtype == torch.uint8 and out["raw_voxels"].dtype == torch.uint16
    assert out["confusion"].shape == (2, 20, 20) and out["n_ignored"].shape == (2,) and len(out["ssc_counts"]) == 6
    assert np.array_equal(out["raw_voxels"].numpy(), LEARNING_MAP_INV[out["pred_voxels"].numpy()].astype(np.uint16))
    for n, world, batch in ((7, 2, 2), (10, 3, 4), (5, 4, 1), (9, 3, 2)):
        want = evaluate_counts(model, _fake_batches(list(range(n)), batch), device="cpu")
        got = evaluate_counts(model, _fake_batches(list(range(n)), batch), device="cpu", fused=True)
        assert got.dtype == torch.float64 and got.shape == (63,) and torch.equal(got, want), (n, batch)
        acc = 0
        for rank in range(world):
            smp = DistributedSampler(range(n), num_replicas=world, rank=rank)
            acc = acc + evaluate_counts(model, _fake_batches(list(smp), batch), device="cpu", sampler=smp, fused=True)
        assert torch.equal(acc, want), (n, world, batch)
    assert evaluate(model, _fake_batches(list(range(7)), 2), device="cpu", fused=True) == \
        evaluate(model, _fake_batches(list(range(7)), 2), device="cpu")
