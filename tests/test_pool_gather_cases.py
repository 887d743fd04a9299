"""The case tables of tests/pool_gather_cases.py are what they claim (CPU): a later edit of a table cannot quietly take the
chunk edges, the stride loops or the ragged depth splits away from the GPU tests of test_gpu_pool_gather.py."""
import numpy as np
import pytest
import torch

import pool_gather_cases as PC
from oracle import path_ref as O


def _counts(t):
    v = t.vox.astype(np.int64)
    return np.bincount(v[v >= 0], minlength=t.B * PC.vox_per_batch(t))


@pytest.mark.parametrize("name", PC.TABLES)
def test_table_is_built_as_asked(name):
    t = PC.table(name)
    P, vpb = PC.points_per_batch(t), PC.vox_per_batch(t)
    assert t.vox.dtype == np.int32 and t.vox.shape == (t.B * P,) and t.B * P < 100000
    counts = _counts(t)
    assert np.array_equal(counts, np.concatenate([np.asarray(l) for l in t.lengths]))      # the target lengths, exactly
    # batch containment: the points of batch element b lie in b's voxel range
    v = t.vox.astype(np.int64).reshape(t.B, P)
    for b in range(t.B):
        kept = v[b][v[b] >= 0]
        assert len(kept) and kept.min() >= b * vpb and kept.max() < (b + 1) * vpb
    assert (t.vox < 0).mean() >= 0.10                                                       # dropped share
    assert t.B == 2 and t.N == 2                                                            # a second camera, a second batch element
    # both cameras feed the lists, and a voxel's points are scattered in point order, not one contiguous run
    q = np.flatnonzero(t.vox >= 0) % P
    assert set(np.unique(q // (t.D * t.H * t.W))) == {0, 1}
    _, starts, order = PC.csr(t)
    longest = int(np.argmax(counts))
    ids = order[starts[longest]:starts[longest] + counts[longest]]
    assert np.all(np.diff(ids) > 0) and np.max(np.diff(ids)) > 1


def test_ragged_holds_every_edge():
    t = PC.table("RAGGED")
    counts = _counts(t)
    nv, vpb = len(counts), PC.vox_per_batch(t)
    assert nv % 4 != 0 and vpb % 4 != 0 and t.D == 5
    for b in range(t.B):          # every required length in every batch element
        assert set(PC.RAGGED_REQUIRED) <= set(counts[b * vpb:(b + 1) * vpb].tolist())
    is_long = counts > PC.POOL_LONG
    assert counts[0] == 0 and is_long[nv - 1]
    runs = [v for v in range(nv - 3) if is_long[v:v + 4].all()]
    assert runs and any(v % 4 == 0 for v in runs) and any(v % 4 != 0 for v in runs)     # one wave's four voxels; two waves' 2 + 2
    assert (vpb - 1) // 4 == vpb // 4 and counts[vpb - 1] > 0 and counts[vpb:vpb + 3].max() > 0     # a wave's four voxels straddle the batch boundary


@pytest.mark.parametrize("name", ["MANY_LONG_128", "MANY_LONG_SPLIT"])
def test_many_long_reaches_the_second_trip(name):
    counts = _counts(PC.table(name))
    long_counts = counts[counts > PC.POOL_LONG]
    assert len(long_counts) >= PC.MIN_LONG[name]
    if name == "MANY_LONG_128":
        assert long_counts.min() == 33 and long_counts.max() == 80
        assert len(set(((long_counts + 15) // 16).tolist())) >= 3          # LDS chunk counts 3, 4, 5
    else:
        assert long_counts.min() == 33 and long_counts.max() > 64          # lists with a second 64-point block among them
    assert ((counts > 0) & (counts <= PC.POOL_LONG)).sum() >= 64 and (counts == 0).sum() > 0


def test_depth_tables():
    assert set(PC.DEPTH_PLANES) == {1, 2, 3, 7, 13, 64, 260, 263} and set(PC.BWD_DEPTH_CHANNELS) == {64, 128, 256, 72}
    for D in PC.DEPTH_PLANES:
        n = D * 6
        for kept in PC.KEPT_PATTERNS:
            t = PC.depth_table(D, kept)
            assert (t.B, t.N, t.H * t.W) == (1, 1, 6) and t.vox.shape == (n,) and t.vox.max() < 18
            share = (t.vox >= 0).mean()
            if kept == "all":
                assert share == 1.0
            elif kept == "none":
                assert share == 0.0
            elif n >= 40:
                assert 0.1 < share < 0.4
    assert (PC.depth_table(263, "quarter").vox >= 0).sum() > 0


def test_channel_sets():
    assert set(PC.CHANNELS["fused"]) == {20, 64, 72, 128, 132, 256, 512}
    assert set(PC.CHANNELS["forward_only"]) == {7, 67}
    assert set(PC.CHANNELS["bev_pool"]) == {7, 16, 64, 128, 256}


def test_all_32_table():
    vox, moved, (B, nx, ny, nz) = PC.all_32_table()
    assert np.all(np.bincount(vox.numpy(), minlength=64) == PC.POOL_LONG)
    c = np.bincount(moved.numpy(), minlength=64)
    assert c[5] == 31 and c[9] == 33 and (c > PC.POOL_LONG).sum() == 1 and int((vox != moved).sum()) == 1


@pytest.mark.parametrize("name,C", [("RAGGED", 20), ("RAGGED", 67), ("MANY_LONG_128", 8)])
def test_fp32_sequential_reference_against_float64(name, C):
    """|seq32 - f64| <= (L + 1) * 2^-24 * sum |w * f| per element, L = list length: one rounding per product and one per addition
    (gamma_L <= (L + 1) u for L^2 u < 1; w * f of two fp32 values is exact in float64).  Checks the reference, not a kernel."""
    t, depth, rows, seq = PC.forward_case(name, C)
    ref, mag = PC.pool_f64(t, depth, rows)
    L = _counts(t).astype(np.float64)[:, None]
    err = np.abs(seq.numpy().astype(np.float64) - ref)
    assert seq.dtype == torch.float32 and np.all(err <= (L + 1) * 2.0 ** -24 * mag)
    assert err.max() > 0 and np.all(seq.numpy()[_counts(t) == 0] == 0)        # fp32 rounding is visible; empty voxels are zero


def test_fp32_sequential_reference_is_the_oracles_bev_pool():
    """The restated walk == oracle.path_ref.bev_pool over the materialised fp32 products, bit for bit."""
    t, depth, rows, seq = PC.forward_case("RAGGED", 20)
    kept = torch.from_numpy(t.vox >= 0)
    vol = depth.reshape(-1, 1) * rows[torch.from_numpy(PC.point_rows(t))]
    nx, ny, nz = t.grid
    want = O.bev_pool(vol[kept].contiguous(), PC.coords_of(t)[kept], t.B, nz, nx, ny)     # [B, C, nz, nx, ny]
    assert torch.equal(want.permute(0, 3, 4, 2, 1).reshape(-1, 20), seq)


def test_float64_gradients_against_autograd():
    """grads_f64 == autograd through the materialised formulation in float64."""
    t = PC.table("RAGGED")
    C = 20
    depth, rows, go = PC.depth_input(t), PC.feat_rows(t, C), PC.gout_rows(t, C)
    gd, gf = PC.grads_f64(t, depth, rows, go)
    dc = depth.double().reshape(-1).requires_grad_(True)
    fc = rows.double().requires_grad_(True)
    kept = torch.from_numpy(t.vox >= 0)
    vol = dc[:, None] * fc[torch.from_numpy(PC.point_rows(t))]
    flat = torch.zeros(go.shape[0], C, dtype=torch.float64).index_add(0, torch.from_numpy(t.vox.astype(np.int64))[kept], vol[kept])
    (flat * go.double()).sum().backward()
    assert np.allclose(gd, dc.grad.numpy(), rtol=1e-12, atol=1e-12) and np.allclose(gf, fc.grad.numpy(), rtol=1e-12, atol=1e-12)
    assert np.all(gd[t.vox < 0] == 0)
