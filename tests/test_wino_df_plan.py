"""CPU: the case table of test_gpu_wino_df.py really reaches every product instance and plan of csrc/winograd_fused.hip.

Every case of wino_df_cases.CASES is asked of the library itself (ssbev_wino43_df_plan_query, which reads df_instance and
dfw_plan, the functions ssbev_wino43_df_gemm, ssbev_wino43_df_wgrad, ssbev_wino43_df_wgrad_workspace and
ssbev_wino43_df_instance read): it reports the intended instance or (kernel, nchunk, stages per chunk), and the plan gives the
case exactly the properties it is listed for.  A threshold of df_instance or dfw_plan that moves a GPU case to another
instance, or takes its split, short last chunk, dead wave or tail away, fails here on a box without a GPU.

Contraction instances 22 and 23 are reachable through the tuning-build hooks only (nw == 3 and nw == 2 force mt = 1 in the
product build): nothing here forces or tests them."""
import ctypes as C
import random

import pytest

import wino_df_cases as T
from stereoscene_amd import capi


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_runs_its_plan_with_its_properties(case):
    B, K, N, D, H, W = case.shape
    Thw = (H // 4) * (W // 4)
    p = T.query(case.shape)
    assert not isinstance(p, int), p
    assert T.case_plan(case, p) == case.plan, T.plan_tuple(p)
    d, n = T.wino_dims(case.shape)
    lib = capi.load()
    assert lib.ssbev_wino43_df_instance(C.byref(d), n) == 10 * p.mt + p.nw
    assert lib.ssbev_wino43_df_wgrad_workspace(C.byref(d), n) == p.w_workspace
    if case.stage == T.FWD:
        assert T.fwd_props(case.shape, p) == case.props, T.plan_tuple(p)
        assert p.nst == K // 32 and p.lds_bytes == 32768 * p.mt
        assert p.nrowgrp == -(-Thw // (32 * p.mt)) and p.ncolgrp == -(-(-(-N // 32)) // p.nw)
        assert p.grid == 36 * B * (D // 2) * p.nrowgrp * p.ncolgrp
    else:
        assert T.wgrad_props(case.shape, p) == case.props, T.plan_tuple(p)
        stages = T.chunk_stages(p)
        assert sum(stages) == p.w_total_stages == B * (D // 2) * -(-Thw // p.w_br) and min(stages) > 0
        assert p.w_grid == 36 * p.w_nchunk * p.w_nkb * p.w_nnb
        assert p.w_workspace == p.w_nchunk * 144 * K * N * 4
        assert p.w_lds_bytes == {(2, 1, 16): 48, (4, 3, 8): 44, (4, 2, 16): 80}[case.plan[0]] * 1024


def test_table_covers_every_instance_plan_and_property():
    fwd = [c for c in T.CASES if c.stage == T.FWD]
    wgrad = [c for c in T.CASES if c.stage == T.WGRAD]
    assert {c.plan for c in fwd} == T.ALL_INSTANCES
    assert set().union(*(c.props for c in fwd)) == T.FWD_PROPS
    # the instance of the production grids with missing rows, two column groups and a batch crossing
    assert any(c.plan == 24 and {T.ROW_TAIL, T.COL_GROUPS, T.BATCHED, T.DEPTH_TILES} <= c.props for c in fwd)
    # N % 32 != 0 on a two-wave and on a four-wave instance; idle waves with one and with two column groups
    assert {c.plan for c in fwd if T.N_TAIL in c.props} >= {12, 14}
    assert {T.COL_GROUPS in c.props for c in fwd if T.IDLE_WAVES in c.props} == {False, True}
    assert any({T.ROW_GROUPS, T.ROW_TAIL} <= c.props and c.plan < 20 for c in fwd)          # ragged second row group, mt = 1
    assert {c.plan[0] for c in wgrad} == T.ALL_WGRAD_KERNELS
    assert set().union(*(c.props for c in wgrad)) == T.WGRAD_PROPS
    assert {c.plan[1] for c in wgrad} == {1, 2, 3}
    for kernel in T.ALL_WGRAD_KERNELS:
        mine = [c for c in wgrad if c.plan[0] == kernel]
        assert any({T.SPLIT, T.SHORT_LAST} <= c.props for c in mine), kernel
        assert any(T.DEAD_KWAVE in c.props for c in mine), kernel
        assert any(T.THW_BELOW in c.props for c in mine), kernel
    for kernel in ((2, 1, 16), (4, 3, 8)):                 # the two that never split in the whole-conv suite: three chunks each
        assert any(T.CHUNKS_3 in c.props for c in wgrad if c.plan[0] == kernel), kernel
    assert {c.plan[0][2] for c in wgrad if T.THW_ONE_PAST in c.props} == {8, 16}
    assert any(c.plan[0] == (4, 2, 16) and c.plan[1] == 1 for c in wgrad)
    # the whole-conv cases split their weight gradient, on <2, 1, 16> and on <4, 3, 8>
    plans = [T.query((B, ci, co, D, H, W)) for B, ci, co, D, H, W in T.CONV_CASES]
    assert [(p.w_kw, p.w_nt, p.w_br, p.w_nchunk) for p in plans] == [(2, 1, 16, 2), (4, 3, 8, 2)]


LEGACY_PLANS = (   # (forward instance, data-gradient instance, (kw, nt, br), nchunk) of test_winograd_depth_fused_f43's nine cases
    (13, 14, (4, 3, 8), 1), (13, 13, (4, 3, 8), 1), (13, 14, (4, 3, 8), 1), (12, 12, (2, 1, 16), 1), (14, 14, (4, 2, 16), 1),
    (14, 14, (4, 2, 16), 1), (14, 13, (4, 3, 8), 1), (14, 14, (4, 2, 16), 2), (12, 14, (4, 2, 16), 1))


def test_plans_of_the_whole_conv_cases_of_test_winograd_depth_fused_f43():
    """What the nine whole-conv cases launch, pinned: none of them reaches <2, 4>, one k-stage, N % 32 != 0 or three chunks,
    which is why the stage table above exists."""
    got = []
    for B, ci, co, D, H, W in T.LEGACY_CONV_CASES:
        f, g = T.query((B, ci, co, D, H, W)), T.query((B, co, ci, D, H, W))
        got.append((10 * f.mt + f.nw, 10 * g.mt + g.nw, (f.w_kw, f.w_nt, f.w_br), f.w_nchunk))
    assert tuple(got) == LEGACY_PLANS


def test_query_matches_a_transcription_of_the_previous_launch_geometry_on_random_dims():
    """The geometry the launchers computed inline moved into df_instance / dfw_plan without changing: 20000 random supported
    dims get the plan that wino_df_cases.reference_plan, a transcription of the code before the move, computes."""
    rng = random.Random(20261019)
    seen = set()
    for i in range(20000):
        K = 32 * rng.choice((1, 2, 2, 3, 4, 4, 5, 6, 8, 8, 12, 16))
        N = 32 * rng.choice((1, 2, 3, 4, 5, 6, 8, 12, 16)) if rng.random() < 0.7 else 4 * rng.randint(1, 130)
        shape = (rng.choice((1, 1, 2, 3)), K, N, 2 * rng.randint(1, 32), 4 * int(2 ** rng.uniform(0, 5.2)),
                 4 * int(2 ** rng.uniform(0, 5.2)))
        p = T.query(shape)
        assert not isinstance(p, int), (i, shape)
        assert T.plan_tuple(p) == T.reference_plan(shape), (i, shape)
        seen.add((10 * p.mt + p.nw, (p.w_kw, p.w_nt, p.w_br), min(p.w_nchunk, 3)))
    assert {s[0] for s in seen} == T.ALL_INSTANCES
    assert {s[1] for s in seen} == T.ALL_WGRAD_KERNELS and {s[2] for s in seen} == {1, 2, 3}


def test_refusals_come_before_any_device_work():
    assert capi.load().ssbev_version() >= 108
    T.check_return_codes()
