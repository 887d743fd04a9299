"""CPU: the case table of test_gpu_norm_paths.py really reaches every statistics, finalize and apply path of csrc/groupnorm.hip.

Every case of norm_cases is asked of the library itself (ssbev_groupnorm_plan_query, which reads the geometry functions the
launchers and the *_workspace queries read) and held to the properties it is listed for: lane width, slabs and chunks, whether
and in which slab the statistics kernel's four-voxel main loop is reached, the outer trips of the finalize kernels, the apply
grid, its trips and how many samples a thread's second trip moves ahead.  A change to a constant of the geometry that takes a
property away from a GPU case fails here on a box without a GPU."""
import ctypes as C
import random

import pytest

import norm_cases as T
from stereoscene_amd import capi


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_reaches_its_paths(case):
    p = T.query(T.dims(case))
    assert not isinstance(p, int), p
    assert T.properties(case, p) == case.expect, T.plan_tuple(p)
    # relu, and the alignment flag where it has no say, do not move the plan
    assert T.plan_tuple(T.query(T.dims(case, relu=1))) == T.plan_tuple(p)
    if p.vw == 4:
        assert T.plan_tuple(T.query(T.dims(case), aligned16=0)) == T.plan_tuple(p)
    # the workspace holds one record per (sample, chunk, channel) + the group coefficients
    lib = capi.load()
    d = T.dims(case)
    assert lib.ssbev_groupnorm_workspace(C.byref(d)) == (case.B * p.chunks * case.C * 2 + case.B * case.G * 2 + 64) * 4


def test_table_covers_every_path():
    e = {c.id: c.expect for c in T.CASES}
    # main loop and tail in every slab and row (A, F), in the first rows only (B, G), in a narrow last slab (C)
    assert e["A"]["main"] == {8: 32} and e["A"]["last_len"] < e["A"]["chunk_len"] and e["A"]["slabs"] == 20
    assert e["B-g1"]["main"] == e["B-g2"]["main"] == e["G"]["main"] == {8: 4}
    assert e["C"]["main"][4] > 0 and T.rows(4) == 64 and e["C"]["slabs"] == 2
    assert e["G"]["vw"] == 8 and {e["H-20"]["vw"], e["H-12"]["vw"]} == {4}
    # a second batch of finalize records: fp32 one group, two slab widths, bf16
    assert [e[i]["fin_batches"] for i in ("B-g1", "C", "G")] == [2, 2, 2] and e["B-g2"]["fin_batches"] == 1
    # pivots from memory, plain and under the GELU, with an uneven last slab
    assert not e["D"]["lds_piv"] and not e["D-gelu"]["lds_piv"] and T.BY_ID["D-gelu"].pre_act == "gelu"
    assert set(e["D"]["main"]) == {8, 2}
    # later apply trips: a rounded grid with B > 1 (E1: four samples ahead, E2: two), the capped grid (F: from sample 0 into sample 1)
    assert e["E1"]["blocks"] == 6 and e["E1"]["trip2"] == (114, 4, 4) and 114 % 64 != 0
    assert e["E2"]["blocks"] == 60 and e["E2"]["trip2"][1:] == (2, 2)
    assert e["F"]["blocks"] == 16384 and e["F"]["trip2"] == (65536, 1, 1) and e["A"]["trip2"] == (320, 1, 1)
    # q = 5 (255 active statistics threads) and q = 3
    assert T.rows(5) * 5 == 255 and e["E3-g1"]["slab_q"] == 5 and e["E1"]["slab_q"] == 3
    # batch-norm variants of A and E1
    assert T.BY_ID["A-gc"].G == T.BY_ID["A-gc"].C and T.BY_ID["E1-gc"].G == T.BY_ID["E1-gc"].C


@pytest.mark.parametrize("cid", ["A", "E1"])
def test_train_mode_batchnorm_of_a_case(cid):
    """Train-mode BatchNorm of a case's shape (B folded into S, G = C): still main loop + tail (A), still a second trip (E1)."""
    case = T.BY_ID[cid]
    p = T.query(T.dims(case, as_batch=True))
    got = T.properties(case, p, as_batch=True)
    if cid == "A":
        assert (got["slabs"], got["chunks"], got["chunk_len"], got["last_len"], got["main"]) == (20, 38, 130, 120, {8: 32})
        assert (got["blocks"], got["trips"]) == (3080, 2)
    else:
        assert (got["slabs"], got["chunks"], got["chunk_len"], got["last_len"], got["main"]) == (1, 9, 64, 38, {3: 0})
        assert (got["blocks"], got["fixed"], got["trips"], got["trip2"][0]) == (6, 1, 2, 114)


def test_bf16_norm_cat_branch_falls_back_to_four_channels_per_lane():
    ctot = sum(T.CAT_CHANNELS)
    S = T.CAT_SP[0] * T.CAT_SP[1] * T.CAT_SP[2]
    assert ctot % 8 != 0 and ctot % 4 == 0
    for ld_y, ld_gy in ((ctot, 0), (0, ctot)):               # forward writes a slice, backward reads one
        d = capi.NormDims(T.CAT_B, 32, T.CAT_GROUPS[0], S, 1e-5, 1, 0, 0, ld_y, ld_gy, 1)
        p = T.query(d)
        assert (p.vw, p.slab_q, p.slabs) == (4, 4, 2)        # slabs of 4 lanes as for 8-channel lanes, twice as many of them
        assert T.query(capi.NormDims(T.CAT_B, 32, T.CAT_GROUPS[0], S, 1e-5, 1, 0, 0, 0, 0, 1)).vw == 8
        assert T.query(capi.NormDims(T.CAT_B, 32, T.CAT_GROUPS[0], S, 1e-5, 1, 0, 0, 0, 0, 1), aligned16=0).vw == 4
    d = capi.NormDims(T.CAT_B, 12, T.CAT_GROUPS[1], S, 1e-5, 1, 0, 0, ctot, 0, 1)
    assert T.query(d).vw == 4


@pytest.mark.parametrize("case", T.DUAL_CASES, ids=T.case_id)
def test_dual_norm_case_reaches_its_rows(case):
    p = T.query(T.dual_dims(case))
    assert not isinstance(p, int), p
    q = case.C // p.vw
    assert dict(q=q, rows=T.rows(q), chunks2=p.chunks2, chunk_len2=p.chunk_len2) == case.expect, T.plan_tuple(p)
    assert T.rows(q) * case.C * 3 * 4 <= 96 * 1024             # the LDS the backward partial kernel asks for
    S = case.sp[0] * case.sp[1] * case.sp[2]
    assert (p.chunks2 - 1) * p.chunk_len2 < S <= p.chunks2 * p.chunk_len2


def test_dual_norm_refuses_more_than_1024_channels():
    B, Cch, Ga, Gb, sp = T.DUAL_REFUSED
    d = capi.Norm2Dims(B, Cch, Ga, Gb, sp[0] * sp[1] * sp[2], 1e-5, 1e-5, 1, 0, 1, 0)
    assert T.query(d) == capi.EINVAL
    assert capi.load().ssbev_groupnorm2_workspace(C.byref(d)) == 0
    d.C = d.Gb = 1024
    assert not isinstance(T.query(d), int)


def _random_single(rng):
    span = lambda hi: int(2 ** rng.uniform(0, hi))
    io = rng.choice((0, 0, 1))
    Cch = 4 * rng.choice((1, 2, 3, 5, 8, 12, 16, 32, 48, 160, 256, 257, 514)) if rng.random() < 0.6 else 4 * span(9.5)
    divs = [g for g in (1, 2, 3, 4, 5, 8, 32, Cch // 4, Cch) if g and Cch % g == 0]
    G = rng.choice(divs)
    B = rng.choice((1, 1, 2, 3, 5, 8)) if rng.random() < 0.8 else span(10)
    S = span(21) if rng.random() < 0.7 else rng.choice((1, 63, 64, 65, 4097, 49152, 76800, 1474560))
    if B * S * Cch >= 1 << 40:        # no device holds it (4 TiB in fp32); apply_blocks counts workgroups in 32 bits up to twice that
        return _random_single(rng)
    ld = lambda: rng.choice((0, 0, Cch, Cch + 4, Cch + 8, Cch + 12, 2 * Cch))
    return io, B, Cch, G, S, ld(), ld(), rng.choice((0, 1))


def test_query_matches_a_transcription_of_the_previous_geometry_on_random_problems():
    """The launchers' lane-width choice moved into gn_stat_vw / gn2_stat_vw without changing any: 60000 random problems (fp32 and
    bf16, dense and strided rows, aligned or not, single and two-norm) get the numbers norm_cases.reference_plan, a transcription
    of gn_vw, gn_rows16, make_geom, gn_slabs, make_geom2 and apply_blocks before the move, computes."""
    rng = random.Random(20261018)
    seen = set()
    zeros = dict(chunks_b=0, chunk_len_b=0, chunks2=0, chunk_len2=0)
    for i in range(60000):
        if rng.random() < 0.75:
            io, B, Cch, G, S, ld_y, ld_gy, al = args = _random_single(rng)
            p = T.query(capi.NormDims(B, Cch, G, S, 1e-5, rng.choice((0, 1)), 0, rng.choice((0, 1)), ld_y, ld_gy, io), al)
            want = dict(T.reference_plan(*args), **zeros)
            seen.add(("single", p.vw, p.fixed, p.blocks == 16384, p.slabs > 1, ld_y % 8 != 0, al))
        else:
            io, B, Cch, Ga, S, _, _, al = _random_single(rng)
            Cch = min(Cch, 1024)
            Ga = Ga if Cch % Ga == 0 else 1
            Gb = rng.choice((Cch, Ga))
            args = (io, B, Cch, Ga, Gb, S, rng.choice((0, 1)), rng.choice((0, 1)), al)
            p = T.query(capi.Norm2Dims(B, Cch, Ga, Gb, S, 1e-5, 1e-5, rng.choice((0, 1)), args[6], args[7], io), al)
            want = T.reference_plan2(*args)
            seen.add(("dual", p.vw, p.fixed, p.blocks == 16384, args[6], args[7]))
        assert not isinstance(p, int), (i, args)
        got = {n: getattr(p, n) for n, _ in capi.GroupnormPlan._fields_}
        assert got == want, (i, args)
    for kind in ("single", "dual"):                        # both lane widths, fixed or not and the capped grid were all drawn
        assert {s[1] for s in seen if s[0] == kind} == {4, 8}
        assert {s[2] for s in seen if s[0] == kind} == {0, 1}
        assert {s[3] for s in seen if s[0] == kind} == {False, True}
    assert {s[4:] for s in seen if s[0] == "dual"} == {(a, b) for a in (0, 1) for b in (0, 1)}


def test_refusals_come_from_the_query_and_the_workspace_alike():
    lib = capi.load()
    assert lib.ssbev_version() >= 107
    good = lambda: capi.NormDims(2, 64, 2, 1000, 1e-5, 1, 0, 0, 0, 0, 0)
    good2 = lambda: capi.Norm2Dims(2, 64, 2, 64, 1000, 1e-5, 1e-5, 1, 0, 1, 0)
    plan = capi.GroupnormPlan()
    q = lib.ssbev_groupnorm_plan_query
    assert q(C.byref(good()), None, 1, C.byref(plan)) == capi.OK and plan.chunks > 0 and plan.chunks2 == 0
    assert q(None, C.byref(good2()), 1, C.byref(plan)) == capi.OK and plan.chunks2 > 0 and plan.chunks_b > 0
    assert q(None, None, 1, C.byref(plan)) == capi.EINVAL
    assert q(C.byref(good()), C.byref(good2()), 1, C.byref(plan)) == capi.EINVAL
    assert q(C.byref(good()), None, 1, None) == capi.EINVAL
    for why, fields in {"C % 4": dict(C=62), "C % G": dict(G=3), "B = 0": dict(B=0), "S = 0": dict(S=0), "ld_y < C": dict(ld_y=60),
                        "ld_gy % 4": dict(ld_gy=66), "pre_act": dict(pre_act=2), "io_dtype": dict(io_dtype=2)}.items():
        d = good()
        for k, v in fields.items():
            setattr(d, k, v)
        assert T.query(d) == capi.EINVAL, why
        assert lib.ssbev_groupnorm_workspace(C.byref(d)) == 0, why
    for why, fields in {"C % 4": dict(C=62, Gb=62), "C > 1024": dict(C=1028, Gb=1028), "C % Ga": dict(Ga=3), "B = 0": dict(B=0)}.items():
        d = good2()
        for k, v in fields.items():
            setattr(d, k, v)
        assert T.query(d) == capi.EINVAL, why
        assert lib.ssbev_groupnorm2_workspace(C.byref(d)) == 0, why
