"""CPU: the case tables of test_gpu_stream_ops.py really reach every layout, chunk and tail path of csrc/image_ops.hip,
csrc/softmax.hip and csrc/trilinear.hip.

Every case of stream_ops_cases is held to the properties it is listed for twice: the pure-Python mirrors of the launch arithmetic
must give the hand-written `expect`, and the library itself must agree with the mirrors wherever it can be asked without a GPU --
the depthwise thread layout (ssbev_dwconv2d_bwd_weight_layout), the chunk counts behind both workspace queries, the grid of the
grid-stride passes (ssbev_stream_blocks) and the softmax instance (ssbev_softmax_axis_slices); all of them read the functions
the launchers read.  A change to a constant of the geometry that takes a path away from a GPU case fails here on a box without a
GPU."""
import ctypes as C
import random

import pytest

import stream_ops_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F


def dw_dims(c):
    Ho, pt, _ = T.same_padding(c.Hi, c.k, c.s)
    Wo, pl, _ = T.same_padding(c.Wi, c.k, c.s)
    return capi.DwDims(c.B, c.C, c.Hi, c.Wi, Ho, Wo, c.k, c.s, pt, pl)


def lib_layout(d):
    Q, L, qb = C.c_int(-1), C.c_int(-1), C.c_int(-1)
    capi.check(capi.load().ssbev_dwconv2d_bwd_weight_layout(C.byref(d), C.byref(Q), C.byref(L), C.byref(qb)), "layout")
    return dict(Q=Q.value, L=L.value, qblocks=qb.value)


@pytest.mark.parametrize("case", T.DW_CASES, ids=T.case_id)
def test_depthwise_case_reaches_its_paths(case):
    got = T.dw_properties(case)
    assert got == case.expect
    d = dw_dims(case)
    assert lib_layout(d) == {k: got[k] for k in ("Q", "L", "qblocks")}
    assert capi.load().ssbev_dwconv2d_bwd_weight_workspace(C.byref(d)) == got["nchunks"] * case.k * case.k * case.C
    for size, k, s in ((case.Hi, case.k, case.s), (case.Wi, case.k, case.s)):
        assert F.same_padding(size, k, s) == T.same_padding(size, k, s)
    assert got["active"] <= T.NT and (got["nchunks"] - 1) * got["ppc"] < case.B * got["out"][0] * got["out"][1]


@pytest.mark.parametrize("case", T.SE_CASES, ids=T.case_id)
def test_se_case_reaches_its_paths(case):
    got = T.se_properties(case)
    assert got == case.expect
    lib = capi.load()
    S = case.H * case.W
    assert lib.ssbev_chan_sum_workspace(case.B, S, case.C) == got["nchunks"] * case.B * case.C
    sb = T.stream_blocks(case.B * S * (case.C // 4))
    assert lib.ssbev_stream_blocks(case.B * S * (case.C // 4)) == sb["blocks"]


@pytest.mark.parametrize("case", T.SWISH_CASES, ids=T.case_id)
def test_swish_case_reaches_its_trips(case):
    got = T.swish_properties(case)
    assert got == case.expect
    if got is not None:
        assert capi.load().ssbev_stream_blocks(T.numel(case.shape) // 4) == got["blocks"]
    else:
        assert T.numel(case.shape) % 4 != 0


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=T.case_id)
def test_softmax_case_reaches_its_instance(case):
    got = T.softmax_properties(case)
    assert got == case.expect
    outer, Cn, inner = T.softmax_view(case.shape, case.dim)
    assert capi.load().ssbev_softmax_axis_slices(Cn, inner) == got["SL"]
    assert case.dim != len(case.shape) - 1 or case.direct          # an innermost axis never reaches these kernels through the wrapper


@pytest.mark.parametrize("case", T.TRILINEAR_CASES, ids=T.case_id)
def test_trilinear_case_reaches_its_paths(case):
    assert T.trilinear_properties(case) == case.expect
    assert case.C % 4 == 0


def test_table_covers_every_path():
    dw = {c.id: c.expect for c in T.DW_CASES}
    # the wide layout (C > 1024): 64 quads x 4 lanes, several quad blocks, a last one that is partly empty / holds one quad
    for i, last in (("W1", 16), ("W2", 1)):
        assert (dw[i]["Q"], dw[i]["L"]) == (T.DW_Q_WIDE, 4) and dw[i]["qblocks"] > 1 and dw[i]["last_quads"] == last < T.DW_Q_WIDE
    assert dw["W1"]["nchunks"] == 2 and dw["W1"]["last_chunk"] == 6 and T.by_id(T.DW_CASES)["W1"].B > 1
    # the boundary: every quad in one workgroup, one pixel lane; and the production widths of EfficientNet-B7 are wide
    assert T.by_id(T.DW_CASES)["W3"].C == 4 * T.DW_Q_ALL and (dw["W3"]["Q"], dw["W3"]["L"], dw["W3"]["qblocks"]) == (T.DW_Q_ALL, 1, 1)
    assert all(T.dw_layout(w)["Q"] == T.DW_Q_WIDE for w in (1344, 2304, 3840))
    # more chunk slabs than reduce lanes, a short last chunk, chunks shorter than L
    assert dw["W4"]["nchunks"] > T.FOLD_LANES and T.fold_trips(dw["W4"]["nchunks"]) == 2
    assert dw["W4"]["last_chunk"] == 2 < dw["W4"]["ppc"] < dw["W4"]["L"] == 128
    assert dw["W6-s1"]["last_chunk"] < dw["W6-s1"]["L"] and dw["W6-s2"]["last_chunk"] < dw["W6-s2"]["L"]
    # idle threads in the layout (Q no divisor of 256), launch totals no multiple of 256, the odd padding column on the right
    assert dw["W5"]["active"] == 255 and dw["W6-s1"]["active"] == 255
    assert dw["W5"]["fwd_quads"] % T.NT and dw["W5"]["dgrad_quads"] % T.NT and dw["W5"]["dgrad_quads"] > T.NT
    assert dw["W5"]["pad_w"] == (1, 2) and dw["W2"]["pad_w"] == (0, 1) and dw["W2"]["pad_h"] == (1, 1)
    # both kernel sizes and both strides; a map smaller than the kernel clips every tap that can be clipped: all but the centre,
    # and with the single output column of stride 2 all but the two taps of the centre row that lie on the map
    assert {(c.k, c.s) for c in T.DW_CASES} == {(3, 1), (3, 2), (5, 1), (5, 2)}
    for i, inside in (("W6-s1", 1), ("W6-s2", 2)):
        c = T.by_id(T.DW_CASES)[i]
        assert c.Hi < c.k and c.Wi < c.k and T.clipped_taps(c) == c.k * c.k - inside

    se = {c.id: c.expect for c in T.SE_CASES}
    assert se["S1"]["qblocks"] == 2 and se["S1"]["last_quads"] == 1 and T.by_id(T.SE_CASES)["S1"].B == 3
    assert se["S1"]["nchunks"] == 3 and se["S1"]["last_chunk"] == 2 < T.CHAN_LANES
    assert se["S2"]["nchunks"] == 68 and se["S2"]["fold_trips"] == 2
    assert T.by_id(T.SE_CASES)["S3"].H * T.by_id(T.SE_CASES)["S3"].W == 1
    # the capped grid: a second trip, all of it in sample 1
    g1 = T.by_id(T.SE_CASES)["G1"]
    per_sample = g1.H * g1.W * (g1.C // 4)
    assert se["G1"]["scale_trips"] == 2 and se["G1"]["scale_trip2"] == 2048 and T.STREAM_CAP * T.NT >= per_sample
    sw = T.by_id(T.SWISH_CASES)
    assert sw["G1"].expect == dict(blocks=T.STREAM_CAP, trips=2, trip2=2048) and T.numel(sw["G1"].shape) == 8396800
    assert sw["G2"].expect is None

    sm = {c.id: c.expect for c in T.SOFTMAX_CASES}
    view = {c.id: T.softmax_view(c.shape, c.dim) for c in T.SOFTMAX_CASES}
    # sliced: uneven slices with outer > 1 and a partial last workgroup; both boundaries; the production depth axis
    assert sm["X1"]["SL"] == 8 and (sm["X1"]["slice_min"], sm["X1"]["slice_max"]) == (8, 9) and view["X1"][0] == 3
    assert 0 < sm["X1"]["last_cols"] < T.NT // 8 and view["X1"][2] == 45
    assert view["X2"][1:] == (T.SM_MIN_C, T.SM_MIN_INNER) and sm["X2"]["SL"] == 8 and sm["X2"]["last_cols"] == T.NT // 8
    assert view["X5"] == (1, 112, 33) and sm["X5"]["SL"] == 8 and sm["X5"]["last_cols"] == 1
    # unsliced just below either boundary
    assert view["X3"][1] == T.SM_MIN_C - 1 and view["X3"][2] >= T.SM_MIN_INNER and sm["X3"]["SL"] == 1
    assert view["X4"][2] == T.SM_MIN_INNER - 1 and view["X4"][1] >= T.SM_MIN_C and sm["X4"]["SL"] == 1
    x6 = T.by_id(T.SOFTMAX_CASES)["X6"]
    assert x6.special and x6.shape == T.by_id(T.SOFTMAX_CASES)["X1"].shape
    assert view["X7-a"] == (4, 5, 1) and view["X7-b"] == (1, 70, 33) and sm["X7-b"]["SL"] == 8 and sm["X7-a"]["SL"] == 1
    assert all(T.by_id(T.SOFTMAX_CASES)[i].direct for i in ("X7-a", "X7-b"))

    tr = {c.id: c.expect for c in T.TRILINEAR_CASES}
    assert tr["T1"]["unit_axes"] == 3
    assert T.by_id(T.TRILINEAR_CASES)["T2"].sp[0] == 1 and T.by_id(T.TRILINEAR_CASES)["T2"].B > 1
    assert T.by_id(T.TRILINEAR_CASES)["T3"].sp[1] == 1
    assert (tr["T4"]["fwd_quads"], tr["T4"]["bwd_quads"]) == (648, 81) and 648 % T.NT and 81 % T.NT and 648 > 2 * T.NT


def test_mirrors_match_the_library_on_random_problems():
    """The mirrors are the library's arithmetic, not only at the table's shapes: 20000 random problems."""
    lib = capi.load()
    rng = random.Random(20261021)
    span = lambda hi: int(2 ** rng.uniform(0, hi))
    seen = set()
    for i in range(20000):
        Cch = 4 * (rng.choice((1, 2, 3, 5, 64, 255, 256, 257, 336, 576, 960)) if rng.random() < 0.5 else span(10.5))
        B, H, W = rng.choice((1, 1, 2, 3, 8)), span(9), span(9)
        k, s = rng.choice((3, 5)), rng.choice((1, 2))
        c = T.DwCase("r", B, Cch, H, W, k, s, None)
        p, d = T.dw_properties(c), dw_dims(c)
        assert lib_layout(d) == {n: p[n] for n in ("Q", "L", "qblocks")}, (i, c)
        assert lib.ssbev_dwconv2d_bwd_weight_workspace(C.byref(d)) == p["nchunks"] * k * k * Cch, (i, c)
        assert lib.ssbev_chan_sum_workspace(B, H * W, Cch) == T.chan_chunks(B, H * W, Cch)["nchunks"] * B * Cch, (i, c)
        n4 = span(24)
        assert lib.ssbev_stream_blocks(n4) == T.stream_blocks(n4)["blocks"], n4
        Cn, inner = rng.choice((1, 5, 63, 64, 65, 192, span(9))), rng.choice((1, 31, 32, 33, span(12)))
        assert lib.ssbev_softmax_axis_slices(Cn, inner) == T.softmax_plan(1, Cn, inner)["SL"], (Cn, inner)
        seen.add((p["Q"] == T.DW_Q_WIDE and p["qblocks"] > 1, p["ppc"] > T.CHUNK_FLOOR, n4 > T.STREAM_CAP * T.NT))
    assert {s[0] for s in seen} == {s[1] for s in seen} == {s[2] for s in seen} == {False, True}


def test_queries_refuse_bad_arguments():
    lib = capi.load()
    assert lib.ssbev_version() >= 121
    Q, L, qb = C.c_int(), C.c_int(), C.c_int()
    good = capi.DwDims(1, 8, 4, 4, 4, 4, 3, 1, 1, 1)
    assert lib.ssbev_dwconv2d_bwd_weight_layout(C.byref(good), C.byref(Q), C.byref(L), C.byref(qb)) == capi.OK
    assert lib.ssbev_dwconv2d_bwd_weight_layout(C.byref(good), None, C.byref(L), C.byref(qb)) == capi.EINVAL
    for why, fields in {"C % 4": dict(C=6), "k": dict(k=4), "stride": dict(stride=3), "B = 0": dict(B=0)}.items():
        d = capi.DwDims(1, 8, 4, 4, 4, 4, 3, 1, 1, 1)
        for n, v in fields.items():
            setattr(d, n, v)
        assert lib.ssbev_dwconv2d_bwd_weight_layout(C.byref(d), C.byref(Q), C.byref(L), C.byref(qb)) == capi.EINVAL, why
        assert lib.ssbev_dwconv2d_bwd_weight_workspace(C.byref(d)) == 0, why
    assert lib.ssbev_stream_blocks(0) == 0 and lib.ssbev_stream_blocks(1) == 1
    assert lib.ssbev_softmax_axis_slices(0, 32) == 0 and lib.ssbev_softmax_axis_slices(64, 0) == 0
    assert lib.ssbev_chan_sum_workspace(1, 10, 6) == 0
