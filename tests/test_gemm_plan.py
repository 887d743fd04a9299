"""CPU: the case table of test_gpu_gemm_paths.py really reaches every kernel, split and tail of csrc/gemm.hip.

Every case of gemm_cases.CASES is asked of the library itself (ssbev_gemm_plan_query, which reads the plan functions the
launchers and the *_workspace queries read): it reports the intended kernel, and nchunk / per_chunk give exactly the properties
the case is listed for.  A change to a cost constant or a threshold that moves a GPU case to another kernel, or takes its split,
short last chunk or empty chunk away, fails here on a box without a GPU.

cfg 4 of gemm_nn_kernel (16-deep k stages) is reachable through the SSBEV_GEMM_CFG hook of a tuning build only; nothing here
forces or tests it."""
import ctypes as C
import random

import pytest

import gemm_cases as T
from stereoscene_amd import capi


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_runs_its_kernel_with_its_properties(case):
    d = T.case_dims(case)
    p = T.query(d, case.form)
    assert not isinstance(p, int), p
    assert (p.kernel, p.nchunk, p.per_chunk) == (case.kernel, case.nchunk, case.per_chunk), T.plan_tuple(p)
    assert T.plan_props(case.form, case.shape, p) == case.props & T.PLAN_PROPS, T.plan_tuple(p)
    assert p.workspace == T.workspace(d, case.form)
    assert (p.workspace > 0) == (T.SPLIT in case.props)
    batch, M, K, N = case.shape
    out_elems = batch * (K if case.form == T.TN else M) * N
    if T.SPLIT in case.props:
        assert p.workspace == p.nchunk * out_elems * 4                 # one partial result per chunk / skinny workgroup
    if case.form != T.TN:
        nst = -(-K // p.bk)
        assert (p.nchunk - 1) * p.per_chunk < nst <= p.nchunk * p.per_chunk      # no split-K chunk is empty
        assert p.grid == batch * p.nchunk * -(-M // p.bm) * -(-N // p.bn)
        if T.SUM_EPILOGUE in case.props:
            assert T.SPLIT in case.props
    elif p.kernel >= T.SK_11:
        assert p.grid == batch * p.nchunk and M >= 32768
        runs = p.nchunk * (1 if p.kernel == T.SK_QUAD else 4)
        assert runs * p.per_chunk >= M and p.per_chunk % 2 == 0
    else:
        assert p.grid == batch * p.nchunk * -(-K // p.bm) * -(-N // p.bn)
        assert p.nchunk * p.per_chunk >= M and p.per_chunk % 32 == 0
        if T.EP_MUL in case.props:
            assert p.nchunk == 1 and M <= 2048
    if T.STRIDED in case.props:
        assert d.lda > K and d.ldb > (K if case.form == T.NT else N)
    if T.STRIDED_C in case.props:
        assert d.ldc > N and d.sc > M * d.ldc


def test_table_covers_every_kernel_and_property():
    for form in (T.NN, T.NT, T.TN):
        cases = [c for c in T.CASES if c.form == form]
        assert {c.kernel for c in cases} == T.ALL_KERNELS[form]
        props = set().union(*(c.props for c in cases))
        if form == T.TN:
            assert props == (T.PLAN_PROPS - {T.SHORT_LAST, T.CAP16}) | {T.STRIDED, T.EP_MUL, T.BOUNDARY}
            assert {c.kernel for c in cases if T.STRIDED in c.props} >= {T.TN_WIDE, T.SK_22}
            assert {c.kernel for c in cases if T.EP_MUL in c.props} == {T.TN_1, T.TN_2}
            assert {c.shape[1] for c in cases if T.BOUNDARY in c.props} == {32767, 32768}
            continue
        assert props == (T.PLAN_PROPS - {T.EMPTY_CHUNK, T.EMPTY_RUN}) | {T.SHARED_B, T.SUM_EPILOGUE, T.STRIDED, T.STRIDED_C}
        for cfg in T.ALL_KERNELS[form]:         # every tile configuration runs unsplit and with split-K (bias + ReLU in the sum pass)
            assert {T.SPLIT in c.props for c in cases if c.kernel == cfg} == {False, True}, cfg
            assert any(T.SUM_EPILOGUE in c.props for c in cases if c.kernel == cfg)
        strided = [c for c in cases if T.STRIDED in c.props]
        assert all(T.STRIDED_C in c.props for c in strided)
        assert {T.SPLIT in c.props for c in strided} == {False, True}
    # the two forms run the same shapes
    assert [c[1:] for c in T.CASES if c.form == T.NN] == [c[1:] for c in T.CASES if c.form == T.NT]


LEGACY_PLANS = {   # shape: (kernel, nchunk, per_chunk) of NN, NN with batch 1, NT, TN, TN with the fused epilogue
    (1, 300, 128, 96): ((1, 1, 4), (1, 1, 4), (1, 1, 4), (11, 1, 320), (11, 1, 320)),
    (1, 7680, 3200, 640): ((3, 2, 50), (3, 2, 50), (3, 2, 50), (11, 8, 960), None),
    (3, 200, 64, 160): ((1, 1, 2), (1, 1, 2), (1, 1, 2), (10, 1, 224), (10, 1, 224)),
    (1, 130, 36, 20): ((1, 1, 2), (1, 1, 2), (1, 1, 2), (10, 1, 160), (10, 1, 160)),
    (2, 1920, 640, 640): ((0, 1, 20), (1, 1, 20), (0, 1, 20), (11, 7, 288), (11, 1, 1920)),
    (1, 64, 192, 7680): ((1, 1, 6), (1, 1, 6), (1, 1, 6), (11, 1, 64), (11, 1, 64)),
    (1, 40000, 32, 64): ((1, 1, 1), (1, 1, 1), (1, 1, 1), (21, 39, 258), None),
    (2, 33000, 64, 36): ((1, 1, 2), (1, 1, 2), (1, 1, 2), (23, 32, 258), None),
    (1, 34000, 128, 100): ((1, 1, 4), (1, 1, 4), (1, 1, 4), (24, 132, 258), None),
    (1, 33000, 96, 128): ((1, 1, 3), (1, 1, 3), (1, 1, 3), (24, 128, 258), None),
}


@pytest.mark.parametrize("shape", T.LEGACY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_plans_of_the_shapes_of_test_gemm_nn_nt_tn_vs_torch(shape):
    """What test_gpu_kernels.py::test_gemm_nn_nt_tn_vs_torch launches, pinned: a later change that moves its shapes shows up."""
    batch, M, K, N = shape
    runs = ((T.NN, shape, None), (T.NN, (1, M, K, N), None), (T.NT, shape, None), (T.TN, shape, None),
            (T.TN, shape, (T.FAKE, T.FAKE)))
    for (form, s, ep), want in zip(runs, LEGACY_PLANS[shape]):
        if want is None:
            assert ep and M > 2048          # the test runs the fused epilogue up to 2048 rows
            continue
        p = T.query(T.dims(form, s, ep=ep), form)
        assert (p.kernel, p.nchunk, p.per_chunk) == want, (form, s, T.plan_tuple(p))


def _random_problem(rng):
    """(form, dims, reference arguments) of a random valid problem: all three forms, plain / d2s / fused epilogue."""
    form = rng.choice((T.NN, T.NT, T.TN))
    span = lambda hi: int(2 ** rng.uniform(0, hi))
    mult4 = lambda hi: 4 * max(1, span(hi) // 4) if rng.random() < 0.7 else rng.choice((32, 64, 128, 160, 192, 320, 640))
    batch = rng.choice((1, 1, 1, 2, 3, 8, 9, 16)) if rng.random() < 0.8 else span(5)
    M, K, N = span(17.5 if form == T.TN else 13.5), mult4(13), mult4(13)
    if form == T.TN and rng.random() < 0.3:          # around the skinny thresholds
        M, K, N = rng.choice((32767, 32768, 40000, 131073)) if rng.random() < 0.5 else M, mult4(7.2), mult4(7.2)
    if rng.random() < 0.15:                          # the BRI family: 192-row tiles
        M = rng.choice((190, 192, 200, 380, 384, 576))
    d = T.dims(form, (batch, M, K, N), (rng.choice((0, 4)), rng.choice((0, 8)), rng.choice((0, 3)), 0))
    Co, ep = 0, False
    kind = rng.random()
    if kind < 0.2:                                   # depth-to-space map of a k == s deconvolution
        taps = rng.choice((1, 2, 4, 8, 27))
        Co = 64 * rng.randint(1, 6)
        grid = rng.choice(((1, 1, 1), (2, 3, 4), (1, 5, 2)))
        M = grid[0] * grid[1] * grid[2] * rng.randint(1, 40)
        wide, batch = taps * Co, 1
        K, N = (wide, N) if form == T.NT else (K, wide)
        d = T.dims(form, (batch, M, K, N))
        d.d2s_D, d.d2s_H, d.d2s_W = grid
        d.d2s_kd, d.d2s_kh, d.d2s_kw = {1: (1, 1, 1), 2: (2, 1, 1), 4: (1, 2, 2), 8: (2, 2, 2), 27: (3, 3, 3)}[taps]
        d.d2s_Co, d.d2s_rowoff = Co, T.FAKE
    elif kind < 0.35 and form == T.TN:
        ep = True
        d.ep_mul = d.ep_rowsub = T.FAKE
    return form, d, (form, M, N, K, batch, Co, ep)


def test_query_matches_a_transcription_of_the_previous_dispatch_on_random_problems():
    """The launchers' choices were moved into plan_nn / plan_tn without changing any: 60000 random problems (NN, NT, TN; plain, d2s
    and fused-epilogue dims) get the plan that gemm_cases.reference_plan, a transcription of the dispatch before the move,
    computes, and the *_workspace functions return the plan's workspace."""
    rng = random.Random(20261018)
    seen, refused = set(), 0
    for i in range(60000):
        form, d, ref_args = _random_problem(rng)
        p = T.query(d, form)
        if ref_args[-1] and T.reference_plan(*ref_args)[0] >= T.SK_11:
            assert p == capi.EINVAL                                   # the fused epilogue has no skinny realisation
            refused += 1
            continue
        assert not isinstance(p, int), (i, ref_args)
        assert T.plan_tuple(p) == T.reference_plan(*ref_args), (i, ref_args)
        assert T.workspace(d, form) == p.workspace, (i, ref_args)
        seen.add((form, p.kernel, p.nchunk > 1, ref_args[5] > 0, ref_args[6]))
    kernels = {(f, k) for f, k, *_ in seen}
    assert kernels == {(f, k) for f in T.ALL_KERNELS for k in T.ALL_KERNELS[f]}
    for form in (T.NN, T.NT, T.TN):                    # split and unsplit, d2s and the fused epilogue were all drawn
        assert {s for f, _, s, _, _ in seen if f == form} == {False, True}
        assert {x for f, _, _, x, _ in seen if f == form} == {False, True}
    assert {e for f, _, _, _, e in seen if f == T.TN} == {False, True} and refused > 0


def _entry(form, d, ws=None, ws_bytes=0, null=()):
    """The real entry point on never-dereferenced pointers (operand i of `null` a null pointer: A, B, C): it must answer before any
    device work."""
    lib = capi.load()
    a, b, c = (None if i in null else C.c_void_p(T.FAKE) for i in range(3))
    if form == T.TN:
        return lib.ssbev_gemm_tn(a, b, c, C.byref(d), ws, ws_bytes, None)
    fn = lib.ssbev_gemm_nn if form == T.NN else lib.ssbev_gemm_nt
    return fn(a, b, None, c, C.byref(d), ws, ws_bytes, None)


def _refused(form, d, why=None):
    """SSBEV_EINVAL from the query and then from the entry point.  The entry point is only called once the query, which reads the
    same dims check, has refused, and it is given no workspace: dims that a later change lets through fail here on the query, or
    come back as SSBEV_EWORKSPACE from a split problem, before anything could be launched on the placeholder pointers."""
    assert T.query(d, form) == capi.EINVAL, why
    assert _entry(form, d) == capi.EINVAL, why


@pytest.mark.parametrize("form", (T.NN, T.NT, T.TN), ids=T.FORM_NAMES.get)
def test_refusals_come_from_the_query_and_the_entry_point_alike(form):
    """Every rejection of gemm_ok and of the entry points is SSBEV_EINVAL from the query and from the entry point (before any HIP
    call: the placeholder pointers are never dereferenced, with or without a GPU); a workspace one byte short is SSBEV_EWORKSPACE."""
    lib = capi.load()
    assert lib.ssbev_version() >= 106
    shape = (2, 1900, 1540, 640)                      # a split-K / row-chunked problem in every form
    good = lambda: T.dims(form, shape)
    dense_b = 1540 if form == T.NT else 640
    p = T.query(good(), form)
    assert not isinstance(p, int) and p.nchunk > 1 and p.workspace > 0
    plan = capi.GemmPlan()
    assert lib.ssbev_gemm_plan_query(None, form, C.byref(plan)) == capi.EINVAL
    assert lib.ssbev_gemm_plan_query(C.byref(good()), form, None) == capi.EINVAL
    assert lib.ssbev_gemm_plan_query(C.byref(good()), 3, C.byref(plan)) == capi.EINVAL
    assert lib.ssbev_gemm_plan_query(C.byref(good()), -1, C.byref(plan)) == capi.EINVAL
    bad = {
        "K % 4": dict(K=1542, lda=1544, ldb=1544 if form == T.NT else 640),
        "N % 4": dict(N=642, ldb=1540 if form == T.NT else 644, ldc=644),
        "lda % 4": dict(lda=1542),
        "ldb % 4": dict(ldb=dense_b + 2),
        "lda < K": dict(lda=1536),
        "ldb too small": dict(ldb=dense_b - 4),
        "M = 0": dict(M=0),
        "batch = 0": dict(batch=0),
        "ldc < 0": dict(ldc=-1),
    }
    if form != T.TN:
        bad["ldc too small"] = dict(ldc=639)
    for why, fields in bad.items():
        d = good()
        for k, v in fields.items():
            setattr(d, k, v)
        _refused(form, d, why)
        fn = (lib.ssbev_gemm_nn_workspace, lib.ssbev_gemm_nt_workspace, lib.ssbev_gemm_tn_workspace)[form]
        if why in ("K % 4", "N % 4", "lda % 4", "ldb % 4", "M = 0", "batch = 0", "ldc < 0"):      # gemm_ok's own: no workspace either
            assert fn(C.byref(d)) == 0, why
    # null operands are this form's entry point's to refuse, each of A, B and C on its own; the query has none
    for null in ((0,), (1,), (2,), (0, 1, 2)):
        assert _entry(form, good(), null=null) == capi.EINVAL, null
    # workspace: missing, or one byte short
    assert _entry(form, good(), None, 0) == capi.EWORKSPACE
    assert _entry(form, good(), C.c_void_p(T.FAKE), p.workspace - 1) == capi.EWORKSPACE
    assert _entry(form, good(), None, p.workspace) == capi.EWORKSPACE
    # d2s dims: answered when consistent, refused otherwise
    d = T.dims(form, (1, 48, 128, 1024) if form != T.NT else (1, 48, 1024, 128))
    d.d2s_D, d.d2s_H, d.d2s_W, d.d2s_kd, d.d2s_kh, d.d2s_kw, d.d2s_Co, d.d2s_rowoff = 2, 3, 4, 2, 2, 2, 128, T.FAKE
    p = T.query(d, form)
    assert not isinstance(p, int)
    assert p.kernel == (T.TN_2 if form == T.TN else T.CFG_128x128)
    assert form != T.NN or p.nchunk == 1                                  # the scatter epilogue writes final values
    for why, fields in {"batch": dict(batch=2), "taps x Co": dict(d2s_Co=64), "Co % 64": dict(d2s_Co=32, d2s_kd=8),
                        "rows": dict(d2s_D=5), "no table": dict(d2s_rowoff=None), "kh = 0": dict(d2s_kh=0)}.items():
        e = capi.GemmDims.from_buffer_copy(d)
        for k, v in fields.items():
            setattr(e, k, v)
        _refused(form, e, why)


def test_fused_epilogue_refusals():
    """ep_mul without ep_rowsub (and the reverse), on a skinny problem and on a d2s problem: SSBEV_EINVAL before any device work;
    forms other than TN ignore the two fields."""
    small, skinny = (1, 1000, 200, 100), (1, 33000, 64, 36)
    for ep in ((T.FAKE, None), (None, T.FAKE)):
        d = T.dims(T.TN, small, ep=ep)
        _refused(T.TN, d, ep)
    d = T.dims(T.TN, small, ep=(T.FAKE, T.FAKE))
    p = T.query(d, T.TN)
    assert (p.kernel, p.nchunk, p.workspace) == (T.TN_2, 1, 0)
    assert T.query(T.dims(T.TN, small), T.TN).nchunk == 3                  # ... which the plain product would cut in three
    d = T.dims(T.TN, skinny, ep=(T.FAKE, T.FAKE))
    _refused(T.TN, d, "skinny")
    assert T.query(T.dims(T.TN, skinny), T.TN).kernel == T.SK_22
    d = T.dims(T.TN, (1, 48, 128, 1024), ep=(T.FAKE, T.FAKE))
    d.d2s_D, d.d2s_H, d.d2s_W, d.d2s_kd, d.d2s_kh, d.d2s_kw, d.d2s_Co, d.d2s_rowoff = 2, 3, 4, 2, 2, 2, 128, T.FAKE
    _refused(T.TN, d, "d2s")
    # the wide TN tile is not taken under the fused epilogue
    wide = (8, 1030, 260, 320)
    assert T.query(T.dims(T.TN, wide), T.TN).kernel == T.TN_WIDE
    assert T.query(T.dims(T.TN, wide, ep=(T.FAKE, T.FAKE)), T.TN).kernel == T.TN_1
