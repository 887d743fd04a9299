"""CPU: the case table of test_gpu_gwc_paths.py really reaches every forward kernel, backward realisation and chunk plan of
csrc/gwc_warp.hip, and every plan the launchers can make is a legal launch.

Every case of gwc_cases.CASES is asked of the library itself (ssbev_gwc_plan_query, which reads the plan functions the launchers
and ssbev_gwc_warp_bwd_workspace read).  A threshold change that moves a GPU case to another kernel, or takes its chunk plan
away, fails here on a box without a GPU.  The sweep asserts, for every shape gwc_dims_ok accepts on a grid of G, cpg, W, D and
row counts, that the block respects the chosen kernel's launch bound and divisibility, that the LDS fits and that the chunk
starts are a partition of the planes: G = 36 (a 576-thread block on a 512-thread kernel before the fix) is among them."""
import ctypes as C

import pytest
import torch

import gwc_cases as T
from stereoscene_amd import capi


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_runs_its_kernels_with_its_properties(case):
    B, Cc, G, H, W, D = case.shape
    for ac in (True, False):                      # the plan does not depend on the convention
        p = T.query(T.dims(case.shape, ac))
        assert not isinstance(p, int), p
        assert (p.fwd_kernel, p.bwd_kernel, p.fwd_nchunks, p.bwd_nchunks) == (case.fwd, case.bwd, case.nf, case.nb), T.plan_tuple(p)
        assert T.plan_props(case.shape, p) == case.props & T.PLAN_PROPS, (sorted(T.plan_props(case.shape, p)), T.plan_tuple(p))
        assert (p.fwd_rc == capi.EINVAL) == (T.F_EINVAL in case.props) and (p.bwd_rc == capi.EINVAL) == (T.B_EINVAL in case.props)
        assert p.direct_rc == p.bwd_rc or p.bwd_kernel != T.BWD_TWO
        assert p.bwd_workspace == capi.load().ssbev_gwc_warp_bwd_workspace(C.byref(T.dims(case.shape, ac)))
    if T.NONFINITE in case.props:
        assert set("npm") <= set(case.cal)
    if T.DIRECT in case.props:
        assert p.bwd_kernel == T.BWD_3 and p.direct_rc == capi.OK
    if T.WORKSPACE in case.props:
        assert p.bwd_nchunks > 1 and p.bwd_workspace > 0
    assert B * G * D * H * W * 4 <= 26e6           # the volume stays small


def test_table_covers_every_kernel_and_property():
    cases = T.CASES
    cpg = lambda c: c.shape[1] // c.shape[2]
    assert {(c.fwd, cpg(c)) for c in cases if c.fwd} == {(k, w) for k in (T.FWD_PLANE, T.FWD_4, T.FWD_5) for w in (1, 2, 4, 8)}
    assert {(c.bwd, cpg(c)) for c in cases if c.bwd} == ({(k, w) for k in (T.BWD_TWO, T.BWD_2) for w in (1, 2, 4, 8)} |
                                                         {(T.BWD_3, 1), (T.BWD_3, 2)})
    assert set().union(*(c.props for c in cases)) == T.PLAN_PROPS | T.RUN_PROPS
    # fwd5 blocks: G / 4 = 1, 3, 5, 8, 16, 64 (256, 192 and 320 threads; 256 .. 4 pixels per tile)
    assert {c.shape[2] // 4 for c in cases if c.fwd == T.FWD_5} >= {1, 3, 5, 8, 16, 64}
    assert {c.shape[2] for c in cases if c.fwd == T.FWD_PLANE} >= {1, 6, 36, 16}
    # bwd3: every group count, both conventions, one chunk / the cap / one plane per chunk
    b3 = [c for c in cases if c.bwd == T.BWD_3]
    assert {c.shape[2] for c in b3} == {4, 8, 16, 32, 64}
    assert set().union(*(c.props for c in b3)) >= {T.B3_256, T.B3_640, T.B3_768, T.N48, T.N_EQ_D, T.ONE_CHUNK, T.LEN1}
    assert {ac for c in b3 for ac in c.acs} == {True, False}
    b2 = [c for c in cases if c.bwd == T.BWD_2]
    assert set().union(*(c.props for c in b2)) >= {T.B2_RAGGED_Q, T.B2_RAGGED_W, T.ONE_CHUNK, T.N48}
    # every calibration regime, and the non-finite ones on a bwd3, a bwd2 and a fwd5 case
    assert set("".join(c.cal for c in cases)) == set("abcdenpm")
    nf = [c for c in cases if T.NONFINITE in c.props]
    assert {T.BWD_3, T.BWD_2} <= {c.bwd for c in nf} and T.FWD_5 in {c.fwd for c in nf}
    for c in cases:
        if len(c.cal) >= 4 and c.bwd in (T.BWD_2, T.BWD_3):
            assert set("acd") <= set(c.cal), c
    # determinism on a bwd3 case and on a bwd2 case with many chunks
    det = [c for c in cases if T.DETERMINISM in c.props]
    assert {c.bwd for c in det} == {T.BWD_3, T.BWD_2} and all(c.nb >= 32 for c in det)
    assert {c.shape[4] for c in cases if T.B_EINVAL in c.props} >= {594, 600, 601, 602}


def _check_plan(shape, p):
    """The properties every plan must have; returns (fwd kernel, bwd kernel)."""
    B, Cc, G, H, W, D = shape
    cpg = Cc // G
    if p.fwd_rc == capi.OK:
        assert p.fwd_kernel in (T.FWD_PLANE, T.FWD_4, T.FWD_5)
        assert p.fwd_threads % 64 == 0 and 64 <= p.fwd_threads <= (256 if p.fwd_kernel == T.FWD_PLANE else 512), shape
        assert p.fwd_lds <= T.LDS_LIMIT, shape
        st = T.starts(p, "fwd")
        assert st[0] == 0 and st[-1] == D and all(a < b for a, b in zip(st, st[1:])), (shape, st)
        if p.fwd_kernel != T.FWD_PLANE:
            assert G % 4 == 0 and p.fwd_threads % (G // 4) == 0, shape
            assert p.fwd_px == p.fwd_threads // (G // 4) and p.fwd_nchunks <= min(D, 48), shape
            assert p.fwd_tiles == (-(-W // p.fwd_px) if p.fwd_kernel == T.FWD_5 else 1)
            need = W * (Cc + 4) * 4 + (12 * D if p.fwd_kernel == T.FWD_5 else 384)
            assert p.fwd_lds == need, shape
        if p.fwd_kernel == T.FWD_4:
            assert max(b - a for a, b in zip(st, st[1:])) <= 32, shape
        if p.fwd_kernel == T.FWD_PLANE:
            assert p.fwd_nchunks == -(-D // 16) and p.fwd_lds == W * (Cc + 4) * 4 + 192
    else:
        assert p.fwd_rc == capi.EINVAL and W * (Cc + 4) * 4 + 192 > T.LDS_LIMIT, shape
        assert (p.fwd_kernel, p.fwd_threads, p.fwd_nchunks, p.fwd_lds) == (0, 0, 0, 0)
    two_lds = W * (Cc + 4) * 4 + D * 12 + G * T.MAX_SRC * 8 + G * 4
    assert (p.direct_rc == capi.OK) == (two_lds <= T.LDS_LIMIT), shape
    if p.direct_rc == capi.OK:
        assert p.direct_lds == two_lds and p.direct_threads == min(1024, max(256, -(-32 * G // 64) * 64))
    if p.bwd_rc == capi.OK:
        assert p.bwd_kernel in (T.BWD_TWO, T.BWD_2, T.BWD_3)
        bound = 1024 if p.bwd_kernel == T.BWD_TWO else 768
        assert p.bwd_threads % 64 == 0 and 64 <= p.bwd_threads <= bound and p.bwd_lds <= T.LDS_LIMIT, shape
        st = T.starts(p, "bwd")
        assert st[0] == 0 and st[-1] == D and all(a < b for a, b in zip(st, st[1:])), (shape, st)
        assert p.bwd_nchunks <= min(D, 48)
        assert p.bwd_workspace == (2 * p.bwd_nchunks * B * H * W * Cc * 4 if p.bwd_nchunks > 1 else 0), shape
        if p.bwd_kernel == T.BWD_TWO:
            assert p.bwd_nchunks == 1 and (p.bwd_threads, p.bwd_lds) == (p.direct_threads, p.direct_lds)
        else:
            maxi = 2 if cpg == 8 else 4 if cpg == 4 else 8
            assert p.bwd_threads % G == 0 and p.bwd_lds == T.bwd2_lds(shape), shape
            assert 2 * p.bwd_threads >= W * G // 4 and maxi * (p.bwd_threads // G) >= W, shape      # every quad and pixel has an owner
        if p.bwd_kernel == T.BWD_3:                # no tails: the kernel has no range checks
            assert cpg in (1, 2) and 2 * p.bwd_threads == W * (G // 4) and 8 * (p.bwd_threads // G) == W, shape
    else:
        assert p.bwd_rc == capi.EINVAL and p.direct_rc == capi.EINVAL, shape
        assert (p.bwd_kernel, p.bwd_threads, p.bwd_nchunks, p.bwd_lds, p.bwd_workspace) == (0, 0, 0, 0, 0)
    return p.fwd_kernel, p.bwd_kernel


def test_every_plan_of_the_sweep_is_a_legal_launch():
    seen = set()
    plan = capi.GwcPlan()
    fn = capi.load().ssbev_gwc_plan_query
    for G in range(1, 257):
        for cpg in (1, 2, 4, 8):
            Cc = G * cpg
            if Cc % 4:
                continue
            for W in (1, 17, 160, 600, 602):
                for D in (1, 5, 48, 192):
                    for B, H in ((1, 1), (2, 1), (2, 65), (3, 100)):
                        shape = (B, Cc, G, H, W, D)
                        assert fn(C.byref(T.dims(shape, 1)), C.byref(plan)) == capi.OK, shape
                        seen.add((_check_plan(shape, plan), cpg))
    assert {k for (k, _), _ in seen} == {0, T.FWD_PLANE, T.FWD_4, T.FWD_5}
    assert {(k, w) for (_, k), w in seen if k} == ({(k, w) for k in (T.BWD_TWO, T.BWD_2) for w in (1, 2, 4, 8)} |
                                                   {(T.BWD_3, 1), (T.BWD_3, 2)})
    # the shapes whose fwd4 / fwd5 block would exceed the kernels' launch bound take the per-plane kernel
    for G in (36, 44, 52, 60, 72, 180):
        p = T.query(T.dims((1, G, G, 1, 17, 5), 1))
        assert (p.fwd_kernel, p.fwd_threads) == (T.FWD_PLANE, 256), G
    for G in (28, 40, 56):                         # 448, 320, 448 threads: legal
        assert T.query(T.dims((1, G, G, 1, 17, 5), 1)).fwd_kernel == T.FWD_5, G


def test_refusals_come_from_the_query_and_the_entry_points_alike():
    """SSBEV_EINVAL and SSBEV_EWORKSPACE are answered before any device work: the placeholder pointers are never dereferenced,
    with or without a GPU."""
    lib = capi.load()
    assert lib.ssbev_version() >= 116
    fake = C.c_void_p(256)
    plan = capi.GwcPlan()
    good = T.dims((4, 32, 32, 1, 160, 192), 1)
    assert lib.ssbev_gwc_plan_query(None, C.byref(plan)) == capi.EINVAL
    assert lib.ssbev_gwc_plan_query(C.byref(good), None) == capi.EINVAL
    for bad in ((1, 30, 15, 1, 8, 8), (1, 64, 24, 1, 8, 8), (1, 64, 4, 1, 8, 8), (1, 64, 32, 1, 0, 8), (0, 64, 32, 1, 8, 8)):
        d = T.dims(bad, 1)
        assert T.query(d) == capi.EINVAL, bad
        assert lib.ssbev_gwc_warp_fwd(fake, fake, fake, fake, C.byref(d), None) == capi.EINVAL
        assert lib.ssbev_gwc_warp_bwd(fake, fake, fake, fake, fake, fake, C.byref(d), None) == capi.EINVAL
        assert lib.ssbev_gwc_warp_bwd_fused(fake, fake, fake, fake, fake, fake, C.byref(d), fake, 1 << 40, None) == capi.EINVAL
        assert lib.ssbev_gwc_warp_bwd_workspace(C.byref(d)) == 0
    # wide rows: every entry point whose plan says SSBEV_EINVAL answers it (the plan is made before anything is launched)
    for W in (594, 600, 601, 602):
        d = T.dims((1, 64, 16, 1, W, 192), 1)
        p = T.query(d)
        assert (p.fwd_rc, p.bwd_rc, p.direct_rc) == (capi.EINVAL if W == 602 else capi.OK, capi.EINVAL, capi.EINVAL)
        assert lib.ssbev_gwc_warp_bwd(fake, fake, fake, fake, fake, fake, C.byref(d), None) == capi.EINVAL
        assert lib.ssbev_gwc_warp_bwd_fused(fake, fake, fake, fake, fake, fake, C.byref(d), fake, 1 << 40, None) == capi.EINVAL
    assert lib.ssbev_gwc_warp_fwd(fake, fake, fake, fake, C.byref(T.dims((1, 64, 16, 1, 602, 192), 1)), None) == capi.EINVAL
    # a multi-chunk plan without its workspace
    p = T.query(good)
    assert p.bwd_nchunks == 48 and p.bwd_workspace == 2 * 48 * 4 * 160 * 32 * 4
    args = (fake, fake, fake, fake, fake, fake, C.byref(good))
    assert lib.ssbev_gwc_warp_bwd_fused(*args, None, p.bwd_workspace, None) == capi.EWORKSPACE
    assert lib.ssbev_gwc_warp_bwd_fused(*args, fake, p.bwd_workspace - 1, None) == capi.EWORKSPACE
    assert lib.ssbev_gwc_warp_bwd_fused(*args, fake, 0, None) == capi.EWORKSPACE


@pytest.mark.parametrize("shape,cal,ac", [((3, 16, 8, 2, 21, 12), (50.4, -2.0, 300.0), True),
                                          ((2, 8, 8, 1, 9, 24), (2.0, 21.6), False),
                                          ((2, 32, 4, 2, 13, 7), (31.2, 0.0), False)])
def test_float64_reference_agrees_with_the_fp32_oracle(shape, cal, ac):
    """Ties the float64 reference to the one the golden files were made from: the fp32 oracle is itself one fp32 evaluation of the
    operation, so it meets the derived bound (its own chains: cpg + 4 forward; the gradient of an input element sums 2 D taps
    of up to MAX_SRC groups)."""
    B, Cc, G, H, W, D = shape
    c = T.Case(shape, "a" * B, (ac,), 0, 0, 0, 0, frozenset())
    L, R, go = T.features(c)
    calib = torch.tensor(cal)
    ref = T.reference(L, R, go, calib, D, G, ac)
    mag = T.magnitude(L, R, go, calib, D, G, ac)
    got = T.reference(L, R, go, calib, D, G, ac, dtype=torch.float32)
    for name, g, r, a, n in zip(("vol", "gL", "gR"), got, ref, mag, (T.n_fwd(shape), 2 * D * T.MAX_SRC, 2 * D * T.MAX_SRC)):
        ratio = ((g.double() - r).abs() / (T.gamma(n) * a).clamp_min(1e-300)).max().item()
        assert ratio <= 1.0, (name, ratio)
        assert ((g.double() - r).abs()[a == 0] == 0).all()
