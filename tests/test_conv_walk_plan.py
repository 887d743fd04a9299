"""CPU: the case table of test_gpu_conv_walks.py really launches multi-block walks.

Every case of conv_walk_cases.CASES is asked of the library itself (ssbev_conv_kernel_class and the host-side plan query
ssbev_conv_chunk_groups, which shares its plan functions with the launchers): the intended kernel serves it, a workgroup walks
at least two row groups, and the launch has exactly the walk properties the case is listed for.  A change to an *_applicable
predicate or to a cost loop that would move a GPU case back to one block per chunk (or onto another kernel) fails here."""
import ctypes as C

import pytest

import conv_walk_cases as T
from stereoscene_amd import capi

WALK_CLASSES = (1, 2, 7, 8, 9, 17)


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_runs_its_kernel_with_a_multi_block_walk(case):
    served = set()
    for name, call in T.calls(case).items():
        for mode in (0, 1):
            want = call["classes"][mode]
            if want is None:
                continue
            cls, gpc = T.query(case, call, mode)
            assert cls == want, (name, mode, cls)
            assert gpc >= 2, (name, mode, gpc)
            NG, H2, nseg = T.walk_geometry(case, cls)
            assert gpc < NG
            props = T.walk_properties(gpc, NG, H2, nseg, case.B)
            assert props == case.props, (name, mode, gpc, NG, H2, nseg, sorted(props))
            # the definitions in words: a straddled plane (pair) needs a chunk that is no divisor of the plane or longer than it,
            # a straddled batch boundary a sample that is no whole number of chunks
            if T.PLANE in props:
                assert gpc % H2 != 0 or gpc > H2
            assert (T.BATCH in props) == (case.B >= 2 and (NG // case.B) % gpc != 0)
            served.add(cls)
        # weight gradient: wgrad_tapdh_kernel walks the same 2 x 2 blocks wherever plan_wgrad_dh takes the problem
        _, wg = T.query(case, call, 2)
        if T.KERNELS[case.kernel][3]:
            assert wg >= 2, (name, wg)
            NG, H2, nseg = T.walk_geometry(case, 9)
            assert T.walk_properties(wg, NG, H2, nseg, case.B) >= case.props - {T.GRID8}
        else:
            assert wg == 0, (name, wg)
    assert served == ({7, 8} if case.kernel == "tap2" else {T.KERNELS[case.kernel][2]})


def test_table_covers_every_kernel_property_and_epilogue():
    by_kernel = {}
    for c in T.CASES:
        by_kernel.setdefault(c.kernel, []).append(c)
    assert set(by_kernel) == set(T.KERNELS)
    covered = set().union(*(c.props for c in T.CASES))
    assert covered == {T.PLANE, T.BATCH, T.SHORT, T.GRID8}
    tapdh = set().union(*(c.props for c in by_kernel["tapdh"]))
    assert tapdh == covered                                   # the XCD remap remainder is conv_tapdh_kernel's
    # ReLU + bias and the accumulating epilogue run on later blocks of a chunk (every case has gpc >= 2, see above)
    epi = [c.kernel for c in T.CASES if c.epilogues]
    assert sorted(epi) == ["tap", "tap2", "tapdh", "tapdh", "taph"]
    for c in T.CASES:
        if c.B >= 2:
            continue
        assert T.BATCH not in c.props


def test_chunk_query_answers_zero_off_the_walking_kernels():
    """ssbev_conv_chunk_groups does no device work and answers 0 for every launch that is not a ring walk."""
    lib = capi.load()
    assert lib.ssbev_version() >= 105
    q = lambda d, mode: lib.ssbev_conv_chunk_groups(C.byref(d), mode)
    assert lib.ssbev_conv_chunk_groups(None, 0) == 0
    small = capi.ConvDims(1, 32, 32, 5, 6, 40, 5, 6, 40, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    assert lib.ssbev_conv_kernel_class(C.byref(small), 0) == 0 and [q(small, m) for m in (0, 1, 2, 3, -1)] == [0] * 5
    # the hinted cases of test_conv_tap_split_lds_kernel are one-block walks: the gap the table above closes
    for hint in (9, 6):
        small.tile_hint = hint
        assert lib.ssbev_conv_kernel_class(C.byref(small), 0) in (1, 2, 9) and q(small, 0) == 1 and q(small, 1) == 1
    wide = capi.ConvDims(1, 64, 64, 8, 8, 8, 8, 8, 8, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    assert [q(wide, m) for m in (0, 1, 2)] == [0, 0, 0]
    # the workload's own 32 -> 32 cost-volume layer: the multi-block walks of the full-size tests
    full = capi.ConvDims(1, 32, 32, 192, 48, 160, 192, 48, 160, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)
    assert lib.ssbev_conv_kernel_class(C.byref(full), 0) == 9
    assert q(full, 0) >= 2 and q(full, 1) == q(full, 0) and q(full, 2) >= 2
    full.tile_hint = 4
    assert lib.ssbev_conv_kernel_class(C.byref(full), 0) == 2 and q(full, 0) >= 2 and q(full, 2) == 0
    full.tile_hint, full.precision = 0, 2
    assert lib.ssbev_conv_kernel_class(C.byref(full), 0) == 17 and q(full, 0) >= 24 and q(full, 2) == 0
