"""CPU: the host-side dispatch of the ssbev_conv_* entry points against a recorded snapshot.

tests/golden/conv_dispatch.json (tools/make_golden_conv_dispatch.py) holds, for a few thousand ssbev_conv_dims, what the library
of the commit named in the file answered: kernel class and chunk groups for modes 0 / 1 / 2, packed-weight elements and the
weight-gradient workspace; the generic-gather rows again under SSBEV_IGEMM=0; and the SSBEV_EINVAL answers of the launchers that
return before any device call.  Every value must be reproduced exactly: a weight packed for one kernel and launched with
another is silently wrong, and a workspace query smaller than what the launcher carves up is an out-of-bounds write.  The
snapshot is only as good as the branches it reaches, so that is asserted as well."""
import ctypes as C
import json
import os

import pytest

from stereoscene_amd import capi

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dispatch.json")
NDIMS = len(capi.ConvDims._fields_)
WGRAD_KINDS = {"bf16", "thinside", "thin", "1x1", "dh", "lds", "cf", "generic"}


@pytest.fixture(scope="module")
def snap():
    with open(GOLDEN) as f:
        s = json.load(f)
    assert s["cols"][:NDIMS] == [n for n, _ in capi.ConvDims._fields_]
    assert s["cols"][NDIMS:] == ["class0", "class1", "class2", "groups0", "groups1", "groups2", "packed_elems",
                                 "wgrad_workspace", "wgrad_kind"]
    return s


def _answers(lib, row):
    d = capi.ConvDims(*row[:NDIMS])
    ref = C.byref(d)
    return [lib.ssbev_conv_kernel_class(ref, m) for m in (0, 1, 2)] + [lib.ssbev_conv_chunk_groups(ref, m) for m in (0, 1, 2)] + \
        [lib.ssbev_conv_packed_weight_elems(ref), lib.ssbev_conv_bwd_weight_workspace(ref)]


def _mismatches(lib, rows):
    bad = [(r[:NDIMS], r[NDIMS:-1], got) for r in rows for got in [_answers(lib, r)] if got != r[NDIMS:-1]]
    return bad[:5], len(bad)


def test_every_recorded_answer_is_reproduced(snap, monkeypatch):
    for k in [k for k in os.environ if k.startswith("SSBEV_")]:
        monkeypatch.delenv(k)
    lib = capi.load()
    lib.ssbev_env_refresh()                                   # the library caches its switches
    try:
        assert _mismatches(lib, snap["rows"]) == ([], 0)
        monkeypatch.setenv("SSBEV_IGEMM", "0")                # the implicit-GEMM rows fall to the gather kernel
        lib.ssbev_env_refresh()
        assert _mismatches(lib, snap["igemm_off"]) == ([], 0)
    finally:
        monkeypatch.undo()
        lib.ssbev_env_refresh()


def test_snapshot_reaches_every_branch(snap):
    rows, off = snap["rows"], snap["igemm_off"]
    assert 2000 <= len(rows) <= 8000
    classes = {r[NDIMS + m] for r in rows for m in (0, 1, 2)}
    assert classes >= {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 20, 21}
    for m in (0, 1):                                          # every fp32 forward / data-gradient class in BOTH modes
        assert {r[NDIMS + m] for r in rows} >= {0, 1, 2, 3, 4, 5, 7, 8, 9, 10, 11}
    for m in (0, 1, 2):
        assert any(r[NDIMS + 3 + m] > 0 for r in rows), m
    # chunk groups of every walking class
    assert {r[NDIMS + m] for r in rows for m in (0, 1) if r[NDIMS + 3 + m] > 0} == {1, 2, 3, 7, 8, 9, 17}
    # The kind label is the generator's own derivation (public queries, two shape predicates restated in Python, the tile_hint 7
    # A/B pair), not something the library reports: it shows that the grid was AIMED at all eight kinds.  What pins the ladder
    # is the workspace size of every row above, whichever kind served it.
    kinds = {r[-1] for r in rows if r[NDIMS + 7] > 0}
    assert kinds == WGRAD_KINDS
    hints = {r[NDIMS - 2] for r in rows}
    assert hints >= {0, 4, 5, 6, 7, 8, 9} and any(h >= 10 for h in hints)
    assert {r[NDIMS - 1] for r in rows} == {0, 1, 2, 3}
    assert {(r[NDIMS - 4], r[NDIMS - 3]) for r in rows} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    # class 5 is a class query only: rows where the launchers' own choice underneath is the thin ring walk (chunk query 0 there)
    assert any(r[NDIMS] == 5 for r in rows) and any(r[NDIMS + 1] == 5 for r in rows)
    # SSBEV_IGEMM=0: every row the implicit GEMM serves by default is there and answers 0
    on = {tuple(r[:NDIMS]): r for r in rows}
    moved = [r for r in off if 11 in on[tuple(r[:NDIMS])][NDIMS:NDIMS + 2]]
    assert len(moved) >= 100 and all(11 not in r[NDIMS:NDIMS + 2] for r in off)
    assert len(moved) == sum(1 for r in rows if 11 in r[NDIMS:NDIMS + 2])


def test_launchers_refuse_before_any_device_call(snap):
    """Null pointers, bf16-storage dims on the fp32 entry points, K-role channels that are no multiple of 4, invalid dims: the
    recorded SSBEV_EINVAL answers.  None of these calls reaches a kernel launch (the box running this test has no GPU)."""
    lib = capi.load()
    buf = (C.c_float * 16)()
    cases = snap["retcodes"]
    assert len(cases) >= 12 and {c[0] for c in cases} >= {"ssbev_conv_fwd", "ssbev_conv_bwd_data", "ssbev_conv_pack_weight"}
    for fn, row, null, want in cases:
        assert want == capi.EINVAL
        d = capi.ConvDims(*row)
        ptr = lambda tag: None if tag == null else C.cast(buf, C.c_void_p)
        if fn == "ssbev_conv_fwd":
            got = lib.ssbev_conv_fwd(ptr("x"), ptr("w"), None, ptr("y"), C.byref(d), None)
        elif fn == "ssbev_conv_bwd_data":
            got = lib.ssbev_conv_bwd_data(ptr("x"), ptr("w"), ptr("y"), C.byref(d), None)
        elif fn == "ssbev_conv_bwd_weight":
            got = lib.ssbev_conv_bwd_weight(ptr("x"), ptr("y"), ptr("w"), C.byref(d), ptr("ws"), 64, None)
        else:
            assert fn == "ssbev_conv_pack_weight"
            got = lib.ssbev_conv_pack_weight(ptr("x"), ptr("w"), C.byref(d), 2 if null == "mode" else 0, None)
        assert got == want, (fn, row, null, got)
