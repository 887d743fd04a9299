"""CPU: the operands functional._ConvNd hands to the library against a recorded snapshot.

tests/golden/conv_operands.json (tools/make_golden_conv_operands.py) holds, for thin, padded and plain channel pairs under both
`transposed` values, kernel sizes, strides, ReLU, the three needs_input_grad combinations, a gradient slot or none, every tile hint,
both fp32 precision modes and OWN_GEMM on and off, what the commit named in the file did at the C boundary: every entry point it
called, in order, with its mode, every ssbev_conv_dims field and the shape and dtype of each tensor argument; the shapes of y, gx,
gw and gb; whether the slot's buffer was set; and how many class queries the call cost.  Every case is replayed here through the
recorder's own stubs and must match field by field; forward and backward together may ask the library fewer questions than
recorded, never more.  A weight padded on the wrong axis, a gradient cropped to the wrong width or a slot taken on a cropped
gradient drops or double-counts a gradient without any error: this is the test that sees it.  The snapshot only guards the branches
it reaches, so that is asserted as well."""
import ctypes as C
import importlib.util
import json
import os

import pytest

from stereoscene_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_operands.json")
FIELDS = ("calls", "y", "out", "slot_set")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_conv_operands", os.path.join(HERE, os.pardir, "tools", "make_golden_conv_operands.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()


@pytest.fixture(scope="module")
def snap():
    with open(GOLDEN) as f:
        return json.load(f)


def _cases(snap):
    """(geometry, variant, record) of every case in the file; the grid itself must be the recorder's."""
    geoms = R.geometries()
    assert snap["geometries"] == json.loads(json.dumps(geoms)) and snap["dim_fields"] == list(R.DIM_FIELDS)
    assert snap["variants"] == {t: [v[0] for v in R.variants(t)] for t in ("full", "some", "few")}
    for g in geoms:
        vs, ix = R.variants(g[10]), snap["cases"][g[0]]
        assert len(vs) == len(ix)
        for v, i in zip(vs, ix):
            yield g, v, R.expand(snap, snap["records"][i])


def test_every_recorded_call_is_reproduced(snap):
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SSBEV_")}
    lib = capi.load()
    lib.ssbev_env_refresh()                                   # the library caches its switches
    bad, n = [], 0
    try:
        for g, v, want in _cases(snap):
            got = json.loads(json.dumps(R.observe(g, v)))
            n += 1
            diff = [f for f in FIELDS if got[f] != want[f]] + ["queries"] * (sum(got["queries"]) > sum(want["queries"]))
            if diff:
                bad.append((g[0], v[0], diff, {f: (got[f], want[f]) for f in diff}))
    finally:
        os.environ.update(saved)
        lib.ssbev_env_refresh()
    assert n >= 3000
    assert (bad[:5], len(bad)) == ([], 0)


# every branch of the operand handling; the snapshot must reach exactly these
BRANCHES = {
    "thin_in_forward",                       # class 4 gathers the 1 / 2 channel input unpadded
    "thin_dgrad",                            # class 4 takes the 1 / 2 channel gradient and the weight as they are
    "thin_wgrad",                            # class 6 takes both operands as they are
    "class5_forward", "class5_dgrad",        # the thin-out entry points
    "kpad", "kpad_transposed",               # x and the weight's K role padded to a multiple of 4
    "cpad_copy",                             # gy (and the weight's N role) padded for a wanted pass
    "cpad_no_copy",                          # Cout % 4 != 0, only unpadded consumers wanted: no padded launch
    "tpad",                                  # thin-in forward, direct weight gradient: x padded there alone
    "tn",                                    # the skinny TN product
    "slot_taken", "slot_accumulated",        # the buffer set; an earlier gradient added to in the epilogue
    "slot_refused:kpad", "slot_refused:thin_dgrad", "slot_refused:class4or5",
}


def _reached(g, v, r):
    _name, tr, cin, cout = g[:4]
    f = {n: i for i, n in enumerate(R.DIM_FIELDS)}
    got = set()
    by = lambda name, mode=None: [c for c in r["calls"] if c[0] == name and mode in (None, c[1])]
    ch = lambda c: (c[2][f["Cin"]], c[2][f["Cout"]])
    fwd, dgr, wgr = by("fwd"), by("bwd_data"), by("bwd_weight")
    if any(ch(c)[0] % 4 for c in fwd):
        got.add("thin_in_forward")
    if any(ch(c)[1] % 4 for c in dgr):
        got.add("thin_dgrad")
    if any(ch(c)[0] % 4 or ch(c)[1] % 4 for c in wgr):
        got.add("thin_wgrad")
    if by("thin_run", 0):
        got.add("class5_forward")
    if by("thin_run", 1):
        got.add("class5_dgrad")
    kpad = any(ch(c)[0] > cin for c in fwd + by("thin_run", 0))
    if kpad:
        got.add("kpad_transposed" if tr else "kpad")
    backward = dgr + wgr + by("thin_run", 1)
    if any(ch(c)[1] > cout for c in backward):
        got.add("cpad_copy")
    elif cout % 4 and backward:
        got.add("cpad_no_copy")
    if any(ch(c)[0] > cin for c in wgr) and not kpad:
        got.add("tpad")
    if by("gemm_tn"):
        got.add("tn")
    wants_gx, slot = "x" in v[2], v[3]
    if r["slot_set"]:
        got.add("slot_taken")
        if any(c[2][f["accumulate"]] for c in dgr):
            got.add("slot_accumulated")
    elif wants_gx and slot != "none":
        thin = any(ch(c)[1] % 4 for c in dgr)
        got.add("slot_refused:kpad" if kpad else ("slot_refused:thin_dgrad" if thin else "slot_refused:class4or5"))
        if not kpad and not thin:                # the remaining reason, asked of the library itself
            (c,) = dgr + by("thin_run", 1)
            sym = {"h": v[4], "p": 1 if v[5] == "bf16_operands" else 0}
            d = capi.ConvDims(*[sym.get(x, x) for x in c[2]])
            assert capi.load().ssbev_conv_kernel_class(C.byref(d), 1) in (4, 5), (g[0], v[0])
    return got


def test_snapshot_reaches_every_branch(snap):
    got = set()
    for g, v, r in _cases(snap):
        assert r["slot_set"] == 0 or (v[3] != "none" and "x" in v[2])
        got |= _reached(g, v, r)
    assert got == BRANCHES, (sorted(BRANCHES - got), sorted(got - BRANCHES))


def test_snapshot_is_a_fixture_not_a_build_product(snap):
    assert len(snap["commit"]) == 40
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "conv_routes.json"))
