"""CPU: the routing of functional.conv3d / conv2d / conv_transpose3d against a recorded snapshot.

tests/golden/conv_routes.json (tools/make_golden_conv_routes.py) holds, for every layer shape of the workload under every
precision mode, tile hint and routing switch, what the commit named in the file did: the leaves it called, in order, with their
plain arguments, tensor shapes and dtypes, whether the bias and the gradient slot went into the leaf, what happened to the
leaf's result on the way out (bias added after, ReLU after, cast back to the activation dtype, squeeze), whether the input
alias still carries its slot, and how many host queries the decision cost.  Every case is replayed here through the recorder's
own stubs and must match field by field; it may ask the library fewer questions than recorded, never more.  A route that takes
the slot where the recorded one left it (or the reverse) double-counts or drops a gradient without any error: this is the test
that sees it.  The snapshot only guards the routes it reaches, so that is asserted as well."""
import importlib.util
import json
import os

import pytest

from stereoscene_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "conv_routes.json")
FIELDS = ("calls", "out", "slot_kept", "epilogue")


def _recorder():
    spec = importlib.util.spec_from_file_location("make_golden_conv_routes", os.path.join(HERE, os.pardir, "tools", "make_golden_conv_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


R = _recorder()


@pytest.fixture(scope="module")
def snap():
    with open(GOLDEN) as f:
        return json.load(f)


def _cases(snap):
    """(layer, variant, record) of every case in the file; the grid itself must be the recorder's."""
    assert snap["layers"] == json.loads(json.dumps(R.LAYERS))
    assert snap["variants"] == {e: [v[0] for v in R.variants(e)] for e in ("conv3d", "conv2d", "conv_transpose3d")}
    for layer in R.LAYERS:
        vs, ix = R.variants(layer[1]), snap["routes"][layer[0]]
        assert len(vs) == len(ix)
        for v, i in zip(vs, ix):
            yield layer, v, snap["records"][i]


def test_every_recorded_route_is_reproduced(snap):
    saved = {k: os.environ.pop(k) for k in list(os.environ) if k.startswith("SSBEV_")}
    lib = capi.load()
    lib.ssbev_env_refresh()                                   # the library caches its switches
    bad, n = [], 0
    try:
        for layer, v, want in _cases(snap):
            got = json.loads(json.dumps(R.observe(layer, v)))
            n += 1
            diff = [f for f in FIELDS if got[f] != want[f]] + ["queries"] * any(g > w for g, w in zip(got["queries"], want["queries"]))
            if diff:
                bad.append((layer[0], v[0], diff, {f: (got[f], want[f]) for f in diff}))
    finally:
        os.environ.update(saved)
        lib.ssbev_env_refresh()
    assert n >= 6000
    assert (bad[:5], len(bad)) == ([], 0)


def _leaves(r):
    return tuple(c[0] for c in r["calls"])


def _on(v, *names):
    """Are these switches at their defaults (on) in the variant, on a GPU tensor, without a tile hint?"""
    over = v[4]
    return v[3] and over.get("TILE_HINT", 0) == 0 and all(over.get(n, True) for n in names)


def test_snapshot_reaches_every_route(snap):
    cases = list(_cases(snap))
    by_name = {(layer[0], v[0]): r for layer, v, r in cases}

    def reached(entry, pred):
        return any(layer[1] == entry and pred(layer, v, r, r["calls"][0]) for layer, v, r in cases)

    prec = lambda v: v[4]["PRECISION"]
    slot_in, bias_in, plain = (lambda c: c[4] == 1), (lambda c: c[3] == 1), (lambda c: c[1])
    # ---- conv3d
    c3 = lambda pred: reached("conv3d", pred)
    wide = "wide 64->64 W%16==0"
    assert _leaves(by_name[wide, "b1 r1 bf16 hint0"]) == ("_ConvNd16",) and _leaves(by_name[wide, "b1 r1 bf16 WIDE16=0"])[0] == "_WinoConv"
    assert by_name[wide, "b1 r1 bf16 hint0"]["queries"][0] >= 1                                     # wide16: the library was asked
    assert c3(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_WinoConv", "torch.relu") and r["epilogue"] == ["Relu", "Add", "leaf0"]
              and not bias_in(c) and slot_in(c))                                                      # bf16 Winograd, bias and ReLU after
    assert c3(lambda l, v, r, c: prec(v) == "bf16" and "WIDE16=0" in v[0] and _leaves(r) == ("_ConvNd16",) and slot_in(c) and plain(c)["relu"])
    assert c3(lambda l, v, r, c: prec(v) == "bf16" and v[3] and _leaves(r) == ("_ConvNd",) and r["epilogue"] == ["ToCopy", "leaf0"]
              and not slot_in(c) and r["slot_kept"])                                                  # fp32 island, slot not taken
    assert c3(lambda l, v, r, c: _leaves(r) == ("linear_cl", "torch.relu") and r["epilogue"] == ["Relu", "leaf0"])
    assert c3(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConv", "torch.relu"))
    assert c3(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConvDF", "torch.relu") and r["epilogue"] == ["Relu", "Add", "leaf0"])
    assert c3(lambda l, v, r, c: not v[3] and _leaves(r) == ("_ConvNd", "torch.relu") and not plain(c)["relu"])      # ReLU outside, no GPU
    assert c3(lambda l, v, r, c: v[3] and prec(v) != "bf16" and _leaves(r) == ("_ConvNd",) and plain(c)["relu"] and slot_in(c) and bias_in(c))
    assert c3(lambda l, v, r, c: _leaves(r) == ("linear_cl",) and bias_in(c) and r["slot_kept"])
    assert c3(lambda l, v, r, c: _leaves(r) == ("_WinoConvDF",) and r["queries"][1] == 2 and slot_in(c) and r["epilogue"] == ["Add", "leaf0"])
    assert c3(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConv",) and slot_in(c) and not bias_in(c))
    assert c3(lambda l, v, r, c: prec(v) == "fp32" and "WINO_DF_MIN_ROWS=0" in v[0] and l[0] == "wide 512->512 few rows" and _leaves(r)[0] == "_WinoConvDF")
    assert _leaves(by_name["wide 512->512 few rows", "b1 r0 fp32 hint0"]) == ("_WinoConv",)
    assert c3(lambda l, v, r, c: v[3] and prec(v) != "bf16" and _leaves(r) == ("_ConvNd",) and not plain(c)["relu"] and slot_in(c))
    # ---- conv2d
    c2 = lambda pred: reached("conv2d", pred)
    sub_batch = lambda l, c: c[2][0][0][0] == l[8][0] ** 2 and l[8][0] > 1                             # the d * d sub-images of the polyphase batch
    assert c2(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_WinoConv",) and sub_batch(l, c) and "Slice" in r["epilogue"]
              and r["epilogue"][0] == "Add" and not slot_in(c) and r["slot_kept"])                    # bf16 polyphase and its inner conv2d
    assert c2(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_WinoConv",) and r["epilogue"] == ["Add", "Squeeze", "leaf0"] and slot_in(c))
    assert c2(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_ConvNd16",) and r["epilogue"] == ["Squeeze", "leaf0"] and bias_in(c))
    assert c2(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_ConvNd",) and r["epilogue"] == ["Squeeze", "ToCopy", "leaf0"] and r["slot_kept"])
    assert c2(lambda l, v, r, c: _leaves(r) == ("linear_cl",) and len(c[2][0][0]) == 4)
    assert c2(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConv",) and plain(c)["dil"] > 1 and slot_in(c))
    assert c2(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConv",) and sub_batch(l, c) and "Slice" in r["epilogue"] and r["slot_kept"])
    assert c2(lambda l, v, r, c: prec(v) == "fp32" and _on(v, "DILATED_POLYPHASE", "WINOGRAD") and l[8][0] > 1 and min(l[2], l[3]) >= 64
              and _leaves(r) == ("_ConvNd",) and plain(c)["dilation"] == [1, l[8][0], l[8][0]])       # polyphase refused: the next route
    assert c2(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_WinoConv",) and plain(c)["dil"] == 1 and c[2][0][0][0] == 1
              and r["epilogue"] == ["Add", "Squeeze", "leaf0"])
    assert c2(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_ConvNd",) and slot_in(c) and r["epilogue"] == ["Squeeze", "leaf0"])
    # ---- conv_transpose3d
    ct = lambda pred: reached("conv_transpose3d", pred)
    assert ct(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_ConvNd16",) and plain(c)["transposed"] and slot_in(c))
    assert ct(lambda l, v, r, c: prec(v) == "bf16" and _leaves(r) == ("_ConvNd",) and r["epilogue"] == ["ToCopy", "leaf0"] and r["slot_kept"])
    assert ct(lambda l, v, r, c: _leaves(r) == ("linear_cl",) and l[5] == (1, 1, 1) and c[2][1][0] == [l[3], l[2]])
    assert ct(lambda l, v, r, c: _leaves(r) == ("_DeconvKS",) and bias_in(c))
    assert ct(lambda l, v, r, c: _leaves(r) == ("torch.mm",) and "Add" in r["epilogue"])
    assert ct(lambda l, v, r, c: prec(v) == "fp32" and _leaves(r) == ("_ConvNd",) and plain(c)["transposed"] and not slot_in(c) and r["slot_kept"])
    # ---- both answers to "is the slot still on the alias", and every tile hint somewhere it changes the route
    assert {r["slot_kept"] for _, _, r in cases} == {0, 1}
    same = lambda a, b: all(a[f] == b[f] for f in FIELDS)
    differs = lambda p, h0, h1: any(not same(by_name[l[0], f"b1 r0 {p} hint{h0}"], by_name[l[0], f"b1 r0 {p} hint{h1}"]) for l in R.LAYERS)
    assert all(differs("fp32", 0, h) for h in (5, 7, 9))                    # any hint takes the fp32 Winograd and GEMM routes away
    # bf16: 0 and 9 admit the bf16 routes everywhere, 7 in conv3d alone, 5 nowhere
    assert differs("bf16", 0, 5) and differs("bf16", 0, 7) and differs("bf16", 5, 7) and differs("bf16", 7, 9) and not differs("bf16", 0, 9)


def test_snapshot_is_a_fixture_not_a_build_product(snap):
    assert len(snap["commit"]) == 40
    assert os.path.getsize(GOLDEN) <= os.path.getsize(os.path.join(HERE, "golden", "conv_dispatch.json"))
