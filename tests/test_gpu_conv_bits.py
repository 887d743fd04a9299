"""GPU: every forward / data-gradient path and every weight-gradient kind of the ssbev_conv_* entry points still writes the
BYTES recorded in tests/golden/conv_bits.json (tools/make_golden_conv_bits.py, from the commit named in the file).

The kernels reduce in a fixed order and the weight gradients fold their partials in a fixed order, so the comparison is
equality of SHA-256 hashes: a differing hash means a launch parameter (grid, chunk length, LDS size, a geometry field, a
workspace offset, the packed layout) changed.  test_conv_dispatch_snapshot.py pins WHICH kernel is chosen; this pins what the
chosen kernel is handed."""
import ctypes as C
import importlib.util
import json
import os

import pytest

import conv_bits_cases as T
from stereoscene_amd import capi

pytestmark = pytest.mark.gpu

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
with open(os.path.join(GOLDEN_DIR, "conv_bits.json")) as _f:
    RECORD = json.load(_f)
GOLDEN = RECORD["cases"]


def test_table_covers_every_path_and_weight_gradient_kind():
    assert set(GOLDEN) == {c.name for c in T.CASES}
    for mode in (0, 1):
        assert {c.classes[mode] for c in T.CASES} - {None} == {4, 3, 7, 8, 10, 9, 2, 1, 11, 0}
    assert {c.wgrad for c in T.CASES} == {"bf16", "thinside", "thin", "1x1", "dh", "lds", "cf", "generic"}
    lib = capi.load()
    with open(os.path.join(GOLDEN_DIR, "conv_dispatch.json")) as f:
        assert json.load(f)["commit"] == RECORD["commit"]            # both recorded from the same build
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(
        os.path.dirname(GOLDEN_DIR), os.pardir, "tools", "make_golden_conv_dispatch.py"))
    labels = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(labels)
    for c in T.CASES:
        want, got = T.queries(c)
        assert want == c.classes, (c.name, got)
        assert labels.wgrad_kind(lib, T.dims(c)) == c.wgrad, c.name
        if c.wgrad == "dh":
            assert lib.ssbev_conv_chunk_groups(C.byref(T.dims(c)), 2) >= 2


@pytest.mark.parametrize("case", T.CASES, ids=lambda c: c.name)
def test_outputs_are_the_recorded_bytes(case):
    got = T.run(case)
    assert got == GOLDEN[case.name], {k: (v[:12], GOLDEN[case.name].get(k, "")[:12]) for k, v in got.items()}
