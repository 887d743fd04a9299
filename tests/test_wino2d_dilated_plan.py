"""CPU: the per-axis tile table of the dilated 2-D Winograd F(2,3) transforms (ssbev_wino2d_axis_tiles, csrc/winograd.hip).

Every residue class ``ph`` modulo the dilation ``d`` of an axis of extent ``n`` is tiled on its own: it holds
``ceil((n - ph) / d)`` positions and takes half as many (rounded up) tiles of two outputs, ``ph + 2 t d`` and ``ph + (2 t + 1) d``.
The table holds the first output coordinate of every tile, phase-major."""
import ctypes as C

import pytest

from stereoscene_amd import capi
from stereoscene_amd import functional as F

CAP = 128
GRID = [(n, d) for d in (1, 2, 3, 5, 6, 7, 12, 18) for n in (1, 2, 3, 4, 7, 9, 10, 11, 13, 20, 37, 48, 160)]


def formula(n, d):
    return sum(-(-(-(-(n - ph) // d)) // 2) for ph in range(d) if ph < n)


def table(n, d):
    lib = capi.load()
    buf = (C.c_uint16 * CAP)()
    cnt = lib.ssbev_wino2d_axis_tiles(n, d, buf, CAP)
    assert 0 < cnt <= CAP, (n, d, cnt)
    return [int(v) for v in buf[:cnt]]


@pytest.mark.parametrize("n,d", GRID)
def test_tiles_cover_every_output_once_and_count_matches_formula(n, d):
    first = table(n, d)
    assert len(first) == formula(n, d) == F.wino2d_axis_tiles(n, d)
    assert capi.load().ssbev_wino2d_axis_tiles(n, d, None, 0) == len(first)          # count-only query
    rows = [r for f in first for r in (f, f + d) if r < n]
    assert sorted(rows) == list(range(n)), (n, d, first)
    assert all(f < n for f in first)                                                  # no tile without an output
    # phase-major, index ascending inside a phase
    keys = [(f % d, f // d) for f in first]
    assert keys == sorted(keys) and all(k[1] % 2 == 0 for k in keys)


def test_aspp_counts_and_refusals():
    assert (F.wino2d_axis_tiles(48, 18), F.wino2d_axis_tiles(160, 18)) == (30, 88)
    assert (F.wino2d_axis_tiles(48, 6), F.wino2d_axis_tiles(160, 6)) == (24, 82)
    assert (F.wino2d_axis_tiles(48, 12), F.wino2d_axis_tiles(160, 12)) == (24, 84)
    assert (F.wino2d_axis_tiles(4, 5), F.wino2d_axis_tiles(13, 5)) == (4, 8)         # d > H: phase 4 has no tile
    lib = capi.load()
    assert lib.ssbev_wino2d_axis_tiles(0, 2, None, 0) == 0 and lib.ssbev_wino2d_axis_tiles(8, 0, None, 0) == 0
    assert lib.ssbev_wino2d_axis_tiles(1000, 3, None, 0) == 501                      # more than the kernels' table holds ...
    fake = C.c_void_p(256)                                                           # ... so the transforms refuse (never dereferenced)
    d = capi.WinoDims(1, 1, 8, 1000, 64, 3)
    for name in ("ssbev_wino2d_input_transform", "ssbev_wino2d_output_transform", "ssbev_wino2d_output_adjoint",
                 "ssbev_wino2d_output_transform_acc"):
        assert getattr(lib, name)(fake, fake, C.byref(d), None) == capi.EINVAL
    d3 = capi.WinoDims(1, 2, 8, 8, 64, 2)                                            # the other families have no dilation
    assert lib.ssbev_wino_input_transform(fake, fake, C.byref(d3), None) == capi.EINVAL
    assert lib.ssbev_wino43_2d_input_transform(fake, fake, C.byref(d3), None) == capi.EINVAL
