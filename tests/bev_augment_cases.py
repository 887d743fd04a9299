"""Cases of the BEV label augmentation (csrc/bev_augment.hip) shared by tools/make_golden_bev_augment.py, test_bev_augment.py
and test_gpu_bev_augment.py: the case list, the inputs and how tests/golden/bev_augment.npz stores them.

A small case stores its labels and both expected grids as they are.  A 256 x 256 x 32 case would be 2 MB per grid, so its labels
come from a seed, ``labels[i, j, z] = (v[i, j] + 7 z) mod 256`` with one random byte ``v`` per column: 65 536 columns that differ,
and 32 voxels that differ inside each.  The rotation moves whole Z columns (its source map does not depend on z), so an expected
grid of such labels is the byte of every column at z = 0 plus one bit per column for "fill value"; the tool stores that only after
checking that it rebuilds scipy's grid byte for byte."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bev_augment.npz")
FILL = 255
Z_STEP = 7

SMALL_SHAPES = [(8, 8, 2), (16, 16, 4), (17, 13, 3), (40, 24, 2), (16, 16, 20), (5, 7, 1)]
ANGLES = [3.75, -22.5, 30.0, 13.37, 90.0, 180.0, 45.0, -45.0, 1e-7]
FLIPS = [(False, False), (True, False), (False, True), (True, True)]


def case_list():
    """[(name, shape, angle, flip_dx, flip_dy, seed or None)]; angle 0.0 = no rotation (np.isclose(angle, 0), as upstream)."""
    cases = []
    for si, shape in enumerate(SMALL_SHAPES):
        angles = [3.75, 90.0, -45.0] if shape == (16, 16, 20) else ANGLES          # (the 5 KB grids: three angles are enough)
        for ai, angle in enumerate(angles):
            fdx, fdy = FLIPS[(si + ai) % 4]
            cases.append((f"s{si}_a{ai}", shape, angle, fdx, fdy, None))
    for fi, (fdx, fdy) in enumerate(FLIPS):                                          # every flip combination behind one rotation
        cases.append((f"flip{fi}_rot", (16, 16, 4), 30.0, fdx, fdy, None))
    for si, shape in ((2, (17, 13, 3)), (4, (16, 16, 20)), (5, (5, 7, 1))):          # rotation-free: flips and widening alone
        for fi, (fdx, fdy) in enumerate(FLIPS):
            cases.append((f"flip{fi}_s{si}", shape, 0.0, fdx, fdy, None))
    cases.append(("skip_1e-9", (16, 16, 4), 1e-9, False, True, None))                # isclose(1e-9, 0): skipped, where 1e-7 rotates
    cases.append(("big_0.3", (256, 256, 32), 0.3, False, True, 11))                  # the deepest dependency chain found: 444 links
    cases.append(("big_3.75", (256, 256, 32), 3.75, True, False, 12))
    return cases


def small_labels(name, shape):
    """Every byte value, the fill value and the 20 classes among them."""
    rng = np.random.RandomState(zlib.crc32(name.encode()))
    return rng.randint(0, 256, size=shape).astype(np.uint8)


def big_labels(seed, shape):
    X, Y, Z = shape
    v = np.random.RandomState(seed).randint(0, 256, size=(X, Y, 1))
    return ((v + Z_STEP * np.arange(Z)) & 255).astype(np.uint8)


def pack_big(grid):
    """(byte of every column at z = 0, packed fill bits) of an expected grid of ``big_labels``, or an AssertionError."""
    fill = (grid == FILL).all(axis=2)
    plane0 = grid[:, :, 0].copy()
    assert np.array_equal(unpack_big(plane0, np.packbits(fill), grid.shape), grid)
    return plane0, np.packbits(fill)


def unpack_big(plane0, fill_bits, shape):
    X, Y, Z = shape
    fill = np.unpackbits(fill_bits)[:X * Y].reshape(X, Y).astype(bool)
    grid = ((plane0[:, :, None].astype(np.int64) + Z_STEP * np.arange(Z)) & 255).astype(np.uint8)
    grid[fill] = FILL
    return grid


_CACHE = []


def load_cases():
    """[dict(name, shape, angle, flip_dx, flip_dy, labels, coeffs (six floats or None), reference, exact)] from the fixture:
    ``reference`` is the host ``pipelines.bev_transform`` (the upstream's in-place rotation), ``exact`` the out-of-place
    ``scipy.ndimage.rotate`` and the same flips, both uint8 [X,Y,Z].  Loaded once; treat the arrays as read-only."""
    if _CACHE:
        return _CACHE
    with np.load(GOLDEN) as z:
        g = {k: z[k] for k in z.files}
    for name, shape, angle, fdx, fdy, seed in case_list():
        assert tuple(g[f"{name}_shape"]) == shape and float(g[f"{name}_angle"]) == angle, name
        assert tuple(bool(v) for v in g[f"{name}_flips"]) == (fdx, fdy), name
        c = g[f"{name}_coeffs"]
        case = dict(name=name, shape=shape, angle=angle, flip_dx=fdx, flip_dy=fdy, coeffs=tuple(float(v) for v in c) if c.size else None)
        if seed is None:
            case["labels"] = g[f"{name}_labels"]
            case["reference"], case["exact"] = g[f"{name}_reference"], g[f"{name}_exact"]
        else:
            case["labels"] = big_labels(seed, shape)
            for q in ("reference", "exact"):
                case[q] = unpack_big(g[f"{name}_{q}_plane0"], g[f"{name}_{q}_fill"], shape)
        for q in ("labels", "reference", "exact"):
            assert case[q].shape == shape and case[q].dtype == np.uint8, (name, q)
            case[q].setflags(write=False)
        _CACHE.append(case)
    return _CACHE
