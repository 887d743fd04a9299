"""CPU: the two rules behind the BEV label augmentation kernels (csrc/bev_augment.hip) as a NumPy model, checked against the
fixture (tests/golden/bev_augment.npz, tools/make_golden_bev_augment.py) and, where scipy imports, against scipy itself;
``pipelines.bev_transform`` on host tensors keeps today's bits; keyword validation."""
import math

import numpy as np
import pytest
import torch

import bev_augment_cases as B
from conftest import load_golden
from stereoscene_amd import pipelines as P

CENTER = torch.tensor([25.6, 0.0, 1.2])


def source_map(X, Y, coeffs):
    """m[p] over the raster p = i*Y + j of a plane: the source index scipy's order-0 ``mode='constant'`` sampling reads, -1 for
    the fill value.  NumPy evaluates every product and sum as its own float64 operation, which is the rule (no FMA)."""
    m00, m01, m10, m11, off0, off1 = (np.float64(v) for v in coeffs)
    i, j = (a.astype(np.float64) for a in np.meshgrid(np.arange(X), np.arange(Y), indexing="ij"))
    ci = (m00 * i + m01 * j) + off0
    cj = (m10 * i + m11 * j) + off1
    inside = (ci >= 0) & (ci <= X - 1) & (cj >= 0) & (cj <= Y - 1)
    q = np.floor(ci + 0.5).astype(np.int64) * Y + np.floor(cj + 0.5).astype(np.int64)
    return np.where(inside, q, -1).reshape(-1)


def resolve_in_place(m):
    """The table of the in-place rotation: scipy writes p = 0, 1, ... over the plane it reads, so m[p] < p reads what was written
    there.  Returns (the source index every p ends up with, -1 = fill; the longest chain in links)."""
    t, links = m.copy(), np.zeros(len(m), dtype=np.int64)
    for p in range(len(m)):
        if 0 <= m[p] < p:
            t[p], links[p] = t[m[p]], links[m[p]] + 1
    return t, int(links.max())


def resolve_by_jumping(m):
    """The same table the way the kernels build it: ceil(log2(n)) rounds of pointer jumping between two tables."""
    n = len(m)
    p = np.arange(n)
    a = np.where((m >= 0) & (m < p), m, np.where(m < 0, -1, -2 - m))           # pointer | fill | resolved source
    for _ in range(math.ceil(math.log2(n)) if n > 1 else 0):
        a = np.where(a >= 0, a[np.maximum(a, 0)], a)
    assert (a < 0).all(), "a chain survived ceil(log2(n)) rounds"
    return np.where(a == -1, -1, -2 - a)


def model(case, inplace):
    labels = case["labels"]
    X, Y, Z = labels.shape
    out = labels
    if case["coeffs"] is not None:
        t = source_map(X, Y, case["coeffs"])
        if inplace:
            t = resolve_in_place(t)[0]
        cols = labels.reshape(X * Y, Z)
        out = np.where((t < 0)[:, None], np.uint8(B.FILL), cols[np.maximum(t, 0)]).reshape(X, Y, Z)
    if case["flip_dy"]:
        out = out[:, ::-1]
    if case["flip_dx"]:
        out = out[::-1]
    return out


def test_numpy_model_reproduces_the_fixture_in_both_modes():
    cases = B.load_cases()
    assert len(cases) == len(B.case_list()) >= 60
    differs = 0
    for case in cases:
        assert np.array_equal(model(case, True), case["reference"]), case["name"]
        assert np.array_equal(model(case, False), case["exact"]), case["name"]
        assert (case["coeffs"] is None) == bool(np.isclose(case["angle"], 0)), case["name"]
        differs += int(not np.array_equal(case["reference"], case["exact"]))
    assert differs >= 40                                       # the aliasing quirk is what most cases are about


def test_pointer_jumping_resolves_every_chain_in_log2_rounds():
    longest = {}
    for case in B.load_cases():
        if case["coeffs"] is None:
            continue
        X, Y, _ = case["shape"]
        m = source_map(X, Y, case["coeffs"])
        t, links = resolve_in_place(m)
        assert np.array_equal(resolve_by_jumping(m), t), case["name"]
        longest[case["name"]] = links
    assert longest["big_0.3"] == 444 and longest["big_3.75"] == 60
    # the bound itself: a chain through every entry of a table (n - 1 links) still resolves
    for n in (1, 2, 3, 5, 64, 65, 1000):
        m = np.arange(n) - 1
        m[0] = 0
        assert (resolve_by_jumping(m) == 0).all(), n


def test_numpy_model_against_scipy_in_place_and_out_of_place():
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.RandomState(5)
    for shape in [(16, 16, 4), (17, 13, 3), (8, 8, 2), (40, 24, 2), (5, 7, 1)]:
        for angle in [3.75, 22.5, -22.5, -7.3, 13.37, 90.0, 45.0, -45.0, 180.0, 1e-7, 0.3, -0.3]:
            labels = rng.randint(0, 256, size=shape).astype(np.uint8)
            case = dict(labels=labels, coeffs=P.bev_rotate_coeffs(shape[0], shape[1], angle), flip_dx=False, flip_dy=False)
            kw = dict(mode="constant", order=0, cval=255, axes=(0, 1), reshape=False)
            assert np.array_equal(model(case, False), ndimage.rotate(labels.copy(), angle, **kw)), (shape, angle)
            aliased = labels.copy()
            ndimage.rotate(aliased, angle, output=aliased, **kw)
            assert np.array_equal(model(case, True), aliased), (shape, angle)


def test_rotation_coefficients_are_exact_at_right_angles():
    pytest.importorskip("scipy")
    assert P.bev_rotate_coeffs(16, 16, 90.0) == (0.0, 1.0, -1.0, 0.0, 0.0, 15.0)
    assert P.bev_rotate_coeffs(17, 13, 180.0) == (-1.0, 0.0, -0.0, -1.0, 16.0, 12.0)
    for case in B.load_cases():                                # the fixture's coefficients are this function's
        if case["coeffs"] is not None:
            assert P.bev_rotate_coeffs(case["shape"][0], case["shape"][1], case["angle"]) == case["coeffs"], case["name"]


def test_host_bev_transform_keeps_its_bits_and_offers_the_exact_rotation():
    pytest.importorskip("scipy")
    from stereoscene_amd import synthetic as S
    g = load_golden("image_loading")
    lab = (S.hash_uniform("bev/lab", (16, 16, 4), 0.0, 20.0).floor()).to(torch.uint8)
    for tag, (rot, fx, fy) in dict(flipx=(0.0, True, False), flipxy=(0.0, True, True), rot=(30.0, False, True)).items():
        for kw in (dict(), dict(device=None, rotate_mode="reference")):
            v, m = P.bev_transform(lab.clone(), rot, 1.0, fx, fy, CENTER, **kw)
            assert v.dtype == torch.int64 and not v.is_cuda and m.dtype == torch.float32 and tuple(m.shape) == (4, 4)
            assert np.array_equal(v.numpy().astype(np.uint8), g[f"bev_{tag}_labels"]), tag
            assert np.abs(m.numpy() - g[f"bev_{tag}_mat"]).max() < 1e-5
    for case in B.load_cases()[:12]:
        for mode in ("reference", "exact"):
            v, _ = P.bev_transform(torch.from_numpy(case["labels"].copy()), case["angle"], 1.0, case["flip_dx"], case["flip_dy"], CENTER,
                                   rotate_mode=mode)
            assert v.dtype == torch.int64 and np.array_equal(v.numpy().astype(np.uint8), case[mode]), (case["name"], mode)
    # int64 labels outside a byte are taken modulo 256, as the upstream's astype(np.uint8) does
    v, _ = P.bev_transform(torch.tensor([[[256 + 7, -1]]]), 0.0, 1.0, False, False, CENTER)
    assert v.tolist() == [[[7, 255]]]


def test_unknown_rotate_modes_raise():
    conf = dict(rot_lim=(0, 0), scale_lim=(0.95, 1.05), flip_dx_ratio=0.5, flip_dy_ratio=0.5)
    with pytest.raises(ValueError, match="rotate_mode"):
        P.bev_transform(torch.zeros(4, 4, 2, dtype=torch.uint8), 0.0, 1.0, False, False, CENTER, rotate_mode="scipy")
    with pytest.raises(ValueError, match="bda_rotate"):
        P.PIPELINES.build(dict(type="LoadSemKittiAnnotation", bda_aug_conf=conf, bda_rotate="inplace"))
    step = P.PIPELINES.build(dict(type="LoadSemKittiAnnotation", bda_aug_conf=conf, apply_bda=True, bda_rotate="exact"))
    assert step.device is None and step.bda_rotate == "exact"


def test_entry_points_validate_their_arguments_on_host():
    """No device work: the workspace query and the refusals of ssbev_bev_label_transform."""
    import ctypes as C
    from stereoscene_amd import capi
    lib = capi.load()
    assert lib.ssbev_version() >= 120
    assert lib.ssbev_bev_label_workspace(256, 256, 1, 1) == 2 * 65536 * 4        # two tables: the rounds go back and forth
    assert lib.ssbev_bev_label_workspace(256, 256, 1, 0) == 65536 * 4
    assert lib.ssbev_bev_label_workspace(256, 256, 0, 1) == 0 and lib.ssbev_bev_label_workspace(0, 256, 1, 1) == 0
    assert lib.ssbev_bev_label_workspace(1, 1, 1, 1) == 4 and lib.ssbev_bev_label_workspace(65536, 32768, 1, 1) == 0
    src, dst, ws = C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)   # never dereferenced: refused on the arguments
    ok6 = (C.c_double * 6)(1, 0, 0, 1, 0, 0)
    for fn in (lib.ssbev_bev_label_transform, lib.ssbev_bev_label_transform_u8):
        def call(s=src, d=dst, X=8, Y=8, Z=2, c=ok6, fill=255, w=ws, nbytes=1 << 20):
            return fn(s, d, X, Y, Z, c, 1, 0, 0, fill, w, nbytes, None)
        assert call(s=None) == capi.EINVAL and call(d=None) == capi.EINVAL and call(w=None) == capi.EINVAL
        assert call(X=0) == capi.EINVAL and call(Y=0) == capi.EINVAL and call(Z=0) == capi.EINVAL and call(X=-3) == capi.EINVAL
        assert call(X=65536, Y=32768) == capi.EINVAL                              # X Y = 2^31: beyond the int32 table
        assert call(fill=256) == capi.EINVAL and call(fill=-1) == capi.EINVAL
        assert call(d=src) == capi.EINVAL and call(d=C.c_void_p((1 << 20) + 64)) == capi.EINVAL      # overlapping grids
        for k in range(6):
            for bad in (float("nan"), float("inf"), -float("inf")):
                c = (C.c_double * 6)(1, 0, 0, 1, 0, 0)
                c[k] = bad
                assert call(c=c) == capi.EINVAL, (k, bad)
        assert call(nbytes=2 * 64 * 4 - 1) == capi.EWORKSPACE
