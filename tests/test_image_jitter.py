"""Colour jitter of the image loader (loading_semkitti.py:213, 273: PhotoMetricDistortionMultiViewImage,
loading_bevdet.py:532-620), host side: the numpy statement of the upstream's arithmetic (OpenCV's float HSV conversions
restated, since OpenCV is not a dependency), the draw restatement against the upstream's RNG stream, the statement against the
reference loader's pixels (tests/golden/image_jitter.npz, tools/make_golden_jitter.py), the argument checks of the new entry
point, and -- where OpenCV is installed -- the HSV restatement against ``cv2.cvtColor``.  No GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, load_golden
from oracle import data_ref as DR
from oracle.make_golden_data import stereo_images
from stereoscene_amd import capi, pipelines as P
from test_image_rotate import AUG_CONFIG, NORM, rotate_gather

FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])     # OpenCV's sector_data
REFERENCE_LOADER = "/root/reference/projects/mmdet3d_plugin/datasets/pipelines/loading_semkitti.py"


def bgr2hsv(img):
    """``cv2.cvtColor(img, COLOR_BGR2HSV)`` of a float32 [..., 3] image as OpenCV's scalar ``RGB2HSV_f`` computes it (hrange
    360; its hscale 360 * (1.f / 360) is exactly 1): h in degrees, s, v."""
    b, g, r = (np.asarray(img[..., k], dtype=np.float32) for k in range(3))
    v = r.copy()
    v = np.where(v < g, g, v)
    v = np.where(v < b, b, v)
    mn = r.copy()
    mn = np.where(mn > g, g, mn)
    mn = np.where(mn > b, b, mn)
    diff = v - mn
    s = diff / (np.abs(v) + FLT_EPSILON)
    k = (60.0 / (diff + FLT_EPSILON).astype(np.float64)).astype(np.float32)
    h = np.where(v == r, (g - b) * k, np.where(v == g, (b - r) * k + np.float32(120), (r - g) * k + np.float32(240)))
    h = np.where(h < 0, h + np.float32(360), h)
    return np.stack([h, s, v], -1).astype(np.float32)


def hsv2bgr(img):
    """``cv2.cvtColor(img, COLOR_HSV2BGR)`` of a float32 [..., 3] image as OpenCV's scalar ``HSV2RGB_f`` computes it."""
    h, s, v = (np.asarray(img[..., k], dtype=np.float32) for k in range(3))
    hh = h * (np.float32(6) / np.float32(360))
    while (m := hh < 0).any():
        hh[m] += np.float32(6)
    while (m := hh >= 6).any():
        hh[m] -= np.float32(6)
    sector = np.floor(hh).astype(np.int64)
    hh = hh - sector.astype(np.float32)
    bad = (sector < 0) | (sector >= 6)
    sector[bad], hh[bad] = 0, 0
    one = np.float32(1)
    tab = np.stack([v, v * (one - s), v * (one - s * hh), v * (one - s * (one - hh))], -1)
    out = np.take_along_axis(tab, SECTORS[sector], -1)
    gray = s == 0
    out[gray] = v[gray][..., None]
    return out.astype(np.float32)


def photometric(img, jitter):
    """PhotoMetricDistortionMultiViewImage.__call__ (loading_bevdet.py:566-620) with one view's drawn values (``sample_jitter``:
    None = step off): uint8 / float BGR [..., 3] -> float32 BGR before the uint8 cast.  The Python floats are rounded to fp32
    where they meet the float32 image, as numpy does."""
    img = np.array(img, dtype=np.float32)
    if jitter["delta"] is not None:
        img += np.float32(jitter["delta"])
    if jitter["mode"] == 1 and jitter["alpha"] is not None:
        img *= np.float32(jitter["alpha"])
    img = bgr2hsv(img)
    if jitter["saturation"] is not None:
        img[..., 1] *= np.float32(jitter["saturation"])
    if jitter["hue"] is not None:
        img[..., 0] += np.float32(jitter["hue"])
        img[..., 0][img[..., 0] > 360] -= 360
        img[..., 0][img[..., 0] < 0] += 360
    img = hsv2bgr(img)
    if jitter["mode"] == 0 and jitter["alpha"] is not None:
        img *= np.float32(jitter["alpha"])
    if jitter["perm"] is not None:
        img = img[..., list(jitter["perm"])]
    return img


def to_u8(x):
    """``astype(np.uint8)`` of the float32 image as numpy does it on x86-64: truncate toward zero, keep the low 8 bits."""
    return x.astype(np.int32).astype(np.uint8)


def jitter_rgb(rgb_u8, jitter):
    """The loader holds RGB; the upstream jitters BGR.  uint8 RGB [..., 3] -> jittered uint8 RGB."""
    return to_u8(photometric(rgb_u8[..., ::-1], jitter))[..., ::-1]


def normalize(rgb_u8, mean, std):
    m = np.asarray(mean, dtype=np.float32)
    si = (1.0 / np.asarray(std, dtype=np.float32).astype(np.float64)).astype(np.float32)
    return ((rgb_u8.astype(np.float32) - m) * si).transpose(2, 0, 1)


def geometry_u8(raw, resize_dims, crop, flip, rotate):
    """The reference's geometric pixel path in numpy: Pillow resize, zero-padded crop, mirror, rotate -> uint8 RGB."""
    r = DR.pil_resize_u8(raw, tuple(resize_dims))
    x0, y0, x1, y1 = (int(v) for v in crop)
    c = np.zeros((y1 - y0, x1 - x0, 3), dtype=np.uint8)
    ys, xs = slice(max(y0, 0), min(y1, r.shape[0])), slice(max(x0, 0), min(x1, r.shape[1]))
    c[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = r[ys, xs]
    if flip:
        c = c[:, ::-1]
    return rotate_gather(np.ascontiguousarray(c), P.pil_rotate_fixed(c.shape[1], c.shape[0], rotate))


def augment_jitter_reference(raw, resize_dims, crop, flip, rotate, jitter, mean, std):
    """numpy composition of the reference's pixel path with the jitter: geometry, colour jitter, mmcv normalise."""
    return normalize(jitter_rgb(geometry_u8(raw, resize_dims, crop, flip, rotate), jitter), mean, std)


def decode_jitter(vec):
    """Fixture layout [delta, mode, alpha, saturation, hue, perm0, perm1, perm2] (NaN = step off) -> ``sample_jitter``'s dict."""
    val = [None if np.isnan(x) else float(x) for x in vec]
    return dict(delta=val[0], mode=int(val[1]), alpha=val[2], saturation=val[3], hue=val[4],
                perm=None if val[5] is None else tuple(int(x) for x in val[5:8]))


def _loader(is_train=True, **kw):
    return P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=AUG_CONFIG, is_train=is_train,
                                  colorjitter=True, img_norm_cfg=NORM, device="cpu", **kw))


def _restated_stream(seed):
    """The draws of one loader call (shared geometric draw, right view's jitter, left view's jitter) and the next value."""
    Hs, Ws = stereo_images()[1].shape[:2]
    step = _loader()
    np.random.seed(seed)
    step.sample_augmentation(H=Hs, W=Ws)
    right, left = step.sample_jitter(), step.sample_jitter()
    return right, left, np.random.uniform()


def test_colorjitter_is_accepted_in_training_and_load_depth_still_refused():
    step = _loader()
    assert step.colorjitter and step.is_train
    with pytest.raises(NotImplementedError, match="load_depth"):
        _loader(load_depth=True)
    with pytest.raises(NotImplementedError, match="training only"):         # the upstream ignores it there
        _loader(is_train=False)
    lib = capi.load()
    assert lib.ssbev_version() >= 102 and hasattr(lib, "ssbev_crop_rotate_jitter_normalize_u8")


def test_draw_restatement_consumes_upstreams_rng_stream():
    """Over the fixture's >= 200 seeds: the same values drawn for each view, and the same next value of the stream."""
    g = load_golden("image_jitter")
    seeds = g["stream_seeds"].tolist()
    assert len(seeds) >= 200
    modes, coins = set(), np.zeros(5, dtype=np.int64)
    for i, seed in enumerate(seeds):
        right, left, nxt = _restated_stream(seed)
        for k, got in enumerate((right, left)):
            want = decode_jitter(g["stream_jitter"][i, k])
            assert got == want, (seed, k, got, want)
            modes.add(got["mode"])
            coins += [got[n] is not None for n in ("delta", "alpha", "saturation", "hue", "perm")]
        assert nxt == float(g["stream_next"][i]), seed
    assert modes == {0, 1} and (coins > 0).all() and (coins < 2 * len(seeds)).all()


@pytest.mark.skipif(not os.path.exists(REFERENCE_LOADER), reason="needs the reference checkout")
def test_draw_restatement_against_the_live_reference_loader():
    """The reference's own loader with colorjitter=True (tools/make_golden_jitter.py --stream, a fresh process: the stand-ins
    replace modules) on 256 seeds, against the restatement."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_jitter.py"), "--stream", "256"],
                         capture_output=True, text=True, check=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"),
                         timeout=600).stdout
    rows = [json.loads(line) for line in out.splitlines() if line.startswith("{")]
    assert len(rows) == 256
    for row in rows:
        right, left, nxt = _restated_stream(row["seed"])
        assert [right, left] == [decode_jitter(np.asarray(v, dtype=np.float64)) for v in row["jitter"]], row
        assert nxt == row["next"], row


def test_numpy_statement_reproduces_reference_loader_pixels():
    """The pixel path the kernel implements, composed in numpy, against the reference loader's ``img``: bit for bit."""
    g = load_golden("image_jitter")
    imgs = stereo_images()
    for seed in g["seeds"].tolist():
        for k, name in enumerate(("left", "right")):
            jitter = decode_jitter(g[f"s{seed}_{name}_jitter"])
            got = augment_jitter_reference(imgs[k], g[f"s{seed}_resize_dims"], g[f"s{seed}_crop"], int(g[f"s{seed}_flip"]),
                                           float(g[f"s{seed}_rotate"]), jitter, NORM["mean"], NORM["std"])
            assert np.array_equal(got, g[f"s{seed}_{name}_img"][0]), (seed, name)


def test_fixture_covers_every_step():
    """The fixture's seeds exercise both modes, each step, a hue wrap on both sides and the uint8 wrap on both sides."""
    g = load_golden("image_jitter")
    imgs = stereo_images()
    seen = set()
    for seed in g["seeds"].tolist():
        for k, name in enumerate(("left", "right")):
            j = decode_jitter(g[f"s{seed}_{name}_jitter"])
            seen.add(f"mode{j['mode']}")
            seen.update(n for n in ("delta", "alpha", "saturation", "perm") if j[n] is not None)
            bgr = geometry_u8(imgs[k], g[f"s{seed}_resize_dims"], g[f"s{seed}_crop"], int(g[f"s{seed}_flip"]),
                              float(g[f"s{seed}_rotate"]))[..., ::-1]
            if j["hue"] is not None:
                pre = bgr.astype(np.float32)                                # steps 1-2: what the HSV conversion sees
                pre += np.float32(j["delta"] if j["delta"] is not None else 0.0)
                pre *= np.float32(j["alpha"] if j["mode"] == 1 and j["alpha"] is not None else 1.0)
                h = bgr2hsv(pre)[..., 0] + np.float32(j["hue"])
                seen.update(["hue>360"] if (h > 360).any() else [])
                seen.update(["hue<0"] if (h < 0).any() else [])
            x = photometric(bgr, j)
            seen.update(["below0"] if (x < 0).any() else [])
            seen.update(["above255"] if (x >= 256).any() else [])
    assert seen >= {"mode0", "mode1", "delta", "alpha", "saturation", "perm", "hue>360", "hue<0", "below0", "above255"}, seen


def test_jitter_params_struct_from_a_draw():
    p = P.jitter_params(dict(delta=-3.25, mode=1, alpha=None, saturation=1.2, hue=None, perm=(2, 0, 1)))
    assert p.flags == capi.JITTER_BRIGHTNESS | capi.JITTER_SATURATION | capi.JITTER_SWAP and p.mode == 1
    assert p.delta == -3.25 and p.alpha == 1.0 and p.saturation == np.float32(1.2) and p.hue == 0.0
    assert list(p.perm) == [2, 0, 1]
    p = P.jitter_params(dict(delta=None, mode=0, alpha=0.75, saturation=None, hue=-17.5, perm=None))
    assert p.flags == capi.JITTER_CONTRAST | capi.JITTER_HUE and p.mode == 0 and list(p.perm) == [0, 1, 2]


def test_crop_rotate_jitter_normalize_entry_point_validates_arguments_on_host():
    import ctypes as C
    lib = capi.load()
    mean = (C.c_float * 3)(1.0, 2.0, 3.0)
    stdinv = (C.c_float * 3)(1.0, 1.0, 1.0)
    aff = (C.c_int32 * 6)(65536, 0, 32768, 0, 65536, 32768)
    src, dst = C.c_void_p(16), C.c_void_p(32)          # never dereferenced: every call below fails its host-side checks
    f = lib.ssbev_crop_rotate_jitter_normalize_u8

    def params(**kw):
        p = capi.JitterParams(flags=31, mode=0, delta=5.0, alpha=1.2, saturation=0.8, hue=10.0)
        p.perm[:] = [2, 0, 1]
        for k, v in kw.items():
            if k == "perm":
                p.perm[:] = v
            else:
                setattr(p, k, v)
        return C.byref(p)
    ok = params()
    assert f(None, 4, 4, dst, 0, 0, 4, 4, 0, aff, ok, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, None, 0, 0, 4, 4, 0, aff, ok, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, None, ok, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, None, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, ok, None, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, ok, mean, None, 0, None) == capi.EINVAL
    for Hs, Ws, w, h in ((0, 4, 4, 4), (4, -1, 4, 4), (4, 4, 0, 4), (4, 4, 4, -2)):
        assert f(src, Hs, Ws, dst, 0, 0, w, h, 0, aff, ok, mean, stdinv, 0, None) == capi.EINVAL
    bad = [dict(perm=[0, 0, 1]), dict(perm=[0, 1, 3]), dict(perm=[-1, 1, 2]), dict(perm=[1, 1, 1]), dict(mode=2),
           dict(mode=-1), dict(flags=32), dict(flags=-1), dict(delta=float("nan")), dict(delta=300.0), dict(alpha=-0.5),
           dict(alpha=float("inf")), dict(saturation=9.0), dict(saturation=float("nan")), dict(hue=361.0),
           dict(hue=float("-inf"))]
    for kw in bad:
        assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, params(**kw), mean, stdinv, 0, None) == capi.EINVAL, kw


def test_hsv_restatement_against_opencv():
    """Nobody has compared the restatement with OpenCV (it is not installed where the fixture was made): where it is, the two
    conversions must agree bit for bit on random float images, including values outside 0..255 as the jitter produces."""
    cv2 = pytest.importorskip("cv2")
    rng = np.random.default_rng(11)
    for lo, hi in ((0, 256), (-48, 431), (-1, 1)):
        img = rng.uniform(lo, hi, (64, 97, 3)).astype(np.float32)
        img[:8] = np.round(img[:8])                       # ties between channels: the v == r / v == g branches
        img[8:12] = img[8:12, :, :1]                      # grey pixels (s == 0)
        hsv = bgr2hsv(img)
        assert np.array_equal(cv2.cvtColor(img, cv2.COLOR_BGR2HSV), hsv), (lo, hi)
        hsv[..., 1] *= np.float32(1.4)
        hsv[..., 0] = (hsv[..., 0] + np.float32(17.0)) % np.float32(360)
        assert np.array_equal(cv2.cvtColor(hsv, cv2.COLOR_HSV2BGR), hsv2bgr(hsv)), (lo, hi)
