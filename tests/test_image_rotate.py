"""Image-view rotation (loading_semkitti.py:120-135), host side: the restatement of Pillow's fixed-point ``Image.rotate``
against Pillow itself, the draw and the pixel map against the reference loader run with the upstream's commented
augmentation config (tests/golden/image_augment.npz, tools/make_golden_augment.py), the refusals, and the argument checks
of the new entry point.  No GPU."""
import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle import data_ref as DR
from oracle.make_golden_data import stereo_images
from stereoscene_amd import capi, pipelines as P

# the config the fixture was generated with (tools/make_golden_augment.py): stereoscene.py:34-36 uncommented, at the
# fixture's image size
AUG_CONFIG = {"input_size": (48, 160), "resize": (-0.06, 0.11), "rot": (-5.4, 5.4), "flip": True, "crop_h": (0.0, 0.0),
              "resize_test": 0.0}
NORM = dict(mean=[123.675, 116.28, 103.53], std=[58.395, 57.12, 57.375], to_rgb=True)


def rotate_gather(img, affine):
    """What libImaging's ``affine_fixed`` does with the 6 fixed-point coefficients: nearest pixel, 0 outside."""
    h, w = img.shape[:2]
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    a = affine.astype(np.int64)
    xi = (a[2] + y * a[1] + x * a[0]) >> 16
    yi = (a[5] + y * a[4] + x * a[3]) >> 16
    ok = (xi >= 0) & (xi < w) & (yi >= 0) & (yi < h)
    out = np.zeros_like(img)
    out[ok] = img[yi[ok], xi[ok]]
    return out


def augment_reference(raw, resize_dims, crop, flip, rotate, mean, std):
    """numpy composition of the reference's pixel path: Pillow resize, zero-padded crop, mirror, rotate, mmcv normalise."""
    r = DR.pil_resize_u8(raw, tuple(resize_dims))
    x0, y0, x1, y1 = (int(v) for v in crop)
    c = np.zeros((y1 - y0, x1 - x0, 3), dtype=np.uint8)
    ys, xs = slice(max(y0, 0), min(y1, r.shape[0])), slice(max(x0, 0), min(x1, r.shape[1]))
    c[ys.start - y0:ys.stop - y0, xs.start - x0:xs.stop - x0] = r[ys, xs]
    if flip:
        c = c[:, ::-1]
    c = rotate_gather(np.ascontiguousarray(c), P.pil_rotate_fixed(c.shape[1], c.shape[0], rotate))
    m = np.asarray(mean, dtype=np.float32)
    si = (1.0 / np.asarray(std, dtype=np.float32).astype(np.float64)).astype(np.float32)
    return ((c.astype(np.float32) - m) * si).transpose(2, 0, 1)


def test_fixed_point_rotate_restatement_is_byte_exact_with_pillow():
    from PIL import Image
    rng = np.random.default_rng(7)
    fixed = [0.0, -0.0, 1e-7, 90.0, 180.0, 270.0, 360.0, 123.456, -90.0]
    for (h, w) in [(48, 160), (384, 1280), (47, 155), (33, 101), (64, 64)]:
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        angles = fixed + list(rng.uniform(-5.4, 5.4, 4)) + list(rng.uniform(-22.5, 22.5, 3))
        for ang in angles:
            a = P.pil_rotate_fixed(w, h, ang)
            assert a.dtype == np.int32 and a.shape == (6,)
            want = np.asarray(Image.fromarray(img).rotate(ang))
            assert np.array_equal(rotate_gather(img, a), want), (h, w, ang)


def test_fixed_point_range_is_refused_outside_pillows_fixed_path():
    P.pil_rotate_fixed(1280, 384, 5.4)                          # KITTI size: far inside
    with pytest.raises(NotImplementedError, match="fixed-point range"):
        P.pil_rotate_fixed(40000, 48, 1.0)
    with pytest.raises(NotImplementedError, match="fixed-point range"):
        P.pil_rotate_fixed(30000, 30000, 45.0)


def test_augmentation_draw_and_pixel_map_match_reference_loader():
    g = load_golden("image_augment")
    Hs, Ws = stereo_images()[1].shape[:2]
    step = P.PIPELINES.build(dict(type="LoadMultiViewImageFromFiles_SemanticKitti", data_config=AUG_CONFIG, is_train=True,
                                  device="cpu"))
    flips, signs = set(), set()
    for seed in g["seeds"].tolist():
        np.random.seed(seed)
        resize, dims, crop, flip, rotate = step.sample_augmentation(H=Hs, W=Ws)
        assert resize == float(g[f"s{seed}_resize"]) and list(dims) == g[f"s{seed}_resize_dims"].tolist()
        assert list(crop) == g[f"s{seed}_crop"].tolist() and int(bool(flip)) == int(g[f"s{seed}_flip"])
        assert rotate == float(g[f"s{seed}_rotate"]) and rotate != 0
        flips.add(bool(flip))
        signs.add(rotate > 0)
        rot2, tran2 = step.pixel_map(torch.eye(2), torch.zeros(2), resize, crop, flip, rotate)
        for name in ("left", "right"):
            assert np.abs(rot2.numpy() - g[f"s{seed}_{name}_post_rot"][0][:2, :2]).max() < 1e-6, (seed, name)
            assert np.abs(tran2.numpy() - g[f"s{seed}_{name}_post_tran"][0][:2]).max() < 1e-5, (seed, name)
    assert flips == {False, True} and signs == {False, True}
    # rotate == 0: no fourth step, the map is the three-step one
    a = step.pixel_map(torch.eye(2), torch.zeros(2), 1.1, (3, 2, 163, 50), True)
    b = step.pixel_map(torch.eye(2), torch.zeros(2), 1.1, (3, 2, 163, 50), True, 0.0)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_numpy_composition_reproduces_reference_loader_pixels():
    """The pixel path the kernel implements, composed in numpy, against the reference loader's ``img``: bit for bit."""
    g = load_golden("image_augment")
    imgs = stereo_images()
    for seed in g["seeds"].tolist():
        for k, name in enumerate(("left", "right")):
            got = augment_reference(imgs[k], g[f"s{seed}_resize_dims"], g[f"s{seed}_crop"], int(g[f"s{seed}_flip"]),
                                    float(g[f"s{seed}_rotate"]), NORM["mean"], NORM["std"])
            assert np.array_equal(got, g[f"s{seed}_{name}_img"][0]), (seed, name)


def test_crop_rotate_normalize_entry_point_validates_arguments_on_host():
    import ctypes as C
    lib = capi.load()
    assert lib.ssbev_version() >= 101
    mean = (C.c_float * 3)(1.0, 2.0, 3.0)
    stdinv = (C.c_float * 3)(1.0, 1.0, 1.0)
    aff = (C.c_int32 * 6)(65536, 0, 32768, 0, 65536, 32768)
    src, dst = C.c_void_p(16), C.c_void_p(32)          # never dereferenced: every call below fails its host-side checks
    f = lib.ssbev_crop_rotate_normalize_u8
    assert f(None, 4, 4, dst, 0, 0, 4, 4, 0, aff, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, None, 0, 0, 4, 4, 0, aff, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, None, mean, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, None, stdinv, 0, None) == capi.EINVAL
    assert f(src, 4, 4, dst, 0, 0, 4, 4, 0, aff, mean, None, 0, None) == capi.EINVAL
    for Hs, Ws, w, h in ((0, 4, 4, 4), (4, -1, 4, 4), (4, 4, 0, 4), (4, 4, 4, -2)):
        assert f(src, Hs, Ws, dst, 0, 0, w, h, 0, aff, mean, stdinv, 0, None) == capi.EINVAL
