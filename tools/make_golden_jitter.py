"""Generate tests/golden/image_jitter.npz: the reference's own LoadMultiViewImageFromFiles_SemanticKitti
(loading_semkitti.py:76-302) in train mode with ``colorjitter=True`` and the rotation config of tools/make_golden_augment.py,
so every view goes through PhotoMetricDistortionMultiViewImage (loading_bevdet.py:532-620).  Build container only (needs the
reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_jitter.py
      PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_jitter.py --stream N   (one JSON line per seed 0..N-1, no file)

Inputs and stand-ins are those of tools/make_golden_augment.py, plus ``mmcv.bgr2hsv`` / ``mmcv.hsv2bgr``: OpenCV is not
installed here, so they are the numpy restatement of OpenCV's float conversions in tests/test_image_jitter.py (whether genuine
OpenCV agrees bit for bit is checked there only where cv2 is present).  The values each view draws are read from a recorder
that stands in for the ``numpy.random`` module inside loading_bevdet.py and logs every call in order.  Stored: per image seed
the shared geometric draw, per view the jitter ([delta, mode, alpha, saturation, hue, perm0..2], NaN = step off) and ``img``,
and the first ``np.random.uniform()`` after the call; for the stream seeds, both views' jitter and that next value."""
import importlib
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import make_golden_augment as MGA  # noqa: E402
import test_image_jitter as TJ  # noqa: E402
from oracle import make_golden_data as MGD  # noqa: E402

SEEDS = (0, 3, 6, 11)              # both modes, every step, hue and uint8 wraps on both sides, both flips and angle signs
STREAM_SEEDS = 256


class Recorder:
    """``numpy.random`` as loading_bevdet.py calls it (``from numpy import random``), logging (name, args, value)."""

    def __init__(self):
        self.log = []

    def _call(self, name, *args):
        v = getattr(np.random, name)(*args)
        self.log.append((name, args, v))
        return v

    def randint(self, *a):
        return self._call("randint", *a)

    def uniform(self, *a):
        return self._call("uniform", *a)

    def permutation(self, *a):
        return self._call("permutation", *a)


def parse(log):
    """One view's call log -> [delta, mode, alpha, saturation, hue, perm0, perm1, perm2] (NaN = step off)."""
    it = iter(log)

    def take(name, *args):
        got, a, v = next(it)
        assert got == name and tuple(a) == args, (got, a, name, args)
        return v
    out = [np.nan] * 8
    if take("randint", 2):
        out[0] = take("uniform", -32, 32)
    out[1] = mode = int(take("randint", 2))
    if mode == 1 and take("randint", 2):
        out[2] = take("uniform", 0.5, 1.5)
    if take("randint", 2):
        out[3] = take("uniform", 0.5, 1.5)
    if take("randint", 2):
        out[4] = take("uniform", -18, 18)
    if mode == 0 and take("randint", 2):
        out[2] = take("uniform", 0.5, 1.5)
    if take("randint", 2):
        out[5:8] = [float(v) for v in take("permutation", 3)]
    assert next(it, None) is None
    return np.asarray(out, dtype=np.float64)


def reference_loader():
    MGA.install_stand_ins()
    sys.modules["mmcv"].bgr2hsv = TJ.bgr2hsv
    sys.modules["mmcv"].hsv2bgr = TJ.hsv2bgr
    LS = importlib.import_module("projects.mmdet3d_plugin.datasets.pipelines.loading_semkitti")
    LB = importlib.import_module("projects.mmdet3d_plugin.datasets.pipelines.loading_bevdet")
    rec = Recorder()
    LB.random = rec
    step = LS.LoadMultiViewImageFromFiles_SemanticKitti(data_config=MGA.AUG_CONFIG, is_train=True, colorjitter=True,
                                                        img_norm_cfg=MGA.NORM)
    views = []
    jitter = step.pipeline_colorjitter

    def recorded(img):
        rec.log = []
        out = jitter(img)
        views.append(parse(rec.log))
        return out
    step.pipeline_colorjitter = recorded
    drawn = []
    draw = step.sample_augmentation
    step.sample_augmentation = lambda *a, **k: drawn.append(draw(*a, **k)) or drawn[-1]

    def run(seed, names, meta):
        views.clear(), drawn.clear()
        np.random.seed(seed)
        results = step(dict(img_filename=names, gt_occ=np.zeros((4, 4, 2), dtype=np.uint8), **meta))
        assert len(views) == 2 and len(drawn) == 1
        return results, drawn[0], views[0], views[1], np.random.uniform()       # views: right first, then left
    return run


def coverage(img, geo, jitter):
    """What one view exercises, on the restatement (see tests/test_image_jitter.py: test_fixture_covers_every_step)."""
    resize, dims, crop, flip, rotate = geo
    j = TJ.decode_jitter(jitter)
    bgr = TJ.geometry_u8(img, dims, crop, int(bool(flip)), rotate)[..., ::-1]
    seen = {f"mode{j['mode']}"} | {n for n in ("delta", "alpha", "saturation", "perm") if j[n] is not None}
    if j["hue"] is not None:
        pre = bgr.astype(np.float32)
        pre += np.float32(j["delta"] if j["delta"] is not None else 0.0)
        pre *= np.float32(j["alpha"] if j["mode"] == 1 and j["alpha"] is not None else 1.0)
        h = TJ.bgr2hsv(pre)[..., 0] + np.float32(j["hue"])
        seen |= ({"hue>360"} if (h > 360).any() else set()) | ({"hue<0"} if (h < 0).any() else set())
    x = TJ.photometric(bgr, j)
    return seen | ({"below0"} if (x < 0).any() else set()) | ({"above255"} if (x >= 256).any() else set())


def main():
    import torch
    from PIL import Image
    torch.set_num_threads(1)
    stream = int(sys.argv[sys.argv.index("--stream") + 1]) if "--stream" in sys.argv else None
    run = reference_loader()
    imgs, meta = MGD.stereo_images(), MGD.stereo_meta()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        names = []
        for im, cam in zip(imgs, ("image_2", "image_3")):
            d = os.path.join(tmp, "sequences", "00", cam)
            os.makedirs(d)
            Image.fromarray(im).save(os.path.join(d, "000123.png"))
            names.append(os.path.join(d, "000123.png"))
        if stream is not None:
            for seed in range(stream):
                _, _, right, left, nxt = run(seed, names, meta)
                print(json.dumps(dict(seed=seed, jitter=[right.tolist(), left.tolist()], next=nxt)))     # NaN: step off
            return
        sj, sn = [], []
        for seed in range(STREAM_SEEDS):
            _, _, right, left, nxt = run(seed, names, meta)
            sj.append([right, left])
            sn.append(nxt)
        out["stream_seeds"] = np.arange(STREAM_SEEDS, dtype=np.int64)
        out["stream_jitter"] = np.asarray(sj, dtype=np.float64)
        out["stream_next"] = np.asarray(sn, dtype=np.float64)
        out["seeds"] = np.asarray(SEEDS, dtype=np.int64)
        seen = set()
        for seed in SEEDS:
            results, geo, right, left, nxt = run(seed, names, meta)
            resize, dims, crop, flip, rotate = geo
            out[f"s{seed}_resize"] = np.float64(resize)
            out[f"s{seed}_resize_dims"] = np.asarray(dims, dtype=np.int64)
            out[f"s{seed}_crop"] = np.asarray(crop, dtype=np.int64)
            out[f"s{seed}_flip"] = np.int64(bool(flip))
            out[f"s{seed}_rotate"] = np.float64(rotate)
            out[f"s{seed}_next"] = np.float64(nxt)
            for k, (name, jit) in enumerate((("left", left), ("right", right))):
                out[f"s{seed}_{name}_jitter"] = jit
                out[f"s{seed}_{name}_img"] = np.asarray(results["img_inputs"][k][0])
                cov = coverage(imgs[k], geo, jit)
                seen |= cov
                print("seed", seed, name, "jitter", np.round(jit, 3).tolist(), sorted(cov))
    want = {"mode0", "mode1", "delta", "alpha", "saturation", "perm", "hue>360", "hue<0", "below0", "above255"}
    assert seen >= want, want - seen
    path = os.path.join(ROOT, "tests", "golden", "image_jitter.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
