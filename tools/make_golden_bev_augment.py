"""Generate tests/golden/bev_augment.npz: the BEV augmentation of the voxel labels (``pipelines.bev_transform``,
loading_semkitti.py:304-356) on the cases of tests/bev_augment_cases.py.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_bev_augment.py        (needs scipy; no GPU)

Per case the file holds the shape, the angle, the two flip flags, the six coefficients of scipy's source map
(``pipelines.bev_rotate_coeffs``: with them in the file the kernel tests need no scipy; empty for a skipped rotation) and two
expected grids, uint8 [X,Y,Z]:
  ``reference``  the HOST ``pipelines.bev_transform`` as it stands: the upstream's rotation IN PLACE, whose raster walk reads
                 voxels it has already overwritten, then the flips;
  ``exact``      plain out-of-place ``scipy.ndimage.rotate`` on a copy, then the same flips.
Small cases store labels and grids as they are; the two 256 x 256 x 32 cases store a seed and the packed form that
bev_augment_cases.pack_big checks to be lossless."""
import os
import sys

import numpy as np
import scipy.ndimage
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import bev_augment_cases as B  # noqa: E402
from stereoscene_amd import pipelines as P  # noqa: E402

CENTER = torch.tensor([25.6, 0.0, 1.2])


def main():
    out = {}
    for name, shape, angle, fdx, fdy, seed in B.case_list():
        labels = B.small_labels(name, shape) if seed is None else B.big_labels(seed, shape)
        rotates = not np.isclose(angle, 0)
        ref, _ = P.bev_transform(torch.from_numpy(labels.copy()), angle, 1.0, fdx, fdy, CENTER)
        ref = ref.numpy().astype(np.uint8)
        exact = labels
        if rotates:
            exact = scipy.ndimage.rotate(labels.copy(), angle, mode="constant", order=0, cval=B.FILL, axes=(0, 1), reshape=False)
        if fdy:
            exact = exact[:, ::-1]
        if fdx:
            exact = exact[::-1]
        exact = np.ascontiguousarray(exact)
        out[f"{name}_shape"] = np.array(shape, dtype=np.int32)
        out[f"{name}_angle"] = np.float64(angle)
        out[f"{name}_flips"] = np.array([fdx, fdy], dtype=np.uint8)
        out[f"{name}_coeffs"] = np.array(P.bev_rotate_coeffs(shape[0], shape[1], angle) if rotates else [], dtype=np.float64)
        if seed is None:
            out[f"{name}_labels"], out[f"{name}_reference"], out[f"{name}_exact"] = labels, ref, exact
        else:
            for q, grid in (("reference", ref), ("exact", exact)):
                out[f"{name}_{q}_plane0"], out[f"{name}_{q}_fill"] = B.pack_big(grid)
        print(f"{name}: {shape} angle {angle} flips ({int(fdx)}, {int(fdy)}): in-place differs from out-of-place in "
              f"{int((ref != exact).sum())} of {ref.size} voxels, {int((exact == B.FILL).sum())} filled")
    path = B.GOLDEN
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()
