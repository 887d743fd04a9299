"""Generate tests/golden/imgseg.npz: the reference's image-view segmentation loss (``imgseg=True``,
occupancy/image2bev/ViewTransformerLSSVoxel.py:418-430 ``get_seg_loss``) in fp32 on the cases of
``stereoscene_amd.synthetic.IMGSEG_CASES``, next to a float64 restatement of the same definition.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_imgseg.py

The reference's method is three torch calls on the CPU, made here as it makes them: ``F.interpolate(seg_preds, size=(H, W))``
(nearest), ``CrossEntropyLoss(weight=1 / log(class frequencies + 0.001), ignore_index=0, reduction="mean")`` on
``seg_labels.long()``, all fp32; the gradient is autograd's.  The float64 yardstick is ``restated`` below, written from the
definition and sharing nothing with those calls but the labels:

    cell(y, x) = (iy[y], ix[x]),  iy = imgseg_nearest_index(h, H), ix = imgseg_nearest_index(w, W)
    valid p: label in [1, 20);   num = sum_valid w[l_p] (lse(L[:, cell(p)]) - L[l_p, cell(p)]);   den = sum_valid w[l_p]
    loss = num / den  (0 without a valid pixel)

The inputs are not stored: the tests rebuild them from ``synthetic.imgseg_case(name)`` (hash-generated, exactly reproducible);
``X_logits_crc`` / ``X_labels_crc`` (crc32 of the fp32 bytes) pin them.  Stored per case X: ``X_f64_loss``, ``X_f64_grad``
(float64), ``X_n_valid``; except for C (nothing labelled: the reference returns NaN) ``X_ref_loss``, ``X_ref_grad`` (fp32),
``X_loss_spread`` = |fp32 - float64| / max(1, |float64|) and ``X_spread`` = max |fp32 grad - float64 grad| / max |float64 grad|.
The loss is the unweighted one (``loss_seg_weight`` = 1)."""
import os
import sys
import zlib

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import functional as F, synthetic as S  # noqa: E402
from stereoscene_amd.plugin.losses import semkitti_class_weights  # noqa: E402


def reference_loss(seg_preds, seg_labels, class_weights):
    """get_seg_loss (VT:418-430) on the CPU, fp32."""
    criterion = nn.CrossEntropyLoss(weight=class_weights, ignore_index=0, reduction="mean")
    if seg_preds.shape[-2:] != seg_labels.shape[-2:]:
        seg_preds = TF.interpolate(seg_preds, size=seg_labels.shape[1:])
    return criterion(seg_preds, seg_labels.long())


def restated(logits, labels, class_weights):
    """The definition of the module docstring in float64."""
    BN, K, h, w = logits.shape
    H, W = labels.shape[1:]
    iy, ix = F.imgseg_nearest_index(h, H), F.imgseg_nearest_index(w, W)
    lab = labels.long()
    valid = (lab >= 1) & (lab < K)
    cells = logits.permute(0, 2, 3, 1)[:, iy][:, :, ix]                  # [BN, H, W, K]
    lse = torch.logsumexp(cells, dim=-1)
    picked = cells.gather(-1, lab.clamp(0, K - 1).unsqueeze(-1)).squeeze(-1)
    wl = class_weights.double()[lab.clamp(0, K - 1)] * valid.double()
    den = wl.sum()
    num = (wl * (lse - picked)).sum()
    return num / den if float(den) > 0 else num * 0.0


def with_grad(fn, logits, dtype):
    x = logits.to(dtype).requires_grad_(True)
    loss = fn(x)
    loss.backward()
    return loss.detach(), x.grad


def cell_counts(labels, h, w):
    """Valid pixels per cell, [BN, h, w]."""
    BN, H, W = labels.shape
    iy, ix = F.imgseg_nearest_index(h, H), F.imgseg_nearest_index(w, W)
    valid = ((labels >= 1) & (labels < S.IMGSEG_CLASSES)).long()
    out = torch.zeros(BN, h, w, dtype=torch.long)
    out.index_put_((torch.arange(BN)[:, None, None].expand(BN, H, W), iy[None, :, None].expand(BN, H, W),
                    ix[None, None, :].expand(BN, H, W)), valid, accumulate=True)
    return out


def main():
    torch.set_num_threads(1)
    cw = semkitti_class_weights()
    out = {}
    for name, (BN, (h, w), (H, W), _) in S.IMGSEG_CASES.items():
        logits, labels = S.imgseg_case(name)
        assert logits.shape == (BN, S.IMGSEG_CLASSES, h, w) and labels.shape == (BN, H, W)
        assert torch.equal(labels, labels.floor()) and 0 <= float(labels.min()) and float(labels.max()) <= 19
        out[f"{name}_logits_crc"] = np.int64(zlib.crc32(logits.numpy().tobytes()))
        out[f"{name}_labels_crc"] = np.int64(zlib.crc32(labels.numpy().tobytes()))
        l64, g64 = with_grad(lambda x: restated(x, labels, cw), logits, torch.float64)
        counts = cell_counts(labels, h, w)
        n_valid = int(counts.sum())
        out[f"{name}_f64_loss"] = np.float64(l64.item())
        out[f"{name}_f64_grad"] = g64.numpy()
        out[f"{name}_n_valid"] = np.int64(n_valid)
        line = f"case {name}: {n_valid} / {labels.numel()} valid pixels, f64 loss {l64.item():.9f} max|grad| {g64.abs().max().item():.3e}"
        if name == "C":
            assert n_valid == 0 and l64.item() == 0.0 and not g64.any()
            print(line)
            continue
        assert n_valid > 0
        if name == "A":
            assert int(counts[1, 2, 4]) == 0 and int((counts == 0).sum()) == 1
            assert not (labels == 0).all() and not labels[labels > 0].eq(0).any()
        if name == "B":
            assert set(labels.unique().long().tolist()) == set(range(20)) and H % h and W % w
            sizes = {(int((F.imgseg_nearest_index(h, H) == i).sum()), int((F.imgseg_nearest_index(w, W) == j).sum()))
                     for i in range(h) for j in range(w)}
            assert len(sizes) > 1 and max(a * b for a, b in sizes) > 64, sizes
        if name == "D":
            assert int(counts[0, 0, 0]) == 1 and int(counts[0, 0, 1]) == 0 and float(logits.abs().max()) > 70
        l32, g32 = with_grad(lambda x: reference_loss(x, labels, cw), logits, torch.float32)
        assert torch.isfinite(l32) and torch.isfinite(g32).all(), name
        empty = (counts == 0).unsqueeze(1).expand_as(g64)
        assert not g64[empty].any() and not g32[empty].any()
        out[f"{name}_ref_loss"] = np.float32(l32.item())
        out[f"{name}_ref_grad"] = g32.numpy()
        spread = ((g32.double() - g64).abs().max() / g64.abs().max()).item()
        lspread = abs(l32.item() - l64.item()) / max(1.0, abs(l64.item()))
        out[f"{name}_spread"] = np.float64(spread)
        out[f"{name}_loss_spread"] = np.float64(lspread)
        print(line + f" | fp32 loss {l32.item():.9f} grad spread {spread:.2e} loss spread {lspread:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "imgseg.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
