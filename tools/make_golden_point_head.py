"""Generate tests/golden/point_head.npz: the point-level branch of the occupancy head (occupancy/dense_heads/occhead.py:171-236
sample_point_feats, 428-453 feature_sampling, 363-398 loss_point_single, dense_heads/mlp.py) on the cases of
``stereoscene_amd.synthetic.POINT_HEAD_CASES`` in float64 on the CPU.

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_point_head.py

The reference's own functions need mmcv / mmdet3d to import, which this generator does not assume: ``restated`` below is the same
``grid_sample`` formulation, sample by sample and level by level as the reference loops, in float64 (recorded in the file as
``source``).  It shares the case inputs and the parameter values with the code under test and nothing else: the normalisation, the
``grid_sample`` calls with the coordinates as the reference hands them over (flipped for ``point_axis_order="xyz"``), the mask, the
camera sum, the soft weights, the MLP with the exact GELU, ``CrossEntropyLoss(ignore_index=0)`` and the Lovasz-softmax over the
classes present (``plugin.losses.lovasz_softmax_tensor``, itself pinned to the reference by tests/golden/lovasz.npz) are written
out here.  Two departures, as documented in ``OccHead``: no labelled point gives two zeros instead of NaN, and
``.squeeze().t()`` is a reshape so that one-point samples work.

Stored per case X and quantity q (logits, ce, lov, g:<parameter> for every parameter of the branch, gfeat<l> per voxel level,
gimg when there are image features; the differentiated scalar is ce + lov): ``X_f64_q`` (float64) and ``X_spread_q`` =
max |fp32 tensor form - f64| / max |f64|, the fp32 tensor form being ``OccHead`` on the CPU (``functional.point_sample_tensor``
and friends) -- never the fused path.  Inputs are not stored: the tests rebuild them from ``synthetic.point_head_case(name)``."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from stereoscene_amd import synthetic as S  # noqa: E402
from stereoscene_amd.plugin import losses as L  # noqa: E402

TF = torch.nn.functional


def restated(c, sd):
    """float64: dict of the quantities for case dict ``c`` and the head's state dict ``sd`` (fp32 values, widened)."""
    spec = c["spec"]
    p = {k: v.double().requires_grad_(True) for k, v in sd.items()
         if k.split(".")[0] in ("img_feat_reduce", "point_soft_weights", "point_occ_mlp")}
    feats = [f.double().requires_grad_(True) for f in c["feats"]]
    img = c["img_feats"].double().requires_grad_(True) if c["img_feats"] is not None else None
    lo = torch.tensor(S.POINT_HEAD_RANGE[:3], dtype=torch.float64)
    rng = torch.tensor(S.POINT_HEAD_RANGE[3:], dtype=torch.float64) - lo
    logits = []
    for b, pts in enumerate(c["points"]):
        n = pts.shape[0]
        if n == 0:
            continue
        g = ((pts[:, :3].double() - lo) / rng) * 2 - 1
        if spec["axis"] == "xyz":
            g = g.flip(-1)
        sets = []
        for f in feats:
            s = TF.grid_sample(f[b].unsqueeze(0), g.view(1, 1, 1, -1, 3), mode="bilinear", align_corners=False)
            sets.append(s.reshape(f.shape[1], n).t())
        if img is not None:
            uv = c["points_uv"][b].double()
            mask = (uv[..., 2] > 1e-5) & (uv[..., 0] > -1.0) & (uv[..., 0] < 1.0) & (uv[..., 1] > -1.0) & (uv[..., 1] < 1.0)
            s = TF.grid_sample(img[b], uv[..., :2].permute(1, 0, 2).unsqueeze(2), mode="bilinear", align_corners=False)
            s = torch.nan_to_num(s.squeeze(-1).permute(2, 0, 1)) * mask.double().unsqueeze(-1)
            sets.append(TF.linear(s.sum(1), p["img_feat_reduce.weight"], p["img_feat_reduce.bias"]))
        if spec["soft"]:
            h = torch.relu(TF.linear(sets[0], p["point_soft_weights.0.weight"], p["point_soft_weights.0.bias"]))
            w = torch.softmax(TF.linear(h, p["point_soft_weights.2.weight"], p["point_soft_weights.2.bias"]), dim=1)
            rows = 0
            for r, wl in zip(sets, torch.unbind(w, dim=1)):
                rows = rows + r * wl.unsqueeze(1)
        else:
            rows = sum(sets)
        h = TF.gelu(TF.linear(rows, p["point_occ_mlp.fc1.weight"], p["point_occ_mlp.fc1.bias"]))
        logits.append(TF.linear(h, p["point_occ_mlp.fc2.weight"], p["point_occ_mlp.fc2.bias"]))
    logits = torch.cat(logits, 0)
    labels = torch.cat([pts[:, -1] for pts in c["points"]], 0).long()
    if int((labels != 0).sum()) == 0:
        ce = lov = logits.sum() * 0.0
    else:
        ce = torch.nn.CrossEntropyLoss(ignore_index=0)(logits, labels)
        N, K = logits.shape
        lov = L.lovasz_softmax_tensor(logits.t().contiguous().view(1, K, N, 1, 1), labels.view(1, N, 1, 1), 0)
    (ce + lov).backward()
    out = {"logits": logits.detach(), "ce": ce.detach(), "lov": lov.detach()}
    for k, v in p.items():
        out[f"g:{k}"] = v.grad if v.grad is not None else torch.zeros_like(v)
    for l, f in enumerate(feats):
        out[f"gfeat{l}"] = f.grad if f.grad is not None else torch.zeros_like(f)
    if img is not None:
        out["gimg"] = img.grad if img.grad is not None else torch.zeros_like(img)
    return out


def main():
    import point_head_cases as X
    torch.set_num_threads(1)
    store = {"source": np.array("float64 grid_sample restatement (the reference's modules need mmcv / mmdet3d to import)")}
    for name in S.POINT_HEAD_ORDER:
        c = S.point_head_case(name)
        head = X.build_head(name)
        want = restated(c, {k: v.detach().clone() for k, v in head.state_dict().items()})
        got = X.run(name, "cpu", head)
        assert set(got) == set(want), (sorted(got), sorted(want))
        worst = 0.0
        for q, w in want.items():
            w = w.numpy()
            scale = float(np.abs(w).max()) if w.size else 0.0
            err = float(np.abs(got[q].double().numpy() - w).max()) if w.size else 0.0
            spread = err / scale if scale > 0 else 0.0
            assert scale > 0 or err == 0.0, (name, q, err)
            store[f"{name}_f64_{q}"] = w
            store[f"{name}_spread_{q}"] = np.float64(spread)
            worst = max(worst, spread)
            print(f"{name:3s} {q:34s} scale {scale:.4e} spread {spread:.3e}")
        print(f"{name}: largest spread {worst:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "point_head.npz")
    np.savez_compressed(path, **store)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
