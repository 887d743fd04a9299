"""Shared by tests/test_point_head.py and tests/test_gpu_point_head.py: the fixture tests/golden/point_head.npz
(tools/make_golden_point_head.py), the cases rebuilt from ``synthetic.point_head_case``, the runner and the bounds.

Bounds, the rule of tests/point_xyz_cases.py: K = 8 times the case's recorded spread of the quantity (fp32 tensor form on the CPU
against the float64 result, relative to the quantity's largest float64 magnitude), floored at the fp32 unit roundoff 2^-23, times
that magnitude, on EVERY element; a quantity that is exactly 0 in float64 (case G, the empty sample's gradients) must be exactly 0.
The same bound serves the fused path and the tensor form on the card.  Spreads recorded by the generator (largest over the
quantities of a case; the smallest sit below the floor): A 2.5e-7, B 5.2e-7, C1 5.4e-7, C2 3.1e-7, D 4.8e-7, E 3.4e-7, F 8.7e-7,
G 2.3e-7 (its logits; everything else of G is exactly 0)."""
import functools
import os

import numpy as np
import torch

from conftest import ROOT
from stereoscene_amd import synthetic as S

GOLDEN = os.path.join(ROOT, "tests", "golden", "point_head.npz")
K = 8.0
EPS = 2.0 ** -23
CASES = S.POINT_HEAD_ORDER


@functools.lru_cache(maxsize=None)
def golden():
    return dict(np.load(GOLDEN))


@functools.lru_cache(maxsize=None)
def case(name):
    """The case's inputs: rebuilt from the hash generator, shared and never modified."""
    return S.point_head_case(name)


def build_head(name, device="cpu"):
    from stereoscene_amd.plugin.voxel_encoder import OccHead
    head = OccHead(**case(name)["head_kwargs"])
    S.fill_state_dict_(head, prefix=f"point_head/{name}/")
    return head.to(device).train()


def point_params(head):
    return {n: p for n, p in head.named_parameters() if n.split(".")[0] in ("img_feat_reduce", "point_soft_weights", "point_occ_mlp")}


def run(name, device, head=None):
    """One forward + backward of the point-level branch: dict logits [N, K], ce, lov (0-dim), g:<parameter>, gfeat<l>
    [B, C, X, Y, Z] and gimg [B, cams, C_img, fH, fW] (CPU tensors).  The scalar that is differentiated is ce + lov."""
    c = case(name)
    head = head or build_head(name, device)
    head.zero_grad()
    feats = [f.clone().to(device).requires_grad_(True) for f in c["feats"]]
    img = c["img_feats"].clone().to(device).requires_grad_(True) if c["img_feats"] is not None else None
    pts = [p.to(device) for p in c["points"]]
    uv = [u.to(device) for u in c["points_uv"]] if c["points_uv"] is not None else None
    logits = torch.cat(head.forward_points(pts, feats, img, uv), 0)
    losses = head.loss_point_single(logits, torch.cat(pts, 0))
    (losses["loss_point_ce_"] + losses["loss_point_lovasz_"]).backward()
    out = {"logits": logits.detach().cpu(), "ce": losses["loss_point_ce_"].detach().cpu(),
           "lov": losses["loss_point_lovasz_"].detach().cpu()}
    for n, p in point_params(head).items():
        out[f"g:{n}"] = p.grad.detach().cpu()
    for l, f in enumerate(feats):
        out[f"gfeat{l}"] = f.grad.detach().cpu()
    if img is not None:
        out["gimg"] = img.grad.detach().cpu()
    return out


def quantities(name):
    return sorted(k[len(name) + 5:] for k in golden() if k.startswith(f"{name}_f64_"))


def tol(name, q):
    g = golden()
    scale = float(np.abs(g[f"{name}_f64_{q}"]).max()) if g[f"{name}_f64_{q}"].size else 0.0
    return K * max(float(g[f"{name}_spread_{q}"]), EPS) * scale


def check(name, got, what):
    g = golden()
    qs = quantities(name)
    assert set(qs) == set(got), (sorted(got), qs)
    for q in qs:
        want = g[f"{name}_f64_{q}"]
        have = got[q].double().numpy()
        assert have.shape == want.shape, (name, what, q, have.shape, want.shape)
        err = float(np.abs(have - want).max()) if want.size else 0.0
        bound = tol(name, q)
        print(name, what, q, "error against float64", err, "bound", bound)
        assert np.isfinite(have).all() and err <= bound, (name, what, q, err, bound)
