"""Generate tests/golden/ohem.npz: the reference's own ``OHEM_CE_ssc_loss`` (utils/semkitti.py:151-185) in fp32 on the cases of
``stereoscene_amd.synthetic.OHEM_CASES``, called as the head calls it (``OHEM_CE_ssc_loss(up, target, class_weights, top_k)``,
``up`` = trilinear, align_corners=False), next to a float64 restatement of the same formulas.  Build container only (needs the
reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_ohem.py [--ref /path/to/reference]

The reference module is loaded BY FILE PATH (it imports only torch and numpy; the package __init__ drags in mmcv).  The inputs
are not stored: the tests rebuild them from ``synthetic.ohem_case(name)`` (hash-generated, exactly reproducible).

The float64 restatement (``ohem_restated``): class-weighted cross entropy per voxel, canonicalised to +0.0; per sample the
``int(M_b * top_k)`` largest, EQUAL LOSSES TO THE LOWEST VOXEL INDEX (a stable descending sort; ``torch.topk`` leaves that choice
open); sum of the kept losses over the clamped sum of the kept class weights.  Which losses are EQUAL is a statement about fp32,
the format the loss is specified in: case H's planted voxels have a loss of exactly 0 in any fp32 evaluation (1 + 19 e^-26 rounds
to 1) and of 1e-12 .. 1e-17 in float64, where they are no ties at all.  So the restatement takes its selection from the per-voxel
losses as the reference evaluates them (fp32 ``cross_entropy``) and evaluates everything else in float64.  For A, B, C and G this
is the pure float64 selection, by the gap condition below (asserted: same index sets); for D (all-zero logits: every loss is
w_t * log 20 in either precision) as well; for H it pins the tie group.

Stored per case X: ``X_f64_loss``; ``X_M`` / ``X_k`` (labelled and kept voxels per sample); for A B C D G H ``X_f64_grad`` (the
float64 logit gradient, stored as fp32) and ``X_spread`` / ``X_loss_spread``; for A B C G ``X_ref_loss`` (reference, fp32) and
``X_ref_delta`` (fp16) with the reference's fp32 gradient = ``ref_grad(npz, X)`` = f64_grad + ref_delta * max|f64_grad| /
DELTA_SCALE (the packing of tests/golden/lovasz.npz); ``D_ref_loss``; ``X_gap`` (float64, per sample: k-th minus (k+1)-th largest
float64 loss) and ``X_l_err`` (largest |fp32 - float64| per-voxel loss).

Spreads.  ``X_spread`` = max |fp32 gradient - float64 gradient| / max |float64 gradient| and ``X_loss_spread`` = |fp32 loss -
float64 loss| / max(1, |float64 loss|), the fp32 side being the REFERENCE for A B C G (and for D's loss: Wsum and the loss do
not depend on which tied voxels are kept).  For D's gradient and for H, where ``torch.topk``'s choice among ties makes the
reference's record no yardstick, the fp32 side is the restatement itself evaluated in fp32 on the same selection.

Gap condition.  For A B C G the fixture is refused unless every sample's gap is at least 64 x ``X_l_err``: then the fp32 and
float64 selections are the same set and no voxel needs excluding from a comparison; a kernel whose per-voxel loss error stays
below gap / 8 selects the same set too.  Otherwise bump the case's entry of ``synthetic.OHEM_SEED``."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import synthetic as S  # noqa: E402
from stereoscene_amd.plugin.losses import semkitti_class_weights  # noqa: E402

GAP_FACTOR = 64.0
DELTA_SCALE = 16384.0
GAP_CHECKED = ("A", "B", "C", "G")
WITH_GRAD = ("A", "B", "C", "D", "G", "H")


def ref_grad(npz, name):
    """The reference's fp32 logit gradient of case ``name`` from the stored float64 gradient and the fp16 difference."""
    g = npz[f"{name}_f64_grad"].astype(np.float64)
    return (g + npz[f"{name}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def load_reference(ref_root):
    path = os.path.join(ref_root, "projects", "mmdet3d_plugin", "utils", "semkitti.py")
    spec = importlib.util.spec_from_file_location("ref_semkitti", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def upsampled(x, lab):
    if tuple(x.shape[-3:]) == tuple(lab.shape[-3:]):
        return x
    return TF.interpolate(x, size=tuple(lab.shape[-3:]), mode="trilinear", align_corners=False)


def voxel_losses(x, lab, cw):
    """[B, N] class-weighted cross entropy in x's dtype, +0.0 for a saturated voxel, 0 where ignored."""
    l = TF.cross_entropy(upsampled(x, lab), lab.long(), weight=cw.to(x.dtype), ignore_index=255, reduction="none")
    return l.flatten(1) + 0.0


def selection(l, lab, top_k):
    """Per sample: indices (into the sample's labelled voxels) of the int(M * top_k) largest losses, ties to the lowest index."""
    keep = []
    for b in range(l.shape[0]):
        li = l[b, lab[b].flatten() != 255].detach()
        keep.append(torch.argsort(li, descending=True, stable=True)[:int(li.shape[0] * top_k)])
    return keep


def ohem_restated(x, lab, cw, keep):
    """sum(kept losses) / clamp_min(sum of the kept class weights, 1e-4) in x's dtype on a given selection."""
    l = voxel_losses(x, lab, cw)
    cw = cw.to(x.dtype)
    top, norm = x.sum() * 0.0, cw.sum() * 0.0
    for b in range(l.shape[0]):
        valid = lab[b].flatten() != 255
        top = top + l[b, valid][keep[b]].sum()
        norm = norm + cw[lab[b].flatten()[valid].long()][keep[b]].sum()
    return top / torch.clamp_min(norm, 1e-4)


def gaps(l64, lab, top_k):
    out = []
    for b in range(l64.shape[0]):
        li = torch.sort(l64[b, lab[b].flatten() != 255].detach(), descending=True).values
        k = int(li.shape[0] * top_k)
        out.append(float(li[k - 1] - li[k]) if 0 < k < li.shape[0] else float("inf"))
    return np.array(out, dtype=np.float64)


def main():
    torch.set_num_threads(1)
    if "--ref" in sys.argv:
        ref_root = sys.argv[sys.argv.index("--ref") + 1]
    else:
        from oracle import make_golden as MG
        ref_root = MG.REF
    ref = load_reference(ref_root)
    cw = semkitti_class_weights()
    out, ref_grads = {}, {}
    for name in S.OHEM_CASES:
        x, lab, top_k = S.ohem_case(name)
        labelled = lab.flatten(1) != 255
        l32 = voxel_losses(x, lab, cw)
        l64 = voxel_losses(x.double(), lab, cw)
        keep = selection(l32, lab, top_k)
        out[f"{name}_M"] = labelled.sum(1).numpy().astype(np.int64)
        out[f"{name}_k"] = np.array([len(k) for k in keep], dtype=np.int64)
        x64 = x.double().requires_grad_(True)
        loss64 = ohem_restated(x64, lab, cw, keep)
        loss64.backward()
        g64 = x64.grad
        out[f"{name}_f64_loss"] = np.float64(loss64.item())
        line = f"case {name}: M {out[f'{name}_M'].tolist()} k {out[f'{name}_k'].tolist()} f64 loss {loss64.item():.9f}"
        if labelled.any():
            out[f"{name}_gap"] = gaps(l64, lab, top_k)
            out[f"{name}_l_err"] = np.float64((l32.double() - l64)[labelled].abs().max().item())
            line += f" gap {out[f'{name}_gap'].tolist()} l_err {out[f'{name}_l_err']:.2e}"
        if name in GAP_CHECKED:
            keep64 = selection(l64, lab, top_k)
            assert all(set(a.tolist()) == set(b.tolist()) for a, b in zip(keep, keep64)), (name, "fp32 / float64 selections differ")
            assert (out[f"{name}_gap"] >= GAP_FACTOR * out[f"{name}_l_err"]).all(), (name, out[f"{name}_gap"], out[f"{name}_l_err"],
                                                                                 "bump synthetic.OHEM_SEED")
        if name == "A":
            assert out["A_M"][0] != out["A_M"][1] and out["A_k"][0] != out["A_k"][1], "bump synthetic.OHEM_SEED['A']"
        if name in WITH_GRAD:
            x32 = x.clone().requires_grad_(True)
            if name in GAP_CHECKED or name == "D":
                loss32 = ref.OHEM_CE_ssc_loss(upsampled(x32, lab), lab.long(), cw, top_k=top_k)
                out[f"{name}_ref_loss"] = np.float32(loss32.item())
            if name not in GAP_CHECKED:
                loss32 = ohem_restated(x32, lab, cw, keep)
            loss32.backward()
            g = g64.numpy().astype(np.float32)
            spread = ((x32.grad.double() - g64).abs().max() / g64.abs().max()).item()
            lspread = abs(loss32.item() - loss64.item()) / max(1.0, abs(loss64.item()))
            out[f"{name}_f64_grad"] = g
            out[f"{name}_spread"] = np.float64(spread)
            out[f"{name}_loss_spread"] = np.float64(lspread)
            if name in GAP_CHECKED:
                ref_grads[name] = x32.grad.numpy().copy()
                out[f"{name}_ref_delta"] = ((ref_grads[name].astype(np.float64) - g) * (DELTA_SCALE / np.abs(g).max())).astype(np.float16)
            line += f" | fp32 loss {loss32.item():.9f} grad spread {spread:.2e} loss spread {lspread:.2e} max|grad| {np.abs(g).max():.3e}"
        print(line)
    path = os.path.join(ROOT, "tests", "golden", "ohem.npz")
    np.savez_compressed(path, **out)
    back = np.load(path)
    for name, g32 in ref_grads.items():
        err = np.abs(ref_grad(back, name) - g32).max() / np.abs(back[f"{name}_f64_grad"]).max()
        assert err < 2e-7, (name, err)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
