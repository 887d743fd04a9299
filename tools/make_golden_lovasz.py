"""Generate tests/golden/lovasz.npz: the reference's own ``lovasz_softmax`` (occupancy/dense_heads/lovasz_softmax.py:21-33,
156-225) in fp32 on the cases of ``stereoscene_amd.synthetic.LOVASZ_CASES``, called as the head calls it
(``lovasz_softmax(torch.softmax(up, 1), target, ignore=255)``, ``up`` = trilinear, align_corners=False), next to a float64
restatement of the same formulas.  Build container only (needs the reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_lovasz.py [--ref /path/to/reference]

The reference module is loaded BY FILE PATH (it imports only torch and numpy; the package __init__ drags in mmcv).  Its
``lovasz_grad`` calls ``.float()``, so it cannot run in float64 itself: the float64 yardstick is ``lovasz_f64`` below.  The
inputs are not stored: the tests rebuild them from ``synthetic.lovasz_case(name)`` (hash-generated, exactly reproducible).
Stored per case X: ``X_f64_loss`` (float64) and, for A B C F G, ``X_f64_grad`` (the float64 logit gradient, stored as fp32),
``X_ref_loss`` (reference, fp32), ``X_ref_delta`` (fp16) with the reference's fp32 gradient = ``ref_grad(npz, X)`` =
f64_grad + ref_delta * max|f64_grad| / DELTA_SCALE (the two gradients differ by rounding noise only, so the difference fits
16 bits with an error below 1e-7 of the largest entry; both in full would double the file), ``X_spread`` =
max |ref_grad - f64_grad| / max |f64_grad| and ``X_loss_spread``.  A fixture
whose spread is above 2.5e-5 is refused: bump its entry of ``synthetic.LOVASZ_SEED`` (nearly equal errors sort differently in
fp32 and float64, and a swapped fg / non-fg pair moves two gradient entries)."""
import importlib.util
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import synthetic as S  # noqa: E402

MAX_SPREAD = 2.5e-5
DELTA_SCALE = 16384.0          # |delta| <= MAX_SPREAD * DELTA_SCALE = 0.41: well inside fp16's normal range


def ref_grad(npz, name):
    """The reference's fp32 logit gradient of case ``name`` from the stored float64 gradient and the fp16 difference."""
    g = npz[f"{name}_f64_grad"].astype(np.float64)
    return (g + npz[f"{name}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def load_reference(ref_root):
    path = os.path.join(ref_root, "projects", "mmdet3d_plugin", "occupancy", "dense_heads", "lovasz_softmax.py")
    spec = importlib.util.spec_from_file_location("ref_lovasz_softmax", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def upsampled(x, lab):
    if tuple(x.shape[-3:]) == tuple(lab.shape[-3:]):
        return x
    return TF.interpolate(x, size=tuple(lab.shape[-3:]), mode="trilinear", align_corners=False)


def lovasz_f64(x, lab, ignore=255):
    """The loss in float64, written from its definition: for every class c with a labelled voxel, e_v = |[t_v == c] - p_v[c]|
    sorted descending, I_i = G - #fg among the first i+1, U_i = G + #non-fg among the first i+1, J_i = 1 - I_i / U_i,
    loss_c = sum_i e_(i) (J_i - J_{i-1}) with J_{-1} = 0; mean over those classes, 0 when no voxel is labelled."""
    p = torch.softmax(upsampled(x, lab), dim=1).permute(0, 2, 3, 4, 1)
    keep = lab != ignore
    p, t = p[keep], lab[keep].long()
    total, n_present = x.sum() * 0.0, 0
    for c in range(x.shape[1]):
        fg = (t == c).double()
        if fg.sum() == 0:
            continue
        e = (fg - p[:, c]).abs()
        order = torch.argsort(e.detach(), descending=True, stable=True)
        f = fg[order]
        G = f.sum()
        J = 1.0 - (G - torch.cumsum(f, 0)) / (G + torch.cumsum(1.0 - f, 0))
        dJ = J - torch.cat((torch.zeros(1, dtype=J.dtype), J[:-1]))
        total = total + (e[order] * dJ).sum()
        n_present += 1
    return total / max(n_present, 1)


def main():
    torch.set_num_threads(1)
    if "--ref" in sys.argv:
        ref_root = sys.argv[sys.argv.index("--ref") + 1]
    else:
        from oracle import make_golden as MG
        ref_root = MG.REF
    ref = load_reference(ref_root)
    out = {}
    for name in S.LOVASZ_CASES:
        x, lab = S.lovasz_case(name)
        x64 = x.double().requires_grad_(True)
        l64 = lovasz_f64(x64, lab)
        l64.backward()
        g64 = x64.grad
        out[f"{name}_f64_loss"] = np.float64(l64.item())
        line = f"case {name}: f64 loss {l64.item():.9f} max|grad| {g64.abs().max().item():.3e}"
        if name in ("A", "B", "C", "F", "G"):
            x32 = x.clone().requires_grad_(True)
            l32 = ref.lovasz_softmax(torch.softmax(upsampled(x32, lab), 1), lab, ignore=255)
            l32.backward()
            spread = ((x32.grad.double() - g64).abs().max() / g64.abs().max()).item()
            lspread = abs(l32.item() - l64.item()) / max(1.0, abs(l64.item()))
            assert spread <= MAX_SPREAD, (name, spread, "bump synthetic.LOVASZ_SEED")
            out[f"{name}_ref_loss"] = np.float32(l32.item())
            g = g64.numpy().astype(np.float32)
            out[f"{name}_f64_grad"] = g
            out[f"{name}_ref_delta"] = ((x32.grad.numpy().astype(np.float64) - g) * (DELTA_SCALE / np.abs(g).max())).astype(np.float16)
            out[f"{name}_spread"] = np.float64(spread)
            out[f"{name}_loss_spread"] = np.float64(lspread)
            line += f" | ref fp32 loss {l32.item():.9f} grad spread {spread:.2e} loss spread {lspread:.2e}"
        print(line)
    path = os.path.join(ROOT, "tests", "golden", "lovasz.npz")
    np.savez_compressed(path, **out)
    back = np.load(path)
    for name in ("A", "B", "C", "F", "G"):
        x, lab = S.lovasz_case(name)
        x32 = x.clone().requires_grad_(True)
        ref.lovasz_softmax(torch.softmax(upsampled(x32, lab), 1), lab, ignore=255).backward()
        err = np.abs(ref_grad(back, name) - x32.grad.numpy()).max() / np.abs(back[f"{name}_f64_grad"]).max()
        assert err < 2e-7, (name, err)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
