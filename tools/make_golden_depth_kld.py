"""Generate tests/golden/depth_kld.npz: the reference's Gaussian KL depth loss (``loss_depth_type='kld'``,
occupancy/image2bev/ViewTransformerLSSVoxel.py:390-416) in fp32 on the cases of ``stereoscene_amd.synthetic.DEPTH_KLD_CASES``,
next to a float64 restatement of the same formulas in both unit modes.  Build container only (needs the reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_depth_kld.py [--ref /path/to/reference]

The reference's ``utils/gaussian.py`` is loaded BY FILE PATH (it imports only numpy and torch; the package __init__ drags in
mmcv) and ``generate_guassian_depth_target(gt_depths, ds, dbound, constant_std=0.5)`` is called as ``get_klv_depth_loss`` calls
it, followed by that method's foreground mask and ``kl_div(log(p + 1e-4), target, reduction='batchmean')``, all in fp32; the
gradient is autograd's.  The float64 yardstick is ``kld_f64`` below, written from the formulas:

    m   = min of the block's non-zero depths, 0 without one;  foreground: float32(d0) <= m <= float32(d1 - dd)
    x_i = (d0 - dd / 2) + i dd, i = 0..D;   mu = m / dd;   s = std / dd;   Phi(z) = (1 + erf(z / sqrt 2)) / 2
    t_d = Phi((e x_{d+1} - mu) / s) - Phi((e x_d - mu) / s),   e = 1 ("reference": edges in metres) or 1 / dd ("bins")
    loss = sum over foreground rows and bins of (t log t - t log(p + 1e-4)) / number of foreground rows  (0 without one)

The inputs are not stored: the tests rebuild them from ``synthetic.depth_kld_case(name)`` (hash-generated, exactly
reproducible).  Stored per case X: ``X_f64_loss``, ``X_f64_grad`` (float64), ``X_n_fg``; for A, B, E (the reference has no bin-unit
mode and returns NaN without a foreground row) ``X_ref_loss``, ``X_ref_grad`` (fp32); ``X_loss_spread`` = |fp32 - float64| /
max(1, |float64|) and ``X_spread`` = max |fp32 grad - float64 grad| / max |float64 grad|, fp32 = the reference for A, B, E and
the restatement evaluated in fp32 for D.  The loss is the unweighted one (``loss_depth_weight`` = 1)."""
import importlib.util
import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import synthetic as S  # noqa: E402

STD = 0.5          # ViewTransformerLSSVoxel.py:298, the only value the reference can run with
REFERENCE_CASES = ("A", "B", "E")


def load_reference(ref_root):
    path = os.path.join(ref_root, "projects", "mmdet3d_plugin", "utils", "gaussian.py")
    spec = importlib.util.spec_from_file_location("ref_gaussian", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def reference_loss(ref, gt, pred, ds, dbound):
    """get_klv_depth_loss (VT:390-403) around the reference's own target generator, fp32."""
    D = pred.shape[1]
    target, depth_values = ref.generate_guassian_depth_target(gt, ds, list(dbound), constant_std=STD)
    depth_values = depth_values.view(-1)
    fg = (depth_values >= dbound[0]) & (depth_values <= (dbound[1] - dbound[2]))
    target = target.view(-1, D)[fg]
    p = pred.permute(0, 2, 3, 1).contiguous().view(-1, D)[fg]
    return TF.kl_div(torch.log(p + 1e-4), target, reduction="batchmean", log_target=False), fg, target


def block_min(gt, ds):
    B, N, H, W = gt.shape
    g = gt.reshape(B * N, H // ds, ds, W // ds, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds)
    big = torch.full_like(g, float("inf"))
    m = torch.where(g != 0, g, big).min(dim=-1).values
    return torch.where(torch.isinf(m), torch.zeros_like(m), m)


def kld_restated(gt, pred, ds, dbound, units, dtype=torch.float64):
    """(loss, foreground mask, targets) from the formulas of the module docstring in ``dtype``."""
    d0, d1, dd = dbound
    D = pred.shape[1]
    m32 = block_min(gt, ds)
    fg = (m32 >= np.float32(d0)) & (m32 <= np.float32(d1 - dd))           # the reference compares fp32 values
    x = torch.tensor([(d0 - dd / 2) + i * dd for i in range(D + 1)], dtype=dtype)
    assert x[-1] < d1 <= x[-1] + dd, "arange(d0 - dd / 2, d1, dd) must have D + 1 entries"
    e = 1.0 if units == "reference" else 1.0 / dd
    z = (x * e - (m32.to(dtype) / dd).unsqueeze(1)) / (STD / dd)
    cdf = 0.5 * (1 + torch.erf(z / math.sqrt(2)))
    t = (cdf[:, 1:] - cdf[:, :-1])[fg]
    p = pred.to(dtype).permute(0, 2, 3, 1).reshape(-1, D)[fg]
    n = int(fg.sum())
    loss = (torch.xlogy(t, t) - t * torch.log(p + 1e-4)).sum() / max(n, 1)
    return loss, fg, t


def with_grad(fn, pred, dtype):
    p = pred.to(dtype).requires_grad_(True)
    loss, fg, t = fn(p)
    loss.backward()
    return loss.detach(), p.grad, fg, t.detach()


def check_case_a(gt, fg, t, ds):
    """The planted pixels of case A land on the sides the case table states."""
    fW = gt.shape[3] // ds
    rows = {col: col for col in S.DEPTH_KLD_PLANTS}                       # camera 0, feature row 0: pixel index = column
    m = block_min(gt, ds)
    want_m = {0: 2.0, 1: 57.5, 2: float(np.nextafter(np.float32(57.5), np.float32(100.0))), 3: 1.9, 4: 33.6}
    want_fg = {0: True, 1: True, 2: False, 3: False, 4: True}
    for col, r in rows.items():
        assert r < fW and float(m[r]) == float(np.float32(want_m[col])), (col, float(m[r]))
        assert bool(fg[r]) == want_fg[col], (col, bool(fg[r]))
    t_full = torch.zeros(fg.numel(), t.shape[1], dtype=t.dtype)
    t_full[fg] = t
    assert int(t_full[0].argmax()) == 4                                    # m = 2.0 peaks at the bin that holds 4 m
    assert float(t_full[4].abs().max()) == 0.0 and float(t_full[1].abs().max()) == 0.0    # all-zero rows, still counted
    counts = (gt.reshape(2, 3, ds, 5, ds) != 0).sum(dim=(2, 4)).reshape(-1)
    assert (counts == 0).any() and (counts == 1).any() and (counts > 2).any(), counts


def main():
    torch.set_num_threads(1)
    if "--ref" in sys.argv:
        ref_root = sys.argv[sys.argv.index("--ref") + 1]
    else:
        from oracle import make_golden as MG
        ref_root = MG.REF
    ref = load_reference(ref_root)
    out = {}
    for name in S.DEPTH_KLD_CASES:
        gt, pred, ds, dbound, units = S.depth_kld_case(name)
        l64, g64, fg, t64 = with_grad(lambda p: kld_restated(gt, p, ds, dbound, units), pred, torch.float64)
        n_fg = int(fg.sum())
        out[f"{name}_f64_loss"] = np.float64(l64.item())
        out[f"{name}_f64_grad"] = g64.numpy()
        out[f"{name}_n_fg"] = np.int64(n_fg)
        line = f"case {name}: {n_fg} / {fg.numel()} foreground rows, f64 loss {l64.item():.9f} max|grad| {g64.abs().max().item():.3e}"
        if name == "C":
            assert n_fg == 0 and l64.item() == 0.0 and not g64.any()
            print(line)
            continue
        assert 0 < n_fg < fg.numel(), (name, n_fg)
        assert float(t64.max()) > 0.1, name                                # some row carries a real target
        if name == "A":
            check_case_a(gt, fg, t64, ds)
        if name in REFERENCE_CASES:
            l32, g32, fg32, _ = with_grad(lambda p: reference_loss(ref, gt, p, ds, dbound), pred, torch.float32)
            assert torch.equal(fg32, fg), name
            assert torch.isfinite(l32) and torch.isfinite(g32).all(), name
            out[f"{name}_ref_loss"] = np.float32(l32.item())
            out[f"{name}_ref_grad"] = g32.numpy()
        else:
            l32, g32, _, _ = with_grad(lambda p: kld_restated(gt, p, ds, dbound, units, torch.float32), pred, torch.float32)
        spread = ((g32.double() - g64).abs().max() / g64.abs().max()).item()
        lspread = abs(l32.item() - l64.item()) / max(1.0, abs(l64.item()))
        out[f"{name}_spread"] = np.float64(spread)
        out[f"{name}_loss_spread"] = np.float64(lspread)
        print(line + f" | fp32 loss {l32.item():.9f} grad spread {spread:.2e} loss spread {lspread:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "depth_kld.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")


if __name__ == "__main__":
    main()
