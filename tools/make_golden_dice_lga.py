"""Generate tests/golden/dice_lga.npz: the reference's own ``SoftDiceLossWithProb`` (utils/dice_loss.py:36-66) and
``PositionAwareLoss`` (utils/pal_loss.py) on the cases of ``stereoscene_amd.synthetic.DICE_LGA_CASES``, called as the head calls
them (occhead.py:331-343: ``dice(softmax(up, 1)[:, 1:].sum(1), target)`` and ``PAL(up, target, class_weights)``, ``up`` = trilinear,
align_corners=False), in fp32 and in float64.  Build container only (needs the reference checkout).

Run:  PYTHONDONTWRITEBYTECODE=1 python tools/make_golden_dice_lga.py [--ref /path/to/reference]

The two reference modules are loaded BY FILE PATH.  ``pal_loss.py`` imports ``mmcv`` without using it: an empty stand-in module
is put into ``sys.modules`` first.  The inputs are not stored: the tests rebuild them from ``synthetic.dice_lga_case(name)``
(hash-generated, exactly reproducible).

The float64 side is the reference's classes on float64 inputs (their formulas do not depend on the dtype).  Case E (nothing
labelled): the reference's PAL divides 0 / 0; the recorded float64 loss is this project's definition, 0 with a zero gradient.

Stored per case X and loss T in (dice, lga): ``X_lga2`` (uint8: the reference's ``get_lga`` x 2, an exact integer), ``X_T_f64_loss``,
``X_T_ref_loss`` (the reference in fp32; not for E's lga), and, except for E, ``X_T_f64_grad`` (the float64 logit gradient, stored
as fp32) with ``X_T_spread`` = max |fp32 gradient - float64 gradient| / max |float64 gradient| and ``X_T_loss_spread`` = |fp32 loss
- float64 loss| / max(1, |float64 loss|), the fp32 side being the REFERENCE.  For A also ``X_T_ref_delta`` (fp16): the
reference's fp32 gradient = ``ref_grad(npz, X, T)`` = f64_grad + ref_delta * max|f64_grad| / DELTA_SCALE (the packing of
tests/golden/ohem.npz).  B, C and K would take the file past the 1 MB limit of a committed fixture (1.24 MB with all three, 1.001 MB
with K alone): their reference fp32 gradients enter through the recorded spreads only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch
import torch.nn.functional as TF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from stereoscene_amd import synthetic as S  # noqa: E402
from stereoscene_amd.plugin import losses as L  # noqa: E402

DELTA_SCALE = 16384.0
WITH_DELTA = ("A",)


def ref_grad(npz, name, loss):
    """The reference's fp32 logit gradient of case ``name`` from the stored float64 gradient and the fp16 difference."""
    g = npz[f"{name}_{loss}_f64_grad"].astype(np.float64)
    return (g + npz[f"{name}_{loss}_ref_delta"].astype(np.float64) * (np.abs(g).max() / DELTA_SCALE)).astype(np.float32)


def load_reference(ref_root):
    sys.modules.setdefault("mmcv", types.ModuleType("mmcv"))
    mods = []
    for name in ("dice_loss", "pal_loss"):
        path = os.path.join(ref_root, "projects", "mmdet3d_plugin", "utils", name + ".py")
        spec = importlib.util.spec_from_file_location("ref_" + name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    return mods


def upsampled(x, lab):
    if tuple(x.shape[-3:]) == tuple(lab.shape[-3:]):
        return x
    return TF.interpolate(x, size=tuple(lab.shape[-3:]), mode="trilinear", align_corners=False)


def main():
    torch.set_num_threads(1)
    if "--ref" in sys.argv:
        ref_root = sys.argv[sys.argv.index("--ref") + 1]
    else:
        from oracle import make_golden as MG
        ref_root = MG.REF
    ref_dice, ref_pal = load_reference(ref_root)
    dice, pal = ref_dice.SoftDiceLossWithProb(), ref_pal.PositionAwareLoss(num_class=20)
    cw = L.semkitti_class_weights()

    def run(kind, x, lab):
        up = upsampled(x, lab)
        if kind == "dice":
            return dice(torch.softmax(up, dim=1)[:, 1:].sum(dim=1), lab)
        return pal(up, lab, cw.to(x.dtype))

    out, ref_grads = {}, {}
    for name in S.DICE_LGA_CASES:
        x, lab = S.dice_lga_case(name)
        lga = pal.get_lga(lab.long()).double() * 2.0
        assert torch.equal(lga, lga.round()) and 0 <= float(lga.min()) and float(lga.max()) <= 12
        out[f"{name}_lga2"] = lga.numpy().astype(np.uint8)
        assert torch.equal(L.lga_weights_tensor(lab), torch.from_numpy(out[f"{name}_lga2"])), name
        for kind in ("dice", "lga"):
            key = f"{name}_{kind}"
            if name == "E" and kind == "lga":
                assert torch.isnan(run(kind, x, lab))
                out[f"{key}_f64_loss"] = np.float64(0.0)
                print(f"case {key}: the reference gives NaN; recorded 0")
                continue
            x64 = x.double().requires_grad_(True)
            loss64 = run(kind, x64, lab)
            loss64.backward()
            x32 = x.clone().requires_grad_(True)
            loss32 = run(kind, x32, lab)
            loss32.backward()
            assert loss64.dtype == torch.float64 and loss32.dtype == torch.float32
            # the tensor forms of plugin/losses.py restate the same formulas
            own = (L.dice_tensor(upsampled(x.double(), lab), lab) if kind == "dice"
                   else L.pal_tensor(upsampled(x.double(), lab), lab, cw.double()))
            assert abs(own.item() - loss64.item()) <= 1e-12 * max(1.0, abs(loss64.item())), (key, own.item(), loss64.item())
            out[f"{key}_f64_loss"] = np.float64(loss64.item())
            out[f"{key}_ref_loss"] = np.float32(loss32.item())
            line = f"case {key}: f64 loss {loss64.item():.9f} fp32 loss {loss32.item():.9f}"
            if name != "E":
                g64 = x64.grad
                g = g64.numpy().astype(np.float32)
                spread = ((x32.grad.double() - g64).abs().max() / g64.abs().max()).item()
                lspread = abs(loss32.item() - loss64.item()) / max(1.0, abs(loss64.item()))
                out[f"{key}_f64_grad"] = g
                out[f"{key}_spread"] = np.float64(spread)
                out[f"{key}_loss_spread"] = np.float64(lspread)
                if name in WITH_DELTA:
                    ref_grads[(name, kind)] = x32.grad.numpy().copy()
                    out[f"{key}_ref_delta"] = ((ref_grads[(name, kind)].astype(np.float64) - g)
                                               * (DELTA_SCALE / np.abs(g).max())).astype(np.float16)
                line += f" grad spread {spread:.2e} loss spread {lspread:.2e} max|grad| {np.abs(g).max():.3e}"
            else:
                assert float(x64.grad.abs().max()) == 0.0 and loss64.item() == 0.0
            print(line)
    path = os.path.join(ROOT, "tests", "golden", "dice_lga.npz")
    np.savez_compressed(path, **out)
    back = np.load(path)
    for (name, kind), g32 in ref_grads.items():
        err = np.abs(ref_grad(back, name, kind) - g32).max() / np.abs(back[f"{name}_{kind}_f64_grad"]).max()
        assert err < 2e-7, (name, kind, err)
    print("wrote", path, os.path.getsize(path) / 1e3, "kB")
    assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
