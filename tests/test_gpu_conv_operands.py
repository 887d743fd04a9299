"""GPU: the operand handling of the fp32 direct leaf (functional._ConvNd), end to end and exact.

tests/test_conv_operands_snapshot.py pins which problems the leaf hands to the library; this runs one or two cases per branch
through F.conv3d / F.conv_transpose3d, forward and backward, and compares y, gx, gw and gb with torch.equal against ATen in float64
on the CPU.  x, the weight, the bias and gy are integers in -2 .. 2, so every product and every partial sum in any order is an
integer far below 2^24 (asserted, on the sums of absolute values, with a factor 16 for the fractional bits the in-kernel F(2,3)
stages add): a channel padded on the wrong axis, a result cropped to the wrong width or a gradient slot taken on a cropped gradient
changes integers, not rounding.  A wrong pad or crop is exactly what the thin, padded and plain channel pairs below tell apart.

Every channel pair and geometry is one an existing GPU test already runs through these kernels (what the library sees after the
padding, in brackets): 1 / 2 / 4 <-> 32 and 32 -> 32 at k3 on 4 x 5 x 6 (test_gpu_kernels.py: CONV_CASES, the thin-side cases),
32 -> 32 at k1 next to k3 on a `fork` (the pointwise-32 test), 3 -> 5 at k3 [4 -> 8: wgrad_cases dir_total_odd / dir_stage] and the
k2 s2 transposed 30 -> 14 up to 4 x 6 x 8 [32 -> 16: wgrad_cases dir_k2s2t].  Two branches of the snapshot have no case here: the TN
product needs 32768 rows (CONV_CASES runs it at 32 x 48 x 160) and the `tpad` copy needs tile hint 7 on a thin pair, which no GPU
test runs."""
from collections import namedtuple

import pytest
import torch
import torch.nn.functional as TF

from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
LIM = 2

# want: which of x / weight (with the bias) require a gradient
Case = namedtuple("Case", "id cin cout tr k s p op relu grid want")
G = (4, 5, 6)
CASES = [
    Case("thin_in_2to32", 2, 32, 0, 3, 1, 1, 0, 0, G, "xw"),          # class 4 forward unpadded, class 5 data gradient, thin weight gradient
    Case("thin_in_1to32", 1, 32, 0, 3, 1, 1, 0, 0, G, "xw"),
    Case("thin_4to32", 4, 32, 0, 3, 1, 1, 0, 0, G, "xw"),             # the same classes with nothing to pad
    Case("thin_out_32to1", 32, 1, 0, 3, 1, 1, 0, 0, G, "xw"),         # class 5 forward, class 4 data gradient on the unpadded gy: no padded copy
    Case("thin_out_32to2_relu", 32, 2, 0, 3, 1, 1, 0, 1, G, "xw"),    # fused ReLU, Cout % 4 != 0: the mask on the unpadded gradient
    Case("thin_out_32to4", 32, 4, 0, 3, 1, 1, 0, 0, G, "xw"),
    Case("thin_out_32to1_x_only", 32, 1, 0, 3, 1, 1, 0, 0, G, "x"),
    Case("thin_out_32to1_w_only", 32, 1, 0, 3, 1, 1, 0, 0, G, "w"),
    Case("kpad_cpad_3to5", 3, 5, 0, 3, 1, 1, 0, 0, G, "xw"),          # x, gy and both weight axes padded; gx and gw cropped
    Case("kpad_cpad_3to5_relu", 3, 5, 0, 3, 1, 1, 0, 1, G, "xw"),
    Case("kpad_cpad_3to5_w_only", 3, 5, 0, 3, 1, 1, 0, 0, G, "w"),
    Case("kpad_cpad_transposed_30to14", 30, 14, 1, 2, 2, 0, 0, 0, (2, 3, 4), "xw"),      # both weight axes of a transposed layer; y on 4 x 6 x 8
]
BY_ID = {c.id: c for c in CASES}


def ints(key, shape):
    return torch.round(S.hash_uniform(f"ops/{key}", shape, -LIM - 0.4999, LIM + 0.4999))


def conv(fn3, fnt, c, x, w, b):
    return fnt(x, w, b, c.s, c.p, c.op) if c.tr else fn3(x, w, b, c.s, c.p)


def reference(c, x, w, b, gy, relu):
    """float64 (y, gx, gw, gb) of ATen on the CPU."""
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = conv(TF.conv3d, TF.conv_transpose3d, c, xd, wd, bd)
    y = torch.relu(y) if relu else y
    y.backward(gy.double())
    return y.detach(), xd.grad, wd.grad, bd.grad


@pytest.fixture(scope="module")
def problems():
    """Inputs and float64 references of every case, computed once."""
    out = {}
    for c in CASES:
        x = ints(f"{c.id}/x", (1, c.cin) + c.grid)
        w = ints(f"{c.id}/w", ((c.cin, c.cout) if c.tr else (c.cout, c.cin)) + (c.k,) * 3)
        b = ints(f"{c.id}/b", (c.cout,))
        yshape = conv(TF.conv3d, TF.conv_transpose3d, c, x, w, b).shape
        gy = ints(f"{c.id}/gy", tuple(yshape))
        ref = reference(c, x, w, b, gy, c.relu)
        bound = reference(c, x.abs(), w.abs(), b.abs(), gy.abs(), False)
        out[c.id] = (x, w, b, gy, ref, bound)
    return out


@pytest.mark.parametrize("cid", [c.id for c in CASES])
def test_forward_and_backward_are_exact(cid, problems):
    c = BY_ID[cid]
    x, w, b, gy, ref, bound = problems[cid]
    for name, r, a in zip(("y", "gx", "gw", "gb"), ref, bound):
        print(f"{cid} {name}: max |reference| {r.abs().max().item():.0f}, sum of absolute values {a.abs().max().item():.0f}")
        assert r.abs().max().item() * 16 < 2 ** 24 and a.abs().max().item() * 16 < 2 ** 24
    xg = x.to(DEV).requires_grad_("x" in c.want)
    wg, bg = (t.to(DEV).requires_grad_("w" in c.want) for t in (w, b))
    y = conv(F.conv3d, F.conv_transpose3d, c, xg, wg, bg) if not c.relu else F.conv3d(xg, wg, bg, c.s, c.p, relu=True)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    assert torch.equal(y.detach().cpu().double(), ref[0]), f"{cid}: y"
    for name, t, r in (("gx", xg, ref[1]), ("gw", wg, ref[2]), ("gb", bg, ref[3])):
        if t.requires_grad:
            assert t.grad.shape == r.shape and torch.equal(t.grad.cpu().double(), r), f"{cid}: {name}"
        else:
            assert t.grad is None


@pytest.mark.parametrize("pair", ["slot_taken", "slot_refused_class4", "slot_refused_kpad"])
def test_fork_into_two_convs_sums_the_data_gradients(pair):
    """x feeds two convolutions through fork(x, 2): gx is the sum of the two data gradients, whether the second one accumulates
    into the first one's buffer (32 -> 32 at k3 and k1: the slot path) or the leaf has to refuse the slot (32 -> 4: class 4
    writes gx without an accumulating epilogue; 3 -> 5: gx is cropped after the launch) and autograd adds two tensors."""
    cin, (ca, ka), (cb, kb) = {"slot_taken": (32, (32, 3), (32, 1)), "slot_refused_class4": (32, (4, 3), (32, 1)),
                               "slot_refused_kpad": (3, (5, 3), (5, 3))}[pair]
    x = ints(f"{pair}/x", (1, cin) + G)
    wa, wb = ints(f"{pair}/wa", (ca, cin) + (ka,) * 3), ints(f"{pair}/wb", (cb, cin) + (kb,) * 3)
    ga, gb = ints(f"{pair}/ga", (1, ca) + G), ints(f"{pair}/gb", (1, cb) + G)
    xr = x.double().requires_grad_(True)
    torch.autograd.backward([TF.conv3d(xr, wa.double(), None, 1, ka // 2), TF.conv3d(xr, wb.double(), None, 1, kb // 2)],
                            [ga.double(), gb.double()])
    xa = x.abs().double().requires_grad_(True)
    torch.autograd.backward([TF.conv3d(xa, wa.abs().double(), None, 1, ka // 2), TF.conv3d(xa, wb.abs().double(), None, 1, kb // 2)],
                            [ga.abs().double(), gb.abs().double()])
    print(f"{pair}: max |reference| {xr.grad.abs().max().item():.0f}, sum of absolute values {xa.grad.max().item():.0f}")
    assert xr.grad.abs().max().item() * 16 < 2 ** 24 and xa.grad.max().item() * 16 < 2 ** 24
    xg = x.to(DEV).requires_grad_(True)
    a, b = F.fork(xg, 2)
    torch.autograd.backward([F.conv3d(a, wa.to(DEV), None, 1, ka // 2), F.conv3d(b, wb.to(DEV), None, 1, kb // 2)],
                            [ga.to(DEV), gb.to(DEV)])
    torch.cuda.synchronize()
    assert torch.equal(xg.grad.cpu().double(), xr.grad), pair
