"""Case table and runner of test_gpu_conv_bits.py (and of tools/make_golden_conv_bits.py, which records its golden hashes).

One small launch per forward / data-gradient path of ssbev_conv_fwd / ssbev_conv_bwd_data and per weight-gradient kind of
ssbev_conv_bwd_weight, through the library's own entry points.  Shapes come from the existing tables: conv_walk_cases.py for
the ring walks (multi-block chunks) and the hinted shapes of test_gpu_kernels.py for the rest.  Inputs are hash-filled
(synthetic.hash_*), every kernel reduces in a fixed order and the weight gradients fold their partials in a fixed order, so
the output BYTES are a function of the launch parameters alone: a SHA-256 per output pins them."""
import collections
import ctypes as C
import hashlib

import torch

from stereoscene_amd import capi
from stereoscene_amd import synthetic as S

Case = collections.namedtuple("Case", "name B Cin Cout grid k stride pad dil transposed hint classes wgrad precision",
                              defaults=(0,))

# classes = kernel class of (forward, data gradient); None = that call is not made (class 5 runs through ssbev_conv_thin_*,
# a K role that is no multiple of 4 is refused).  wgrad = weight-gradient kind (the label of tests/golden/conv_dispatch.json).
# grid = input grid (D, H, W).
CASES = [
    Case("thinin_fwd", 2, 2, 32, (2, 3, 70), 3, 1, 1, 1, 0, 0, (4, None), "thinside"),
    Case("thinin_dgrad", 1, 32, 2, (3, 3, 31), 3, 1, 1, 1, 0, 0, (None, 4), "thinside"),
    Case("thin_fwd", 1, 24, 4, (4, 5, 45), 3, 1, 1, 1, 0, 9, (3, 1), "thin"),
    Case("thin_dgrad", 1, 4, 24, (4, 5, 45), 3, 1, 1, 1, 0, 9, (1, 3), "generic"),
    Case("tap2_down", 2, 32, 64, (18, 60, 40), 3, 2, 1, 1, 0, 5, (7, 8), "generic"),
    Case("tap2_up", 2, 64, 32, (9, 30, 20), 3, 2, 1, 1, 1, 5, (8, 7), "generic"),
    Case("pw32", 1, 32, 16, (16, 32, 64), 1, 1, 0, 1, 0, 0, (10, 10), "1x1"),
    Case("tapdh", 2, 32, 32, (10, 26, 33), 3, 1, 1, 1, 0, 9, (9, 9), "dh"),
    Case("taph", 2, 32, 32, (5, 26, 33), 3, 1, 1, 1, 0, 9, (2, 2), "generic"),
    Case("tap", 1, 32, 32, (9, 61, 32), 3, 1, 1, 1, 0, 6, (1, 1), "lds"),
    Case("igemm", 1, 64, 64, (16, 32, 32), 3, 2, 1, 1, 0, 0, (11, 11), "lds"),
    Case("gather_dilated", 1, 16, 48, (6, 8, 12), 3, 1, 2, 2, 0, 0, (0, 0), "cf"),
    Case("gather_k2s2t", 2, 32, 16, (3, 4, 6), 2, 2, 0, 1, 1, 0, (0, 0), "generic"),
    Case("wgrad_bf16", 2, 32, 32, (7, 41, 33), 3, 1, 1, 1, 0, 9, (None, None), "bf16", 2),
]


def dims(c, relu=0, accumulate=0):
    k, s, p, dl = c.k, c.stride, c.pad, c.dil
    if c.transposed:
        out = [(n - 1) * s - 2 * p + dl * (k - 1) + (1 if (k == 3 and s == 2) else 0) + 1 for n in c.grid]
    else:
        out = [(n + 2 * p - dl * (k - 1) - 1) // s + 1 for n in c.grid]
    return capi.ConvDims(c.B, c.Cin, c.Cout, *c.grid, *out, k, k, k, s, s, s, p, p, p, dl, dl, dl, c.transposed, relu,
                         accumulate, c.hint, c.precision)


def queries(c):
    """(class of mode 0, class of mode 1) as the table states them: host only."""
    lib = capi.load()
    d = dims(c)
    got = tuple(lib.ssbev_conv_kernel_class(C.byref(d), m) for m in (0, 1))
    return tuple(g if w is not None else None for g, w in zip(got, c.classes)), got


def _sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _packed(lib, w, d, mode):
    wp = torch.empty(lib.ssbev_conv_packed_weight_elems(C.byref(d)), dtype=torch.float32, device=w.device)
    capi.check(lib.ssbev_conv_pack_weight(capi.ptr(w), capi.ptr(wp), C.byref(d), mode, capi.stream()), "ssbev_conv_pack_weight")
    return wp


def run(c, dev="cuda"):
    """name of output -> SHA-256 of its bytes: y (bias + fused ReLU), gx, gx_acc (accumulating epilogue, where the same kernel
    takes the call), gw."""
    lib = capi.load()
    d = dims(c)
    tag = "bits/" + c.name
    x = S.hash_normal(tag + "/x", (c.B, *c.grid, c.Cin)).to(dev)                      # channels-last buffers
    go = S.hash_normal(tag + "/go", (c.B, d.Do, d.Ho, d.Wo, c.Cout)).to(dev)
    wshape = ((c.Cin, c.Cout) if c.transposed else (c.Cout, c.Cin)) + (c.k,) * 3
    w = (S.hash_uniform(tag + "/w", wshape, -1, 1) * (3.0 / (c.Cin * c.k ** 3)) ** 0.5).to(dev)
    b = S.hash_uniform(tag + "/b", (c.Cout,), -0.5, 0.5).to(dev)
    out = {}
    if c.classes[0] is not None:
        dr = dims(c, relu=1)
        y = torch.empty_like(go)
        capi.check(lib.ssbev_conv_fwd(capi.ptr(x), capi.ptr(_packed(lib, w, dr, 0)), capi.ptr(b), capi.ptr(y), C.byref(dr),
                                      capi.stream()), "ssbev_conv_fwd")
        out["y"] = _sha(y)
    if c.classes[1] is not None:
        gx = torch.empty_like(x)
        capi.check(lib.ssbev_conv_bwd_data(capi.ptr(go), capi.ptr(_packed(lib, w, d, 1)), capi.ptr(gx), C.byref(d), capi.stream()),
                   "ssbev_conv_bwd_data")
        out["gx"] = _sha(gx)
        da = dims(c, accumulate=1)
        if lib.ssbev_conv_kernel_class(C.byref(da), 1) == c.classes[1]:
            acc = S.hash_normal(tag + "/old", tuple(x.shape)).to(dev)
            capi.check(lib.ssbev_conv_bwd_data(capi.ptr(go), capi.ptr(_packed(lib, w, da, 1)), capi.ptr(acc), C.byref(da),
                                               capi.stream()), "ssbev_conv_bwd_data")
            out["gx_acc"] = _sha(acc)
    gw = torch.empty(wshape, dtype=torch.float32, device=dev)
    ws = torch.empty(max(16, lib.ssbev_conv_bwd_weight_workspace(C.byref(d))), dtype=torch.uint8, device=dev)
    if c.precision == 2:
        xb, gb = x.to(torch.bfloat16), go.to(torch.bfloat16)
        capi.check(lib.ssbev_conv_bwd_weight_bf16(capi.ptr(xb), capi.ptr(gb), capi.ptr(gw), C.byref(d), capi.ptr(ws), ws.numel(),
                                                  capi.stream()), "ssbev_conv_bwd_weight_bf16")
    else:
        capi.check(lib.ssbev_conv_bwd_weight(capi.ptr(x), capi.ptr(go), capi.ptr(gw), C.byref(d), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_conv_bwd_weight")
    out["gw"] = _sha(gw)
    return out
