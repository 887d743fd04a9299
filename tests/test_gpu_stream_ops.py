"""GPU: every layout, chunk and tail path of the streaming operators (csrc/image_ops.hip, csrc/softmax.hip, csrc/trilinear.hip)
against a float64 reference of the same operation.

The cases are stream_ops_cases.* (test_stream_ops_plan.py pins on the CPU which thread layout, chunks, trips and kernel instance
each one reaches).  Every case runs through two entry levels:

  (a) the stereoscene_amd.functional wrappers under autograd (depthwise_conv2d_same, swish, global_avg_pool, chan_scale, softmax,
      upsample_trilinear), forward and every gradient;
  (b) the C entry points through capi, on buffers of this test: every output is NaN before the launch and has a band of 256
      sentinel floats behind it, every workspace is NaN, exactly as large as its query says, and has the same band.  Afterwards no
      NaN may be left in an output (an element no thread wrote, a chunk slab nobody filled) and every band must be bit-unchanged
      (a thread that wrote past the end) -- both can hide behind torch.empty in the wrappers.

Reference, on the CPU in float64: TF.conv2d with groups = C on the explicitly "same"-padded input; x sigmoid(x); means and sums;
torch.softmax; TF.interpolate -- with autograd for the gradients.

Gates.  Sums of products (depthwise forward, data and weight gradient, chan_sum, chan_scale, trilinear): the reference also
computes A = sum |a_i b_i| per output element, and the gate is (n + 4) 2^-24 A, n the number of terms of that element (k^2; the
output pixels of the tensor for the weight gradient and the pixels of a sample for the gate gradient and the pool; 1 for the
element-wise products; 8 forward and 64 backward for trilinear): the standard bound of an fp32 sum in any order, with or without
fused multiply-adds; a dropped or doubled term is orders of magnitude outside.  Where A = 0 the result must be exactly 0.
Exponential operators (swish, softmax): the device exponential has no bound derived here; the gate is the larger of the
suite's own gate (1e-6 for softmax outputs, 1e-6 max(1, max|ref|) for its gradient, 2e-6 max(1, max|ref|) for Swish and its
gradient) and 4 x the largest error of ATen's fp32 CPU result against the same float64 reference on the same inputs, computed
here at run time.  Every comparison prints its error, gate and ratio (profiles/stream_ops_parity.txt keeps one run).

The reductions that claim a fixed summation order (depthwise weight gradient, chan_sum, the column sums of the softmax) must
give bit-identical results when run twice."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as TF

import stream_ops_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
U = 2.0 ** -24
BAND = 256
_data = {}
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def release_data():
    """Inputs and references are shared by the tests of a case and given back after the last."""
    yield
    _data.clear()
    _refs.clear()
    torch.cuda.empty_cache()


def draw(tag, shape, std=1.0):
    """Seeded fp32 CPU tensor, keyed by `tag`: hashed normals; for the one large case a hashed uniform of the same variance."""
    if tag not in _data:
        if T.numel(shape) > (1 << 20):
            r = std * 3.0 ** 0.5
            _data[tag] = S.hash_uniform(tag, shape, -r, r)
        else:
            _data[tag] = S.hash_normal(tag, shape, std)
    return _data[tag]


def cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


# ---- buffers with a sentinel band -------------------------------------------------------------------------------------------------
def sentinel():
    return (torch.arange(BAND, dtype=torch.int32, device=DEV) * 40503 + 0x5EA70000)


def banded(shape):
    """NaN-filled device tensor of `shape` (a view) followed in memory by BAND sentinel floats -> (view, whole buffer)."""
    n = T.numel(shape)
    buf = torch.empty(n + BAND, dtype=torch.float32, device=DEV)
    buf[:n] = NAN
    buf[n:].view(torch.int32).copy_(sentinel())
    return buf[:n].view(shape), buf


def band_intact(buf):
    return torch.equal(buf[-BAND:].view(torch.int32), sentinel())


def assert_written(label, **bufs):
    """bufs: name -> (view, buffer, is_output): bands bit-unchanged, no NaN left in an output."""
    for name, (view, buf, is_out) in bufs.items():
        assert band_intact(buf), f"{label}: something wrote behind the end of {name}"
        if is_out:
            assert not torch.isnan(view).any(), f"{label}: an element of {name} was never written"


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def compare(label, rows):
    """rows: (name, got, want float64 CPU, gate: float64 CPU tensor, number or (number, how it came about)).  Prints error, gate
    and ratio at the worst element of each tensor; every element must be within its gate (exactly equal where the gate is 0)."""
    worst = 0.0
    for name, got, want, gate in rows:
        gate, note = gate if isinstance(gate, tuple) else (gate, "")
        got = got.detach().to("cpu").double().reshape(want.shape)
        gate = gate.expand_as(want) if torch.is_tensor(gate) else torch.full_like(want, gate)
        err = (got - want).abs()
        err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)        # a NaN is infinitely wrong
        ratio = torch.where(gate > 0, err / gate.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")),
                                                                                torch.zeros_like(err)))
        i = int(ratio.argmax())
        r = float(ratio.flatten()[i])
        print(f"{label} {name}: error {float(err.flatten()[i]):.3e} gate {float(gate.flatten()[i]):.3e} ratio {r:.4f} {note}")
        worst = max(worst, r)
    assert worst <= 1.0, f"{label}: error / gate {worst}"


def exp_gate(project, aten32, want, scaled=True):
    """Gate of an exponential operator: the suite's own, or 4 x what ATen's fp32 CPU kernel misses the float64 reference by."""
    own = project * (max(1.0, want.abs().max().item()) if scaled else 1.0)
    aten = 4.0 * (aten32.double() - want).abs().max().item()
    return max(own, aten), f"(gate: the larger of {own:.3e} and 4 x ATen fp32's {aten / 4.0:.3e})"


def dev(t):
    return t.to(DEV).contiguous()


# ---- depthwise convolution --------------------------------------------------------------------------------------------------------
def dw_geometry(c):
    Ho, pt, pb = T.same_padding(c.Hi, c.k, c.s)
    Wo, pl, pr = T.same_padding(c.Wi, c.k, c.s)
    return Ho, Wo, pt, pb, pl, pr


def dw_inputs(c):
    """x [B, Hi, Wi, C], w [k*k, C], gy [B, Ho, Wo, C]: channels-last fp32 on the CPU."""
    Ho, Wo = dw_geometry(c)[:2]
    return (draw(f"so/{c.id}/x", (c.B, c.Hi, c.Wi, c.C)), draw(f"so/{c.id}/w", (c.k * c.k, c.C), 0.3),
            draw(f"so/{c.id}/gy", (c.B, Ho, Wo, c.C)))


def dw_reference(c):
    def make():
        Ho, Wo, pt, pb, pl, pr = dw_geometry(c)
        x, w, gy = dw_inputs(c)
        nchw = lambda t: t.permute(0, 3, 1, 2).double()
        kern = lambda t: t.t().reshape(c.C, 1, c.k, c.k).double()

        def run(x, w, gy):
            x, w = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            y = TF.conv2d(TF.pad(x, (pl, pr, pt, pb)), w, stride=c.s, groups=c.C)
            assert y.shape[2:] == (Ho, Wo)
            y.backward(gy)
            cl = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
            return cl(y), cl(x.grad), w.grad.reshape(c.C, c.k * c.k).t().contiguous()

        want = run(nchw(x), kern(w), nchw(gy))
        A = run(nchw(x).abs(), kern(w).abs(), nchw(gy).abs())
        n = (c.k * c.k, c.k * c.k, c.B * Ho * Wo)
        return {name: (want[i], (n[i] + 4) * U * A[i]) for i, name in enumerate(("y", "gx", "gw"))}
    return cached(("dw", c.id), make)


def dw_dims(c):
    Ho, Wo, pt, _, pl, _ = dw_geometry(c)
    return capi.DwDims(c.B, c.C, c.Hi, c.Wi, Ho, Wo, c.k, c.s, pt, pl)


def dw_direct(c):
    """All three C entry points on banded buffers -> dict of views, after the write checks."""
    lib = capi.load()
    x, w, gy = (dev(t) for t in dw_inputs(c))
    d = dw_dims(c)
    y, ybuf = banded(gy.shape)
    capi.check(lib.ssbev_dwconv2d_fwd(capi.ptr(x), capi.ptr(w), capi.ptr(y), C.byref(d), capi.stream()), c.id)
    gx, gxbuf = banded(x.shape)
    capi.check(lib.ssbev_dwconv2d_bwd_data(capi.ptr(gy), capi.ptr(w), capi.ptr(gx), C.byref(d), capi.stream()), c.id)
    nws = lib.ssbev_dwconv2d_bwd_weight_workspace(C.byref(d))
    assert nws == c.expect["nchunks"] * c.k * c.k * c.C
    gw, gwbuf = banded(w.shape)
    ws, wsbuf = banded((nws,))
    capi.check(lib.ssbev_dwconv2d_bwd_weight(capi.ptr(x), capi.ptr(gy), capi.ptr(gw), C.byref(d), capi.ptr(ws), nws, capi.stream()), c.id)
    torch.cuda.synchronize()
    assert_written(c.id, y=(y, ybuf, True), gx=(gx, gxbuf, True), gw=(gw, gwbuf, True), ws=(ws, wsbuf, True))
    return dict(y=y, gx=gx, gw=gw)


@pytest.mark.parametrize("case", T.DW_CASES, ids=T.case_id)
def test_depthwise_functional_vs_float64(case):
    x, w, gy = dw_inputs(case)
    xl = F.from_cl(dev(x)).requires_grad_(True)
    wl = dev(w.t().reshape(case.C, 1, case.k, case.k)).requires_grad_(True)
    y = F.depthwise_conv2d_same(xl, wl, case.s)
    y.backward(F.from_cl(dev(gy)))
    got = dict(y=F.to_cl(y), gx=F.to_cl(xl.grad), gw=wl.grad.reshape(case.C, case.k * case.k).t())
    ref = dw_reference(case)
    compare(f"dw {case.id} functional", [(k, got[k], *ref[k]) for k in ("y", "gx", "gw")])


@pytest.mark.parametrize("case", T.DW_CASES, ids=T.case_id)
def test_depthwise_entry_points_vs_float64(case):
    got = dw_direct(case)
    ref = dw_reference(case)
    compare(f"dw {case.id} C ABI", [(k, got[k], *ref[k]) for k in ("y", "gx", "gw")])


@pytest.mark.parametrize("case", T.DW_CASES, ids=T.case_id)
def test_depthwise_weight_gradient_is_bit_identical_twice(case):
    one, two = dw_direct(case)["gw"], dw_direct(case)["gw"]
    assert torch.equal(one.view(torch.int32), two.view(torch.int32))


# ---- squeeze-excitation pieces ----------------------------------------------------------------------------------------------------
def se_inputs(c):
    """x, gy [B, S, C]; gate, g [B, C] (g: the gradient arriving at the pooled vector)."""
    S_ = c.H * c.W
    return (draw(f"so/{c.id}/x", (c.B, S_, c.C)), draw(f"so/{c.id}/gy", (c.B, S_, c.C)),
            S.hash_uniform(f"so/{c.id}/gate", (c.B, c.C), 0.05, 1.0), draw(f"so/{c.id}/g", (c.B, c.C)))


def se_reference(c):
    def make():
        S_ = c.H * c.W
        x, gy, gate, g = (t.double() for t in se_inputs(c))
        one = lambda t: (t, 5 * U * t.abs())                                          # a single product, rounded once or twice
        return dict(pool=(x.sum(1) / S_, (S_ + 4) * U * x.abs().sum(1) / S_),
                    pool_gx=one((g / S_)[:, None, :].expand(c.B, S_, c.C).contiguous()),
                    scale=one(x * gate[:, None, :]), scale_gx=one(gy * gate[:, None, :]),
                    ggate=((gy * x).sum(1), (S_ + 4) * U * (gy * x).abs().sum(1)))
    return cached(("se", c.id), make)


def chan_sum_direct(c, a, bmul, scale, label):
    lib = capi.load()
    S_ = c.H * c.W
    nws = lib.ssbev_chan_sum_workspace(c.B, S_, c.C)
    assert nws == c.expect["nchunks"] * c.B * c.C
    out, obuf = banded((c.B, c.C))
    ws, wsbuf = banded((nws,))
    capi.check(lib.ssbev_chan_sum(capi.ptr(a), capi.ptr(bmul), capi.ptr(out), c.B, S_, c.C, scale, capi.ptr(ws), nws, capi.stream()), label)
    torch.cuda.synchronize()
    assert_written(label, out=(out, obuf, True), ws=(ws, wsbuf, True))
    return out


def chan_scale_direct(c, x, gate, scale, label):
    S_ = c.H * c.W
    y, ybuf = banded((c.B, S_, c.C))
    capi.check(capi.load().ssbev_chan_scale(capi.ptr(x), capi.ptr(gate), capi.ptr(y), c.B, S_, c.C, scale, capi.stream()), label)
    torch.cuda.synchronize()
    assert_written(label, y=(y, ybuf, True))
    return y


@pytest.mark.parametrize("case", T.SE_CASES, ids=T.case_id)
def test_se_functional_vs_float64(case):
    x, gy, gate, g = (dev(t) for t in se_inputs(case))
    sp = (case.B, case.H, case.W, case.C)
    xl = F.from_cl(x.view(sp)).requires_grad_(True)
    pool = F.global_avg_pool(xl)
    assert pool.shape == (case.B, case.C, 1, 1)
    pool.backward(g.view(case.B, case.C, 1, 1))
    x2 = F.from_cl(x.view(sp)).requires_grad_(True)
    gt = gate.view(case.B, case.C, 1, 1).clone().requires_grad_(True)
    y = F.chan_scale(x2, gt)
    y.backward(F.from_cl(gy.view(sp)))
    got = dict(pool=pool, pool_gx=F.to_cl(xl.grad), scale=F.to_cl(y), scale_gx=F.to_cl(x2.grad), ggate=gt.grad)
    ref = se_reference(case)
    compare(f"se {case.id} functional", [(k, got[k], *ref[k]) for k in ("pool", "pool_gx", "scale", "scale_gx", "ggate")])


@pytest.mark.parametrize("case", T.SE_CASES, ids=T.case_id)
def test_se_entry_points_vs_float64(case):
    x, gy, gate, g = (dev(t) for t in se_inputs(case))
    S_ = case.H * case.W
    got = dict(pool=chan_sum_direct(case, x, None, 1.0 / S_, f"{case.id} pool"),
               ggate=chan_sum_direct(case, gy, x, 1.0, f"{case.id} gate gradient"),
               scale=chan_scale_direct(case, x, gate, 1.0, f"{case.id} rescale"),
               scale_gx=chan_scale_direct(case, gy, gate, 1.0, f"{case.id} rescale gradient"),
               pool_gx=chan_scale_direct(case, None, g, 1.0 / S_, f"{case.id} broadcast"))
    ref = se_reference(case)
    compare(f"se {case.id} C ABI", [(k, got[k], *ref[k]) for k in ("pool", "pool_gx", "scale", "scale_gx", "ggate")])


@pytest.mark.parametrize("case", T.SE_CASES, ids=T.case_id)
def test_chan_sum_is_bit_identical_twice(case):
    x, gy, _, _ = (dev(t) for t in se_inputs(case))
    for a, bmul, scale in ((x, None, 1.0 / (case.H * case.W)), (gy, x, 1.0)):
        one, two = (chan_sum_direct(case, a, bmul, scale, case.id) for _ in range(2))
        assert torch.equal(one.view(torch.int32), two.view(torch.int32))


# ---- Swish ------------------------------------------------------------------------------------------------------------------------
def swish_inputs(c):
    """x, gy in the memory order the kernel walks (channels-last for the 4-D cases); the large case takes the tensors of the SE
    case of the same shape.  The operator is fed 3 x: +-5 for the large case, beyond for the others."""
    if c.id == T.BIG:
        x, gy = se_inputs(T.by_id(T.SE_CASES)[T.BIG])[:2]
    else:
        shape = (c.shape[0],) + tuple(c.shape[2:]) + (c.shape[1],) if len(c.shape) >= 3 else c.shape
        x, gy = draw(f"so/swish{c.id}/x", shape), draw(f"so/swish{c.id}/gy", shape)
    return x, gy


def swish_reference(c):
    def make():
        x, gy = swish_inputs(c)
        x32 = (x * 3.0).requires_grad_(True)
        y32 = x32 * torch.sigmoid(x32)
        y32.backward(gy)
        x64 = x32.detach().double().requires_grad_(True)
        y64 = x64 * torch.sigmoid(x64)
        y64.backward(gy.double())
        return dict(x=x32.detach(), y=(y64.detach(), exp_gate(2e-6, y32.detach(), y64.detach())),
                    gx=(x64.grad, exp_gate(2e-6, x32.grad, x64.grad)))
    return cached(("swish", c.id), make)


@pytest.mark.parametrize("case", T.SWISH_CASES, ids=T.case_id)
def test_swish_functional_vs_float64(case):
    ref = swish_reference(case)
    gy = dev(swish_inputs(case)[1])
    x = dev(ref["x"])
    if len(case.shape) >= 3:                                             # logical [B, C, *spatial] over the channels-last buffer
        cl = (case.shape[0],) + tuple(case.shape[2:]) + (case.shape[1],)
        x, gy = F.from_cl(x.view(cl)), F.from_cl(gy.view(cl))
        assert tuple(x.shape) == tuple(case.shape)
    x = x.requires_grad_(True)
    y = F.swish(x)
    y.backward(gy)
    flat = (lambda t: F.to_cl(t)) if len(case.shape) >= 3 else (lambda t: t)
    compare(f"swish {case.id} functional", [("y", flat(y), *ref["y"]), ("gx", flat(x.grad), *ref["gx"])])


@pytest.mark.parametrize("case", T.SWISH_CASES, ids=T.case_id)
def test_swish_entry_points_vs_float64(case):
    lib = capi.load()
    ref = swish_reference(case)
    x, gy = dev(ref["x"]), dev(swish_inputs(case)[1])
    n = x.numel()
    y, ybuf = banded(x.shape)
    gx, gxbuf = banded(x.shape)
    if case.expect is None:                        # n % 4 != 0 is refused by design; the wrapper serves it with tensor operations
        assert lib.ssbev_swish_fwd(capi.ptr(x), capi.ptr(y), n, capi.stream()) == capi.EINVAL
        assert lib.ssbev_swish_bwd(capi.ptr(x), capi.ptr(gy), capi.ptr(gx), n, capi.stream()) == capi.EINVAL
        torch.cuda.synchronize()
        assert band_intact(ybuf) and band_intact(gxbuf) and torch.isnan(y).all() and torch.isnan(gx).all()
        return
    capi.check(lib.ssbev_swish_fwd(capi.ptr(x), capi.ptr(y), n, capi.stream()), case.id)
    capi.check(lib.ssbev_swish_bwd(capi.ptr(x), capi.ptr(gy), capi.ptr(gx), n, capi.stream()), case.id)
    torch.cuda.synchronize()
    assert_written(f"swish {case.id}", y=(y, ybuf, True), gx=(gx, gxbuf, True))
    compare(f"swish {case.id} C ABI", [("y", y, *ref["y"]), ("gx", gx, *ref["gx"])])


# ---- softmax along a strided axis -------------------------------------------------------------------------------------------------
def softmax_inputs(c):
    """x, gy as [outer, C, inner].  The special case: one column masked to -inf but for one entry, one column offset by +80, one
    (the very last) by -80, one constant."""
    outer, Cn, inner = T.softmax_view(c.shape, c.dim)
    x = draw(f"so/{c.id}/x", (outer, Cn, inner), 3.0)
    gy = draw(f"so/{c.id}/gy", (outer, Cn, inner))
    if c.special:
        x = x.clone()
        keep = x[0, 40, 0].item()
        x[0, :, 0] = float("-inf")
        x[0, 40, 0] = keep                          # slices 0..3 and 5..7 of this column sum to zero
        x[1, :, 23] += 80.0
        x[outer - 1, :, inner - 1] -= 80.0
        x[0, :, 10] = 0.5
    return x, gy


def softmax_reference(c):
    def make():
        x, gy = softmax_inputs(c)
        x32 = x.clone().requires_grad_(True)
        y32 = torch.softmax(x32, 1)
        y32.backward(gy)
        x64 = x.double().requires_grad_(True)
        y64 = torch.softmax(x64, 1)
        y64.backward(gy.double())
        return dict(y=(y64.detach(), exp_gate(1e-6, y32.detach(), y64.detach(), scaled=False)),
                    gx=(x64.grad, exp_gate(1e-6, x32.grad, x64.grad)))
    return cached(("softmax", c.id), make)


def softmax_direct(c):
    lib = capi.load()
    outer, Cn, inner = T.softmax_view(c.shape, c.dim)
    assert lib.ssbev_softmax_axis_slices(Cn, inner) == c.expect["SL"]
    x, gy = (dev(t) for t in softmax_inputs(c))
    y, ybuf = banded(x.shape)
    capi.check(lib.ssbev_softmax_axis_fwd(capi.ptr(x), capi.ptr(y), outer, Cn, inner, capi.stream()), c.id)
    gx, gxbuf = banded(x.shape)
    capi.check(lib.ssbev_softmax_axis_bwd(capi.ptr(y), capi.ptr(gy), capi.ptr(gx), outer, Cn, inner, capi.stream()), c.id)
    torch.cuda.synchronize()
    assert_written(f"softmax {c.id}", y=(y, ybuf, True), gx=(gx, gxbuf, True))
    return dict(y=y, gx=gx)


@pytest.mark.parametrize("case", [c for c in T.SOFTMAX_CASES if not c.direct], ids=T.case_id)
def test_softmax_functional_vs_float64(case):
    x, gy = (dev(t).view(case.shape) for t in softmax_inputs(case))
    x = x.requires_grad_(True)
    y = F.softmax(x, case.dim)
    y.backward(gy)
    ref = softmax_reference(case)
    compare(f"softmax {case.id} functional", [("y", y, *ref["y"]), ("gx", x.grad, *ref["gx"])])
    if case.special:
        assert (y.view(T.softmax_view(case.shape, case.dim))[0, :, 0] != 0).sum().item() == 1          # the masked column: one 1


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=T.case_id)
def test_softmax_entry_points_vs_float64(case):
    got = softmax_direct(case)
    ref = softmax_reference(case)
    compare(f"softmax {case.id} C ABI", [("y", got["y"], *ref["y"]), ("gx", got["gx"], *ref["gx"])])


@pytest.mark.parametrize("case", T.SOFTMAX_CASES, ids=T.case_id)
def test_softmax_is_bit_identical_twice(case):
    one, two = softmax_direct(case), softmax_direct(case)
    for k in one:
        assert torch.equal(one[k].view(torch.int32), two[k].view(torch.int32)), k


# ---- trilinear x2 -----------------------------------------------------------------------------------------------------------------
def tri_inputs(c):
    D, H, W = c.sp
    return draw(f"so/{c.id}/x", (c.B, D, H, W, c.C)), draw(f"so/{c.id}/gy", (c.B, 2 * D, 2 * H, 2 * W, c.C))


def tri_reference(c):
    def make():
        x, gy = tri_inputs(c)
        size = tuple(2 * s for s in c.sp)

        def run(x, gy):
            x = x.permute(0, 4, 1, 2, 3).double().contiguous().requires_grad_(True)
            y = TF.interpolate(x, size=size, mode="trilinear", align_corners=False)
            y.backward(gy.permute(0, 4, 1, 2, 3).double())
            cl = lambda t: t.detach().permute(0, 2, 3, 4, 1).contiguous()
            return cl(y), cl(x.grad)

        want, A = run(x, gy), run(x.abs(), gy.abs())                    # the interpolation weights are non-negative
        return dict(y=(want[0], (8 + 4) * U * A[0]), gx=(want[1], (64 + 4) * U * A[1]))
    return cached(("tri", c.id), make)


@pytest.mark.parametrize("case", T.TRILINEAR_CASES, ids=T.case_id)
def test_trilinear_functional_vs_float64(case):
    x, gy = (dev(t) for t in tri_inputs(case))
    xl = F.from_cl(x).requires_grad_(True)
    y = F.upsample_trilinear(xl, tuple(2 * s for s in case.sp))
    assert tuple(y.shape) == (case.B, case.C) + tuple(2 * s for s in case.sp)
    y.backward(F.from_cl(gy))
    ref = tri_reference(case)
    compare(f"trilinear {case.id} functional", [("y", F.to_cl(y), *ref["y"]), ("gx", F.to_cl(xl.grad), *ref["gx"])])


@pytest.mark.parametrize("case", T.TRILINEAR_CASES, ids=T.case_id)
def test_trilinear_entry_points_vs_float64(case):
    lib = capi.load()
    x, gy = (dev(t) for t in tri_inputs(case))
    d = capi.UpsampleDims(case.B, *case.sp, case.C)
    y, ybuf = banded(gy.shape)
    capi.check(lib.ssbev_trilinear2x_fwd(capi.ptr(x), capi.ptr(y), C.byref(d), capi.stream()), case.id)
    gx, gxbuf = banded(x.shape)
    capi.check(lib.ssbev_trilinear2x_bwd(capi.ptr(gy), capi.ptr(gx), C.byref(d), capi.stream()), case.id)
    torch.cuda.synchronize()
    assert_written(f"trilinear {case.id}", y=(y, ybuf, True), gx=(gx, gxbuf, True))
    ref = tri_reference(case)
    compare(f"trilinear {case.id} C ABI", [("y", y, *ref["y"]), ("gx", gx, *ref["gx"])])
