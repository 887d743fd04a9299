"""GPU: every kind, fold and tail path of ssbev_conv_bwd_weight (csrc/conv_mfma.hip, csrc/conv_thin_mfma.hip) against a float64
reference of the same operation.

The cases are wgrad_cases.CASES (test_wgrad_plan.py pins on the CPU which kind, chunking and fold each one reaches).  Every case
runs through two entry levels:

  (a) functional.conv3d / conv2d / conv_transpose3d under autograd with F.TILE_HINT as the case says (and the Winograd and GEMM
      routes of the wrappers off, so that the call arrives at ssbev_conv_bwd_weight: the test watches the entry point and requires
      the kind of the dims it was handed to be the case's);
  (b) ssbev_conv_bwd_weight through capi on buffers of this test: gw is NaN before the launch, the workspace is NaN and exactly as
      large as ssbev_conv_wgrad_plan_query says, both are followed by a band of 256 sentinel floats.  Afterwards gw holds no NaN
      (an element no thread wrote; a partial slab nobody filled but a fold read; the channels-first kind not clearing its own
      padded copy) and the bands are bit-unchanged.  The plan is queried and held to the case's `expect` right before the launch.

Reference, on the CPU in float64: autograd of TF.conv3d / TF.conv_transpose3d (wgrad_cases.reference).

Exact regime.  x and gy are hashed integers in -lim .. lim (lim = 2, 1 for the largest case): every product and every partial
sum is an integer below 2^24 in any order, and the F(2,3) transforms of the Dh and WINO Lds kinds only add multipliers of 1/2
and 1/4 (at most 4 fractional bits over two nested stages; test_wgrad_plan.py checks max A x 16 < 2^24 per case), so every kind
must reproduce the reference with equality.  The indicator input keeps the coarse-grid tensor (gy; x of a transposed layer) at four voxels only (first, last, last of
the first chunk, first of the last chunk, in the chunk order of the kind: wgrad_cases.boundary_voxels): taps that fall into the padding there must be exactly 0.

Rounding regime.  Hashed normals.  Direct kinds: |got - ref| <= (n + 4) 2^-24 A per element, A = the float64 weight gradient of
|x|, |gy|, n the voxels summed: the standard bound of an fp32 sum of n exact-product terms in any order, with or without fused
multiply-adds.  Where A = 0 the result must be exactly 0.  Winograd-domain kinds (Dh: F(2,3) along d and h; Lds instances 1, 2:
along h): the kernel sums products of transformed operands over n / 2^a tiles (a transformed axes) and applies G^T afterwards.
Each transformed operand is a sum of two values, one rounding (relative 2^-24 of its absolute sum) per axis; the products then
carry 2 a roundings, the accumulation n / 2^a, the output transform two additions per axis (halvings are exact): the gate is
(n / 2^a + 4 + 4 a) 2^-24 A_w with A_w the same Winograd-domain expression evaluated on absolute values in float64
(wgrad_cases.wino_abs_bound).  No constant here comes from a measured error.  Every comparison prints error, gate and ratio
(profiles/wgrad_parity.txt keeps one run).

Every launch is made twice and must give identical bits: all folds claim a fixed order."""
import ctypes as C

import pytest
import torch

import wgrad_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = 2.0 ** -24
BAND = 256
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def release_refs():
    """Inputs and references are shared by the tests of a case and given back after the last."""
    yield
    _refs.clear()
    torch.cuda.empty_cache()


def cached(key, make):
    if key not in _refs:
        _refs[key] = make()
    return _refs[key]


def plan_of(c):
    return T.query(T.dims(c))


def inputs(c, regime):
    def make():
        if regime == "exact":
            return T.exact_inputs(c)
        if regime == "indicator":
            return T.indicator_inputs(c, plan_of(c))
        xs, gs = T.shapes(c)
        return S.hash_normal(f"wg/{c.id}/x", xs), S.hash_normal(f"wg/{c.id}/gy", gs)
    return cached((c.id, regime, "in"), make)


def reference(c, regime):
    return cached((c.id, regime, "ref"), lambda: T.reference(c, *inputs(c, regime)))


def gate(c):
    """(per-element gate, note) of the rounding regime."""
    def make():
        x, gy = inputs(c, "round")
        axes = T.wino_axes(c, plan_of(c))
        n = T.summed_voxels(c)
        if axes:
            a = len(axes)
            return (n // 2 ** a + 4 + 4 * a) * U * T.wino_abs_bound(c, x, gy, axes), f"(F(2,3) along {a} axes, {n // 2 ** a} tiles)"
        return (n + 4) * U * T.reference(c, x.abs(), gy.abs()), f"({n} voxels)"
    return cached((c.id, "gate"), make)


# ---- buffers with a sentinel band -------------------------------------------------------------------------------------------------
def sentinel():
    return torch.arange(BAND, dtype=torch.int32, device=DEV) * 40503 + 0x5EA70000


def banded(n):
    """NaN-filled device buffer of n floats followed in memory by BAND sentinel floats -> (view of n, whole buffer)."""
    buf = torch.empty(n + BAND, dtype=torch.float32, device=DEV)
    buf[:n] = float("nan")
    buf[n:].view(torch.int32).copy_(sentinel())
    return buf[:n], buf


def band_intact(buf):
    return torch.equal(buf[-BAND:].view(torch.int32), sentinel())


def cl(t):
    """[B, C, D, H, W] on the CPU -> channels-last [B, D, H, W, C] on the device."""
    return t.permute(0, 2, 3, 4, 1).contiguous().to(DEV)


# ---- the two entry levels ---------------------------------------------------------------------------------------------------------
def run_capi(c, x, gy):
    lib = capi.load()
    d = T.dims(c)
    plan = plan_of(c)
    assert {k: v for k, v in plan.items() if v or k == "kind"} == c.expect, (c.id, plan)
    assert lib.ssbev_conv_bwd_weight_workspace(C.byref(d)) == plan["workspace"]
    assert plan["workspace"] % 4 == 0
    xd, gd = cl(x), cl(gy)
    outs = []
    for _ in range(2):
        gw, gw_buf = banded(c.Cin * c.Cout * c.k[0] * c.k[1] * c.k[2])
        ws, ws_buf = banded(plan["workspace"] // 4)
        capi.check(lib.ssbev_conv_bwd_weight(capi.ptr(xd), capi.ptr(gd), capi.ptr(gw), C.byref(d), capi.ptr(ws), plan["workspace"],
                                             capi.stream()), "ssbev_conv_bwd_weight")
        torch.cuda.synchronize()
        assert band_intact(gw_buf), f"{c.id}: something wrote behind the end of gw"
        assert band_intact(ws_buf), f"{c.id}: something wrote behind the end of the workspace"
        assert not torch.isnan(gw).any(), f"{c.id}: an element of gw was never written, or a fold read a slab nobody wrote"
        outs.append(gw.view(T.wshape(c)).clone())
    assert torch.equal(outs[0], outs[1]), f"{c.id}: two launches differ"
    return outs[0].cpu()


class _Watch:
    """Stands in front of ssbev_conv_bwd_weight and records the dims of every call."""

    def __init__(self, lib):
        self.lib, self.fn, self.seen = lib, lib.ssbev_conv_bwd_weight, []

    def __call__(self, x, gy, gw, d, *rest):
        dd = capi.ConvDims()
        C.memmove(C.byref(dd), d, C.sizeof(dd))
        self.seen.append(dd)
        return self.fn(x, gy, gw, d, *rest)

    def __enter__(self):
        self.lib.ssbev_conv_bwd_weight = self
        return self

    def __exit__(self, *exc):
        self.lib.ssbev_conv_bwd_weight = self.fn


def run_autograd(c, x, gy):
    two_d = c.k[0] == 1 and c.grid[0] == 1 and c.k != (1, 1, 1) and not c.tr
    saved = F.TILE_HINT, F.WINOGRAD, F.OWN_GEMM, F.GEMM_LAYERS
    F.TILE_HINT, F.WINOGRAD, F.OWN_GEMM, F.GEMM_LAYERS = c.hint, False, False, False
    outs = []
    try:
        with _Watch(capi.load()) as watch:
            for _ in range(2):
                w = torch.zeros(T.wshape(c), device=DEV)
                xd, gd = x.to(DEV), gy.to(DEV)
                if two_d:
                    w = w[:, :, 0].contiguous().requires_grad_(True)
                    y = F.conv2d(xd[:, :, 0], w, None, c.s[1:], c.p[1:], c.dl[1:])
                    y.backward(gd[:, :, 0])
                else:
                    w.requires_grad_(True)
                    y = F.conv_transpose3d(xd, w, None, c.s, c.p, c.op) if c.tr else F.conv3d(xd, w, None, c.s, c.p, c.dl)
                    y.backward(gd)
                torch.cuda.synchronize()
                outs.append(w.grad.reshape(T.wshape(c)).clone())
    finally:
        F.TILE_HINT, F.WINOGRAD, F.OWN_GEMM, F.GEMM_LAYERS = saved
    assert len(watch.seen) == 2, f"{c.id}: the wrappers did not hand the weight gradient to ssbev_conv_bwd_weight"
    seen = T.query(watch.seen[0])
    if c.id in T.AUTOGRAD_PADDED:      # a channel count that is no multiple of 4: the wrappers pad it, the kind must stay
        cin, cout, kind, two_stage = T.AUTOGRAD_PADDED[c.id]
        assert (watch.seen[0].Cin, watch.seen[0].Cout, T.KINDS[seen["kind"]], seen["two_stage"]) == (cin, cout, kind, two_stage), c.id
    else:                              # the case's own dims (the thin-side kind takes its 1 / 2 / 4 channels unpadded)
        assert (watch.seen[0].Cin, watch.seen[0].Cout) == (c.Cin, c.Cout), c.id
        assert {k: v for k, v in seen.items() if v or k == "kind"} == c.expect, (c.id, seen)
    assert torch.equal(outs[0], outs[1]), f"{c.id}: two backward passes differ"
    return outs[0].cpu()


LEVELS = {"capi": run_capi, "autograd": run_autograd}


# ---- comparison -------------------------------------------------------------------------------------------------------------------
def compare(label, got, want, gate_t, note=""):
    got = got.double().reshape(want.shape)
    err = (got - want).abs()
    err = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)            # a NaN is infinitely wrong
    ratio = torch.where(gate_t > 0, err / gate_t.clamp_min(1e-300),
                        torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    i = int(ratio.argmax())
    r = float(ratio.flatten()[i])
    print(f"{label}: error {float(err.flatten()[i]):.3e} gate {float(gate_t.flatten()[i]):.3e} ratio {r:.4f} {note}")
    assert r <= 1.0, f"{label}: error / gate {r}"


IDS = [c.id for c in T.CASES]


@pytest.mark.parametrize("level", sorted(LEVELS))
@pytest.mark.parametrize("cid", IDS)
def test_exact_integers(cid, level):
    c = T.BY_ID[cid]
    got = LEVELS[level](c, *inputs(c, "exact"))
    want = reference(c, "exact")
    bad = (got.double() != want).sum().item()
    print(f"{cid} {level} exact: {bad} of {want.numel()} elements differ, max |ref| {want.abs().max().item():.0f}")
    assert torch.equal(got.double(), want), f"{cid} {level}: {bad} elements differ from the float64 reference"


@pytest.mark.parametrize("level", sorted(LEVELS))
@pytest.mark.parametrize("cid", IDS)
def test_indicator_voxels(cid, level):
    c = T.BY_ID[cid]
    got = LEVELS[level](c, *inputs(c, "indicator"))
    want = reference(c, "indicator")
    bad = (got.double() != want).sum().item()
    print(f"{cid} {level} indicator: {bad} of {want.numel()} elements differ, {int((want == 0).sum())} exact zeros expected")
    assert torch.equal(got.double(), want), f"{cid} {level}: {bad} elements differ from the float64 reference"


@pytest.mark.parametrize("level", sorted(LEVELS))
@pytest.mark.parametrize("cid", IDS)
def test_rounding_regime(cid, level):
    c = T.BY_ID[cid]
    got = LEVELS[level](c, *inputs(c, "round"))
    g, note = gate(c)
    compare(f"{cid} {level} gw", got, reference(c, "round"), g, note)
