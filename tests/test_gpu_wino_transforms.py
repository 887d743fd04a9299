"""GPU: every entry point of csrc/winograd.hip, stage by stage through the C ABI, against the float64 reference wino_ref.py.

The cases are wino_cases.CASES; test_wino_ref.py proves the reference and pins, on the CPU, which tails, blocks, waves and ring
states each case reaches.  Inputs come from synthetic.hash_normal; the GEMM plans are queried and asserted again right before
the launch.  Every output is NaN before the launch and finite afterwards, between guard bands that must come back untouched.

Bounds, per element, derived and not tuned (eps = 2^-24, `mag` = the magnitude companion: the same transform with
|coefficients| on |input|; n = wino_ref.chain: per axis the longest row's additions plus one per coefficient that is not +-1,
summed over the axes):
  fp32 transforms and weight transforms      |got - ref| <= n eps mag
  a bf16 destination (`_bf16`, `_bf16a`)     + half a bf16 ulp of the stored value: one round-to-nearest-even.  bf16 keeps 8
                                             significant bits, so that is 2^(e-8) for a value in [2^e, 2^(e+1)): 2^-9 |ref| at
                                             the top of a binade and 2^-8 |ref| at its bottom.  (2^-9 |ref| throughout, the
                                             first derivation, is exceeded by correct rounding: 1 + 2^-8 is stored as 1.)  The
                                             binade is taken at |ref| plus the fp32 part of the bound.  A bf16 source is fed
                                             bf16-exact values, and the reference gets the same values: no input rounding
  accumulating output transforms             |got - (old + ref)| <= n eps mag + eps |old + ref|; and from old = 0 and old = 1:
                                             |got1 - got0 - 1| <= eps |got0 + 1| at every position -- each one is read, added
                                             to and written exactly once
  the two GEMMs                              |got - ref| <= (K + n_depth) eps sum |a| |u|, the bound of a length-K fp32 dot product
                                             in any order; n_depth = 3 (depth B^T and A^T in registers) for ssbev_wino_dgemm
                                             with the magnitude sum taken through the depth transform, 0 for ssbev_wino_bgemm.
The GEMM weights are integers / 8: G (x) G (x) G of them is exact in fp32, the packed operand is compared bit for bit with the
reference layout, and the bound holds as stated with u the exact U.  The pack's own rounding is measured separately, on hashed
normal weights, against the weight-transform bound in the packed layout (padding must be exactly 0).

Every run also shows that its bound means something: the largest error / bound is printed and is above 0 (the kernel did not
hand back zeros, or the reference) -- except from a bf16-exact source into an fp32 destination, where fp32 holds every partial
sum of the handful of 8-bit significands exactly and 0 is the right error; there the output must merely be non-zero -- and the
same reference with one coefficient negated (of B^T, A^T or G; computed on the CPU, no kernel is altered) violates the bound at
the same shape.

The whole-path tests run one convolution per default route at the smallest routed shape against float64 conv at the gates of
test_gpu_kernels.py, so that two stages that are each self-consistent cannot disagree about a layout unnoticed."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as TF

import wino_cases as T
import wino_ref as R
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
GUARD = 1024                     # elements of a guard band
PATTERN = 0x5A5AA5A5


def bf16_half_ulp(v):
    """Half a unit in the last place of bf16 (8 significant bits) at |v|: the largest error of one round-to-nearest-even."""
    _, ex = torch.frexp(v)                                       # |v| = m 2^ex, m in [0.5, 1)
    return torch.where(v > 0, torch.ldexp(torch.ones_like(v), ex - 9), torch.zeros_like(v))


class Guarded:
    """A NaN-filled tensor of `shape` and `dtype` between two guard bands of PATTERN."""

    def __init__(self, shape, dtype=torch.float32):
        self.elems = 1
        for s in shape:
            self.elems *= s
        self.width = 2 if dtype == torch.bfloat16 else 4
        per = 4 // self.width                                   # elements per 32-bit guard word
        words = -(-self.elems // per)
        self.raw = torch.full((words + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.words = words
        self.body = self.raw[GUARD:GUARD + words].view(dtype)[:self.elems].view(shape)
        self.body.fill_(float("nan"))

    def intact(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.words:] == PATTERN).all())


def upload(t, bf16):
    return t.to(DEV, torch.bfloat16 if bf16 else torch.float32).contiguous()


def judge(kind, case, got, ref, bound, wrong, exact_ok=False):
    """Assert |got - ref| <= bound everywhere, a meaningful bound, and print the largest error / bound."""
    got = got.detach().to("cpu", torch.float64)
    assert got.shape == ref.shape and torch.isfinite(got).all()
    err = (got - ref).abs()
    live = bound > 0
    worst = (err[live] / bound[live]).max().item() if live.any() else 0.0
    print(f"wino-stage {kind} {T.case_id(case)}: worst err / bound {worst:.4f}")
    assert (err <= bound).all(), (worst, int((err > bound).sum()))
    assert (got != 0).any()
    assert worst > 0 or exact_ok, "zero error everywhere"
    assert ((got - wrong).abs() > bound).any(), "the bound does not notice a negated coefficient"
    return worst


# -------------------------------------------------------------------------------------------------------------- transforms
@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.TRANSFORM], ids=T.case_id)
def test_transform_matches_float64(case):
    lib = capi.load()
    tiling, role, storage = case.what
    B, D, H, W, Cc = case.shape
    act_shape, freq_shape = (B, D, H, W, Cc), (R.nfreq(tiling), R.ntiles(tiling, B, D, H, W), Cc)
    act_bf, freq_bf = storage == T.BF16A, storage in (T.BF16, T.BF16A)
    assert T.threads(case) == case.plan
    if role == T.INPUT:
        fn, which, tr, src_shape, src_bf, dst_shape, dst_bf = R.input_transform, "Bt", False, act_shape, act_bf, freq_shape, freq_bf
    elif role == T.ADJOINT:
        fn, which, tr, src_shape, src_bf, dst_shape, dst_bf = R.output_adjoint, "At", True, act_shape, act_bf, freq_shape, freq_bf
    else:
        def fn(M, tl, **kw):
            return R.output_transform(M, tl, (B, D, H, W), **kw)
        which, tr, src_shape, src_bf, dst_shape, dst_bf = "At", False, freq_shape, freq_bf, act_shape, act_bf
    src = S.hash_normal(f"wst/{case.names[0]}{case.shape}", src_shape)
    if src_bf:
        src = R.to_bf16_exact(src)
    ref, mag, wrong = fn(src, tiling), fn(src, tiling, absolute=True), fn(src, tiling, negate=(2, 1, 2))
    bound = R.chain(tiling, which, tr) * EPS * mag
    if dst_bf:
        bound = bound + bf16_half_ulp(ref.abs() + bound)
    dims = capi.WinoDims(B, D, H, W, Cc, 1 if role == T.OUTPUT_ACC else 0)
    entry = getattr(lib, case.names[0])
    src_d = upload(src, src_bf)

    def run(old=None):
        dst = Guarded(dst_shape, torch.bfloat16 if dst_bf else torch.float32)
        if old is not None:
            dst.body.copy_(old)
        capi.check(entry(capi.ptr(src_d), capi.ptr(dst.body), C.byref(dims), capi.stream()), case.names[0])
        torch.cuda.synchronize()
        assert dst.intact()
        return dst.body.clone()

    if role != T.OUTPUT_ACC:
        judge(f"{role}/{storage}", case, run(), ref, bound, wrong, exact_ok=src_bf and not dst_bf)
        return
    old = S.hash_normal(f"wst/old{case.shape}", dst_shape)
    want = old.double() + ref
    judge(f"{role}/{storage}", case, run(old.to(DEV)), want, bound + EPS * want.abs(), old.double() + wrong)
    got0, got1 = run(torch.zeros(dst_shape, device=DEV)).cpu().double(), run(torch.ones(dst_shape, device=DEV)).cpu().double()
    assert ((got0 - ref).abs() <= bound).all()
    assert ((got1 - got0 - 1).abs() <= EPS * (got0 + 1).abs()).all()            # every position added to exactly once


# ----------------------------------------------------------------------------------------------------------------- weights
@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.WEIGHT], ids=T.case_id)
def test_weight_stage_matches_float64(case):
    lib = capi.load()
    tiling, role, prefix, ndim, mode = case.what
    cout, cin = case.shape
    fd = R.families(tiling)[0]
    taps = (3, 3) if fd.r == 1 else (3, 3, 3)
    nf = R.nfreq(tiling)
    entry = getattr(lib, case.names[0])
    if role == T.W_TRANSFORM:
        w = S.hash_normal(f"wst/w{case.names[0]}{ndim}{case.shape}", (cout, cin) + taps)
        ref, mag = R.weight_transform(w, tiling, mode), R.weight_transform(w, tiling, mode, absolute=True)
        wrong = R.weight_transform(w, tiling, mode, negate=(2, 1, 2))
        dst = Guarded(tuple(ref.shape))
        assert tuple(ref.shape) == ((nf, cin, cout) if mode == 0 else (nf, cout, cin))
        capi.check(entry(capi.ptr(w.to(DEV)), capi.ptr(dst.body), cout, cin, ndim, mode, capi.stream()), case.names[0])
        n = R.chain(tiling, "G")
    else:
        gU = S.hash_normal(f"wst/gu{case.names[0]}{ndim}{case.shape}", (nf, cin, cout))
        two_d = fd.r == 1
        ref, mag = R.weight_grad(gU, tiling, two_d), R.weight_grad(gU, tiling, two_d, absolute=True)
        wrong = R.weight_grad(gU, tiling, two_d, negate=(2, 1, 2))
        dst = Guarded(tuple(ref.shape))
        assert tuple(ref.shape) == (cout, cin) + taps
        capi.check(entry(capi.ptr(gU.to(DEV)), capi.ptr(dst.body), cout, cin, ndim, capi.stream()), case.names[0])
        n = R.chain(tiling, "G", transposed=True)
    torch.cuda.synchronize()
    assert dst.intact()
    judge(role, case, dst.body, ref, n * EPS * mag, wrong)


# ------------------------------------------------------------------------------------------------------------- GEMM stages
def exact_weights(tag, cout, cin):
    """Integers in [-4, 4] over 8: G23 (x) G23 (x) G23 of them (entries 0, 1/2, 1) is exact in fp32."""
    return torch.round(S.hash_uniform(tag, (cout, cin, 3, 3, 3), -4.49, 4.49)) / 8.0


def packed(lib, w, cout, cin, mode):
    """ssbev_wino_dgemm_pack into a guarded NaN buffer of ssbev_wino_dgemm_packed_elems floats; (buffer, this mode's part)."""
    K, N = (cin, cout) if mode == 0 else (cout, cin)
    wp = Guarded((lib.ssbev_wino_dgemm_packed_elems(cout, cin),))
    capi.check(lib.ssbev_wino_dgemm_pack(capi.ptr(w.to(DEV)), capi.ptr(wp.body), cout, cin, mode, capi.stream()), "ssbev_wino_dgemm_pack")
    torch.cuda.synchronize()
    assert wp.intact()
    used = 64 * (-(-K // 8) * 8) * (-(-N // 32) * 32)
    assert wp.elems >= used and torch.isnan(wp.body[used:]).all()        # nothing behind this mode's own layout is written
    return wp, wp.body[:used].view(64, -(-K // 8), 2, -(-N // 32) * 32, 4)


def check_pack(lib, case, K, N, mode):
    """The pack on hashed normal weights: the weight-transform bound in the packed layout, exact zeros in the padding."""
    cout, cin = (N, K) if mode == 0 else (K, N)
    w = S.hash_normal(f"wst/pw{mode}{case.shape}", (cout, cin, 3, 3, 3))
    _, got = packed(lib, w, cout, cin, mode)
    ref = R.dgemm_pack_layout(R.weight_transform(w, "w3d", mode))
    mag = R.dgemm_pack_layout(R.weight_transform(w, "w3d", mode, absolute=True))
    wrong = R.dgemm_pack_layout(R.weight_transform(w, "w3d", mode, negate=(2, 1, 2)))
    live = R.dgemm_pack_layout(torch.ones(64, K, N, dtype=torch.float64)) > 0
    assert (got.cpu()[~live] == 0).all()
    judge(f"pack/mode{mode}", case, got, ref, R.chain("w3d", "G") * EPS * mag, wrong)


def exact_pack(lib, tag, K, N, mode):
    """(device buffer of the packed exact weights, their float64 U [64][K][N]); the packed operand is checked bit for bit."""
    cout, cin = (N, K) if mode == 0 else (K, N)
    w = exact_weights(tag, cout, cin)
    wp, got = packed(lib, w, cout, cin, mode)
    U = R.weight_transform(w, "w3d", mode)
    assert torch.equal(got.cpu().double(), R.dgemm_pack_layout(U))
    return wp, w, U


@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.DGEMM], ids=T.case_id)
def test_dgemm_matches_float64(case):
    lib = capi.load()
    B, D, H, W, K, N = case.shape
    Thw = (H // 2) * (W // 2)
    rows = B * D * Thw
    p = T.query(case)
    assert T.case_plan(case, p) == case.plan and T.dgemm_props(case.shape, p) == case.props
    d = capi.WinoDims(B, D, H, W, K)
    P = S.hash_normal(f"wst/dp{case.shape}", (16, rows, K))
    P_d = P.to(DEV)
    for mode in (0, 1):
        check_pack(lib, case, K, N, mode)
        wp, w, U = exact_pack(lib, f"wst/dw{mode}{case.shape}", K, N, mode)
        mo = Guarded((16, rows, N))
        capi.check(lib.ssbev_wino_dgemm(capi.ptr(P_d), capi.ptr(wp.body), capi.ptr(mo.body), C.byref(d), N, capi.stream()), "ssbev_wino_dgemm")
        torch.cuda.synchronize()
        assert mo.intact() and wp.intact()
        ref, mag = R.dgemm(P, U, B, D), R.dgemm(P, U, B, D, absolute=True)
        wrong = R.dgemm(P, U, B, D, negate=(0, 2))
        judge(f"dgemm/mode{mode}", case, mo.body, ref, (K + R.N_DEPTH_DGEMM) * EPS * mag, wrong)


@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.BGEMM], ids=T.case_id)
def test_bgemm_matches_float64(case):
    lib = capi.load()
    Tr, K, N = case.shape
    p = T.query(case)
    assert T.case_plan(case, p) == case.plan and T.bgemm_props(case.shape, p) == case.props
    A = S.hash_normal(f"wst/ba{case.shape}", (64, Tr, K))
    A_d = A.to(DEV)
    for mode in (0, 1):
        check_pack(lib, case, K, N, mode)
        wp, w, U = exact_pack(lib, f"wst/bw{mode}{case.shape}", K, N, mode)
        cm = Guarded((64, Tr, N))
        capi.check(lib.ssbev_wino_bgemm(capi.ptr(A_d), capi.ptr(wp.body), capi.ptr(cm.body), Tr, K, N, capi.stream()), "ssbev_wino_bgemm")
        torch.cuda.synchronize()
        assert cm.intact() and wp.intact()
        ref, mag = R.bgemm(A, U), R.bgemm(A, U, absolute=True)
        wrong = R.bgemm(A, R.weight_transform(w, "w3d", mode, negate=(2, 1, 2)))
        judge(f"bgemm/mode{mode}", case, cm.body, ref, K * EPS * mag, wrong)


# -------------------------------------------------------------------------------------------------------------- whole path
def _conv_problem(route):
    B, cin, cout, D, H, W = T.CONV_CASES[route]
    nd = 3 if D else 2
    shape = (B, cin, D, H, W) if D else (B, cin, H, W)
    x = S.hash_normal(f"wst/cx{route}", shape)
    w = S.hash_uniform(f"wst/cw{route}", (cout, cin) + (3,) * nd, -1, 1) * (3.0 / (cin * 3 ** nd)) ** 0.5
    xc, wc = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = (TF.conv3d if D else TF.conv2d)(xc, wc, None, 1, 1)
    go = S.hash_normal(f"wst/cgo{route}", tuple(want.shape))
    want.backward(go.double())
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    return (F.conv3d if D else F.conv2d), xg, wg, go, (want.detach(), xc.grad, wc.grad)


def _calls(monkeypatch, counted):
    """Count the C entry points the transforms of a run go through (F._wino_call) by name."""
    real = F._wino_call

    def spy(name, *a, **kw):
        counted[name] = counted.get(name, 0) + 1
        return real(name, *a, **kw)
    monkeypatch.setattr(F, "_wino_call", spy)


@pytest.mark.parametrize("route", ["f23_2d", "own_gemm"])
def test_whole_conv_f23_routes_match_float64(route, monkeypatch):
    """2-D F(2,3) (the default of the wide conv2d layers) and F(2,3)^3 with ssbev_wino_bgemm on two row blocks (T = 66), at the
    gates of test_winograd_conv2d_matches_aten / test_winograd_conv3d_matches_aten."""
    B, cin, cout, D, H, W = T.CONV_CASES[route]
    own = route == "own_gemm"
    monkeypatch.setattr(F, "WINO_OWN_GEMM", own)
    monkeypatch.setattr(F, "WINO_DEPTH_FUSED", False)
    conv, xg, wg, go, refs = _conv_problem(route)
    assert F.PRECISION == "fp32" and F.WINOGRAD
    assert F._WinoConv._plan(own, max(D, 1), H, W, False, cin)[:3] == ((0, "ssbev_wino_", 64) if own else (0, "ssbev_wino2d_", 16))
    counted, bg = {}, []
    _calls(monkeypatch, counted)
    real_bgemm = F._wino_bgemm
    monkeypatch.setattr(F, "_wino_bgemm", lambda V, *a: bg.append(V.shape[1]) or real_bgemm(V, *a))
    y = conv(xg, wg, None, 1, 1)
    y.backward(go.to(DEV))
    pre = "ssbev_wino_" if own else "ssbev_wino2d_"
    assert counted.get(pre + "input_transform") == 2 and counted.get(pre + "output_adjoint") == 1, counted
    assert bg == ([66, 66] if own else [])
    for name, got, ref, gate in zip(("y", "gx", "gw"), (y, xg.grad, wg.grad), refs, (2e-5, 2e-5, 5e-5)):
        err = (got.detach().cpu().double() - ref).abs().max().item()
        print(f"wino-stage conv/{route} {name}: max err {err:.3e} gate {gate * max(1.0, ref.abs().max().item()):.3e}")
        assert err < gate * max(1.0, ref.abs().max().item()), (name, err)


def test_whole_conv_f244_gemm_nn_matches_float64(monkeypatch):
    """F(2x4x4) transforms around gemm_nn: the default of the wide 3-D layers below WINO_DF_MIN_ROWS rows, at the gates of
    test_winograd_f43_tiles."""
    B, cin, cout, D, H, W = T.CONV_CASES["f244_gemm_nn"]
    conv, xg, wg, go, refs = _conv_problem("f244_gemm_nn")
    assert F.PRECISION == "fp32" and F.WINOGRAD and F.own_gemm_site("wino")
    assert not F._wino_df_applicable(B, D, H, W, cin, cout)
    assert F._WinoConv._plan(True, D, H, W, False, cin)[:3] == (1, "ssbev_wino43_", 144)
    counted, gemms = {}, []
    _calls(monkeypatch, counted)
    real_nn = F.gemm_nn
    monkeypatch.setattr(F, "gemm_nn", lambda a, b, **kw: gemms.append(tuple(a.shape)) or real_nn(a, b, **kw))
    y = conv(xg, wg, None, 1, 1)
    y.backward(go.to(DEV))
    assert counted.get("ssbev_wino43_input_transform") == 2 and counted.get("ssbev_wino43_output_adjoint") == 1, counted
    rows = B * (D // 2) * (H // 4) * (W // 4)
    assert gemms == [(144, rows, cin), (144, rows, cout)], gemms
    for name, got, ref in zip(("y", "gx", "gw"), (y, xg.grad, wg.grad), refs):
        a = got.detach().cpu().double()
        rel_max, rel_l2 = (a - ref).abs().max().item() / ref.abs().max().item(), ((a - ref).norm() / ref.norm()).item()
        print(f"wino-stage conv/f244_gemm_nn {name}: rel max {rel_max:.3e} rel l2 {rel_l2:.3e}")
        assert rel_max < 2e-4 and rel_l2 < 1e-4, (name, rel_max, rel_l2)
