"""GPU: every product instance and plan of csrc/winograd_fused.hip, stage by stage, against float64 references.

The cases are wino_df_cases.CASES (test_wino_df_plan.py pins on the CPU which instance, chunk split, tails and dead waves each one
reaches); the plan is queried and asserted again right before every launch, so a run cannot silently test another kernel.  The
stages are driven through the C ABI on P, Z and w from synthetic.hash_*: every stage is linear in its inputs, so they need not be
real transforms.  Instances 22 / 23 of the contraction exist in tuning builds only and are not tested.

Definitions (float64, written out in torch below; nothing is shared with the kernels):

  U[fd][e][f][k][n] = sum_{d,h,w} G23[fd][d] G43[e][h] G43[f][w] g[n][k][d][h][w],   g = w (mode 0: K = Cin, N = Cout) or
                      g[n][k][d][h][w] = w[k][n][2-d][2-h][2-w] (mode 1: K = Cout, N = Cin; transposed, mirrored taps)
  pack:        Wp[xhw = 6 e + f][fd][q][kh][n][t] = U[fd][e][f][8 q + 4 kh + t][n], zero for k >= K and n >= N (K, N padded to 8, 32)
  contraction: for depth tile i, p0..p3 = planes 2i-1 .. 2i+2 of P[xhw] (zero outside [0, D)),
               v0 = p0 - p2, v1 = p1 + p2, v2 = p2 - p1, v3 = p1 - p3,  m_f = v_f U[f][xhw],
               Mo[xhw][plane 2i] = m0 + m1 + m2,  Mo[xhw][plane 2i+1] = m1 - m2 - m3
  weight gradient: g0, g1 = planes 2i, 2i+1 of Z[xhw],  z = (g0, g0 + g1, g0 - g1, -g1),
               gU[fd][xhw] = sum over (b, i, hw tile) of v_fd^T z_fd,   gw[n][k][d][h][w] = sum G23[fd][d] G43[e][h] G43[f][w] gU[fd][e][f][k][n]

Gate, per element: |got - ref| <= 2 (n + 8) 2^-24 A, where A is the same expression evaluated in float64 on absolute values
(|v|, |U|, |z|, |G|, every sign of the depth and G^T combinations positive) and n the number of terms summed into the element:
4 K for the contraction, 2 rows for the weight gradient (rows = B (D/2) Thw, the rows a frequency's product sums), 27 for the
pack.  That is the worst-case bound of fp32 summation in any order; one dropped k-step, row pair, plane or chunk is a missing
term of the size of A / n and exceeds it by orders of magnitude.  Each test prints its largest error / bound.

Every output (Mo, gw, Wp) is NaN before the launch and must be finite afterwards; it, and the weight-gradient workspace (sized
exactly to ssbev_wino43_df_wgrad_workspace), lie between guard bands of a fixed bit pattern that must be bit-identical
afterwards; every stage runs twice and must give the same bits."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as TF

import wino_df_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -24
GUARD = 1024                     # elements of a guard band (4 KiB: the buffers keep their 16-byte alignment)
PATTERN = 0x5A5AA5A5

G23 = ((1, 0, 0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0, 0, 1))
G43 = ((1 / 4, 0, 0), (-1 / 6, -1 / 6, -1 / 6), (-1 / 6, 1 / 6, -1 / 6), (1 / 24, 1 / 12, 1 / 6), (1 / 24, -1 / 12, 1 / 6), (0, 0, 1))


def mats(absolute=False):
    g23, g43 = (torch.tensor(m, dtype=torch.float64, device=DEV) for m in (G23, G43))
    return (g23.abs(), g43.abs()) if absolute else (g23, g43)


class Guarded:
    """`elems` float32 of NaN between two guard bands of PATTERN."""

    def __init__(self, elems):
        self.elems = elems
        self.raw = torch.full((elems + 2 * GUARD,), PATTERN, dtype=torch.int32, device=DEV)
        self.body = self.raw[GUARD:GUARD + elems].view(torch.float32)
        self.refill()

    def refill(self):
        self.body.fill_(float("nan"))

    def guards_intact(self):
        return bool((self.raw[:GUARD] == PATTERN).all()) and bool((self.raw[GUARD + self.elems:] == PATTERN).all())


def hashed(tag, shape, std=1.0):
    return S.hash_normal(tag, shape, std).to(DEV)


def weight_matrix(w64, mode, absolute=False):
    """U [4][6][6][K][N] of w64 [Cout][Cin][3][3][3] (absolute: |G| (x) |G| (x) |G| applied to |g|, the pack's bound)."""
    g = w64 if mode == 0 else w64.flip(2, 3, 4).transpose(0, 1)
    g23, g43 = mats(absolute)
    return torch.einsum("ad,be,cf,nkdef->abckn", g23, g43, g43, g.abs() if absolute else g)


def depth_planes(T5, ND, axis):
    """p0..p3 of every depth tile: planes 2i-1 .. 2i+2 along `axis` (zero outside [0, D)), each with ND entries along it."""
    t = T5.movedim(axis, 0)
    zero = torch.zeros_like(t[:1])
    pp = torch.cat([zero, t, zero])
    return [pp[a::2][:ND].movedim(0, axis) for a in range(4)]


def depth_inputs(p):
    return (p[0] - p[2], p[1] + p[2], p[2] - p[1], p[1] - p[3])


def worst_ratio(got, ref, bound):
    """(elements beyond the bound, largest |got - ref| / bound) on the device."""
    err = (got.double() - ref).abs()
    return (err > bound).sum(), (err / bound.clamp_min(1e-300)).max()


# ---------------------------------------------------------------------------------------------------------- contraction
def pack(lib, w, Cout, Cin, mode):
    """ssbev_wino43_df_pack into a guarded NaN buffer of ssbev_wino43_df_packed_elems floats."""
    wp = Guarded(lib.ssbev_wino43_df_packed_elems(Cout, Cin))
    capi.check(lib.ssbev_wino43_df_pack(capi.ptr(w), capi.ptr(wp.body), Cout, Cin, mode, capi.stream()), "ssbev_wino43_df_pack")
    return wp


@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.FWD], ids=T.case_id)
def test_contraction_matches_float64(case):
    lib = capi.load()
    B, K, N, D, H, W = case.shape
    Thw, ND = (H // 4) * (W // 4), D // 2
    R = B * D * Thw
    d, _ = T.wino_dims(case.shape)
    p = T.query(case.shape)
    assert T.case_plan(case, p) == case.plan, T.plan_tuple(p)
    P = hashed(f"wdfs/p{case.shape}", (36, R, K))
    P5 = P.view(36, B, D, Thw, K).double()
    mo = Guarded(36 * R * N)
    for mode in (0, 1):
        Cout, Cin = (N, K) if mode == 0 else (K, N)
        w = hashed(f"wdfs/w{mode}{case.shape}", (Cout, Cin, 3, 3, 3), (3.0 / (K * 27)) ** 0.5)
        wp = pack(lib, w, Cout, Cin, mode)
        runs = []
        for _ in range(2):
            mo.refill()
            capi.check(lib.ssbev_wino43_df_gemm(capi.ptr(P), capi.ptr(wp.body), capi.ptr(mo.body), C.byref(d), N, capi.stream()),
                       "ssbev_wino43_df_gemm")
            runs.append(mo.body.clone())
        assert wp.guards_intact() and mo.guards_intact()
        assert torch.isfinite(runs[0]).all()
        assert torch.equal(runs[0], runs[1])
        got = runs[0].view(36, B, D, Thw, N)
        U = weight_matrix(w.double(), mode).reshape(4, 36, K, N)
        bad, worst = torch.zeros((), dtype=torch.int64, device=DEV), torch.zeros((), dtype=torch.float64, device=DEV)
        for xhw in range(36):                                  # one frequency = one row slab of the reference at a time
            v = depth_inputs(depth_planes(P5[xhw], ND, 1))     # 4 x [B][ND][Thw][K]
            m = [v[f] @ U[f, xhw] for f in range(4)]
            a = [v[f].abs() @ U[f, xhw].abs() for f in range(4)]
            ref = torch.stack([m[0] + m[1] + m[2], m[1] - m[2] - m[3]], 2).reshape(B, D, Thw, N)
            A = torch.stack([a[0] + a[1] + a[2], a[1] + a[2] + a[3]], 2).reshape(B, D, Thw, N)
            nb, wr = worst_ratio(got[xhw], ref, 2 * (4 * K + 8) * EPS * A)
            bad, worst = bad + nb, torch.maximum(worst, wr)
        print(f"wino-df {T.case_id(case)} mode {mode}: instance {10 * p.mt + p.nw} grid {p.grid} nst {p.nst} "
              f"worst err / bound {worst.item():.4f}")
        assert bad.item() == 0, (mode, worst.item())


PACK_CASES = ((36, 32), (32, 36), (100, 32), (32, 100))      # (Cout, Cin): N = 36 and N = 100, and K = 36 and K = 100, in both modes


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("cout_cin", PACK_CASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_pack_matches_float64_and_pads_with_zeros(cout_cin, mode):
    lib = capi.load()
    Cout, Cin = cout_cin
    K, N = (Cin, Cout) if mode == 0 else (Cout, Cin)
    KPad, NPad = -(-K // 8) * 8, -(-N // 32) * 32
    used = 144 * KPad * NPad
    w = hashed(f"wdfs/pw{cout_cin}", (Cout, Cin, 3, 3, 3))
    first, second = pack(lib, w, Cout, Cin, mode), pack(lib, w, Cout, Cin, mode)
    assert first.guards_intact() and second.guards_intact()
    assert first.elems >= used and torch.isnan(first.body[used:]).all()          # nothing behind this mode's own layout is written
    assert torch.equal(first.body[:used], second.body[:used])
    got = first.body[:used].view(36, 4, KPad // 8, 2, NPad, 4)
    assert torch.isfinite(got).all()

    def layout(u):               # [4][6][6][K][N] -> [xhw][fd][q][kh][n][t], zero padded
        full = torch.zeros(4, 36, KPad, NPad, dtype=torch.float64, device=DEV)
        full[:, :, :K, :N] = u.reshape(4, 36, K, N)
        return full.view(4, 36, KPad // 8, 2, 4, NPad).permute(1, 0, 2, 3, 5, 4)

    ref, A = layout(weight_matrix(w.double(), mode)), layout(weight_matrix(w.double(), mode, absolute=True))
    live = layout(torch.ones(4, 6, 6, K, N, dtype=torch.float64, device=DEV)) > 0
    assert (~live).sum().item() == 144 * (KPad * NPad - K * N) > 0
    assert (got[~live] == 0).all()                                                # padded columns and k entries: exactly 0
    bad, worst = worst_ratio(got, ref, 2 * (27 + 8) * EPS * A)
    print(f"wino-df pack {Cout}x{Cin} mode {mode}: K {K} N {N} worst err / bound {worst.item():.4f}")
    assert bad.item() == 0, worst.item()


# ------------------------------------------------------------------------------------------------------ weight gradient
@pytest.mark.parametrize("case", [c for c in T.CASES if c.stage == T.WGRAD], ids=T.case_id)
def test_weight_gradient_matches_float64(case):
    lib = capi.load()
    B, K, N, D, H, W = case.shape
    Thw, ND = (H // 4) * (W // 4), D // 2
    R = B * D * Thw
    d, _ = T.wino_dims(case.shape)
    p = T.query(case.shape)
    assert T.case_plan(case, p) == case.plan, T.plan_tuple(p)
    assert p.w_workspace == lib.ssbev_wino43_df_wgrad_workspace(C.byref(d), N) and p.w_workspace % 4 == 0
    P, Z = hashed(f"wdfs/gp{case.shape}", (36, R, K)), hashed(f"wdfs/gz{case.shape}", (36, R, N))
    gw, ws = Guarded(N * K * 27), Guarded(p.w_workspace // 4)
    runs = []
    for _ in range(2):
        gw.refill()
        ws.refill()
        capi.check(lib.ssbev_wino43_df_wgrad(capi.ptr(P), capi.ptr(Z), capi.ptr(gw.body), C.byref(d), N, capi.ptr(ws.body),
                                             p.w_workspace, capi.stream()), "ssbev_wino43_df_wgrad")
        runs.append(gw.body.clone())
    assert gw.guards_intact() and ws.guards_intact()
    assert torch.isfinite(runs[0]).all()
    assert torch.isfinite(ws.body).all()                       # every chunk wrote every partial of its tiles
    assert torch.equal(runs[0], runs[1])
    v = depth_inputs(depth_planes(P.view(36, B, D, Thw, K).double(), ND, 2))
    Z5 = Z.view(36, B, D, Thw, N).double()
    g0, g1 = Z5[:, :, 0::2], Z5[:, :, 1::2]
    z = (g0, g0 + g1, g0 - g1, -g1)

    def reduce(vs, zs, absolute):
        gU = torch.stack([torch.einsum("xbitk,xbitn->xkn", a, b) for a, b in zip(vs, zs)]).view(4, 6, 6, K, N)
        g23, g43 = mats(absolute)
        return torch.einsum("ad,be,cf,abckn->nkdef", g23, g43, g43, gU)

    ref = reduce(v, z, False)
    A = reduce([t.abs() for t in v], [t.abs() for t in z], True)
    bad, worst = worst_ratio(runs[0].view(N, K, 3, 3, 3), ref, 2 * (2 * B * ND * Thw + 8) * EPS * A)
    print(f"wino-df {T.case_id(case)}: kernel <{p.w_kw},{p.w_nt},{p.w_br}> chunks {T.chunk_stages(p)} grid {p.w_grid} "
          f"worst err / bound {worst.item():.4f}")
    assert bad.item() == 0, worst.item()


def test_refusals_come_before_any_launch():
    T.check_return_codes()


# ----------------------------------------------------------------------------------------------------------- whole path
def _conv_run(x, w, go, df, monkeypatch):
    monkeypatch.setattr(F, "WINO_DF", df)
    monkeypatch.setattr(F, "WINO_DF_MIN_ROWS", 0)
    assert F._wino_df_applicable(x.shape[0], *x.shape[2:], x.shape[1], w.shape[0]) == df
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    timer = F.KernelTimer(families=set())
    F.KERNEL_TIMER = timer
    try:
        y = F.conv3d(xg, wg, None, 1, 1)
        y.backward(go.to(DEV))
    finally:
        F.KERNEL_TIMER = None
    fused = sum(c["launches"] for f, c in timer.counts.items() if f.split(":")[0] == "conv_wino_fused")
    assert fused == (2 if df else 0) and ("conv_wino_fused_wgrad" in timer.counts) == df
    return [t.detach().cpu().double() for t in (y, xg.grad, wg.grad)]


@pytest.mark.parametrize("case", T.CONV_CASES, ids=lambda c: "x".join(map(str, c)))
def test_whole_conv_matches_float64_conv3d(case, monkeypatch):
    """F.conv3d and its backward on the depth-fused path (weight gradient split in two chunks, see test_wino_df_plan.py) against
    float64 conv3d on the CPU.  The gate is measured, not on the depth-fused output: the same problem runs on the fp32
    F(2x4x4) pipeline of SSBEV_WINO_DF=0 (the same F(4,3) (h, w) transform constants, library GEMMs in between) in the same test,
    and every tensor of the depth-fused run may be at most 4x as far from the float64 reference (largest absolute error) as that
    pipeline is.  Measured on the MI355X, largest |error| of (y, gx, gw), fp32 pipeline -> depth-fused:
      (1, 64, 64, 34, 4, 4): y 2.35e-05 -> 2.60e-05, gx 2.28e-05 -> 2.92e-05, gw 5.09e-04 -> 3.75e-04
      (1, 96, 96, 34, 4, 4): y 3.40e-05 -> 3.34e-05, gx 4.14e-05 -> 4.18e-05, gw 3.98e-04 -> 3.48e-04"""
    B, Cin, Cout, D, H, W = case
    x = S.hash_normal(f"wdfs/cx{case}", (B, Cin, D, H, W))
    w = S.hash_uniform(f"wdfs/cw{case}", (Cout, Cin, 3, 3, 3), -1, 1) * (3.0 / (Cin * 27)) ** 0.5
    xc, wc = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = TF.conv3d(xc, wc, None, 1, 1)
    go = S.hash_normal(f"wdfs/cgo{case}", tuple(want.shape))
    want.backward(go.double())
    refs = [want.detach(), xc.grad, wc.grad]
    base = _conv_run(x, w, go, False, monkeypatch)
    got = _conv_run(x, w, go, True, monkeypatch)
    for name, a, b, r in zip(("y", "gx", "gw"), got, base, refs):
        err, floor = (a - r).abs().max().item(), (b - r).abs().max().item()
        print(f"wino-df conv {case} {name}: fp32 pipeline {floor:.3e} depth-fused {err:.3e} ratio {err / floor:.3f}")
        assert floor > 0 and torch.isfinite(a).all()
        assert err <= 4 * floor, (name, err, floor)
