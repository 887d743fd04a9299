"""CPU: the float64 Winograd reference (wino_ref.py) is right, and the case table (wino_cases.py) is honest.

The reference is proved before test_gpu_wino_transforms.py measures a kernel against it: for each of the five tilings of
csrc/winograd.hip -- F(2,3)^3, 2-D F(2,3)^2, and F(4,3) over (h, w) with DA = 0, 2 and 4 outputs per tile along d --
transform, multiply and transform back is torch's float64 convolution (conv3d; conv2d with D as a batch axis for the two 2-D
tilings) to 1e-12 relative on a shape with distinct extents; mode 1 gives the data gradient, sum_t V (.) Z through weight_grad
the weight gradient; the adjoint pairs are adjoint.

The table: every case has exactly the properties it is listed for, recomputed from its dims and -- for the two frequency GEMMs
-- from ssbev_wino_gemm_plan_query, which answers from the functions the launchers read; every property has a case where it is
required; every ssbev_wino* entry point of capi.SIGNATURES is named by a case."""
import ctypes as C
import random

import pytest
import torch
import torch.nn.functional as TF

import wino_cases as T
import wino_ref as R
from stereoscene_amd import capi
from stereoscene_amd import synthetic as S

# (B, D, H, W) with distinct extents and more than one tile on every tiled axis; Cin = 3, Cout = 5
COMPOSE_DIMS = {"w3d": (2, 4, 6, 10), "w2d": (2, 3, 4, 10), "w43_2d": (2, 3, 8, 12), "w43": (2, 4, 8, 12), "w444": (2, 8, 4, 12)}
CIN, COUT = 3, 5


def _problem(tiling):
    B, D, H, W = COMPOSE_DIMS[tiling]
    taps = (R.families(tiling)[0].r, 3, 3)
    x = S.hash_normal(f"wref/x{tiling}", (B, D, H, W, CIN)).double()
    w = S.hash_normal(f"wref/w{tiling}", (COUT, CIN) + taps).double()
    go = S.hash_normal(f"wref/go{tiling}", (B, D, H, W, COUT)).double()
    return x, w, go


def _conv(x_cl, w):
    """float64 'same' convolution of a channels-last volume: conv3d for 3 depth taps, else conv2d on every plane."""
    x = x_cl.permute(0, 4, 1, 2, 3)
    return TF.conv3d(x, w, None, 1, (w.shape[2] // 2, 1, 1)).permute(0, 2, 3, 4, 1)


def _close(a, b, rel=1e-12):
    assert a.shape == b.shape
    assert (a - b).abs().max().item() <= rel * b.abs().max().item(), (a - b).abs().max().item() / b.abs().max().item()


@pytest.mark.parametrize("tiling", list(R.TILINGS))
def test_composition_is_the_float64_convolution(tiling):
    x, w, go = _problem(tiling)
    B, D, H, W = COMPOSE_DIMS[tiling]
    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    want = _conv(xr, wr)
    want.backward(go)
    V = R.input_transform(x, tiling)
    assert V.shape == (R.nfreq(tiling), R.ntiles(tiling, B, D, H, W), CIN)
    y = R.output_transform(R.bgemm(V, R.weight_transform(w, tiling, 0)), tiling, (B, D, H, W))
    _close(y, want.detach())
    # mode 1: the data gradient is the same pipeline on the incoming gradient
    gx = R.output_transform(R.bgemm(R.input_transform(go, tiling), R.weight_transform(w, tiling, 1)), tiling, (B, D, H, W))
    _close(gx, xr.grad)
    # the weight gradient: gU = sum over tiles of V (.) Z, then G^T gU G
    gU = torch.einsum("xtk,xtn->xkn", V, R.output_adjoint(go, tiling))
    _close(R.weight_grad(gU, tiling), wr.grad)
    if tiling in T.TWO_D:                    # the 2-D tilings take torch's 4-D weights and give them back
        w4 = w.squeeze(2)
        assert torch.equal(R.weight_transform(w4, tiling, 0), R.weight_transform(w, tiling, 0))
        assert torch.equal(R.weight_grad(gU, tiling, two_d=True), R.weight_grad(gU, tiling).squeeze(2))
        plane = TF.conv2d(x[1, 2].permute(2, 0, 1)[None], w4, None, 1, 1)[0].permute(1, 2, 0)       # D is a batch axis
        _close(y[1, 2], plane)


@pytest.mark.parametrize("tiling", list(R.TILINGS))
def test_adjoint_pairs(tiling):
    x, w, go = _problem(tiling)
    B, D, H, W = COMPOSE_DIMS[tiling]
    M = S.hash_normal(f"wref/m{tiling}", (R.nfreq(tiling), R.ntiles(tiling, B, D, H, W), COUT)).double()
    lhs, rhs = (R.output_adjoint(go, tiling) * M).sum(), (go * R.output_transform(M, tiling, (B, D, H, W))).sum()
    assert abs(lhs - rhs).item() <= 1e-12 * abs(rhs).item()
    gU = S.hash_normal(f"wref/gu{tiling}", (R.nfreq(tiling), CIN, COUT)).double()
    lhs, rhs = (R.weight_transform(w, tiling, 0) * gU).sum(), (w * R.weight_grad(gU, tiling)).sum()
    assert abs(lhs - rhs).item() <= 1e-12 * abs(rhs).item()


def test_depth_fused_product_and_pack_layout():
    """dgemm on (h, w)-transformed planes is the 3-D F(2,3)^3 pipeline; the packed layout holds U[xi][8 q + 4 kh + t][n]."""
    x, w, _ = _problem("w3d")
    B, D, H, W = COMPOSE_DIMS["w3d"]
    U = R.weight_transform(w, "w3d", 0)
    Mo = R.dgemm(R.input_transform(x, "w2d"), U, B, D)
    _close(R.output_transform(Mo, "w2d", (B, D, H, W)), _conv(x, w))
    Wp = R.dgemm_pack_layout(U)
    assert Wp.shape == (64, 1, 2, 32, 4)
    for xi, k, n in ((0, 0, 0), (17, 2, 4), (63, 1, 3)):
        assert Wp[xi, k // 8, (k // 4) % 2, n, k % 4] == U[xi, k, n]
    assert (Wp != 0).sum() == (U != 0).sum() and (Wp[:, :, :, COUT:] == 0).all() and (Wp[:, :, 1] == 0).all()


def test_magnitude_companions_and_chains():
    """|transform(x)| <= transform_abs(|x|) elementwise; a negated coefficient changes the result; the chain lengths."""
    for tiling in R.TILINGS:
        x, w, go = _problem(tiling)
        for fn, arg, which in ((R.input_transform, x, "Bt"), (R.output_adjoint, go, "At")):
            ref, mag = fn(arg, tiling), fn(arg, tiling, absolute=True)
            assert (ref.abs() <= mag * (1 + 1e-15)).all() and (mag > 0).any()
            wrong = fn(arg, tiling, negate=(2, 1, 2))
            assert (wrong - ref).abs().max() > 1e-3 * mag.max()
        U, Um = R.weight_transform(w, tiling, 0), R.weight_transform(w, tiling, 0, absolute=True)
        assert (U.abs() <= Um * (1 + 1e-15)).all()
    # F(2,3): B^T rows have two +-1 entries, A^T three, A two, G three halves, G^T (1, .5, .5, 0)
    assert (R.chain("w3d", "Bt"), R.chain("w3d", "At"), R.chain("w3d", "At", True)) == (3, 6, 3)
    assert (R.chain("w3d", "G"), R.chain("w3d", "G", True)) == (15, 12)
    # F(4,3): B^T row (0, -4, -4, 1, 1, 0): 3 + 2; A^T row (0, 1, -1, 8, -8, 1): 4 + 2; A row (1, 2, 4, 8): 3 + 3
    assert (R.chain("w43_2d", "Bt"), R.chain("w43_2d", "At"), R.chain("w43_2d", "At", True)) == (10, 12, 12)
    assert R.chain("w43", "Bt") == 11 and R.chain("w444", "Bt") == 15 and R.chain("w2d", "Bt") == 2
    assert R.N_DEPTH_DGEMM == 3


# ------------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_has_exactly_its_properties(case):
    if case.stage == T.TRANSFORM:
        assert T.threads(case) == case.plan
        assert T.transform_props(case) == case.props
        assert T.transform_entry(*case.what) == case.names[0]
    elif case.stage == T.WEIGHT:
        assert T.threads(case) == case.plan
        assert T.weight_props(case) == case.props
    else:
        p = T.query(case)
        assert not isinstance(p, int), p
        assert T.case_plan(case, p) == case.plan
        props = T.bgemm_props(case.shape, p) if case.stage == T.BGEMM else T.dgemm_props(case.shape, p)
        assert props == case.props, (sorted(props - case.props), sorted(case.props - props))
    for name in case.names:
        assert name in capi.SIGNATURES, name


def _props(cases):
    return set().union(*(c.props for c in cases)) if cases else set()


def test_every_required_property_has_a_case():
    tr = [c for c in T.CASES if c.stage == T.TRANSFORM]
    assert _props(tr) == T.TRANSFORM_PROPS
    for tiling, storages in T.STORAGES.items():
        for storage in storages:
            roles = (T.INPUT, T.OUTPUT, T.ADJOINT) + ((T.OUTPUT_ACC,) if storage == T.FP32 and tiling in T.ACC_TILINGS else ())
            for role in roles:
                mine = _props([c for c in tr if c.what == (tiling, role, storage)])
                need = {T.ONE_TILE, T.DISTINCT_EXTENTS, T.GRID_TAIL}
                if storage == T.BF16A:
                    need |= {T.ODD_C, T.EVEN_C, T.PACKED_MIN}
                if tiling in T.TWO_D:
                    need.add(T.BATCH_AXIS_D)
                if role == T.OUTPUT_ACC:
                    need.add(T.ACC)
                assert need <= mine, (tiling, role, storage, sorted(need - mine))
    # the packed and the single-channel `_bf16a` instance each meet a second workgroup
    for c_parity in (T.ODD_C, T.EVEN_C):
        assert all(any({c_parity, T.GRID_TAIL} <= c.props for c in tr if c.what == (tiling, role, T.BF16A))
                   for tiling in ("w3d", "w2d") for role in (T.INPUT, T.OUTPUT, T.ADJOINT))
    we = [c for c in T.CASES if c.stage == T.WEIGHT]
    assert _props(we) == T.WEIGHT_PROPS
    for (prefix, ndim), tiling in T.WEIGHT_TILINGS.items():
        fwd = _props([c for c in we if c.what[1:4] == (T.W_TRANSFORM, prefix, ndim)])
        grad = _props([c for c in we if c.what[1:4] == (T.W_GRAD, prefix, ndim)])
        assert fwd == T.WEIGHT_PROPS and grad == {T.RECT, T.W_GRID_TAIL}, (prefix, ndim)
        assert any(c.what[1:] == (T.W_TRANSFORM, prefix, ndim, 1) and T.W_GRID_TAIL in c.props for c in we)
    dg = [c for c in T.CASES if c.stage == T.DGEMM]
    assert _props(dg) == T.DGEMM_PROPS, sorted(T.DGEMM_PROPS - _props(dg))
    assert {c.plan[2] for c in dg if T.ROW_GROUPS in c.props} == {2, 5}                 # Thw = 33 and Thw = 129
    assert {c.plan[:2] for c in dg} == {(1, 2)}                                          # the product build's only instance
    bg = [c for c in T.CASES if c.stage == T.BGEMM]
    assert _props(bg) == T.BGEMM_PROPS, sorted(T.BGEMM_PROPS - _props(bg))
    assert {c.shape[0] for c in bg if T.ONE_PARTIAL_BLOCK in c.props} == {1, 63}
    assert {c.plan[0] for c in bg} == {1, 2}
    assert any({T.IDLE_WORKGROUP, T.K_ONE_QUAD} <= c.props and c.shape[2] <= 128 for c in bg)
    assert any({T.TWO_BLOCKS, T.K_RING_WRAP} <= c.props for c in bg) and any({T.TWO_BLOCKS, T.K_RING_REUSE} <= c.props for c in bg)


def test_every_wino_entry_point_is_named_by_a_case():
    named = {n for c in T.CASES for n in c.names}
    mine = {n for n in capi.SIGNATURES
            if n.startswith("ssbev_wino") and not n.startswith(T.FOREIGN_PREFIXES) and n not in T.FOREIGN_NAMES}
    assert mine - named == set(), sorted(mine - named)
    assert named - mine == set(), sorted(named - mine)
    assert len(mine) == 44


def test_whole_path_cases_reach_their_rows():
    B, ci, co, D, H, W = T.CONV_CASES["own_gemm"]
    assert B * (D // 2) * (H // 2) * (W // 2) >= 65
    p = T.query(T.Case(T.BGEMM, (), (B * (D // 2) * (H // 2) * (W // 2), ci, co), None, None, None))
    assert p.b_nrb == 2 and p.b_gx == 1


def test_query_matches_a_transcription_of_the_previous_launch_geometry_on_random_dims():
    """The geometry the two launchers computed inline moved into wino_bgemm_plan / wino_dgemm_plan without changing."""
    rng = random.Random(20261021)
    lib = capi.load()
    p = capi.WinoGemmPlan()
    for i in range(5000):
        Tr, K, N = int(2 ** rng.uniform(0, 17)), 4 * rng.randint(1, 160), rng.randint(1, 700)
        assert lib.ssbev_wino_gemm_plan_query(Tr, K, N, None, C.byref(p)) == capi.OK
        assert T.case_plan(T.Case(T.BGEMM, (), None, None, None, None), p) == T.reference_bgemm_plan(Tr, K, N), (Tr, K, N)
        assert (p.d_mt, p.d_nt, p.d_tgroups, p.d_grid_x, p.d_Q) == (0, 0, 0, 0, 0)
        dims = (rng.choice((1, 1, 2, 3)), 2 * rng.randint(1, 16), 2 * rng.randint(1, 40), 2 * rng.randint(1, 40), K)
        d = capi.WinoDims(*dims)
        assert lib.ssbev_wino_gemm_plan_query(0, 0, N, C.byref(d), C.byref(p)) == capi.OK
        assert T.case_plan(T.Case(T.DGEMM, (), None, None, None, None), p) == T.reference_dgemm_plan(*dims, N), (dims, N)
        assert (p.b_nt, p.b_gx, p.b_nrb) == (0, 0, 0)


def test_query_refuses_what_the_launchers_refuse():
    lib = capi.load()
    assert lib.ssbev_version() >= 124
    p = capi.WinoGemmPlan()
    fake = C.c_void_p(256)                    # never dereferenced: the launchers refuse on their arguments
    good = capi.WinoDims(1, 2, 4, 4, 8)
    assert lib.ssbev_wino_gemm_plan_query(64, 8, 32, C.byref(good), C.byref(p)) == capi.OK and p.b_nrb == 1 and p.d_tgroups == 1
    assert lib.ssbev_wino_gemm_plan_query(64, 8, 32, C.byref(good), None) == capi.EINVAL
    assert lib.ssbev_wino_gemm_plan_query(0, 8, 32, None, C.byref(p)) == capi.EINVAL
    for T_, K, N in ((64, 6, 32), (64, 0, 32), (64, 8, 0)):
        assert lib.ssbev_wino_gemm_plan_query(T_, K, N, None, C.byref(p)) == capi.EINVAL
        assert lib.ssbev_wino_bgemm(fake, fake, fake, T_, K, N, None) == capi.EINVAL
    for dims, N in (((1, 3, 4, 4, 8), 32), ((1, 2, 5, 4, 8), 32), ((1, 2, 4, 4, 6), 32), ((1, 2, 4, 4, 8), 0), ((0, 2, 4, 4, 8), 32)):
        d = capi.WinoDims(*dims)
        assert lib.ssbev_wino_gemm_plan_query(0, 0, N, C.byref(d), C.byref(p)) == capi.EINVAL, dims
        assert lib.ssbev_wino_dgemm(fake, fake, fake, C.byref(d), N, None) == capi.EINVAL, dims
    for null in range(3):
        a = [None if i == null else fake for i in range(3)]
        assert lib.ssbev_wino_bgemm(*a, 64, 8, 32, None) == capi.EINVAL
        assert lib.ssbev_wino_dgemm(*a, C.byref(good), 32, None) == capi.EINVAL
