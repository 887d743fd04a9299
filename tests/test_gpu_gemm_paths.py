"""GPU: every tile configuration, split and skinny path of csrc/gemm.hip against torch.matmul in float64.

The cases are gemm_cases.CASES (test_gemm_plan.py pins on the CPU which kernel, chunk count and tails each one reaches); every
launch here goes through the C ABI with the case's own ssbev_gemm_dims, and the plan is queried and asserted again right before
it, so a run cannot silently test another kernel.  Operands are S.hash_normal, tolerances the project's own from
test_gemm_nn_nt_tn_vs_torch: 2e-5 sqrt(K) for NN / NT, 2e-5 sqrt(R) for TN (times max(1, |ep_mul|max) under the fused epilogue).
Each test prints its largest error / tolerance: how far a summation-order bug of one chunk would have to move a result to be seen.

Operand rows beyond the dense width, the gaps of a strided C, a tail behind every output and the whole split-K / row-chunk
workspace are NaN before the launch: a read past K or N, a store outside the [batch][M][N] blocks, or a partial that was never
written shows up as NaN.

cfg 4 of gemm_nn_kernel (16-deep k stages) is reachable in a tuning build only; nothing here forces or tests it."""
import ctypes as C

import pytest
import torch

import gemm_cases as T
from stereoscene_amd import capi
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
_operands = {}


@pytest.fixture(scope="module", autouse=True)
def release_operands():
    """The operands and float64 references are shared by every test of this module and given back to the allocator after the last."""
    yield
    _operands.clear()
    torch.cuda.empty_cache()


def operands(case):
    """Dense operands and float64 references of a case's shape, computed once and shared by its forms, layouts and tests."""
    tn, ep = case.form == T.TN, T.EP_MUL in case.props
    key = (tn, ep, case.shape)
    if key not in _operands:
        batch, M, K, N = case.shape
        o = {"a": S.hash_normal(f"gp/a{case.shape}", (batch, M, K)).to(DEV)}
        if tn:
            o["b"] = S.hash_normal(f"gp/b2{case.shape}", (batch, M, N)).to(DEV)
            o["ref"] = torch.matmul(o["a"].double().transpose(1, 2), o["b"].double())
            if ep:
                o["em"] = S.hash_normal(f"gp/em{case.shape}", (batch, K, N)).to(DEV)
                o["rs"] = S.hash_normal(f"gp/rs{case.shape}", (batch, K)).to(DEV)
                o["ref_ep"] = o["em"].double() * (o["ref"] - o["rs"].double().unsqueeze(-1))
        else:
            o["b"] = S.hash_normal(f"gp/b{case.shape}", (batch, K, N)).to(DEV)
            o["w"] = o["b"].transpose(1, 2).contiguous()                       # NT reads [N][K]
            o["bias"] = S.hash_normal(f"gp/c{case.shape}", (N,)).to(DEV)
            o["ref"] = torch.matmul(o["a"].double(), o["b"].double())
            o["ref_shared"] = torch.matmul(o["a"].double(), o["b"][0].double())
        _operands[key] = o
    return _operands[key]


def place(t, ld, stride):
    """t [batch, rows, cols] laid out with leading dimension ld and batch stride `stride` in a NaN-filled buffer."""
    batch, rows, cols = t.shape
    buf = torch.full((max(batch * stride, (batch - 1) * stride + rows * ld) + 64,), NAN, dtype=torch.float32, device=DEV)
    buf.as_strided((batch, rows, cols), (max(stride, 1), ld, 1)).copy_(t)
    return buf


def launch(case, o, bias=None, relu=0, ep=False):
    """One launch through the C ABI -> (result view [batch][rows][N], whole output buffer, mask of the elements outside the view)."""
    lib = capi.load()
    batch, M, K, N = case.shape
    form = case.form
    d = T.case_dims(case, relu, (o["em"].data_ptr(), o["rs"].data_ptr()) if ep else None)
    assert (d.ep_mul is not None) == ep
    p = T.query(d, form)
    assert not isinstance(p, int), p
    assert (p.kernel, p.nchunk, p.per_chunk) == (case.kernel, case.nchunk, case.per_chunk), T.plan_tuple(p)
    b = o["w"] if form == T.NT else o["b"]
    if T.SHARED_B in case.props:
        b = b[:1]
    a_buf, b_buf = place(o["a"], d.lda, d.sa), place(b, d.ldb, d.sb)
    rows = K if form == T.TN else M
    out = torch.full((batch * d.sc + 64,), NAN, dtype=torch.float32, device=DEV)
    ws = torch.full((p.workspace // 4 + 1,), NAN, dtype=torch.float32, device=DEV)
    args = (capi.ptr(out), C.byref(d), capi.ptr(ws), p.workspace, capi.stream())
    if form == T.TN:
        rc = lib.ssbev_gemm_tn(capi.ptr(a_buf), capi.ptr(b_buf), *args)
    else:
        fn = lib.ssbev_gemm_nn if form == T.NN else lib.ssbev_gemm_nt
        rc = fn(capi.ptr(a_buf), capi.ptr(b_buf), capi.ptr(bias), *args)
    capi.check(rc, T.case_id(case))
    view = out.as_strided((batch, rows, N), (d.sc, d.ldc, 1))
    outside = torch.ones_like(out, dtype=torch.bool)
    outside.as_strided((batch, rows, N), (d.sc, d.ldc, 1)).fill_(False)
    return view, out, outside, p


def tolerance(case, o, ep=False):
    batch, M, K, N = case.shape
    if case.form != T.TN:
        return 2e-5 * K ** 0.5
    return 2e-5 * M ** 0.5 * (max(1.0, o["em"].abs().max().item()) if ep else 1.0)


def runs_of(case, o):
    """(label, launch keywords, float64 reference) of every epilogue the case is run with."""
    if case.form == T.TN:
        return [("ep_mul", dict(ep=True), o["ref_ep"])] if T.EP_MUL in case.props else [("plain", {}, o["ref"])]
    ref = o["ref_shared"] if T.SHARED_B in case.props else o["ref"]
    biased = ref + o["bias"].double()
    return [("plain", {}, ref), ("bias", dict(bias=o["bias"]), biased), ("bias+relu", dict(bias=o["bias"], relu=1), torch.relu(biased))]


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_forward_matches_float64_and_stores_stay_inside_c(case):
    o = operands(case)
    worst = 0.0
    for label, kw, ref in runs_of(case, o):
        view, out, outside, p = launch(case, o, **kw)
        tol = tolerance(case, o, "ep" in kw)
        err = (view.double() - ref).abs().max().item()
        print(f"gemm-path {T.case_id(case)} {label}: plan (kernel, tile, nchunk, per_chunk) = {T.plan_tuple(p)[:6]} grid {p.grid} "
              f"err {err:.3e} tol {tol:.3e} ratio {err / tol:.4f}")
        assert err < tol, (label, err, tol)              # (a NaN left in the view fails this comparison too)
        # the NaN canary: gaps between rows and batch elements of a strided C and the tail behind the last block are untouched
        assert outside.sum().item() >= 64 + (T.STRIDED_C in case.props) * (case.shape[1] * 5 + 7)
        assert torch.isnan(out[outside]).all(), label
        worst = max(worst, err / tol)
    print(f"gemm-path-worst {T.case_id(case)} {worst:.4f}")


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_two_runs_are_bit_identical(case):
    o = operands(case)
    label, kw, _ = runs_of(case, o)[-1]                  # bias + ReLU (in the sum pass of a split) / the TN epilogue of the case
    first = launch(case, o, **kw)[0]
    second = launch(case, o, **kw)[0]
    assert torch.equal(first, second), label
