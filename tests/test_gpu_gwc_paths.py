"""GPU: every forward kernel, backward realisation and chunk plan of csrc/gwc_warp.hip against the oracle on float64 data.

The cases are gwc_cases.CASES (test_gwc_plan.py pins on the CPU which kernels and chunk plan each one reaches, and that every
plan is a legal launch); the plan is queried and asserted again right before each launch, so a run cannot silently test another
kernel.  Forward and backward go through F.gwc_warp, the direct two-launch entry and the workspace refusals through the C ABI.
Reference, calibrations and the derived per-element bound gamma * A are described in gwc_cases.py; where A is zero (left of the
disparity, taps out of range, a non-finite calibration) the result must be exactly zero.  Each test prints its largest
error / bound (profiles/gwc_paths.txt keeps one run)."""
import ctypes as C

import pytest
import torch

import gwc_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
_refs = {}


@pytest.fixture(scope="module", autouse=True)
def release_references():
    """Operands and float64 references are computed once per (case, convention) and shared by the tests of this module."""
    yield
    _refs.clear()
    torch.cuda.empty_cache()


def operands(case, ac):
    key = (case.shape, case.cal, ac)
    if key not in _refs:
        B, Cc, G, H, W, D = case.shape
        L, R, go = T.features(case)
        calib = T.calibration(case)
        grads = case.bwd != 0
        o = dict(L=L, R=R, go=go, calib=calib)
        if case.fwd:
            o["ref"] = T.reference(L, R, go, calib, D, G, ac, grads)
            o["mag"] = T.magnitude(L, R, go, calib, D, G, ac, grads)
        _refs[key] = o
    return _refs[key]


def assert_plan(case, ac):
    p = T.query(T.dims(case.shape, ac))
    assert not isinstance(p, int), p
    assert (p.fwd_kernel, p.bwd_kernel, p.fwd_nchunks, p.bwd_nchunks) == (case.fwd, case.bwd, case.nf, case.nb), T.plan_tuple(p)
    return p


def ratio(got, ref, mag, n, what):
    """max error / (gamma(n) A); where the bound is zero the result is exactly zero, and everything is finite."""
    got = got.detach().double().cpu()
    assert torch.isfinite(got).all(), what
    err, bound = (got - ref).abs(), T.gamma(n) * mag
    zero = bound == 0
    assert (got[zero] == 0).all(), what
    return (err[~zero] / bound[~zero]).max().item() if (~zero).any() else 0.0


def run(case, ac, o):
    """forward (+ backward) through F.gwc_warp -> (volume, grad_left, grad_right), the gradients None without a backward kernel."""
    B, Cc, G, H, W, D = case.shape
    Lg, Rg = o["L"].to(DEV).requires_grad_(case.bwd != 0), o["R"].to(DEV).requires_grad_(case.bwd != 0)
    vol = F.gwc_warp(Lg, Rg, o["calib"].to(DEV), D, G, ac)
    if not case.bwd:
        return vol, None, None
    vol.backward(o["go"].to(DEV))
    return vol.detach(), Lg.grad, Rg.grad


def channels_last(case, o):
    """The C ABI's operands: left / right [B, H, W, C], grad_vol [B, D, H, W, G], calib."""
    return (o["L"].permute(0, 2, 3, 1).contiguous().to(DEV), o["R"].permute(0, 2, 3, 1).contiguous().to(DEV),
            o["go"].permute(0, 2, 3, 4, 1).contiguous().to(DEV), o["calib"].to(DEV))


RUNS = [(c, ac) for c in T.CASES for ac in c.acs]


@pytest.mark.parametrize("case,ac", RUNS, ids=lambda v: T.case_id(v) if isinstance(v, tuple) else f"ac{int(v)}")
def test_forward_and_backward_match_float64_within_the_derived_bound(case, ac):
    lib = capi.load()
    B, Cc, G, H, W, D = case.shape
    p = assert_plan(case, ac)
    o = operands(case, ac)
    tag = f"gwc-path {T.case_id(case)} ac{int(ac)} fwd={T.FWD_NAMES[p.fwd_kernel]}/{p.fwd_threads}t/{p.fwd_nchunks}ch " \
          f"bwd={T.BWD_NAMES[p.bwd_kernel]}/{p.bwd_threads}t/{p.bwd_nchunks}ch"
    if not case.fwd:                                   # no kernel fits the row: refused before anything is launched
        with pytest.raises(capi.SsbevError):
            run(case, ac, o)
        print(f"{tag} SSBEV_EINVAL")
        return
    with torch.set_grad_enabled(case.bwd != 0):
        vol, gl, gr = run(case, ac, o)
    nf = T.n_fwd(case.shape)
    rv = ratio(vol, o["ref"][0], o["mag"][0], nf, "vol")
    line = f"{tag} n_fwd {nf} vol {rv:.4f}"
    assert rv <= 1.0, line
    if T.NONFINITE in case.props or "n" in case.cal:
        dead = ~torch.isfinite(o["calib"])
        assert torch.count_nonzero(vol[dead.to(DEV)]) == 0 and torch.count_nonzero(vol[(~dead).to(DEV)]) > 0
    if not case.bwd:                                   # the wide rows: both backward entries refuse, nothing is launched
        l, r, g, cal = channels_last(case, o)
        out_l, out_r = torch.full_like(l, NAN), torch.full_like(r, NAN)
        args = (capi.ptr(g), capi.ptr(l), capi.ptr(r), capi.ptr(cal), capi.ptr(out_l), capi.ptr(out_r), C.byref(T.dims(case.shape, ac)))
        ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
        assert lib.ssbev_gwc_warp_bwd(*args, capi.stream()) == capi.EINVAL
        assert lib.ssbev_gwc_warp_bwd_fused(*args, capi.ptr(ws), ws.numel(), capi.stream()) == capi.EINVAL
        torch.cuda.synchronize()
        assert torch.isnan(out_l).all() and torch.isnan(out_r).all()
        print(f"{line} bwd SSBEV_EINVAL")
        return
    nb = T.n_bwd(case, p, ac)
    rl = ratio(gl, o["ref"][1], o["mag"][1], nb, "grad_left")
    rr = ratio(gr, o["ref"][2], o["mag"][2], nb, "grad_right")
    line += f" n_bwd {nb} gL {rl:.4f} gR {rr:.4f}"
    if T.DIRECT in case.props:                         # the two-launch entry at a bwd3 shape, against float64 and against bwd3
        l, r, g, cal = channels_last(case, o)
        dl, dr = torch.full_like(l, NAN), torch.full_like(r, NAN)
        capi.check(lib.ssbev_gwc_warp_bwd(capi.ptr(g), capi.ptr(l), capi.ptr(r), capi.ptr(cal), capi.ptr(dl), capi.ptr(dr),
                                          C.byref(T.dims(case.shape, ac)), capi.stream()), "ssbev_gwc_warp_bwd")
        nd = T.n_bwd(case, p, ac, T.BWD_TWO)
        for name, d, fused, k in (("gL", dl, gl, 1), ("gR", dr, gr, 2)):
            d = d.permute(0, 3, 1, 2)
            rd = ratio(d, o["ref"][k], o["mag"][k], nd, "direct " + name)
            both = ((d.double().cpu() - fused.double().cpu()).abs() - (T.gamma(nd) + T.gamma(nb)) * o["mag"][k]).max().item()
            line += f" direct(n {nd}) {name} {rd:.4f}"
            assert rd <= 1.0 and both <= 0.0, line
    print(line)
    assert rl <= 1.0 and rr <= 1.0, line


@pytest.mark.parametrize("case", [c for c in T.CASES if T.DETERMINISM in c.props], ids=T.case_id)
def test_two_runs_are_bit_identical(case):
    ac = case.acs[0]
    assert_plan(case, ac)
    o = operands(case, ac)
    first, second = run(case, ac, o), run(case, ac, o)
    for a, b in zip(first, second):
        assert torch.equal(a, b)


@pytest.mark.parametrize("case", [c for c in T.CASES if T.WORKSPACE in c.props], ids=T.case_id)
def test_short_or_missing_workspace_is_refused_before_any_launch(case):
    lib = capi.load()
    ac = case.acs[0]
    p = assert_plan(case, ac)
    assert p.bwd_nchunks > 1 and p.bwd_workspace > 0
    l, r, g, cal = channels_last(case, operands(case, ac))
    out_l, out_r = torch.full_like(l, NAN), torch.full_like(r, NAN)
    ws = torch.full((p.bwd_workspace // 4,), NAN, dtype=torch.float32, device=DEV)
    args = (capi.ptr(g), capi.ptr(l), capi.ptr(r), capi.ptr(cal), capi.ptr(out_l), capi.ptr(out_r), C.byref(T.dims(case.shape, ac)))
    assert lib.ssbev_gwc_warp_bwd_fused(*args, capi.ptr(ws), p.bwd_workspace - 1, capi.stream()) == capi.EWORKSPACE
    assert lib.ssbev_gwc_warp_bwd_fused(*args, None, p.bwd_workspace, capi.stream()) == capi.EWORKSPACE
    torch.cuda.synchronize()
    assert torch.isnan(out_l).all() and torch.isnan(out_r).all() and torch.isnan(ws).all()
