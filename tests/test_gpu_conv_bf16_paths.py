"""GPU: every kernel, tile and epilogue of csrc/conv_bf16.hip against float64 ATen, through the C ABI.

The cases are conv_bf16_cases.CASES (test_conv_bf16_plan.py pins on the CPU which kernel, instance and chunking each one
reaches); every launch here uses the case's own ssbev_conv_dims, and the plan is queried and asserted again right before it, so
a run cannot silently test another kernel.  Operands are S.hash_normal / S.hash_uniform rounded to bf16; the reference is the
float64 ATen operator on the CPU on those same rounded tensors, computed once per shape and shared.

The bound is per element and needs no measurement: with exact bf16 x bf16 products (16 significant bits) summed in fp32 in any
order, one ulp per addition,  |got - ref| <= n 2^-23 A,  n the products per output and A the same convolution of |x| and |w| (plus
|bias| and the |old| value of an accumulating call).  A bf16 result adds its one rounding, 2^-8 |ref|.  Each test prints the plan
and its largest error / bound.

Sources sit inside NaN-filled buffers (a depth plane and more in front and behind), results carry NaN guards, the weight-gradient
workspace is NaN before the launch: a read outside the tensor that reaches a product, a store outside it or a partial slab that
was never written shows up as NaN.

The 256 x 32 and 128 x 32 tiles of conv_igemm16_kernel and forced stage depths are reachable in a tuning build only: nothing
here forces or tests them."""
import ctypes as C
import os

import pytest
import torch
import torch.nn.functional as TF

import conv_bf16_cases as T
from stereoscene_amd import capi
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
GUARD = 8192                          # elements; a multiple of 8, so that guarded tensors keep their 16-byte alignment
BF16, F32 = torch.bfloat16, torch.float32
FWD_CASES = [c for c in T.CASES if c.mode != T.WGRAD]
WGRAD_CASES = [c for c in T.CASES if c.mode == T.WGRAD]
IGEMM_CASES = [c for c in T.CASES if c.plan[0] == T.IGEMM16]
_operands = {}


@pytest.fixture(scope="module", autouse=True)
def release_operands():
    """The operands and float64 references are shared by every test of this module and given back after the last."""
    yield
    _operands.clear()
    torch.cuda.empty_cache()


def _r16(t):
    return t.to(BF16).double()


def _cl(t):
    """[B, C, D, H, W] -> channels-last [B, D, H, W, C], contiguous."""
    return t.permute(0, 2, 3, 4, 1).contiguous()


def _geom(d):
    k, s, p, dl = (d.kd, d.kh, d.kw), (d.sd, d.sh, d.sw), (d.pd, d.ph, d.pw), (d.dd, d.dh, d.dw)
    return k, s, p, dl, (d.Di, d.Hi, d.Wi), (d.Do, d.Ho, d.Wo)


def _forward64(x, w, d):
    k, s, p, dl, gi, go = _geom(d)
    if d.transposed:
        op = tuple(o - ((i - 1) * st - 2 * pd + l * (kk - 1) + 1) for i, o, kk, st, pd, l in zip(gi, go, k, s, p, dl))
        y = TF.conv_transpose3d(x, w, None, s, p, op, 1, dl)
    else:
        y = TF.conv3d(x, w, None, s, p, dl)
    assert tuple(y.shape[2:]) == go
    return y


def _dgrad64(gy, w, d):
    k, s, p, dl, gi, go = _geom(d)
    if d.transposed:
        gx = TF.conv3d(gy, w, None, s, p, dl)
    else:
        op = tuple(i - ((o - 1) * st - 2 * pd + l * (kk - 1) + 1) for i, o, kk, st, pd, l in zip(gi, go, k, s, p, dl))
        gx = TF.conv_transpose3d(gy, w, None, s, p, op, 1, dl)
    assert tuple(gx.shape[2:]) == gi
    return gx


def _wgrad64(x, gy, w, d):
    wv = w.clone().requires_grad_(True)
    return torch.autograd.grad(_forward64(x, wv, d), wv, gy)[0]


def operands(case):
    """Operands (bf16-representable, float64 on the CPU) of a case's shape, shared by its hints, modes and tests; ``ref(kind)``
    adds the float64 result and the |x| * |w| bound tensor of a mode on first use."""
    key = case.dims[:22]                                   # everything but relu, accumulate, tile_hint, precision
    if key not in _operands:
        d = T.dims_of(case)
        taps = d.kd * d.kh * d.kw
        wshape = ((d.Cin, d.Cout) if d.transposed else (d.Cout, d.Cin)) + (d.kd, d.kh, d.kw)
        o = {"x": _r16(S.hash_normal(f"c16/x{key}", (d.B, d.Cin, d.Di, d.Hi, d.Wi))),
             "gy": _r16(S.hash_normal(f"c16/gy{key}", (d.B, d.Cout, d.Do, d.Ho, d.Wo))),
             "w": _r16(S.hash_uniform(f"c16/w{key}", wshape, -1, 1) * (3.0 / (d.Cin * taps)) ** 0.5),
             "bias": (S.hash_normal(f"c16/b{key}", (d.Cout,)) * 0.1).double(),
             "old_y": _r16(S.hash_uniform(f"c16/oy{key}", (d.B, d.Cout, d.Do, d.Ho, d.Wo), -2, 2)),
             "old_gx": _r16(S.hash_uniform(f"c16/ox{key}", (d.B, d.Cin, d.Di, d.Hi, d.Wi), -2, 2))}
        o["w_dev"] = o["w"].float().to(DEV)
        _operands[key] = o
    return _operands[key]


def ref(case, kind):
    """(float64 reference, bound tensor A) of mode `kind`, channels-last (the weight gradient: the torch layout)."""
    o, d = operands(case), T.dims_of(case)
    if kind not in o:
        with torch.no_grad():
            if kind == T.FWD:
                o[kind] = (_cl(_forward64(o["x"], o["w"], d)), _cl(_forward64(o["x"].abs(), o["w"].abs(), d)))
            elif kind == T.DGRAD:
                o[kind] = (_cl(_dgrad64(o["gy"], o["w"], d)), _cl(_dgrad64(o["gy"].abs(), o["w"].abs(), d)))
        if kind == T.WGRAD:
            o[kind] = (_wgrad64(o["x"], o["gy"], o["w"], d), _wgrad64(o["x"].abs(), o["gy"].abs(), o["w"], d))
    return o[kind]


def guarded_source(t, halo):
    """channels-last bf16 copy of t [B, C, D, H, W] in the middle of a NaN-filled buffer."""
    g = (GUARD + halo + 7) // 8 * 8
    flat = _cl(t).reshape(-1)
    buf = torch.full((flat.numel() + 2 * g,), NAN, dtype=BF16, device=DEV)
    buf[g:g + flat.numel()].copy_(flat.to(BF16))
    return buf[g:g + flat.numel()]


def guarded_result(shape, dtype, old=None):
    """(whole buffer, view of the result, mask of the guards): NaN everywhere, or `old` (channels-last) inside the view."""
    n = 1
    for s in shape:
        n *= s
    buf = torch.full((n + 2 * GUARD,), NAN, dtype=dtype, device=DEV)
    view = buf[GUARD:GUARD + n]
    if old is not None:
        view.copy_(old.reshape(-1).to(dtype))
    return buf, view.view(shape)


def guards_intact(buf):
    return bool(torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[-GUARD:]).all())


def sync(case):
    """Wait for the launch; a GPU fault ends the whole session there (nothing more is started on a faulted device)."""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit(f"GPU fault in {T.case_id(case)}: {e}", returncode=3)


def check_plan(case, d, expect=True):
    p = T.query(d, case.mode)
    assert not isinstance(p, int), p
    if expect:
        assert T.plan_tuple(p) == case.plan, T.full_tuple(p)
    return p


def launch(case, precision=3, bias=False, relu=0, accumulate=0, batch=None, expect=True):
    """One forward / data-gradient launch through the C ABI -> (result [B, D, H, W, C] on the GPU, plan).  batch = b: the B = 1
    call on batch element b."""
    lib = capi.load()
    o = operands(case)
    mode = case.mode
    d = T.dims_of(case, precision, relu if mode == T.FWD else 0, accumulate, B=None if batch is None else 1)
    p = check_plan(case, d, expect and batch is None)
    sl = slice(None) if batch is None else slice(batch, batch + 1)
    src, old = (o["x"], o["old_y"]) if mode == T.FWD else (o["gy"], o["old_gx"])
    halo = src.shape[1] * src.shape[3] * src.shape[4] + src.shape[1] * (src.shape[4] + 1)        # a depth plane, a row, a voxel
    xs = guarded_source(src[sl], halo)
    shape = (d.B, d.Do, d.Ho, d.Wo, d.Cout) if mode == T.FWD else (d.B, d.Di, d.Hi, d.Wi, d.Cin)
    buf, y = guarded_result(shape, BF16 if precision == 2 else F32, _cl(old[sl]) if accumulate else None)
    wp = torch.zeros(lib.ssbev_conv_packed_weight_elems(C.byref(d)), dtype=F32, device=DEV)
    capi.check(lib.ssbev_conv_pack_weight(capi.ptr(o["w_dev"]), capi.ptr(wp), C.byref(d), mode, capi.stream()), "pack")
    if mode == T.FWD:
        b = o["bias"].float().to(DEV) if bias else None
        rc = lib.ssbev_conv_fwd_bf16(capi.ptr(xs), capi.ptr(wp), capi.ptr(b), capi.ptr(y), C.byref(d), capi.stream())
    else:
        rc = lib.ssbev_conv_bwd_data_bf16(capi.ptr(xs), capi.ptr(wp), capi.ptr(y), C.byref(d), capi.stream())
    capi.check(rc, T.case_id(case))
    sync(case)
    assert guards_intact(buf), "store outside the result"
    return y, p


def expected(case, bias=False, relu=0, accumulate=0):
    """(float64 reference, per-element fp32 summation bound) of an epilogue variant."""
    o, d = operands(case), T.dims_of(case)
    r, a = ref(case, case.mode)
    n = (d.Cin if case.mode == T.FWD else d.Cout) * d.kd * d.kh * d.kw
    if bias:
        r, a = r + o["bias"], a + o["bias"].abs()
    if accumulate:
        old = _cl(o["old_y"] if case.mode == T.FWD else o["old_gx"])
        r, a = r + old, a + old.abs()
    if relu:
        r = torch.relu(r)
    return r, n * 2.0 ** -23 * a


def worst_ratio(got, want, bound):
    got = got.double().cpu()
    assert not torch.isnan(got).any(), "NaN in the result: a guard was read, or an element was never written"
    return ((got - want).abs() / bound.clamp_min(1e-300)).max().item()


def variants(case):
    if case.mode == T.FWD:
        return [("plain", {}), ("bias", dict(bias=True)), ("bias+relu", dict(bias=True, relu=1)), ("accumulate", dict(accumulate=1))]
    return [("plain", {}), ("accumulate", dict(accumulate=1))]


@pytest.mark.parametrize("case", FWD_CASES, ids=T.case_id)
def test_fp32_result_is_within_the_summation_bound(case):
    y, p = launch(case, precision=3)
    want, bound = expected(case)
    ratio = worst_ratio(y, want, bound)
    print(f"conv16-path {T.case_id(case)} plain p3: plan {T.plan_tuple(p)} grid {p.grid} ratio {ratio:.4f}")
    assert ratio <= 1.0


@pytest.mark.parametrize("case", FWD_CASES, ids=T.case_id)
def test_bf16_result_is_the_rounded_fp32_result(case):
    """One round-to-nearest-even of the same fp32 value, bias and ReLU included."""
    kw = dict(bias=True, relu=1) if case.mode == T.FWD else {}
    p3 = check_plan(case, T.dims_of(case, 3, kw.get("relu", 0)))
    p2 = check_plan(case, T.dims_of(case, 2, kw.get("relu", 0)))
    assert T.full_tuple(p2) == T.full_tuple(p3)
    y32, _ = launch(case, precision=3, **kw)
    y16, p = launch(case, precision=2, **kw)
    print(f"conv16-path {T.case_id(case)} p2 == round(p3): plan {T.plan_tuple(p)}")
    assert not torch.isnan(y32).any()
    assert torch.equal(y16.view(torch.int16), y32.to(BF16).view(torch.int16))


@pytest.mark.parametrize("case", FWD_CASES, ids=T.case_id)
def test_epilogues_in_both_result_types(case):
    worst = 0.0
    for label, kw in variants(case):
        want, bound = expected(case, **kw)
        for prec in case.precisions:
            if prec == 3 and not kw:
                continue                                   # test_fp32_result_is_within_the_summation_bound
            y, p = launch(case, precision=prec, **kw)
            b = bound + 2.0 ** -8 * want.abs() if prec == 2 else bound
            ratio = worst_ratio(y, want, b)
            print(f"conv16-path {T.case_id(case)} {label} p{prec}: plan {T.plan_tuple(p)} grid {p.grid} ratio {ratio:.4f}")
            assert ratio <= 1.0, (label, prec)
            worst = max(worst, ratio)
    print(f"conv16-path-worst {T.case_id(case)} {worst:.4f}")


@pytest.mark.parametrize("case", IGEMM_CASES, ids=T.case_id)
def test_igemm16_is_bit_identical_to_gather16(case):
    """conv_igemm16_kernel sums every output over (tap, channel) in conv_gather16_kernel's order: every tile gives the same bits."""
    lib = capi.load()
    kw = dict(bias=True, relu=1) if case.mode == T.FWD else {}
    before = os.environ.get("SSBEV_IGEMM16")
    ys = {}
    for prec in case.precisions:
        ys[prec], p = launch(case, precision=prec, **kw)
    try:
        os.environ["SSBEV_IGEMM16"] = "0"
        lib.ssbev_env_refresh()                            # the library caches its switches
        for prec in case.precisions:
            y, pg = launch(case, precision=prec, expect=False, **kw)
            assert pg.kernel == T.GATHER16, T.full_tuple(pg)
            print(f"conv16-path {T.case_id(case)} p{prec}: {T.plan_tuple(p)} == {T.plan_tuple(pg)}")
            assert not torch.isnan(y).any() and torch.equal(y, ys[prec])
    finally:
        if before is None:
            del os.environ["SSBEV_IGEMM16"]
        else:
            os.environ["SSBEV_IGEMM16"] = before
        lib.ssbev_env_refresh()
    assert check_plan(case, T.dims_of(case)).kernel == T.IGEMM16


@pytest.mark.parametrize("case", FWD_CASES, ids=T.case_id)
def test_two_runs_and_the_batch_split_are_bit_identical(case):
    kw = dict(bias=True) if case.mode == T.FWD else {}
    first, p = launch(case, precision=2, **kw)
    second, _ = launch(case, precision=2, **kw)
    assert not torch.isnan(first).any() and torch.equal(first, second)
    if T.BATCH2 in case.props:
        halves = [launch(case, precision=2, batch=b, **kw) for b in (0, 1)]
        print(f"conv16-path {T.case_id(case)} batch split: {T.plan_tuple(p)} == 2 x {T.plan_tuple(halves[0][1])}")
        assert torch.equal(first, torch.cat([h[0] for h in halves]))


def launch_wgrad(case):
    lib = capi.load()
    o, d = operands(case), T.dims_of(case)
    p = check_plan(case, d)
    assert p.workspace == lib.ssbev_conv_bwd_weight_workspace(C.byref(d)) and p.workspace % 4 == 0
    halo = lambda t: t.shape[1] * t.shape[3] * t.shape[4] + t.shape[1] * (t.shape[4] + 1)
    xs, gs = guarded_source(o["x"], halo(o["x"])), guarded_source(o["gy"], halo(o["gy"]))
    buf, gw = guarded_result(tuple(o["w"].shape), F32)
    ws = torch.full((p.workspace // 4 + GUARD,), NAN, dtype=F32, device=DEV)
    rc = lib.ssbev_conv_bwd_weight_bf16(capi.ptr(xs), capi.ptr(gs), capi.ptr(gw), C.byref(d), capi.ptr(ws), p.workspace, capi.stream())
    capi.check(rc, T.case_id(case))
    sync(case)
    assert guards_intact(buf), "store outside gw"
    assert torch.isnan(ws[p.workspace // 4:]).all(), "store past the workspace"
    return gw, p


@pytest.mark.parametrize("case", WGRAD_CASES, ids=T.case_id)
def test_weight_gradient_is_within_the_summation_bound(case):
    d = T.dims_of(case)
    gw, p = launch_wgrad(case)
    want, a = ref(case, T.WGRAD)
    ratio = worst_ratio(gw, want, d.B * d.Do * d.Ho * d.Wo * 2.0 ** -23 * a)
    print(f"conv16-path {T.case_id(case)}: plan {T.plan_tuple(p)} grid {p.grid} workspace {p.workspace} ratio {ratio:.4f}")
    assert ratio <= 1.0
    again, _ = launch_wgrad(case)
    assert torch.equal(gw, again)
