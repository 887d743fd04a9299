"""GPU: every statistics, finalize and apply path of csrc/groupnorm.hip against a float64 reference.

The cases are norm_cases.CASES / DUAL_CASES (test_norm_plan.py pins on the CPU which loops, finalize batches, slabs and apply
trips each one reaches).  Single norms go through the C ABI (ssbev_groupnorm_fwd_ext / _bwd_ext) with the case's own
ssbev_norm_dims; the plan is queried and asserted again right before the launch, so a run cannot silently test another path.
Outputs, statistics, gradients, the ReLU mask and the workspace are NaN (the mask all ones) before each launch: a record, a lane or
a trip that is never written shows up.  The two-norm operator and the layer entry point go through stereoscene_amd.functional /
.layers, which allocate their own results.

Reference: plain tensor operations in float64 with autograd (mean, biased variance, affine, residual, ReLU), on the CPU; for
tensors above 4 M elements the same code runs on the device (ATen's double kernels share nothing with groupnorm.hip).  bf16 cases
are referenced on the bf16-rounded inputs.

Tolerances (the suite's own for these operators): 2e-5 max(1, max|want|) for outputs and statistics, 5e-5 max(1, max|want|) for
gradients, 1e-5 max(1, max|want|) for BatchNorm running statistics; tensors stored as bf16 add half an ulp, 2^-8 |want|.

The sign of the fused ReLU at an element whose float64 pre-activation lies within the output tolerance of zero is not decided by
the reference; there -- a few elements per million -- the reference gradient takes the sign the kernel's own forward stored, and
the backward pass is held to be consistent with it.  Every test prints its largest error / tolerance."""
import ctypes as C
import zlib

import pytest
import torch

import norm_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
EPS = 1e-5
BIG = 4 << 20             # elements above which inputs are drawn and the float64 reference is evaluated on the device
_data = {}


@pytest.fixture(scope="module", autouse=True)
def release_data():
    """Inputs are shared by every test of a case and given back to the allocator after the last."""
    yield
    _data.clear()
    torch.cuda.empty_cache()


def draw(tag, shape, dtype=torch.float32, scale=1.0, shift=0.0):
    """Seeded N(shift, scale^2) on the device, channels-last [B, S, C]; bf16: rounded once, here."""
    n = 1
    for s in shape:
        n *= s
    if n > BIG:
        g = torch.Generator(device=DEV)
        g.manual_seed(zlib.crc32(tag.encode()))
        t = torch.randn(shape, generator=g, device=DEV)
    else:
        t = S.hash_normal(tag, shape).to(DEV)
    return (t * scale + shift).to(dtype).contiguous()


def inputs(B, Cch, Sv, dtype, tag):
    key = (B, Cch, Sv, dtype, tag)
    if key not in _data:
        _data[key] = dict(x=draw(f"np/x{key}", (B, Sv, Cch), dtype, 1.5, 0.3), r=draw(f"np/r{key}", (B, Sv, Cch), dtype),
                          go=draw(f"np/go{key}", (B, Sv, Cch), dtype),
                          w=(1 + S.hash_uniform(f"np/w{key}", (Cch,), -0.3, 0.3)).to(DEV),
                          b=S.hash_uniform(f"np/b{key}", (Cch,), -0.2, 0.2).to(DEV))
    return _data[key]


def case_inputs(case):
    return inputs(case.B, case.C, T.spatial(case), torch.bfloat16 if case.dtype == "bf16" else torch.float32, case.id.split("-")[0])


def out_tol(want, bf16=False, k=2e-5):
    """Bound per element: k max(1, max|want|), plus half a bf16 ulp of the stored value for tensors stored as bf16."""
    t = k * max(1.0, want.abs().max().item())
    return want.abs() * 2.0 ** -8 + t if bf16 else torch.full_like(want, t)


def worst(got, want, tol):
    """Largest |got - want| / tol; a NaN anywhere in `got` is infinitely wrong."""
    ratio = (got.to(want.device).double() - want).abs() / tol
    return float("inf") if torch.isnan(ratio).any() else ratio.max().item()


def normalise(x, w, b, B, G, pre_act):
    """float64 GroupNorm of channels-last x [B, S, C] -> (n, mean [B * G], rstd [B * G], biased variance)."""
    Cch = x.shape[-1]
    u = torch.nn.functional.gelu(x) if pre_act else x
    v = u.reshape(B, -1, G, Cch // G)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    rstd = (var + EPS).rsqrt()
    n = ((v - mean) * rstd).reshape(x.shape) * w + b
    return n, mean.reshape(-1), rstd.reshape(-1), var.reshape(-1)


def reference(ts, B, G, relu, res, pre_act, got_y, bf16):
    """float64 forward and backward of relu?(GroupNorm(act?(x)) + r?) on the (already rounded) inputs; `B` is 1 for batch
    statistics.  -> dict of float64 tensors on the reference device."""
    dev = DEV if ts["x"].numel() > BIG else "cpu"
    x, r, w, b = (ts[k].to(dev).double().requires_grad_(True) for k in ("x", "r", "w", "b"))
    n, mean, rstd, var = normalise(x, w, b, B, G, pre_act)
    pre = n + r if res else n
    y = pre
    undecided = 0
    if relu:
        m = pre.detach() > 0
        near = pre.detach().abs() <= out_tol(pre.detach(), bf16)
        undecided = int(near.sum())
        m = torch.where(near, got_y.to(dev).reshape(pre.shape) > 0, m)
        y = pre * m
    y.backward(ts["go"].to(dev).double())
    out = dict(y=torch.relu(pre.detach()) if relu else pre.detach(), mean=mean.detach(), rstd=rstd.detach(), var=var.detach(),
               gx=x.grad, gw=w.grad, gb=b.grad, undecided=undecided)
    if res:
        out["gr"] = r.grad
    return out


def run_single(case, ts, relu, res, sign="mask", as_batch=False, running=None):
    """Forward and backward of one norm through the C ABI on poisoned buffers -> dict of device tensors."""
    lib = capi.load()
    d = T.dims(case, relu, as_batch)
    p = T.query(d)
    assert not isinstance(p, int), p
    if not as_batch:
        assert T.properties(case, p) == case.expect, T.plan_tuple(p)
    x, r, go = ts["x"], (ts["r"] if res else None), ts["go"]
    nstat = d.B * d.G
    y = torch.full_like(x, NAN)
    mean, rstd = (torch.full((nstat,), NAN, device=DEV) for _ in range(2))
    nws = lib.ssbev_groupnorm_workspace(C.byref(d))
    assert nws > 0
    use_mask = bool(relu) and sign == "mask"
    mask = torch.full((lib.ssbev_groupnorm_mask_words(C.byref(d)),), -1, dtype=torch.int64, device=DEV) if use_mask else None
    ext = capi.NormExt(None, None, 0.0, d.B * d.S)
    if running is not None:
        ext.running_mean, ext.running_var, ext.momentum = running[0].data_ptr(), running[1].data_ptr(), running[2]
    ws = torch.full((nws // 4 + 1,), NAN, device=DEV)
    capi.check(lib.ssbev_groupnorm_fwd_ext(capi.ptr(x), capi.ptr(ts["w"]), capi.ptr(ts["b"]), capi.ptr(r), capi.ptr(y), capi.ptr(mean),
                                           capi.ptr(rstd), capi.ptr(mask), C.byref(d), C.byref(ext), capi.ptr(ws), nws, capi.stream()),
               case.id)
    gx = torch.full_like(x, NAN)
    gr = torch.full_like(x, NAN) if res else None
    gw, gb = (torch.full((case.C,), NAN, device=DEV) for _ in range(2))
    ws = torch.full((nws // 4 + 1,), NAN, device=DEV)
    ext = capi.NormExt(None, None, 0.0, 0)
    capi.check(lib.ssbev_groupnorm_bwd_ext(capi.ptr(go), capi.ptr(x), capi.ptr(y) if relu and not use_mask else None, capi.ptr(mask),
                                           capi.ptr(ts["w"]), capi.ptr(mean), capi.ptr(rstd), capi.ptr(gx), capi.ptr(gr), capi.ptr(gw),
                                           capi.ptr(gb), C.byref(d), C.byref(ext), capi.ptr(ws), nws, capi.stream()), case.id)
    out = dict(y=y, mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb)
    if res:
        out["gr"] = gr
    return out


def check(got, want, bf16, label):
    """Every result against the reference; prints the worst error / tolerance per tensor."""
    ratios = {}
    for k in ("y", "mean", "rstd"):
        ratios[k] = worst(got[k].reshape(want[k].shape), want[k], out_tol(want[k], bf16 and k == "y"))
    for k in ("gx", "gr", "gw", "gb"):
        if k in want:
            ratios[k] = worst(got[k].reshape(want[k].shape), want[k], out_tol(want[k], bf16 and k in ("gx", "gr"), 5e-5))
    print(f"{label}: worst error / tolerance " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) +
          f" (ReLU sign taken from the kernel at {want['undecided']} elements)")
    assert max(ratios.values()) < 1.0, ratios
    return ratios


COMBOS = [(False, False), (True, False), (True, True), (False, True)]


def case_combos():
    for c in T.CASES:
        for relu, res in COMBOS if c.id != "F" else COMBOS[2:]:        # F (17 M elements): the fullest and the plainest combination
            yield pytest.param(c, relu, res, id=f"{c.id}-relu{int(relu)}-res{int(res)}")


@pytest.mark.parametrize("case,relu,res", case_combos())
def test_norm_fwd_bwd_vs_float64(case, relu, res):
    ts = case_inputs(case)
    bf16 = case.dtype == "bf16"
    got = run_single(case, ts, relu, res)
    want = reference(ts, case.B, case.G, relu, res, case.pre_act, got["y"], bf16)
    check(got, want, bf16, f"{case.id} relu={int(relu)} res={int(res)}")


@pytest.mark.parametrize("cid", ["A", "B-g1", "B-g2", "G"])
def test_relu_backward_from_the_saved_output(cid):
    """Backward without the bit mask: the ReLU's sign is read from the saved y (gn_partial_kernel's RM = 2 and the y branch of
    the apply kernel), as functional does under SSBEV_GN_RELU_MASK=0."""
    case = T.BY_ID[cid]
    ts = case_inputs(case)
    bf16 = case.dtype == "bf16"
    got = run_single(case, ts, True, True, sign="y")
    want = reference(ts, case.B, case.G, True, True, case.pre_act, got["y"], bf16)
    check(got, want, bf16, f"{cid} sign from y")


def test_functional_takes_the_saved_output_path_when_the_mask_is_off(monkeypatch):
    """The Python entry point of the same path: functional.group_norm with the mask switched off saves y and passes no mask."""
    case = T.BY_ID["B-g2"]
    ts = case_inputs(case)
    monkeypatch.setattr(F, "GN_RELU_MASK", False)
    sp = (case.B,) + case.sp + (case.C,)
    x, r = (F.from_cl(ts[k].view(sp)).detach().requires_grad_(True) for k in ("x", "r"))
    w, b = (ts[k].detach().clone().requires_grad_(True) for k in ("w", "b"))
    y = F.group_norm(x, case.G, w, b, EPS, residual=r, relu=True)
    y.backward(F.from_cl(ts["go"].view(sp)))
    got = dict(y=F.to_cl(y.detach()), gx=F.to_cl(x.grad), gr=F.to_cl(r.grad), gw=w.grad, gb=b.grad)
    want = reference(ts, case.B, case.G, True, True, None, got["y"].reshape(ts["x"].shape), False)
    got["mean"], got["rstd"] = want["mean"], want["rstd"]                # not returned by this entry point
    check(got, want, False, "B-g2 functional, sign from y")


@pytest.mark.parametrize("cid", ["A", "E1"])
@pytest.mark.parametrize("relu,res", [(True, True), (False, False)])
def test_train_mode_batchnorm_vs_float64(cid, relu, res):
    """The case's shape as a training-mode BatchNorm (statistics over batch and space, the per-channel finalize kernels) with
    the running statistics updated in the finalize kernel."""
    case = T.BY_ID[cid]
    ts = case_inputs(case)
    rm, rv = torch.zeros(case.C, device=DEV), torch.ones(case.C, device=DEV)
    got = run_single(case, ts, relu, res, as_batch=True, running=(rm, rv, 0.1))
    want = reference(ts, 1, case.C, relu, res, None, got["y"], False)
    check(got, want, False, f"{cid} batch norm relu={int(relu)} res={int(res)}")
    n = case.B * T.spatial(case)
    want_rm, want_rv = 0.1 * want["mean"], 0.9 + 0.1 * want["var"] * n / (n - 1)
    assert worst(rm, want_rm, out_tol(want_rm, k=1e-5)) < 1.0 and worst(rv, want_rv, out_tol(want_rv, k=1e-5)) < 1.0


@pytest.mark.parametrize("cid", ["B-g1", "B-g2", "C", "G"])
def test_two_runs_are_bit_identical(cid):
    case = T.BY_ID[cid]
    ts = case_inputs(case)
    one, two = run_single(case, ts, True, True), run_single(case, ts, True, True)
    for k in one:
        assert torch.equal(one[k], two[k]), k


def test_bf16_slices_of_a_row_stride_that_is_no_multiple_of_8():
    """What norm_cat does for branches of 32 and 12 channels, on bf16 tensors: each norm writes its channel slice of the [B, S, 44]
    output (ld_y) and reads its slice of the gradient (ld_gy).  88-byte rows rule out 16-byte lanes, so the 32-channel branch runs
    4 channels per lane.  (functional.norm_cat widens a bf16 concatenation with such a branch to fp32, so this path is reached
    through the C ABI only.)"""
    lib = capi.load()
    ctot, B = sum(T.CAT_CHANNELS), T.CAT_B
    Sv = T.CAT_SP[0] * T.CAT_SP[1] * T.CAT_SP[2]
    xs = [torch.ones(B, Cb, *T.CAT_SP, device=DEV, dtype=torch.bfloat16) for Cb in T.CAT_CHANNELS]
    assert F.norm_cat_supported(xs)
    out = torch.full((B, Sv, ctot), NAN, device=DEV, dtype=torch.bfloat16)
    go = draw("np/catgo", (B, Sv, ctot), torch.bfloat16)
    c0 = 0
    for Cb, G in zip(T.CAT_CHANNELS, T.CAT_GROUPS):
        ts = inputs(B, Cb, Sv, torch.bfloat16, "cat")
        d = capi.NormDims(B, Cb, G, Sv, EPS, 1, 0, 0, ctot, 0, 1)
        assert T.query(d).vw == 4
        mean, rstd = (torch.full((B * G,), NAN, device=DEV) for _ in range(2))
        mask = torch.full((lib.ssbev_groupnorm_mask_words(C.byref(d)),), -1, dtype=torch.int64, device=DEV)
        nws = lib.ssbev_groupnorm_workspace(C.byref(d))
        ws = torch.full((nws // 4 + 1,), NAN, device=DEV)
        before = out.clone()
        capi.check(lib.ssbev_groupnorm_fwd_ext(capi.ptr(ts["x"]), capi.ptr(ts["w"]), capi.ptr(ts["b"]), None,
                                               C.c_void_p(out.data_ptr() + 2 * c0), capi.ptr(mean), capi.ptr(rstd), capi.ptr(mask),
                                               C.byref(d), None, capi.ptr(ws), nws, capi.stream()), "cat fwd")
        y = out[..., c0:c0 + Cb]
        outside = torch.ones(ctot, dtype=torch.bool, device=DEV)
        outside[c0:c0 + Cb] = False
        assert torch.equal(out[..., outside].view(torch.int16), before[..., outside].view(torch.int16))     # nothing outside the slice
        d = capi.NormDims(B, Cb, G, Sv, EPS, 1, 0, 0, 0, ctot, 1)
        assert T.query(d).vw == 4
        gx = torch.full_like(ts["x"], NAN)
        gw, gb = (torch.full((Cb,), NAN, device=DEV) for _ in range(2))
        ws = torch.full((nws // 4 + 1,), NAN, device=DEV)
        capi.check(lib.ssbev_groupnorm_bwd_ext(C.c_void_p(go.data_ptr() + 2 * c0), capi.ptr(ts["x"]), None, capi.ptr(mask),
                                               capi.ptr(ts["w"]), capi.ptr(mean), capi.ptr(rstd), capi.ptr(gx), None, capi.ptr(gw),
                                               capi.ptr(gb), C.byref(d), None, capi.ptr(ws), nws, capi.stream()), "cat bwd")
        ref_in = dict(ts, go=go[..., c0:c0 + Cb].contiguous())
        want = reference(ref_in, B, G, True, False, None, y.contiguous(), True)
        check(dict(y=y.contiguous(), mean=mean, rstd=rstd, gx=gx, gw=gw, gb=gb), want, True, f"bf16 slice {c0}:{c0 + Cb} of {ctot}")
        c0 += Cb
    assert not torch.isnan(out.float()).any()


def dual_reference(case_or_dims, ts_a, ts_b, relu, got_y):
    B, Ga, Gb, a_batch, b_batch = case_or_dims
    xa, wa, ba = (ts_a[k].cpu().double().requires_grad_(True) for k in ("x", "w", "b"))
    xb, wb, bb = (ts_b[k].cpu().double().requires_grad_(True) for k in ("x", "w", "b"))
    na, mean_a, rstd_a, var_a = normalise(xa, wa, ba, 1 if a_batch else B, Ga, None)
    nb, mean_b, rstd_b, var_b = normalise(xb, wb, bb, 1 if b_batch else B, Gb, None)
    pre = na + nb
    y, undecided = pre, 0
    if relu:
        near = pre.detach().abs() <= out_tol(pre.detach())
        undecided = int(near.sum())
        y = pre * torch.where(near, got_y.cpu().reshape(pre.shape) > 0, pre.detach() > 0)
    y.backward(ts_a["go"].cpu().double())
    return dict(y=torch.relu(pre.detach()) if relu else pre.detach(), mean_a=mean_a.detach(), rstd_a=rstd_a.detach(),
                mean_b=mean_b.detach(), rstd_b=rstd_b.detach(), var_b=var_b.detach(), gxa=xa.grad, gwa=wa.grad, gba=ba.grad,
                gxb=xb.grad, gwb=wb.grad, gbb=bb.grad, undecided=undecided)


def check_dual(got, want, label):
    ratios = {k: worst(got[k].reshape(want[k].shape), want[k], out_tol(want[k], k=5e-5 if k.startswith("g") else 2e-5))
              for k in got}
    print(f"{label}: worst error / tolerance " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()) +
          f" (ReLU sign taken from the kernel at {want['undecided']} elements)")
    assert max(ratios.values()) < 1.0, ratios


@pytest.mark.parametrize("case", T.DUAL_CASES, ids=T.case_id)
def test_dual_norm_fwd_bwd_vs_float64(case):
    """relu?(N_a(xa) + N_b(xb)) with wide rows in gn2_partial_bwd_kernel: one voxel row per workgroup with idle threads, q = 256,
    q = 3; per-sample statistics and batch statistics (with the running-statistics update) on side b."""
    p = T.query(T.dual_dims(case))
    assert dict(q=case.C // p.vw, rows=T.rows(case.C // p.vw), chunks2=p.chunks2, chunk_len2=p.chunk_len2) == case.expect
    Sv = case.sp[0] * case.sp[1] * case.sp[2]
    ts_a, ts_b = inputs(case.B, case.C, Sv, torch.float32, "dual-a"), inputs(case.B, case.C, Sv, torch.float32, "dual-b")
    sp = (case.B,) + case.sp + (case.C,)
    xa, xb = (F.from_cl(t["x"].view(sp)).detach().requires_grad_(True) for t in (ts_a, ts_b))
    ps = [t[k].detach().clone().requires_grad_(True) for t in (ts_a, ts_b) for k in ("w", "b")]
    rm, rv = torch.zeros(case.C, device=DEV), torch.ones(case.C, device=DEV)
    y, (mean_a, rstd_a), (mean_b, rstd_b) = F.dual_norm(xa, ps[0], ps[1], case.Ga, EPS, xb, ps[2], ps[3], case.Gb, EPS, relu=case.relu,
                                                        a_batch=case.a_batch, b_batch=case.b_batch,
                                                        running_b=(rm, rv, 0.1) if case.b_batch else None)
    y.backward(F.from_cl(ts_a["go"].view(sp)))
    got = dict(y=F.to_cl(y.detach()), mean_a=mean_a, rstd_a=rstd_a, mean_b=mean_b, rstd_b=rstd_b, gxa=F.to_cl(xa.grad),
               gwa=ps[0].grad, gba=ps[1].grad, gxb=F.to_cl(xb.grad), gwb=ps[2].grad, gbb=ps[3].grad)
    want = dual_reference((case.B, case.Ga, case.Gb, case.a_batch, case.b_batch), ts_a, ts_b, case.relu, got["y"])
    check_dual(got, want, case.id)
    if case.b_batch:
        n = case.B * Sv
        want_rm, want_rv = 0.1 * want["mean_b"], 0.9 + 0.1 * want["var_b"] * n / (n - 1)
        assert worst(rm, want_rm, out_tol(want_rm, k=1e-5)) < 1.0 and worst(rv, want_rv, out_tol(want_rv, k=1e-5)) < 1.0


def test_layer_entry_point_falls_back_above_1024_channels():
    """C = 1028: dual_norm_supported refuses, and norm_pair still computes relu(GroupNorm(xa) + BatchNorm(xb))."""
    from stereoscene_amd.layers import BatchNorm3d, GroupNorm, norm_pair
    B, Cch, Ga, Gb, spd = T.DUAL_REFUSED
    Sv = spd[0] * spd[1] * spd[2]
    ts_a, ts_b = inputs(B, Cch, Sv, torch.float32, "dual-a"), inputs(B, Cch, Sv, torch.float32, "dual-b")
    sp = (B,) + spd + (Cch,)
    xa, xb = (F.from_cl(t["x"].view(sp)).detach().requires_grad_(True) for t in (ts_a, ts_b))
    assert not F.dual_norm_supported(xa, xb)
    gn, bn = GroupNorm(Ga, Cch).to(DEV), BatchNorm3d(Cch).to(DEV)
    with torch.no_grad():
        for t, v in zip((gn.weight, gn.bias, bn.weight, bn.bias), (ts_a["w"], ts_a["b"], ts_b["w"], ts_b["b"])):
            t.copy_(v)
    y = norm_pair(gn, xa, bn, xb, relu=True)
    y.backward(F.from_cl(ts_a["go"].view(sp)))
    got = dict(y=F.to_cl(y.detach()), gxa=F.to_cl(xa.grad), gwa=gn.weight.grad, gba=gn.bias.grad, gxb=F.to_cl(xb.grad),
               gwb=bn.weight.grad, gbb=bn.bias.grad)
    want = dual_reference((B, Ga, Gb, False, True), ts_a, ts_b, True, got["y"])
    check_dual(got, want, "norm_pair C=1028")
    n = B * Sv
    want_rm, want_rv = 0.1 * want["mean_b"], 0.9 + 0.1 * want["var_b"] * n / (n - 1)
    assert worst(bn.running_mean, want_rm, out_tol(want_rm, k=1e-5)) < 1.0
    assert worst(bn.running_var, want_rv, out_tol(want_rv, k=1e-5)) < 1.0
