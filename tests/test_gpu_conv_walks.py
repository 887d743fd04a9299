"""GPU: the row-walking convolution kernels on launches with MORE THAN ONE BLOCK PER CHUNK, against float64 ATen on the CPU.

conv_tapdh / conv_taph / conv_tap / conv_tap2 / conv_tap2up / wgrad_tapdh (fp32) and conv_tap16 (bf16 storage) keep an LDS ring
alive across the row groups of a workgroup's chunk: a `fresh` flag, ring slots, a restage at every plane crossing, old values and
bias parked beside the rows.  The small hinted cases of test_gpu_kernels.py all launch with one row group per chunk, so none of
that runs there.  The shapes here (conv_walk_cases.py; test_conv_walk_plan.py proves on the CPU that each one walks >= 2 row
groups per chunk with the listed properties) are the smallest that do: second blocks, plane(-pair) crossings inside a chunk,
chunks across two batch samples, short last chunks, grids that are no multiple of 8, and the ReLU + bias and accumulating
epilogues on later blocks.

Tolerances are the project's own for these kernels (test_conv_tap_split_lds_kernel, test_conv_bf16_storage_error_budget), against
a float64 reference.  Two checks need none: chunking must not change a forward or data-gradient value, so a batched call equals
its per-sample calls (other chunk boundaries, other ring history) bit for bit; and two runs of one call are bit-identical."""
import contextlib

import pytest
import torch
import torch.nn.functional as TF

import conv_walk_cases as T
from stereoscene_amd import capi
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"

_REF = {}       # (case, call name) -> inputs and float64 results, computed once and shared between the tests; never modified


def _r16(t):
    return t.to(torch.bfloat16).float()


def _conv64(call, x, w, b):
    if call["transposed"]:
        return TF.conv_transpose3d(x, w, b, 2, 1, 1)
    return TF.conv3d(x, w, b, call["stride"], 1)


def _problem(case, name):
    """Inputs (fp32, hash-filled, scaled as in test_conv_tap_split_lds_kernel) and the float64 forward / gradients of one call."""
    key = (case, name)
    if key in _REF:
        return _REF[key]
    call = T.calls(case)[name]
    cin, cout, tr = call["cin"], call["cout"], call["transposed"]
    tag = f"walk/{T.case_id(case)}/{name}"
    x = S.hash_normal(tag + "/x", (case.B, cin) + tuple(call["grid"]))
    if tr:
        w = S.hash_uniform(tag + "/w", (cin, cout, 3, 3, 3), -1, 1) * (3.0 / (cin * 27 / 8)) ** 0.5
    else:
        w = S.hash_uniform(tag + "/w", (cout, cin, 3, 3, 3), -1, 1) * (3.0 / (cin * 27)) ** 0.5
    b = S.hash_uniform(tag + "/b", (cout,), -0.5, 0.5)
    if case.kernel == "tap16":      # bf16 storage: the reference sees the same bf16-rounded tensors (test_gpu_bf16_storage.py)
        x, w = _r16(x), _r16(w)
    xd, wd, bd = (t.double().requires_grad_(True) for t in (x, w, b))
    y = _conv64(call, xd, wd, bd)
    go = S.hash_normal(tag + "/go", tuple(y.shape))
    if case.kernel == "tap16":
        go = _r16(go)
    y.backward(go.double())
    _REF[key] = dict(call=call, x=x, w=w, b=b, go=go, y=y.detach(), gx=xd.grad, gw=wd.grad, gb=bd.grad)
    return _REF[key]


@contextlib.contextmanager
def _forced(case, monkeypatch):
    """The tile hint (and storage mode) that puts the case on its kernel."""
    monkeypatch.setattr(F, "TILE_HINT", T.KERNELS[case.kernel][0])
    bf16 = case.kernel == "tap16"
    if bf16:
        monkeypatch.setattr(F, "WINO_BF16S", False)
        F.set_precision("bf16")
    try:
        yield
    finally:
        if bf16:
            F.set_precision("fp32")


def _dev(case, t):
    t = t.to(DEV)
    if case.kernel == "tap16" and t.dim() == 5:
        t = t.to(torch.bfloat16).contiguous(memory_format=torch.channels_last_3d)
    return t


def _conv(call, x, w, b, relu=False):
    if call["transposed"]:
        return F.conv_transpose3d(x, w, b, 2, 1, 1)
    return F.conv3d(x, w, b, call["stride"], 1, relu=relu)


def _run(case, p, x=None, go=None, bias=True, relu=False):
    """One forward + backward of the call on the GPU: (y, gx, gw, gb), detached."""
    xg = _dev(case, p["x"] if x is None else x).requires_grad_(True)
    wg = p["w"].to(DEV).requires_grad_(True)
    bg = p["b"].to(DEV).requires_grad_(True) if bias else None
    y = _conv(p["call"], xg, wg, bg, relu)
    y.backward(_dev(case, p["go"] if go is None else go))
    return y.detach(), xg.grad, wg.grad, (bg.grad if bias else None)


def _maxdiff(a, b):
    return (a.detach().double().cpu() - b).abs().max().item()


def _close(case, name, what, got, ref):
    """The project's bounds for these kernels, against the float64 reference."""
    assert got.shape == ref.shape, (name, what)
    if case.kernel == "tap16":      # test_conv_bf16_storage_error_budget: one bf16 rounding of y / gx; gw, gb are fp32 results
        d = got.detach().double().cpu() - ref
        rel_max, rel_l2 = d.abs().max().item() / ref.abs().max().item(), (d.norm() / ref.norm()).item()
        lim = {"y": (8e-3, 3e-3), "gx": (8e-3, 3e-3), "gw": (2e-4, 1e-4), "gb": (float("inf"), 1e-3)}[what]
        print(f"{T.case_id(case)} {name} {what}: rel max {rel_max:.3e} rel l2 {rel_l2:.3e}")
        assert rel_max < lim[0] and rel_l2 < lim[1], (name, what, rel_max, rel_l2)
        return
    tol = (2e-5 if what in ("y", "gx") else 5e-5) * max(1.0, ref.abs().max().item())
    err = _maxdiff(got, ref)
    print(f"{T.case_id(case)} {name} {what}: max err {err:.3e} tol {tol:.3e}")
    assert err < tol, (name, what, err, tol)


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_multi_block_walk_matches_float64_reference(case, monkeypatch):
    """Forward, data gradient (the same kernel with roles swapped; the opposite stride-2 kernel for conv_tap2 / conv_tap2up) and
    weight gradient (wgrad_tapdh_kernel on the conv_tapdh cases; the plan query says so in test_conv_walk_plan.py) of every call
    of the case against float64; run twice: identical bits; batched against per-sample calls: identical bits."""
    for name in T.calls(case):
        p = _problem(case, name)
        with _forced(case, monkeypatch):
            first = _run(case, p)
            again = _run(case, p)
            singles = [_run(case, p, p["x"][i:i + 1], p["go"][i:i + 1]) for i in range(case.B)] if case.B >= 2 else []
        for what, got in zip(("y", "gx", "gw", "gb"), first):
            assert torch.isfinite(got).all(), (name, what)
            _close(case, name, what, got, p[what])
        for what, a, b in zip(("y", "gx", "gw"), first, again):
            assert torch.equal(a, b), (name, what, "two runs differ")
        if singles:
            for i, what in enumerate(("y", "gx")):
                stacked = torch.cat([s[i] for s in singles])
                assert torch.equal(first[i], stacked), (name, what, "batched call differs from its per-sample calls",
                                                        (first[i].float() - stacked.float()).abs().max().item())


@pytest.mark.parametrize("case", [c for c in T.CASES if c.epilogues], ids=T.case_id)
def test_multi_block_walk_epilogues(case, monkeypatch):
    """Bias + fused ReLU in the forward, and the accumulating epilogue of the data gradient (a second consumer's gradient is
    already in the buffer: gradient slot, functional.fork), on launches whose chunks hold later blocks.  References: float64
    relu(conv + bias) and float64 `old + conv`."""
    names = ("down", "up") if case.kernel == "tap2" else ("conv",)
    for name in names:
        p = _problem(case, name)
        call = p["call"]
        if not call["transposed"]:
            # ---- bias + ReLU.  The backward of the fused form masks go with the sign of the STORED output, so the reference
            # gradients use the kernel's own mask; the two masks may differ only where the pre-activation is within the bound
            with _forced(case, monkeypatch):
                y, gx, gw, gb = _run(case, p, relu=True)
            z = p["y"]
            _close(case, name, "y", y, torch.relu(z))
            mask = (y > 0).cpu()
            tol = 2e-5 * max(1.0, z.abs().max().item())
            assert not ((mask != (z > 0)) & (z.abs() >= tol)).any(), (name, "ReLU mask")
            xd, wd = p["x"].double().requires_grad_(True), p["w"].double().requires_grad_(True)
            gm = p["go"].double() * mask
            _conv64(call, xd, wd, None).backward(gm)
            _close(case, name, "gx", gx, xd.grad)
            _close(case, name, "gw", gw, wd.grad)
            _close(case, name, "gb", gb, gm.sum((0, 2, 3, 4)))
        tag = f"walk/{T.case_id(case)}/{name}"
        if call["transposed"]:
            # ---- accumulate, conv_tap2_kernel as the data gradient of the transposed conv.  functional.conv_transpose3d hands
            # no gradient slot on, so this is the library call itself on a buffer that already holds `old`
            old = S.hash_normal(tag + "/old", tuple(p["x"].shape))
            with _forced(case, monkeypatch):
                d = F._conv_dims((case.B,) + tuple(call["grid"]) + (call["cin"],), tuple(p["w"].shape), (2, 2, 2), (1, 1, 1),
                                 (1, 1, 1), True, (1, 1, 1), accumulate=1)
                lib = capi.load()
                assert lib.ssbev_conv_kernel_class(F.C.byref(d), 1) == 7 and lib.ssbev_conv_chunk_groups(F.C.byref(d), 1) >= 2
                gcl, buf = F.to_cl(p["go"].to(DEV)), F.to_cl(old.to(DEV))
                wpt = F._packed(p["w"].to(DEV), d, 1)
                capi.check(lib.ssbev_conv_bwd_data(capi.ptr(gcl), capi.ptr(wpt), capi.ptr(buf), F.C.byref(d), capi.stream()),
                           "ssbev_conv_bwd_data")
            _close(case, name, "gx", F.from_cl(buf), old.double() + p["gx"])
            continue
        # ---- accumulate: two layers on the same kernel share their input; the second data gradient lands on the first one's
        w2 = S.hash_uniform(tag + "/w2", tuple(p["w"].shape), -1, 1) * 0.05
        go2 = S.hash_normal(tag + "/go2", tuple(p["go"].shape))
        hits = []
        slot_target = F._slot_target

        def spy(slot, like):
            into = slot_target(slot, like)
            hits.append(into is not None)
            return into

        monkeypatch.setattr(F, "_slot_target", spy)
        with _forced(case, monkeypatch):
            xa = p["x"].to(DEV).requires_grad_(True)
            a, b = F.fork(xa)
            ya, yb = _conv(call, a, p["w"].to(DEV), None), _conv(call, b, w2.to(DEV), None)
            torch.autograd.backward([ya, yb], [p["go"].to(DEV), go2.to(DEV)])
        monkeypatch.setattr(F, "_slot_target", slot_target)
        assert hits == [False, True], (name, hits)              # the second data gradient ran with accumulate = 1
        x2 = p["x"].double().requires_grad_(True)
        (old,) = torch.autograd.grad(_conv64(call, x2, w2.double(), None), x2, go2.double())
        _close(case, name, "gx", xa.grad, old + p["gx"])
