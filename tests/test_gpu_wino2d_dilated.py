"""GPU: the strided-tile (dilated) 2-D Winograd F(2x2, 3x3) path -- ssbev_wino_dims.dil > 1 on the wino2d transform kernels
(csrc/winograd.hip), functional._WinoConv(dil) and the fp32 route of functional.conv2d -- against torch's conv2d in float64
on the CPU: forward, data gradient and weight gradient.

Shapes are the smallest at which the tiling can go wrong (tile rows x tile columns in brackets):
  7 x 10, d = 2    odd and even row counts per class, half-empty last tiles                      [4 x 6]
  9 x 11, d = 3    three classes of 3 / 3 / 3 rows and 4 / 4 / 3 columns                         [6 x 6]
  20 x 37, d = 18  classes of 2 and 1 rows, 3 and 2 columns: the ASPP d = 18 pattern in small    [18 x 19]
  4 x 13, d = 5    d > H: row class 4 is empty, every other one a single half-empty tile         [4 x 8]
Tolerances are those of test_gpu_kernels.py::test_winograd_conv2d_matches_aten (same transforms, same accumulation depth)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

from conftest import load_golden
from stereoscene_amd import functional as F
from stereoscene_amd import synthetic as S

pytestmark = pytest.mark.gpu
DEV = "cuda"

SHAPES = [(7, 10, 2), (9, 11, 3), (20, 37, 18), (4, 13, 5)]
CHANNELS = [(1, 64, 96), (2, 96, 64)]                     # (B, Cin, Cout)


def maxdiff(a, b):
    return (a.detach().cpu().double() - b.detach().cpu().double()).abs().max().item()


def problem(tag, B, Cin, Cout, H, W, d):
    """Seeded inputs and the float64 CPU reference (y, gx, gw) of the 3x3 / dilation d / padding d layer."""
    x = S.hash_normal(f"{tag}/x", (B, Cin, H, W))
    w = S.hash_uniform(f"{tag}/w", (Cout, Cin, 3, 3), -1, 1) * (3.0 / (Cin * 9)) ** 0.5
    go = S.hash_normal(f"{tag}/go", (B, Cout, H, W))
    xc, wc = x.double().requires_grad_(True), w.double().requires_grad_(True)
    want = TF.conv2d(xc, wc, None, 1, d, d)
    want.backward(go.double())
    return x, w, go, (want.detach(), xc.grad, wc.grad)


def check(got, ref):
    (y, gx, gw), (wy, wgx, wgw) = got, ref
    e = (maxdiff(y, wy), maxdiff(gx, wgx), maxdiff(gw, wgw))
    print("max abs errors y / gx / gw:", e, "of", wy.abs().max().item(), wgx.abs().max().item(), wgw.abs().max().item())
    assert y.shape == wy.shape and gx.shape == wgx.shape and gw.shape == wgw.shape
    assert e[0] < 2e-5 * max(1.0, wy.abs().max().item())
    assert e[1] < 2e-5 * max(1.0, wgx.abs().max().item())
    assert e[2] < 5e-5 * max(1.0, wgw.abs().max().item())


@pytest.mark.parametrize("chan", CHANNELS)
@pytest.mark.parametrize("shape", SHAPES)
def test_dilated_winograd_matches_float64_conv2d(shape, chan):
    (H, W, d), (B, Cin, Cout) = shape, chan
    x, w, go, ref = problem(f"wdil{shape}{chan}", B, Cin, Cout, H, W, d)
    xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
    timer = F.KERNEL_TIMER = F.KernelTimer()
    try:
        got = F._WinoConv.apply(xg.unsqueeze(2), wg.unsqueeze(2), None, d).squeeze(2)
        got.backward(go.to(DEV))
        tags = {tag for (_fam, tag) in timer.by_tag()}
    finally:
        F.KERNEL_TIMER = None
    assert any(t and t.startswith("wino fwd") and t.endswith(f" d{d}") for t in tags), tags
    check((got, xg.grad, wg.grad), ref)
    # the frequency buffers hold exactly the tiles of the formula
    T = B * F.wino2d_axis_tiles(H, d) * F.wino2d_axis_tiles(W, d)
    assert got.grad_fn is not None and T == B * {(7, 10, 2): 24, (9, 11, 3): 36, (20, 37, 18): 342, (4, 13, 5): 32}[shape]


def test_accumulating_output_transform_adds_only_inside_the_map():
    """ssbev_wino2d_output_transform_acc with dil > 1 (gradient slots): y += A^T M A on every position of the map, once."""
    import ctypes as C
    from stereoscene_amd import capi
    B, H, W, d, Cc = 2, 7, 10, 2, 64
    T = B * F.wino2d_axis_tiles(H, d) * F.wino2d_axis_tiles(W, d)
    M = S.hash_normal("wdil/acc/M", (16, T, Cc)).to(DEV)
    old = S.hash_normal("wdil/acc/y", (B, 1, H, W, Cc)).to(DEV)
    dims = capi.WinoDims(B, 1, H, W, Cc, d)
    fresh = F._wino_call("ssbev_wino2d_output_transform", M, dims, (B, 1, H, W, Cc))
    acc = old.clone()
    lib = capi.load()
    capi.check(lib.ssbev_wino2d_output_transform_acc(capi.ptr(M), capi.ptr(acc), C.byref(dims), capi.stream()), "acc")
    assert torch.equal(acc, fresh + old)


def test_dilation_one_is_bit_identical_to_the_kernels_before_the_dilation_parameter():
    """8 x 12, d = 1: y, gx and gw equal, bit for bit, what the commit before the dilation parameter computed on these inputs
    (tests/golden/wino2d_d1.npz, written by tools/make_golden_wino2d_d1.py on that commit) -- through functional.conv2d and
    with the dilation passed explicitly."""
    gold = load_golden("wino2d_d1")
    x = S.hash_normal("wino2d_d1/x", (1, 64, 8, 12))
    w = S.hash_uniform("wino2d_d1/w", (64, 64, 3, 3), -1, 1) * (3.0 / (64 * 9)) ** 0.5
    go = S.hash_normal("wino2d_d1/go", (1, 64, 8, 12))
    assert F._WinoConv._plan(False, 1, 8, 12, False)[1] == "ssbev_wino2d_"
    for explicit in (False, True):
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        if explicit:
            y = F._WinoConv.apply(xg.unsqueeze(2), wg.unsqueeze(2), None, 1).squeeze(2)
        else:
            y = F.conv2d(xg, wg, None, 1, 1, 1)
        y.backward(go.to(DEV))
        for name, t in (("y", y), ("gx", xg.grad), ("gw", wg.grad)):
            assert torch.equal(t.detach().cpu(), torch.from_numpy(gold[name])), (name, explicit)


def test_conv2d_route_and_polyphase_fallback_agree(monkeypatch):
    """functional.conv2d on 12 x 20, d = 6: the strided-tile route ([6 x 12] tiles against 6 x 10 undilated = 1.2x) and, with the
    route switched off, the polyphase batch of d*d sub-images; both against the float64 reference, and against each other."""
    B, Cin, Cout, H, W, d = 2, 96, 64, 12, 20, 6
    x, w, go, ref = problem("wdil/route", B, Cin, Cout, H, W, d)
    assert F.WINO_DILATED and F.WINO_DILATED_MAX_TILES == F.POLYPHASE_MAX_PAD + 0.05
    res = {}
    for route in (True, False):
        monkeypatch.setattr(F, "WINO_DILATED", route)
        xg, wg = x.to(DEV).requires_grad_(True), w.to(DEV).requires_grad_(True)
        assert F._wino_dilated_applicable(xg, wg, d) and F._dilated_polyphase(xg.detach(), wg.detach(), d) is not None
        timer = F.KERNEL_TIMER = F.KernelTimer()
        try:
            got = F.conv2d(xg, wg, None, 1, d, d)
            got.backward(go.to(DEV))
            tags = {tag for (_fam, tag) in timer.by_tag()}
        finally:
            F.KERNEL_TIMER = None
        # route on: one layer on the 12 x 20 map; off: the batch of 36 sub-images of 2 x 4
        assert (f"wino fwd {Cin}->{Cout} 1x{H}x{W} d{d}" in tags) == route, tags
        assert (f"wino fwd {Cin}->{Cout} 1x2x4" in tags) == (not route), tags
        res[route] = (got.detach(), xg.grad, wg.grad)
        check(res[route], ref)
    for a, b, tol in zip(res[True], res[False], (2e-5, 2e-5, 5e-5)):
        assert maxdiff(a, b) < tol * max(1.0, b.abs().max().item())


def test_route_precondition():
    """The ASPP branches (48 x 160, d = 6 / 12 / 18) take the route; a map whose classes are mostly half-empty tiles does not."""
    w = torch.empty(640, 640, 3, 3, device="meta")
    for d in (6, 12, 18):
        assert F._wino_dilated_applicable(torch.empty(1, 640, 48, 160, device="meta"), w, d)
    assert not F._wino_dilated_applicable(torch.empty(1, 640, 12, 40, device="meta"), w, 18)       # 12 x 22 tiles against 6 x 20
    assert not F._wino_dilated_applicable(torch.empty(1, 640, 48, 1000, device="meta"), w, 3)      # 501 tile columns > table
    assert np.isclose(30 * 88 / (24 * 80), 1.375)
