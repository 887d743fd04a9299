"""torch.autograd wrappers around the C ABI (stereoscene_amd.capi).  Host-side mirror of the
operator boundary the reference sits behind:

    voxel_index / pool_prepare / bev_pool  <-  VT:432-476 + mmdet3d.ops.bev_pool (VT:473)
    lift_splat                             <-  VT:517-523 fused
    gwc_warp                               <-  VT:104-114 + VT:128-156 fused
    conv_nd / conv_transpose_nd            <-  ATen conv3d / conv_transpose3d / conv2d call sites

Tensors are logical NC[D]HW (what the reference modules exchange) held in channels-last memory,
which is the layout the kernels read and write; nothing is permuted on the way in or out.
"""
import ctypes as C
import math
from typing import NamedTuple, Optional

import os

import numpy as np
import torch

from . import capi, streams

# -------------------------------------------------------------------------------------------------
# optional per-launch timing (bench.py's roofline leg): HIP events on the launch stream
# -------------------------------------------------------------------------------------------------


class KernelTimer:
    """Collects (kernel family, algorithmic flops, algorithmic bytes, executed flops) per C-ABI launch.  Families in
    ``families`` (None = all) are additionally bracketed by HIP events on the launch stream; the others are only
    COUNTED (no event traffic), which is what bench.py's whole-step roofline floor needs."""

    def __init__(self, families=None):
        self.records = []
        self.counts = {}              # family -> dict(launches, flops, bytes, executed): every span, timed or not
        self.families = families      # None = every instrumented family; a set restricts the event traffic

    def span(self, family, flops, nbytes=0.0, tag=None, executed=None):
        c = self.counts.setdefault(family, dict(launches=0, flops=0.0, bytes=0.0, executed=0.0))
        c["launches"] += 1
        c["flops"] += flops
        c["bytes"] += nbytes
        c["executed"] += flops if executed is None else executed
        if self.families is not None and family.split(":")[0] not in self.families:      # "family:instance" = one kernel symbol
            return _NOSPAN
        return _Span(self, family, flops, nbytes, tag, flops if executed is None else executed)

    def by_tag(self):
        """{(family, tag): dict(launches, flops, ms)} -- the per-layer table of tools/layer_table.py."""
        torch.cuda.synchronize()
        out = {}
        for fam, flops, nbytes, a, b, tag, ex in self.records:
            d = out.setdefault((fam, tag), dict(launches=0, flops=0.0, bytes=0.0, ms=0.0, executed=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["executed"] += ex
            d["ms"] += a.elapsed_time(b)
        return out

    def summary(self):
        torch.cuda.synchronize()
        out = {}
        for fam, flops, nbytes, a, b, _tag, ex in self.records:
            d = out.setdefault(fam, dict(launches=0, flops=0.0, bytes=0.0, ms=0.0, executed=0.0))
            d["launches"] += 1
            d["flops"] += flops
            d["bytes"] += nbytes
            d["executed"] += ex
            d["ms"] += a.elapsed_time(b)
        return out


class _Span:
    def __init__(self, timer, family, flops, nbytes, tag=None, executed=0.0):
        self.t, self.family, self.flops, self.nbytes, self.tag, self.executed = timer, family, flops, nbytes, tag, executed

    def __enter__(self):
        self.a = torch.cuda.Event(enable_timing=True)
        self.b = torch.cuda.Event(enable_timing=True)
        self.a.record()          # torch's current stream == the stream handed to the C ABI

    def __exit__(self, *exc):
        self.b.record()
        self.t.records.append((self.family, self.flops, self.nbytes, self.a, self.b, self.tag, self.executed))


class _NoSpan:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


KERNEL_TIMER = None
_NOSPAN = _NoSpan()


def _span(family, flops, nbytes=0.0, tag=None, executed=None):
    return KERNEL_TIMER.span(family, flops, nbytes, tag, executed) if KERNEL_TIMER is not None else _NOSPAN


def _conv_tag(d, role):
    return (f"{role:5s} {'T' if d.transposed else 'C'} {d.Cin:3d}->{d.Cout:3d} in {d.Di}x{d.Hi}x{d.Wi} "
            f"k{d.kd}{d.kh}{d.kw} s{d.sd}{d.sh}{d.sw} d{d.dd}{d.dh}{d.dw}")


def _conv_family(lib, d, mode, cls=None):
    """Span family of a direct conv launch: the <= 32-channel layers on conv_taph_kernel execute 2/3 of the operator's
    multiply-adds (F(2,3) along h), on conv_tapdh_kernel 4/9 (F(2,3) along d and h), which bench.py's executed-FLOP figure
    accounts for.  ``cls``: the kernel class of (d, mode) where the caller knows it (else it is asked, when a timer listens)."""
    if KERNEL_TIMER is None:
        return "conv_gather"
    cls = lib.ssbev_conv_kernel_class(C.byref(d), mode) if cls is None else cls
    return {2: "conv_tap_h", 9: "conv_tap_dh"}.get(cls, "conv_gather")


# conv_taph_kernel runs F(2,3) along h inside the direct kernel: 2/3 of the operator's multiply-adds are executed;
# conv_tapdh_kernel (round 4) F(2,3) along d and h: 4/9
_EXEC_DIV = {"conv_gather": 1.0, "conv_tap_h": 1.5, "conv_tap_dh": 2.25}


def conv_bytes(d):
    """Algorithmic bytes of one conv problem: every input, weight and output element touched once."""
    taps = d.kd * d.kh * d.kw
    return 4.0 * (d.B * d.Di * d.Hi * d.Wi * d.Cin + d.B * d.Do * d.Ho * d.Wo * d.Cout + taps * d.Cin * d.Cout)


def conv_flops(d):
    """Algorithmic flops (2*MAC) of one conv / deconv problem (any of fwd, dgrad, wgrad)."""
    taps = d.kd * d.kh * d.kw
    vox = d.B * (d.Di * d.Hi * d.Wi if d.transposed else d.Do * d.Ho * d.Wo)
    return 2.0 * vox * d.Cin * d.Cout * taps


# -------------------------------------------------------------------------------------------------
# layout helpers
# -------------------------------------------------------------------------------------------------


def to_cl(x):
    """Logical [B,C,*spatial] -> contiguous [B,*spatial,C] buffer (no copy if already channels-last)."""
    perm = (0,) + tuple(range(2, x.dim())) + (1,)
    return x.permute(perm).contiguous()


def from_cl(buf):
    """Contiguous [B,*spatial,C] buffer -> logical [B,C,*spatial] view (channels-last strides)."""
    n = buf.dim()
    return buf.permute((0, n - 1) + tuple(range(1, n - 1)))


def _f32(t, what):
    """Input of an fp32 operator.  In the bf16 storage mode a bf16 activation is widened here (an fp32 island: the autograd
    engine narrows the gradient the operator returns back to the input's dtype); anything else is an error."""
    if t.dtype == torch.bfloat16 and PRECISION == "bf16":
        return t.float()
    if t.dtype != torch.float32:
        raise capi.SsbevError(f"{what}: fp32 expected, got {t.dtype}")
    return t


def _act(t, what):
    """Input of an operator with fp32 AND bf16 kernels: returns (tensor, io_dtype code of the C ABI)."""
    if t.dtype == torch.bfloat16:
        return t, 1
    if t.dtype != torch.float32:
        raise capi.SsbevError(f"{what}: fp32 or bf16 expected, got {t.dtype}")
    return t, 0


_WS_NONE = {}


def _ws(nbytes, device):
    """Caller-owned workspace of an entry point.  Most calls need none (size 0: the kernels never touch the pointer); those share
    one 16-byte buffer per device instead of an allocator round trip each (~600 per step: tools/host_profile.py)."""
    n = int(nbytes)
    if n == 0:
        key = (device.type, device.index) if isinstance(device, torch.device) else device
        t = _WS_NONE.get(key)
        if t is None:
            t = _WS_NONE[key] = torch.empty(16, dtype=torch.uint8, device=device)
        return t
    return torch.empty(max(n, 16), dtype=torch.uint8, device=device)


# -------------------------------------------------------------------------------------------------
# frustum -> voxel scatter
# -------------------------------------------------------------------------------------------------


def _pool_dims(B, P, Cch, nx, ny, nz, origin=(0, 0, 0), dx=(1, 1, 1)):
    d = capi.PoolDims()
    d.B, d.P, d.C, d.nx, d.ny, d.nz = int(B), int(P), int(Cch), int(nx), int(ny), int(nz)
    for i in range(3):
        d.origin[i] = float(origin[i])
        d.dx[i] = float(dx[i])
    return d


def grid_origin(bx, dx):
    """fp32(bx - dx/2) computed in fp32 exactly as VT:441 does."""
    return (bx.detach().float().cpu() - dx.detach().float().cpu() / 2.0)


GEOM_FUSED = os.environ.get("SSBEV_GEOM_FUSED", "1") != "0"     # per-point chain of get_geometry in one kernel (0 = ATen passes)


def frustum_geometry(frustum, m1, t0, m2, t2, tr, m3, t3):
    """Per-point part of get_geometry (BD:123-156): frustum [D,H,W,3]; m1, m2 [B,N,3,3]; t0, tr (, t2) [B,N,3]; m3 [B,3,3]
    (, t3 [B,3]) -> geom [B,N,D,H,W,3], bit-identical to the broadcast tensor expression (ssbev_frustum_geometry)."""
    lib = capi.load()
    B, N = m1.shape[:2]
    D, H, W = frustum.shape[:3]
    dev = m1.device

    def c(t):
        return None if t is None else t.to(device=dev, dtype=torch.float32).contiguous()
    fr, m1, t0, m2, t2, tr, m3, t3 = (c(t) for t in (frustum, m1, t0, m2, t2, tr, m3, t3))
    out = torch.empty(B, N, D, H, W, 3, dtype=torch.float32, device=dev)
    d = capi.GeomDims(B, N, D, H, W)
    capi.check(lib.ssbev_frustum_geometry(capi.ptr(fr), capi.ptr(m1), capi.ptr(t0), capi.ptr(m2), capi.ptr(t2), capi.ptr(tr),
                                          capi.ptr(m3), capi.ptr(t3), capi.ptr(out), C.byref(d), capi.stream()),
               "ssbev_frustum_geometry")
    return out


def voxel_index(geom, bx, dx, nx, return_idx=False, grid_host=None):
    """geom [B, ..., 3] fp32 (cuda) -> vox int32 [B*P] (linear voxel or -1) [, idx3 int32 [B*P,3]].
    ``grid_host`` = (origin, dx, n) python lists, if the caller already holds host copies of the grid parameters."""
    lib = capi.load()
    B = geom.shape[0]
    g = _f32(geom, "voxel_index").reshape(B, -1, 3).contiguous()
    P = g.shape[1]
    if grid_host is None:
        grid_host = (grid_origin(bx, dx).tolist(), dx.detach().float().cpu().tolist(), [int(v) for v in nx.tolist()])
    origin, dxl, n = grid_host
    d = _pool_dims(B, P, 1, n[0], n[1], n[2], origin, dxl)
    vox = torch.empty(B * P, dtype=torch.int32, device=geom.device)
    idx3 = torch.empty(B * P, 3, dtype=torch.int32, device=geom.device) if return_idx else None
    capi.check(lib.ssbev_voxel_index(capi.ptr(g), capi.ptr(vox), capi.ptr(idx3), C.byref(d), capi.stream()),
               "ssbev_voxel_index")
    return (vox, idx3) if return_idx else vox


class _Order(torch.Tensor):
    """The `order` tensor of a CSR table carrying the compacted long-voxel list of ssbev_pool_prepare2 (`.long_list`), so that the
    (starts, order) pairs handed around by callers keep their shape."""
    long_list = None


def pool_prepare(vox, B, nx, ny, nz):
    """CSR table (starts int32 [NV+1], order int32 [n]) of the voxel -> ascending point lists; `order.long_list` (int32: count,
    then the ids of the voxels with more than 32 points) is the work list of the fused gather's long-list waves."""
    lib = capi.load()
    n = vox.numel()
    d = _pool_dims(B, max(n // max(B, 1), 0), 1, nx, ny, nz)
    nv = B * nx * ny * nz
    starts = torch.empty(nv + 1, dtype=torch.int32, device=vox.device)
    order = torch.empty(max(n, 1), dtype=torch.int32, device=vox.device).as_subclass(_Order)
    order.long_list = torch.empty(lib.ssbev_pool_long_list_elems(n), dtype=torch.int32, device=vox.device)
    ws = _ws(lib.ssbev_pool_prepare_workspace(n, C.byref(d)), vox.device)
    capi.check(lib.ssbev_pool_prepare2(capi.ptr(vox), n, capi.ptr(starts), capi.ptr(order), capi.ptr(order.long_list), C.byref(d),
                                       capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_pool_prepare2")
    return starts, order


class _BevPool(torch.autograd.Function):
    @staticmethod
    def forward(ctx, feats, coords, B, nz, nx, ny):
        lib = capi.load()
        feats = _f32(feats, "bev_pool").contiguous()
        n, Cch = feats.shape
        d = _pool_dims(B, 0, Cch, nx, ny, nz)
        c32 = coords.to(torch.int32).contiguous()
        vox = torch.empty(max(n, 1), dtype=torch.int32, device=feats.device)
        capi.check(lib.ssbev_coords_to_vox(capi.ptr(c32), n, capi.ptr(vox), C.byref(d), capi.stream()),
                   "ssbev_coords_to_vox")
        vox = vox[:n]
        starts, order = pool_prepare(vox, B, nx, ny, nz)
        out = torch.empty(B, nx, ny, nz, Cch, dtype=torch.float32, device=feats.device)
        capi.check(lib.ssbev_bev_pool_fwd(capi.ptr(feats), capi.ptr(starts), capi.ptr(order), capi.ptr(out),
                                          C.byref(d), capi.stream()), "ssbev_bev_pool_fwd")
        ctx.save_for_backward(vox)
        ctx.dims = (B, Cch, nx, ny, nz, n)
        # upstream returns [B, C, nz, nx, ny]
        return out.permute(0, 4, 3, 1, 2)

    @staticmethod
    def backward(ctx, gout):
        lib = capi.load()
        (vox,) = ctx.saved_tensors
        B, Cch, nx, ny, nz, n = ctx.dims
        g = gout.permute(0, 3, 4, 2, 1).contiguous()     # -> [B, nx, ny, nz, C]
        d = _pool_dims(B, 0, Cch, nx, ny, nz)
        gf = torch.empty(n, Cch, dtype=torch.float32, device=gout.device)
        capi.check(lib.ssbev_bev_pool_bwd(capi.ptr(g), capi.ptr(vox), n, capi.ptr(gf), C.byref(d), capi.stream()),
                   "ssbev_bev_pool_bwd")
        return gf, None, None, None, None, None


def bev_pool(feats, coords, B, D, H, W):
    """Drop-in for ``mmdet3d.ops.bev_pool.bev_pool(x, geom_feats, B, D, H, W)`` (VT:473):
    feats [n,C], coords [n,4]=(ix,iy,iz,b), D=nz, H=nx, W=ny -> [B, C, D, H, W]."""
    if feats.shape[0] != coords.shape[0]:
        raise ValueError("bev_pool: feats and coords disagree on the number of points")
    return _BevPool.apply(feats, coords, int(B), int(D), int(H), int(W))


# role-split gather over the compacted long-voxel list (round 4); SSBEV_GATHER_SPLIT=0: the one-kernel gather5
GATHER_SPLIT = os.environ.get("SSBEV_GATHER_SPLIT", "1") != "0"


class _LiftSplat(torch.autograd.Function):
    @staticmethod
    def forward(ctx, depth, feat, vox, starts, order, B, N, grid):
        lib = capi.load()
        nx, ny, nz = grid
        BN, D, H, W = depth.shape
        Cch = feat.shape[1]
        depth = _f32(depth, "lift_splat").contiguous()
        feat_cl = to_cl(_f32(feat, "lift_splat"))                 # [BN, H, W, C]
        d = _pool_dims(B, N * D * H * W, Cch, nx, ny, nz)
        l = capi.LiftDims(N, D, H * W)
        out = torch.empty(B, nx, ny, nz, Cch, dtype=torch.float32, device=depth.device)
        # algorithmic bytes: depth + features + the int32 voxel table in, the BEV volume out
        nby = 4.0 * (depth.numel() + feat_cl.numel() + order.numel() + starts.numel() + out.numel())
        with _span("lift_splat", 2.0 * depth.numel() * Cch, nby, f"fwd   lift_splat D={D} HW={H * W} C={Cch} grid={nx}x{ny}x{nz}"):
            capi.check(lib.ssbev_lift_splat_fwd2(capi.ptr(depth), capi.ptr(feat_cl), capi.ptr(starts), capi.ptr(order),
                                                 capi.ptr(getattr(order, "long_list", None) if GATHER_SPLIT else None),
                                                 capi.ptr(out), C.byref(d), C.byref(l), capi.stream()),
                       "ssbev_lift_splat_fwd2")
        ctx.save_for_backward(depth, feat_cl, vox)
        ctx.meta = (B, N, grid)
        return from_cl(out)                                       # logical [B, C, X, Y, Z]

    @staticmethod
    def backward(ctx, gout):
        lib = capi.load()
        depth, feat_cl, vox = ctx.saved_tensors
        B, N, (nx, ny, nz) = ctx.meta
        BN, D, H, W = depth.shape
        Cch = feat_cl.shape[-1]
        g = to_cl(gout)
        d = _pool_dims(B, N * D * H * W, Cch, nx, ny, nz)
        l = capi.LiftDims(N, D, H * W)
        gd = torch.empty_like(depth)
        gf = torch.empty_like(feat_cl)
        nby = 4.0 * (g.numel() + 2 * depth.numel() + 2 * feat_cl.numel() + vox.numel())
        with _span("lift_splat", 4.0 * depth.numel() * Cch, nby, f"bwd   lift_splat D={D} HW={H * W} C={Cch}"):
            capi.check(lib.ssbev_lift_splat_bwd(capi.ptr(g), capi.ptr(depth), capi.ptr(feat_cl), capi.ptr(vox),
                                                capi.ptr(gd), capi.ptr(gf), C.byref(d), C.byref(l), capi.stream()),
                       "ssbev_lift_splat_bwd")
        return gd, from_cl(gf), None, None, None, None, None, None


def lift_splat_tables(geom, bx, dx, nx, grid_host=None):
    """The frustum -> voxel tables of one geometry: (vox, starts, order).  They depend on the calibration only (SURVEY 8 row
    a10: "static -> cacheable"): a caller that sees the same calibration again can keep them (``lift_splat(tables=...)``)."""
    B = geom.shape[0]
    n = grid_host[2] if grid_host is not None else [int(v) for v in nx.tolist()]
    with torch.no_grad():
        vox = voxel_index(geom, bx, dx, nx, grid_host=grid_host)
        starts, order = pool_prepare(vox, B, n[0], n[1], n[2])
    return vox, starts, order


def lift_splat(depth_prob, img_feat, geom, bx, dx, nx, grid_host=None, tables=None):
    """Fused Lift+Splat: depth_prob [B*N,D,H,W], img_feat [B*N,C,H,W], geom [B,N,D,H,W,3]
    -> bev [B,C,X,Y,Z] (channels-last memory).  Equivalent of VT:517-523.  ``tables`` = lift_splat_tables(geom, ...) of a
    previous call with the same geometry (``geom`` may then be None)."""
    n = grid_host[2] if grid_host is not None else [int(v) for v in nx.tolist()]
    vox, starts, order = tables if tables is not None else lift_splat_tables(geom, bx, dx, nx, grid_host)
    B = starts.numel() // (n[0] * n[1] * n[2])
    N = depth_prob.shape[0] // B
    return _LiftSplat.apply(depth_prob, img_feat, vox, starts, order, B, N, tuple(n))


# -------------------------------------------------------------------------------------------------
# stereo cost volume
# -------------------------------------------------------------------------------------------------


class _GwcWarp(torch.autograd.Function):
    @staticmethod
    def forward(ctx, left, right, calib, ndisp, groups, align_corners):
        lib = capi.load()
        B, Cch, H, W = left.shape
        l = to_cl(_f32(left, "gwc_warp"))
        r = to_cl(_f32(right, "gwc_warp"))
        cal = calib.to(device=left.device, dtype=torch.float32).contiguous()
        d = capi.GwcDims(B, Cch, groups, ndisp, H, W, 1.0, int(bool(align_corners)))
        vol = torch.empty(B, ndisp, H, W, groups, dtype=torch.float32, device=left.device)
        nby = 4.0 * (l.numel() + r.numel() + vol.numel())        # read both feature maps, write the volume
        with _span("gwc_warp_fwd", 8.0 * vol.numel() * (Cch // groups), nby, f"fwd   gwc_warp D={ndisp} {H}x{W} G={groups}"):
            capi.check(lib.ssbev_gwc_warp_fwd(capi.ptr(l), capi.ptr(r), capi.ptr(cal), capi.ptr(vol), C.byref(d),
                                              capi.stream()), "ssbev_gwc_warp_fwd")
        ctx.save_for_backward(l, r, cal)
        ctx.meta = (ndisp, groups, int(bool(align_corners)))
        return from_cl(vol)                                       # logical [B, G, D, H, W]

    @staticmethod
    def backward(ctx, gvol):
        lib = capi.load()
        l, r, cal = ctx.saved_tensors
        ndisp, groups, ac = ctx.meta
        B, H, W, Cch = l.shape
        g = to_cl(gvol)
        d = capi.GwcDims(B, Cch, groups, ndisp, H, W, 1.0, ac)
        gl = torch.empty_like(l)
        gr = torch.empty_like(r)
        nby = 4.0 * (g.numel() + 2 * l.numel() + 2 * r.numel())  # the gradient volume ONCE + both maps in, both gradients out
        with _span("gwc_warp_bwd", 16.0 * g.numel() * (Cch // groups), nby, f"bwd   gwc_warp D={ndisp} {H}x{W} G={groups}"):
            ws = _ws(lib.ssbev_gwc_warp_bwd_workspace(C.byref(d)), g.device)
            capi.check(lib.ssbev_gwc_warp_bwd_fused(capi.ptr(g), capi.ptr(l), capi.ptr(r), capi.ptr(cal), capi.ptr(gl),
                                                    capi.ptr(gr), C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_gwc_warp_bwd_fused")
        return from_cl(gl), from_cl(gr), None, None, None, None


def gwc_warp(left, right, calib, ndisp, groups=32, align_corners=True):
    """Fused ``build_gwc_volume`` + ``warp`` (VT:104-156): left/right [B,C,H,W], calib [B]
    -> volume [B, G, ndisp, H, W] sampled at metric depths 1..ndisp."""
    return _GwcWarp.apply(left, right, calib, int(ndisp), int(groups), align_corners)


# -------------------------------------------------------------------------------------------------
# gradient slots: one gradient buffer for all consumers of a multi-consumer activation
# -------------------------------------------------------------------------------------------------
# An activation with two consumers (the input of an hourglass feeds its stride-2 conv and its 1x1 redirect; a residual
# block's input feeds the first conv and the closing add) gets its gradient from autograd as the SUM of two tensors: one
# elementwise pass over three 189 MB tensors per such activation on the cost volume (7 per step, 1.3 ms with the narrower
# levels).  ``fork`` hands every consumer an alias of the activation carrying a shared ``GradSlot``; in backward the first
# consumer leaves its gradient tensor in the slot, the next ones run their data-gradient kernel with ``accumulate = 1`` INTO
# that buffer (the kernels add in their epilogue) and return the same tensor, and ``_Fork.backward`` counts a buffer once.
# Consumers that do not know about slots still work: their gradient is a different tensor and is added as before.
GRAD_SLOTS = os.environ.get("SSBEV_GRAD_SLOTS", "1") != "0"


class GradSlot:
    __slots__ = ("buf",)

    def __init__(self):
        self.buf = None


class _Fork(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, slot, n):
        ctx.slot = slot
        return tuple(x.view_as(x) for _ in range(n))

    @staticmethod
    def backward(ctx, *gs):
        ctx.slot.buf = None
        uniq = []
        for g in gs:
            # same buffer = same gradient (strides are not compared: those of size-1 axes are arbitrary)
            if g is not None and not any(g.data_ptr() == u.data_ptr() and g.shape == u.shape for u in uniq):
                uniq.append(g)
        total = None
        for g in uniq:
            total = g if total is None else total + g
        return total, None, None


def fork(x, n=2):
    """``n`` aliases of ``x`` for ``n`` consumers whose data gradients should meet in one buffer (see above)."""
    if not (GRAD_SLOTS and x.is_cuda and x.requires_grad and torch.is_grad_enabled()):
        return (x,) * n
    slot = GradSlot()
    outs = _Fork.apply(x, slot, n)
    for o in outs:
        o._ssbev_grad_slot = slot
    return outs


class _SpatialMean(torch.autograd.Function):
    """x.mean over the spatial axes of a channels-last volume, [B, C].  Its data gradient is a per-channel constant: with a
    gradient slot it is ADDED into the buffer another consumer has already filled (one in-place pass) instead of being
    materialised as a full tensor and added by autograd (CA3D's squeeze step on the 189 MB activation, ATT:100-104)."""

    @staticmethod
    def forward(ctx, x, slot):
        ctx.slot, ctx.shape, ctx.dtype = slot, tuple(x.shape), x.dtype
        return to_cl(x).mean(dim=tuple(range(1, x.dim() - 1)), dtype=torch.float32)     # fp32 vector also for bf16 activations

    @staticmethod
    def backward(ctx, g):
        B, Cch = ctx.shape[0], ctx.shape[1]
        sp = ctx.shape[2:]
        n = 1
        for v in sp:
            n *= v
        gb = (g / float(n)).view((B,) + (1,) * len(sp) + (Cch,))
        buf = ctx.slot.buf if ctx.slot is not None else None
        if buf is not None and buf.is_contiguous() and buf.numel() == B * n * Cch and buf.shape[-1] == Cch and buf.shape[0] == B:
            tgt = buf.view((B,) + sp + (Cch,))
            tgt.add_(gb)
            return from_cl(tgt), None
        full = gb.to(ctx.dtype).expand((B,) + sp + (Cch,)).contiguous()
        if ctx.slot is not None:
            ctx.slot.buf = full
        return from_cl(full), None


def spatial_mean(x):
    """[B, C, *spatial] -> [B, C] mean; slot-aware (see _SpatialMean)."""
    if not (x.is_cuda and x.requires_grad and torch.is_grad_enabled()):
        return x.mean(dim=tuple(range(2, x.dim())), dtype=torch.float32 if x.dtype in (torch.bfloat16, torch.float16) else None)
    return _SpatialMean.apply(x, _slot_of(x))


def _slot_of(t):
    """The gradient slot an alias from ``fork`` carries -- handed out ONCE: the consumer that asks takes it off the alias.  A
    second slot-aware consumer of the same alias gets None and returns a fresh gradient tensor, which autograd adds as usual
    (with the slot still attached it would have accumulated into the shared buffer AND returned it: autograd's own sum of the
    alias' two gradients would then count that buffer twice without any error)."""
    if t is None:
        return None
    slot = getattr(t, "_ssbev_grad_slot", None)
    if slot is not None:
        t._ssbev_grad_slot = None
    return slot


def _slot_target(slot, like):
    """The tensor a data-gradient kernel should accumulate into, or None (then it writes a fresh tensor)."""
    if slot is None or slot.buf is None:
        return None
    b = slot.buf
    # same channels-last volume (a 2-D layer sees [B, 1, H, W, C] where the norm before it saw [B, H, W, C])
    ok = b.is_contiguous() and b.dtype == like.dtype and b.numel() == like.numel() and b.shape[-1] == like.shape[-1] and \
        b.shape[0] == like.shape[0]
    return b.view(tuple(like.shape)) if ok else None


# -------------------------------------------------------------------------------------------------
# convolution family
# -------------------------------------------------------------------------------------------------


def _triple(v, n):
    if isinstance(v, int):
        return (v,) * n
    v = tuple(int(a) for a in v)
    return v if len(v) == n else (v[0],) * n


TILE_HINT = int(os.environ.get("SSBEV_TILE_HINT", "0"))   # tuning hook (tools/probe_conv.py, A/B runs): forwarded to ssbev_conv_dims.tile_hint


def _conv_dims(xshape_cl, wshape, stride, padding, dilation, transposed, output_padding, relu=0, accumulate=0):
    """xshape_cl = (B, Di, Hi, Wi, Cin); weights in the torch layout."""
    B, Di, Hi, Wi, Cin = xshape_cl
    kd, kh, kw = wshape[2:]
    if transposed:
        Cout = wshape[1]
        outs = [(i - 1) * s - 2 * p + dl * (k - 1) + op + 1
                for i, s, p, dl, k, op in zip((Di, Hi, Wi), stride, padding, dilation, (kd, kh, kw), output_padding)]
    else:
        Cout = wshape[0]
        outs = [(i + 2 * p - dl * (k - 1) - 1) // s + 1
                for i, s, p, dl, k in zip((Di, Hi, Wi), stride, padding, dilation, (kd, kh, kw))]
    d = capi.ConvDims(B, Cin, Cout, Di, Hi, Wi, outs[0], outs[1], outs[2], kd, kh, kw, *stride, *padding, *dilation,
                      int(transposed), int(relu), int(accumulate), int(TILE_HINT), 1 if PRECISION == "bf16_operands" else 0)
    return d


# -------------------------------------------------------------------------------------------------
# operand plan of the fp32 direct leaf: which problem each pass of _ConvNd hands to the library
# -------------------------------------------------------------------------------------------------
# ONE place decides and ONE place executes, like _conv_route / _conv_run one level up.  `_conv_operands` is a pure function of
# shapes, the geometry tuple, the module switches (TILE_HINT, PRECISION, OWN_GEMM, read at call time) and the host-only class
# query; it touches no tensor and returns a `_ConvPlan` with the ssbev_conv_dims of each pass.  `_ConvNd` makes the plan once in
# forward, keeps it on ctx and only executes: it pads an operand's channels up to what the pass's dims say (_pad_channels,
# _pad_weight), launches, and crops the result back to the layer's own channel counts.  tests/test_conv_operands_snapshot.py pins
# what reaches the C boundary for thin, padded and plain channel pairs under every switch.
#
# The rules, each a detail of forward or backward once and kept as found:
#   * the kernels load their K role in float4: Cin of the forward (`kpad`) and Cout of the data gradient (`cpad`) are padded to a
#     multiple of 4, and so is the matching axis of the weight; the direct weight gradient gets both tensors padded and its result
#     is cropped to the parameter's shape;
#   * the thin-side kernels (conv_thin_mfma.hip) take 1 / 2 / 4 channels against 32 as they are.  Class 4 (mode 0): the forward
#     runs unpadded and x is SAVED unpadded, so a direct weight gradient pads x by itself (`tpad`); class 4 (mode 1): the data
#     gradient takes gy and the weight unpadded; class 6 (mode 2): the weight gradient takes both operands unpadded ("thin").
#     They are only asked where x was saved unpadded, and never for a transposed layer;
#   * class 5 (forward or data gradient) runs on the thin-out entry points instead of ssbev_conv_fwd / _bwd_data;
#   * the `fork` slot may be taken unless gx is cropped afterwards (kpad) or class 4 / 5 writes it: their kernels have no
#     accumulating epilogue.  A slot taken on a cropped gradient would double-count or drop it silently;
#   * a pointwise layer's weight gradient over >= 32768 rows with <= 128 channels on both sides is the skinny TN product of
#     gemm_tn ("tn": OWN_GEMM, fp32 operands, nothing padded).
# A pass that autograd does not want (`want`) is not planned: its dims are None and it costs no query.  The class is asked at most
# once per distinct (dims, mode).  The switches are read HERE, when the forward runs, for the backward too.
class _ConvPlan(NamedTuple):
    cin: int                          # the layer's own channel counts: what gx and gw are cropped back to
    cout: int
    fwd: capi.ConvDims                # Cin after kpad, unpadded when class 4 takes the thin input; x is saved with fwd.Cin channels
    fwd_class: int                    # 5: the thin-out entry points run it; 2 / 9 name the span family
    dgrad: Optional[capi.ConvDims]    # Cout after cpad (the own dims when class 4 takes gy unpadded), Cin = fwd.Cin
    dgrad_class: int
    slot_ok: bool                     # the data gradient may take the `fork` slot
    wgrad_kind: str                   # "tn" | "thin" | "direct"
    wgrad: Optional[capi.ConvDims]    # direct: Cin after kpad / tpad, Cout after cpad; tn, thin: the own dims


def _conv_operands(xshape_cl, wshape, geom, relu, want=(True, True)):
    """xshape_cl = (B, Di, Hi, Wi, Cin), weight shape in the torch layout, geom = (stride, padding, dilation, transposed,
    output_padding); want = (data gradient, weight gradient) wanted."""
    lib = capi.load()
    stride, padding, _, transposed, _ = geom
    cin, cout, k = xshape_cl[-1], wshape[1 if transposed else 0], tuple(wshape[2:])
    asked = {}

    def dims(ci, co, relu=0):
        return _conv_dims(tuple(xshape_cl[:-1]) + (ci,), ((ci, co) if transposed else (co, ci)) + k, *geom, relu=int(relu))

    def cls(d, mode):
        key = (bytes(d), mode)
        if key not in asked:
            asked[key] = lib.ssbev_conv_kernel_class(C.byref(d), mode)
        return asked[key]

    kpad, cpad = (-cin) % 4, (-cout) % 4
    own = dims(cin, cout)
    thin_in = bool(kpad) and not transposed and cls(own, 0) == 4
    kin = cin if thin_in else cin + kpad
    fwd = dims(kin, cout, relu)
    unpadded = not transposed and kin == cin                 # x is saved as it came: the thin-side kernels can be asked
    dgrad, dgrad_class, slot_ok = None, 0, False
    if want[0]:
        thin_d = unpadded and bool(cpad) and cls(own, 1) == 4
        dgrad = own if thin_d else dims(kin, cout + cpad)
        dgrad_class = cls(dgrad, 1)
        slot_ok = kin == cin and dgrad_class not in (4, 5)
    wgrad, wgrad_kind = None, ""
    if want[1]:
        if (not transposed and k == (1, 1, 1) and tuple(stride) == (1, 1, 1) and tuple(padding) == (0, 0, 0) and not kpad and not cpad
                and wshape[0] <= 128 and wshape[1] <= 128 and own.B * own.Do * own.Ho * own.Wo >= 32768
                and OWN_GEMM and PRECISION == "fp32"):
            wgrad_kind, wgrad = "tn", own
        elif unpadded and (cpad or kpad) and cls(own, 2) == 6:
            wgrad_kind, wgrad = "thin", own
        else:
            wgrad_kind, wgrad = "direct", dims(cin + kpad, cout + cpad)
    return _ConvPlan(cin, cout, fwd, cls(fwd, 0), dgrad, dgrad_class, slot_ok, wgrad_kind, wgrad)


def _pad_channels(tcl, n):
    """A channels-last tensor with its last axis zero-padded to ``n`` channels (the tensor itself where it has them)."""
    return tcl if tcl.shape[-1] == n else torch.nn.functional.pad(tcl, (0, n - tcl.shape[-1]))


def _pad_weight(w5, kn, nn, transposed):
    """A torch-layout weight with its K-role axis (Cin: axis 1, axis 0 of a transposed layer) zero-padded to ``kn`` and its N-role
    axis (Cout) to ``nn`` channels."""
    ka, na = (0, 1) if transposed else (1, 0)
    pads = [0, 0, 0, 0]                                      # F.pad counts from the last axis: (axis 1 lo, hi, axis 0 lo, hi)
    pads[3 - 2 * ka], pads[3 - 2 * na] = kn - w5.shape[ka], nn - w5.shape[na]
    return w5 if not any(pads) else torch.nn.functional.pad(w5, [0] * 6 + pads)


def _masked_gradient(ctx, gy):
    """The incoming gradient as a channels-last buffer; after a fused ReLU times [y > 0] of the saved output, in one pass."""
    gcl = to_cl(gy)
    return torch.ops.aten.threshold_backward(gcl, ctx.saved_tensors[2], 0.0) if ctx.relu else gcl


def _into_slot(slot, like, d, launch):
    """Run ``launch(gxcl)``, the data gradient of dims ``d``, into the buffer another consumer has left in ``slot`` (the kernels
    add in their epilogue: accumulate = 1) or into a fresh tensor like ``like``, and leave the result in the slot."""
    into = _slot_target(slot, like)
    gxcl = into if into is not None else torch.empty_like(like)
    d.accumulate = int(into is not None)
    launch(gxcl)
    d.accumulate = 0
    if slot is not None:
        slot.buf = gxcl
    return gxcl


def _bias_gradient(gcl):
    """Column sum of a channels-last gradient, fp32."""
    return gcl.reshape(-1, gcl.shape[-1]).sum(0, dtype=torch.float32)


def _packed(weight5, d, mode):
    """MFMA operand layout of a weight tensor (packed on the device; a few microseconds)."""
    lib = capi.load()
    wp = torch.empty(lib.ssbev_conv_packed_weight_elems(C.byref(d)), dtype=torch.float32, device=weight5.device)
    capi.check(lib.ssbev_conv_pack_weight(capi.ptr(weight5.contiguous()), capi.ptr(wp), C.byref(d), mode,
                                          capi.stream()), "ssbev_conv_pack_weight")
    return wp


def _thin_out_run(lib, src, weight5, bias, out, d, mode):
    """32 -> 1 / 2 / 4 channel 3x3x3 layers on the two-pass MFMA kernels (ssbev_conv_thin_*, kernel class 5)."""
    wp = torch.empty(lib.ssbev_conv_thin_packed_elems(C.byref(d), mode), dtype=torch.float32, device=src.device)
    capi.check(lib.ssbev_conv_thin_pack(capi.ptr(weight5.contiguous()), capi.ptr(wp), C.byref(d), mode, capi.stream()),
               "ssbev_conv_thin_pack")
    ws = _ws(lib.ssbev_conv_thin_workspace(C.byref(d), mode), src.device)
    capi.check(lib.ssbev_conv_thin_run(capi.ptr(src), capi.ptr(wp), capi.ptr(bias), capi.ptr(out), C.byref(d), mode,
                                       capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_conv_thin_run")


def _conv_grads(device, weight, want, bias_leaf, reads, weight_gradient, data_gradient, bias_gradient=None):
    """The order in which a conv backward issues its gradients -> (gx, gw, gb); ``want``: which of the three autograd asks for.
    The weight gradient is a leaf of the backward chain: on the side stream (streams.py) it runs NEXT to the data gradient and
    the normalisation passes that follow it instead of in front of them, and so does the gradient of a leaf bias (a column sum
    of gy); ``reads`` are the tensors the side stream has to wait for.  Then the data gradient, then whatever did not go aside."""
    want_gx, want_gw, want_gb = want
    gx = gw = gb = None
    gw_side = want_gw and streams.wgrad_on_side(weight)
    gb_side = gw_side and want_gb and bias_leaf
    if gw_side:
        with streams.on_side(device, *reads) as side:
            gw = weight_gradient()
            if gb_side:
                gb = bias_gradient()
            side.publish(gw, gb)
    if want_gx:
        gx = data_gradient()
    if want_gw and not gw_side:
        gw = weight_gradient()
    if want_gb and not gb_side:
        gb = bias_gradient()
    return gx, gw, gb


class _ConvNd(torch.autograd.Function):
    """x logical [B,Cin,D,H,W] (channels-last memory), weight in the torch layout (5-D)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, transposed, output_padding, slot=None, relu=False):
        lib = capi.load()
        ctx.slot = slot
        if ctx.needs_input_grad[1]:
            streams.note_use(weight)
        xcl = to_cl(_f32(x, "conv"))
        p = _conv_operands(tuple(xcl.shape), tuple(weight.shape), (stride, padding, dilation, transposed, output_padding), relu,
                           ctx.needs_input_grad[:2])
        d = p.fwd
        xcl = _pad_channels(xcl, d.Cin)
        w5 = _pad_weight(weight.detach(), d.Cin, d.Cout, transposed)
        y = torch.empty(d.B, d.Do, d.Ho, d.Wo, d.Cout, dtype=torch.float32, device=x.device)
        b = bias.detach().contiguous() if bias is not None else None
        fam = _conv_family(lib, d, 0, p.fwd_class)
        with _span(fam, conv_flops(d), conv_bytes(d), _conv_tag(d, "fwd"), conv_flops(d) / _EXEC_DIV[fam]):
            if p.fwd_class == 5:
                _thin_out_run(lib, xcl, w5, b, y, d, 0)
            else:
                wp = _packed(w5, d, 0)
                capi.check(lib.ssbev_conv_fwd(capi.ptr(xcl), capi.ptr(wp), capi.ptr(b), capi.ptr(y), C.byref(d),
                                              capi.stream()), "ssbev_conv_fwd")
        # fused ReLU (the kernels' epilogue): backward masks the incoming gradient with the saved output's sign
        ctx.relu = bool(relu)
        ctx.save_for_backward(xcl, weight, *((y,) if relu else ()))
        ctx.plan, ctx.cfg = p, (transposed, bias is not None)
        ctx.bias_leaf = bias is not None and bias.is_leaf and bias.grad is None
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        lib = capi.load()
        xcl, weight = ctx.saved_tensors[:2]
        p, (transposed, has_bias) = ctx.plan, ctx.cfg
        gcl0 = _masked_gradient(ctx, gy)                    # gradient as it arrives: Cout channels
        # ... padded ONCE if a wanted pass takes it padded (the thin-side kernels and the TN product take it as it is)
        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2])
        gcl = _pad_channels(gcl0, max([p.cout] + [d.Cout for d, on in zip((p.dgrad, p.wgrad), want) if on]))
        gy_of = lambda d: gcl if d.Cout == gcl.shape[-1] else gcl0

        def weight_gradient():
            d = p.wgrad
            if p.wgrad_kind == "tn":
                # 1x1x1 layers on the cost volume: gw[co][ci] = sum_rows gy[row][co] x[row][ci], an HBM-streaming skinny TN product
                with _span("conv_wgrad", conv_flops(d), conv_bytes(d), _conv_tag(d, "wgrad")):
                    return gemm_tn(gcl0.reshape(-1, p.cout), xcl.reshape(-1, p.cin)).view_as(weight)
            xw = _pad_channels(xcl, d.Cin)                  # (a copy only after a forward on the unpadded thin input)
            gwp = torch.empty(((d.Cin, d.Cout) if transposed else (d.Cout, d.Cin)) + tuple(weight.shape[2:]), dtype=torch.float32,
                              device=gy.device)
            ws = _ws(lib.ssbev_conv_bwd_weight_workspace(C.byref(d)), gy.device)
            with _span("conv_wgrad", conv_flops(d), conv_bytes(d), _conv_tag(d, "wgrad")):
                capi.check(lib.ssbev_conv_bwd_weight(capi.ptr(xw), capi.ptr(gy_of(d)), capi.ptr(gwp), C.byref(d),
                                                     capi.ptr(ws), ws.numel(), capi.stream()),
                           "ssbev_conv_bwd_weight")
            return gwp if gwp.shape == weight.shape else gwp[: weight.shape[0], : weight.shape[1]].contiguous()

        def data_gradient():
            d = p.dgrad
            gdl, wd = gy_of(d), _pad_weight(weight.detach(), d.Cin, d.Cout, transposed)

            def launch(gxcl):
                fam = _conv_family(lib, d, 1, None if d.accumulate else p.dgrad_class)     # (the class was asked without accumulate)
                with _span(fam, conv_flops(d), conv_bytes(d), _conv_tag(d, "dgrad"), conv_flops(d) / _EXEC_DIV[fam]):
                    if p.dgrad_class == 5:
                        _thin_out_run(lib, gdl, wd, None, gxcl, d, 1)
                    else:
                        wpt = _packed(wd, d, 1)
                        capi.check(lib.ssbev_conv_bwd_data(capi.ptr(gdl), capi.ptr(wpt), capi.ptr(gxcl), C.byref(d),
                                                           capi.stream()), "ssbev_conv_bwd_data")
            gxcl = _into_slot(ctx.slot if p.slot_ok else None, xcl, d, launch)
            return from_cl(gxcl if d.Cin == p.cin else gxcl[..., : p.cin])

        return _conv_grads(gy.device, weight, want, ctx.bias_leaf, (xcl, gcl0, gcl), weight_gradient, data_gradient,
                           lambda: _bias_gradient(gcl0)) + (None,) * 7


def _conv16_family(lib, d, mode):
    """Span family of a bf16-storage conv launch (the class query only when a timer listens)."""
    if KERNEL_TIMER is None:
        return "conv_gather16"
    return {17: "conv_tap16", 19: "conv_wide16"}.get(lib.ssbev_conv_kernel_class(C.byref(d), mode), "conv_gather16")


class _ConvNd16(torch.autograd.Function):
    """Convolution / transposed convolution in the bf16 STORAGE mode (csrc/conv_bf16.hip, ssbev_conv_dims.precision = 2 / 3):
    x and y (and gy, gx) are bf16 channels-last tensors, the weight stays an fp32 master (packed to bf16 operands per launch),
    its gradient comes back in fp32.  ``out_fp32``: fp32 result (the layer in front of an fp32 island)."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, padding, dilation, transposed, output_padding, slot=None, relu=False, out_fp32=False):
        lib = capi.load()
        ctx.slot = slot
        if ctx.needs_input_grad[1]:
            streams.note_use(weight)
        xcl = to_cl(x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16))
        d = _conv_dims(tuple(xcl.shape), tuple(weight.shape), stride, padding, dilation, transposed, output_padding, relu=int(relu))
        d.precision = 3 if out_fp32 else 2
        y = torch.empty(d.B, d.Do, d.Ho, d.Wo, d.Cout, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=x.device)
        b = bias.detach().float().contiguous() if bias is not None else None
        with _span(_conv16_family(lib, d, 0), conv_flops(d), conv_bytes(d) / 2.0, _conv_tag(d, "fwd")):
            wp = _packed(weight.detach(), d, 0)
            capi.check(lib.ssbev_conv_fwd_bf16(capi.ptr(xcl), capi.ptr(wp), capi.ptr(b), capi.ptr(y), C.byref(d), capi.stream()),
                       "ssbev_conv_fwd_bf16")
        ctx.relu = bool(relu)
        ctx.save_for_backward(xcl, weight, *((y,) if relu else ()))
        ctx.cfg = (stride, padding, dilation, transposed, output_padding, bias is not None)
        ctx.bias_leaf = bias is not None and bias.is_leaf and bias.grad is None
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        lib = capi.load()
        xcl, weight = ctx.saved_tensors[:2]
        stride, padding, dilation, transposed, output_padding, has_bias = ctx.cfg
        gcl = _masked_gradient(ctx, gy)
        if gcl.dtype != torch.bfloat16:
            gcl = gcl.to(torch.bfloat16)
        d = _conv_dims(tuple(xcl.shape), tuple(weight.shape), stride, padding, dilation, transposed, output_padding)
        d.precision = 2

        def weight_gradient():
            if (WIDE16_WGRAD == "wino" and not transposed and lib.ssbev_conv_kernel_class(C.byref(d), 0) == 19
                    and all(int(n) % 2 == 0 for n in xcl.shape[1:4])):
                with _span("conv_winograd_wgrad", conv_flops(d), conv_bytes(d) / 2.0, _conv_tag(d, "wgrad(wino)"), conv_flops(d) / 3.375):
                    return _wino_wgrad_bf16(xcl, gcl, weight)
            gwp = torch.empty(tuple(weight.shape), dtype=torch.float32, device=gy.device)
            ws = _ws(lib.ssbev_conv_bwd_weight_workspace(C.byref(d)), gy.device)
            fam = "wgrad_ring16" if (KERNEL_TIMER is not None and lib.ssbev_conv_kernel_class(C.byref(d), 2) == 20) else "wgrad16"
            with _span(fam, conv_flops(d), conv_bytes(d) / 2.0, _conv_tag(d, "wgrad")):
                capi.check(lib.ssbev_conv_bwd_weight_bf16(capi.ptr(xcl), capi.ptr(gcl), capi.ptr(gwp), C.byref(d), capi.ptr(ws),
                                                          ws.numel(), capi.stream()), "ssbev_conv_bwd_weight_bf16")
            return gwp

        def data_gradient():
            def launch(gxcl):
                with _span(_conv16_family(lib, d, 1), conv_flops(d), conv_bytes(d) / 2.0, _conv_tag(d, "dgrad")):
                    wpt = _packed(weight.detach(), d, 1)
                    capi.check(lib.ssbev_conv_bwd_data_bf16(capi.ptr(gcl), capi.ptr(wpt), capi.ptr(gxcl), C.byref(d), capi.stream()),
                               "ssbev_conv_bwd_data_bf16")
            return from_cl(_into_slot(ctx.slot, xcl, d, launch))

        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], has_bias and ctx.needs_input_grad[2])
        return _conv_grads(gy.device, weight, want, ctx.bias_leaf, (xcl, gcl), weight_gradient, data_gradient,
                           lambda: _bias_gradient(gcl)) + (None,) * 8


# bf16 storage mode: the wide stride-1 3x3x3 layers on grids with W % 16 == 0 (voxel encoder level 0, head conv, the 64 -> 64
# hourglass layers) run on conv_wide16_kernel (LDS-ring implicit GEMM) instead of the F(2,3) Winograd pipeline (0 = Winograd)
WIDE16 = os.environ.get("SSBEV_WIDE16", "1") != "0"
# ... and their weight gradient on the LDS-ring kernel wgrad_ring16_kernel ("direct", default) or on the Winograd-domain product
# (input transform + adjoint + batched bf16 library GEMM: "wino", kept for A/B runs)
WIDE16_WGRAD = os.environ.get("SSBEV_WIDE16_WGRAD", "direct")


def _wino_wgrad_bf16(xcl, gcl, weight):
    """Weight gradient of a 3x3x3 / stride 1 / pad 1 layer in the F(2,3)^3 Winograd domain, bf16 tensors on both sides:
    gU[xi] = V[xi]^T Z[xi] (batched bf16 GEMM, fp32 result), gw = G^T gU G."""
    lib = capi.load()
    B, D, H, W, Cin = xcl.shape
    Cout = gcl.shape[-1]
    T = B * (D // 2) * (H // 2) * (W // 2)
    V = _wino_call("ssbev_wino_input_transform_bf16a", xcl, capi.WinoDims(B, D, H, W, Cin), (64, T, Cin), torch.bfloat16)
    Z = _wino_call("ssbev_wino_output_adjoint_bf16a", gcl, capi.WinoDims(B, D, H, W, Cout), (64, T, Cout), torch.bfloat16)
    gU = _bmm16_tn(V, Z)
    gwt = torch.empty(tuple(weight.shape), dtype=torch.float32, device=xcl.device)
    capi.check(lib.ssbev_wino_weight_grad(capi.ptr(gU), capi.ptr(gwt), Cout, Cin, 3, capi.stream()), "ssbev_wino_weight_grad")
    return gwt


def _to_act(y):
    """Result of an fp32-island convolution on its way back into the bf16 chain (channel counts that cannot be bf16 sources --
    the 1-channel volumes -- stay fp32)."""
    if storage_bf16() and y.dtype == torch.float32 and y.shape[1] % 8 == 0:
        return y.to(torch.bfloat16)
    return y


WINOGRAD = os.environ.get("SSBEV_WINOGRAD", "1") != "0"   # wide 3x3x3 stride-1 layers via F(2,3)^3 (0 = direct MFMA conv)
# bf16 storage mode: wide stride-1 3x3(x3) layers on the F(2,3) Winograd pipeline with bf16 tensors on both sides (1), or on the
# direct bf16 MFMA kernels (0): 3.4x / 2.25x fewer multiply-adds against 8x / 4x larger transformed tensors
WINO_BF16S = os.environ.get("SSBEV_WINO_BF16S", "1") != "0"


# -------------------------------------------------------------------------------------------------
# plain fp32 GEMMs on the matrix cores (csrc/gemm.hip): no library GEMM on the hot path
# -------------------------------------------------------------------------------------------------
# SSBEV_OWN_GEMM=0 sends these products back to rocBLAS (torch.mm / torch.bmm), for A/B runs.
OWN_GEMM = os.environ.get("SSBEV_OWN_GEMM", "1") != "0"
# Per call site: comma list out of deconv, linear, wino, bri; "all" = every site.  Default = where the own kernels win or tie
# in the step (profiles/r2l_own_gemm_sites.txt, ms/step against 91.3 with none): deconv -0.75 (the depth-to-space permute
# copies disappear), bri +0.2 (no operand transposes; the north-star block on own kernels).  The wide pointwise layers
# (+1.5) and the batched frequency products of the 2-D / weight-streaming Winograd layers (+1.0) are plain library GEMMs
# where rocBLAS's tuned kernels run at 90 % of the fp32 matrix peak against ~75 % here: they stay on rocBLAS by default.
# r3 (one side stream, DepthNet off the critical chain; profiles/r3m_own_gemm_sites.txt, ms/step): deconv,bri 78.85 |
# + linear 78.92 (now free: default) | + wino 79.48 | all 79.85.  The batched frequency products of the 2-D / weight-streaming
# Winograd layers stay on the library: 0.6 ms per step is what its tuned kernels are still worth there.
# r5: "wino" joins the default -- no Cijk_* frequency product is left on a1-a16.  The price, measured with the
# r5 tile configurations (128 x 160 tiles on the 640-column products, 128 x 64 on the 512-channel layer; profiles/
# r5_gemm_cfg_probe.txt): 72.2-72.4 ms per step against 71.4-71.6 with rocBLAS on those 33 launches (own NN 113 vs 122 TF/s, own
# TN 85 vs 99 TF/s on 16 x [1920 x 640 x 640]).  SSBEV_OWN_GEMM_SITES=deconv,bri,linear restores the library there.
OWN_GEMM_SITES = set(os.environ.get("SSBEV_OWN_GEMM_SITES", "deconv,bri,linear,wino").split(","))


def own_gemm_site(name):
    return OWN_GEMM and ("all" in OWN_GEMM_SITES or name in OWN_GEMM_SITES)


def _rows(t):
    """[.., R, C] tensor with a contiguous last axis and uniform row / batch strides -> (tensor, ld, batch_stride)."""
    if t.stride(-1) != 1 or (t.dim() == 3 and t.shape[0] > 1 and t.stride(0) % 4 != 0) or t.stride(-2) % 4 != 0 or t.stride(-2) < t.shape[-1]:
        t = t.contiguous()
    if t.data_ptr() % 16:            # the kernels issue 16-byte global_load_lds: a last-axis slice view may start misaligned
        t = t.clone(memory_format=torch.contiguous_format)
    return t, t.stride(-2), (t.stride(0) if t.dim() == 3 else 0)


def _rawptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _gemm_supported(*ts):
    return OWN_GEMM and all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def _gdims(M, N, K, batch, lda, ldb, ldc, sa, sb, sc, relu=0, d2s=None):
    g = capi.GemmDims(int(M), int(N), int(K), int(batch), int(lda), int(ldb), int(ldc), int(sa), int(sb), int(sc), int(relu),
                      0, 0, 0, 0, 0, 0, 0, None, None, None)
    if d2s is not None:
        (g.d2s_D, g.d2s_H, g.d2s_W, g.d2s_kd, g.d2s_kh, g.d2s_kw, g.d2s_Co), table = d2s
        g.d2s_rowoff = table.data_ptr()
    return g


def gemm_nn(a, b, bias=None, relu=False, tag=None):
    """C = A @ B (+ bias, ReLU): a [M,K] or [Bt,M,K]; b [K,N] or [Bt,K,N] (a 2-D b is shared by the batch)."""
    if not _gemm_supported(a, b) or a.shape[-1] % 4 or b.shape[-1] % 4:
        y = torch.matmul(a, b)
        y = y if bias is None else y + bias
        return torch.relu(y) if relu else y
    a, lda, sa = _rows(a)
    b, ldb, sb = _rows(b)
    batch = a.shape[0] if a.dim() == 3 else 1
    M, K, N = a.shape[-2], a.shape[-1], b.shape[-1]
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    g = _gdims(M, N, K, batch, lda, ldb, N, sa, sb if b.dim() == 3 else 0, M * N, relu)
    fl = 2.0 * batch * M * N * K
    lib = capi.load()
    ws = _ws(lib.ssbev_gemm_nn_workspace(C.byref(g)), a.device)
    with _span("gemm_own", fl, 4.0 * (a.numel() + b.numel() + out.numel()), tag or f"nn {batch}x{M}x{K}x{N}"):
        capi.check(lib.ssbev_gemm_nn(_rawptr(a), _rawptr(b), _rawptr(bias.contiguous() if bias is not None else None),
                                     capi.ptr(out), C.byref(g), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_gemm_nn")
    return out


def gemm_nt(a, w, bias=None, relu=False, tag=None):
    """C = A @ W^T (+ bias, ReLU): a [M,K] / [Bt,M,K], w [N,K] / [Bt,N,K] -- the nn.Linear layout, nothing transposed."""
    if not _gemm_supported(a, w) or a.shape[-1] % 4 or w.shape[-2] % 4:
        y = torch.matmul(a, w.transpose(-1, -2))
        y = y if bias is None else y + bias
        return torch.relu(y) if relu else y
    a, lda, sa = _rows(a)
    w, ldb, sb = _rows(w)
    batch = a.shape[0] if a.dim() == 3 else 1
    M, K, N = a.shape[-2], a.shape[-1], w.shape[-2]
    out = torch.empty(*a.shape[:-1], N, dtype=torch.float32, device=a.device)
    g = _gdims(M, N, K, batch, lda, ldb, N, sa, sb if w.dim() == 3 else 0, M * N, relu)
    fl = 2.0 * batch * M * N * K
    lib = capi.load()
    ws = _ws(lib.ssbev_gemm_nt_workspace(C.byref(g)), a.device)
    with _span("gemm_own", fl, 4.0 * (a.numel() + w.numel() + out.numel()), tag or f"nt {batch}x{M}x{K}x{N}"):
        capi.check(lib.ssbev_gemm_nt(_rawptr(a), _rawptr(w), _rawptr(bias.contiguous() if bias is not None else None),
                                     capi.ptr(out), C.byref(g), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_gemm_nt")
    return out


def gemm_tn(a, b, tag=None, ep_mul=None, ep_rowsub=None):
    """C = A^T @ B over the ROW axis: a [R,K] / [Bt,R,K], b [R,N] / [Bt,R,N] -> [K,N] / [Bt,K,N] (weight gradients).
    ``ep_mul`` [.., K, N] (contiguous) and ``ep_rowsub`` [.., K]: fused epilogue C = ep_mul * (A^T B - ep_rowsub[..., None])."""
    if not _gemm_supported(a, b) or a.shape[-1] % 4 or b.shape[-1] % 4:
        c = torch.matmul(a.transpose(-1, -2), b)
        return c if ep_mul is None else ep_mul * (c - ep_rowsub.unsqueeze(-1))
    a, lda, sa = _rows(a)
    b, ldb, sb = _rows(b)
    batch = a.shape[0] if a.dim() == 3 else 1
    R, K, N = a.shape[-2], a.shape[-1], b.shape[-1]
    out = torch.empty(*a.shape[:-2], K, N, dtype=torch.float32, device=a.device)
    g = _gdims(R, N, K, batch, lda, ldb, N, sa, sb, K * N)
    if ep_mul is not None:
        ep_mul, ep_rowsub = ep_mul.contiguous(), ep_rowsub.contiguous().float()
        if tuple(ep_mul.shape) != tuple(out.shape) or ep_rowsub.numel() != batch * K:
            raise capi.SsbevError("gemm_tn: epilogue operand shapes")
        g.ep_mul, g.ep_rowsub = ep_mul.data_ptr(), ep_rowsub.data_ptr()
    lib = capi.load()
    ws = _ws(lib.ssbev_gemm_tn_workspace(C.byref(g)), a.device)
    fl = 2.0 * batch * R * N * K
    with _span("gemm_own", fl, 4.0 * (a.numel() + b.numel() + out.numel() * (2 if ep_mul is not None else 1)),
               tag or f"tn {batch}x{R}x{K}x{N}"):
        capi.check(lib.ssbev_gemm_tn(_rawptr(a), _rawptr(b), capi.ptr(out), C.byref(g), capi.ptr(ws), ws.numel(), capi.stream()),
                   "ssbev_gemm_tn")
    return out


class _LinearCL(torch.autograd.Function):
    """Pointwise (1x1 / stride 1) convolution of a channels-last map = y[rows, Cout] = x[rows, Cin] @ W[Cout, Cin]^T + b:
    NT forward, NN data gradient, TN weight gradient on the gemm.hip kernels, no transposes anywhere."""

    @staticmethod
    def forward(ctx, x2, w2, bias):
        ctx.save_for_backward(x2, w2)
        ctx.has_bias = bias is not None
        return gemm_nt(x2, w2, bias, tag=f"linear fwd {w2.shape[1]}->{w2.shape[0]} rows={x2.shape[0]}")

    @staticmethod
    def backward(ctx, gy):
        x2, w2 = ctx.saved_tensors
        gy = gy.contiguous()
        gx = gw = gb = None
        if ctx.needs_input_grad[0]:
            gx = gemm_nn(gy, w2, tag=f"linear dgrad {w2.shape[1]}->{w2.shape[0]} rows={x2.shape[0]}")
        if ctx.needs_input_grad[1]:
            gw = gemm_tn(gy, x2, tag=f"linear wgrad {w2.shape[1]}->{w2.shape[0]} rows={x2.shape[0]}")
        if ctx.has_bias and ctx.needs_input_grad[2]:
            gb = gy.sum(0)
        return gx, gw, gb


_D2S_TABLES = {}


def _d2s_table(B, D, H, W, k, Co, device):
    key = (B, D, H, W, k, Co, str(device))
    t = _D2S_TABLES.get(key)
    if t is None:
        t = torch.empty(B * D * H * W, dtype=torch.int64, device=device)
        capi.check(capi.load().ssbev_gemm_d2s_rowoff(capi.ptr(t), B * D * H * W, D, H, W, k[0], k[1], k[2], Co, capi.stream()),
                   "ssbev_gemm_d2s_rowoff")
        _D2S_TABLES[key] = t
    return t


class _DeconvKS(torch.autograd.Function):
    """kernel == stride ConvTranspose3d (SECONDFPN3D levels, second_fpn_3d.py:50-69) as the GEMM it is, with the
    depth-to-space index map inside the kernels: forward = NN with a scattering epilogue (the [B,D,H,W,kd,kh,kw,Co] ->
    [B,D kd,H kh,W kw,Co] permute copy of the library realisation never happens), data gradient = NT with gathered rows,
    weight gradient = TN with gathered rows."""

    @staticmethod
    def forward(ctx, xcl, weight, bias, k):
        B, D, H, W, Ci = xcl.shape
        Co = weight.shape[1]
        kd, kh, kw = k
        taps = kd * kh * kw
        wk = weight.detach().permute(0, 2, 3, 4, 1).reshape(Ci, taps * Co).contiguous()       # [Ci][tap][co]: a few MB
        table = _d2s_table(B, D, H, W, k, Co, xcl.device)
        y = torch.empty(B, D * kd, H * kh, W * kw, Co, dtype=torch.float32, device=xcl.device)
        x2 = xcl.reshape(-1, Ci)
        R = x2.shape[0]
        g = _gdims(R, taps * Co, Ci, 1, Ci, taps * Co, 0, 0, 0, 0, 0, ((D, H, W, kd, kh, kw, Co), table))
        fl = 2.0 * R * Ci * taps * Co
        with _span("gemm_own", fl, 4.0 * (x2.numel() + wk.numel() + y.numel()), f"deconv k=s fwd {Ci}->{Co} k{kd}{kh}{kw}"):
            capi.check(capi.load().ssbev_gemm_nn(capi.ptr(x2), capi.ptr(wk), capi.ptr(bias.detach().contiguous() if bias is not None else None),
                                                 capi.ptr(y), C.byref(g), None, 0, capi.stream()), "ssbev_gemm_nn")
        ctx.save_for_backward(x2, wk)
        ctx.meta = (B, D, H, W, Ci, Co, k, bias is not None)
        return y

    @staticmethod
    def backward(ctx, gy):
        x2, wk = ctx.saved_tensors
        B, D, H, W, Ci, Co, k, has_bias = ctx.meta
        kd, kh, kw = k
        taps = kd * kh * kw
        gy = gy.contiguous()
        table = _d2s_table(B, D, H, W, k, Co, gy.device)
        d2s = ((D, H, W, kd, kh, kw, Co), table)
        R = x2.shape[0]
        lib = capi.load()
        gx = gw = gb = None
        fl = 2.0 * R * Ci * taps * Co
        if ctx.needs_input_grad[0]:      # gx[r][ci] = sum_(tap,co) gy_fine[r; tap, co] wk[ci][(tap,co)]  (NT, gathered A)
            gx2 = torch.empty(R, Ci, dtype=torch.float32, device=gy.device)
            g = _gdims(R, Ci, taps * Co, 1, 0, taps * Co, Ci, 0, 0, 0, 0, d2s)
            ws = _ws(lib.ssbev_gemm_nt_workspace(C.byref(g)), gy.device)
            with _span("gemm_own", fl, 4.0 * (gy.numel() + wk.numel() + gx2.numel()), f"deconv k=s dgrad {Ci}->{Co} k{kd}{kh}{kw}"):
                capi.check(lib.ssbev_gemm_nt(capi.ptr(gy), capi.ptr(wk), None, capi.ptr(gx2), C.byref(g), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_gemm_nt")
            gx = gx2.view(B, D, H, W, Ci)
        if ctx.needs_input_grad[1]:      # gwk[ci][(tap,co)] = sum_r x[r][ci] gy_fine[r; tap, co]               (TN, gathered B)
            gwk = torch.empty(Ci, taps * Co, dtype=torch.float32, device=gy.device)
            g = _gdims(R, taps * Co, Ci, 1, Ci, 0, taps * Co, 0, 0, Ci * taps * Co, 0, d2s)
            ws = _ws(lib.ssbev_gemm_tn_workspace(C.byref(g)), gy.device)
            with _span("gemm_own", fl, 4.0 * (gy.numel() + x2.numel() + gwk.numel()), f"deconv k=s wgrad {Ci}->{Co} k{kd}{kh}{kw}"):
                capi.check(lib.ssbev_gemm_tn(capi.ptr(x2), capi.ptr(gy), capi.ptr(gwk), C.byref(g), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_gemm_tn")
            gw = gwk.view(Ci, kd, kh, kw, Co).permute(0, 4, 1, 2, 3).contiguous()
        if has_bias and ctx.needs_input_grad[2]:
            gb = gy.reshape(-1, Co).sum(0)
        return gx, gw, gb, None


# Layers that are plain GEMMs in the channels-last layout go to rocBLAS (forward, data and weight gradient through
# autograd's mm): wide pointwise convolutions ([pixels, Cin] x [Cin, Cout]) and the kernel == stride transposed
# convolutions of the FPN ([voxels, Cin] x [Cin, k^3 * Cout] followed by a depth-to-space copy).  The hand-written
# kernels stay on everything with spatial taps.  SSBEV_GEMM_LAYERS=0 keeps these layers on the MFMA conv kernels.
GEMM_LAYERS = os.environ.get("SSBEV_GEMM_LAYERS", "1") != "0"
GEMM_MIN_CIN = int(os.environ.get("SSBEV_GEMM_MIN_CIN", "512"))       # pointwise convs narrower than this stay on the HIP kernels


# A 3x3 convolution with dilation d and padding d only couples pixels of the same residue class modulo d: it is d*d
# independent ordinary 3x3 / pad 1 convolutions on the (H/d) x (W/d) sub-grids.  The ASPP branches of DepthNet (640 -> 640,
# dilation 6 / 12 / 18 on the 48 x 160 map) are therefore sent through the Winograd path as a batch of d*d small images
# (space-to-batch / batch-to-space are two tensor copies of 20 MB): 2.25x fewer multiply-adds than the direct dilated
# kernel.  Only when zero-padding the map to multiples of 2d costs < 35 % extra pixels (not for d = 18 at 48 x 160).
# (The route of the bf16 modes, and of fp32 with SSBEV_WINO_DILATED=0; fp32 otherwise takes the strided-tile transforms below.)
DILATED_POLYPHASE = os.environ.get("SSBEV_DILATED_POLYPHASE", "1") != "0"
POLYPHASE_MAX_PAD = float(os.environ.get("SSBEV_POLYPHASE_MAX_PAD", "1.35"))


# fp32: the residue classes are an addressing pattern of the F(2x2, 3x3) transform kernels (csrc/winograd.hip, ssbev_wino_dims.dil),
# not a data layout: every class is tiled on its own, so nothing is padded to multiples of 2d and no sub-image batch is built
# (no pad / permute clone / to_cl clone / slice, forward or backward).  Tiles per axis = sum over the classes ph < min(d, n) of
# ceil(ceil((n - ph) / d) / 2) (ssbev_wino2d_axis_tiles).  The route is taken while that costs at most WINO_DILATED_MAX_TILES
# times the tiles of the undilated layer: POLYPHASE_MAX_PAD + 0.05 = 1.40 admits the ASPP d = 18 branch (30 x 88 tiles against
# 24 x 80 = 1.375x), which at 2.25 / 1.375 is still 1.64x fewer multiply-adds than the direct dilated kernels.
# SSBEV_WINO_DILATED=0: the polyphase batch / direct kernels as before (A/B runs).
WINO_DILATED = os.environ.get("SSBEV_WINO_DILATED", "1") != "0"
WINO_DILATED_MAX_TILES = float(os.environ.get("SSBEV_WINO_DILATED_MAX_TILES", str(POLYPHASE_MAX_PAD + 0.05)))
WINO_DILATED_AXIS_CAP = 128          # tile-table entries per axis the transform kernels take (SSBEV_WINO2D_MAX_AXIS_TILES)


def wino2d_axis_tiles(n, d):
    """F(2,3) tiles along an axis of extent ``n`` when each residue class modulo ``d`` is tiled on its own."""
    return sum(-(-(-(-(n - ph) // d)) // 2) for ph in range(min(d, n)))


def _wino_dilated_fits(H, W, cin, d):
    th, tw = wino2d_axis_tiles(H, d), wino2d_axis_tiles(W, d)
    return (max(th, tw) <= WINO_DILATED_AXIS_CAP and cin % 4 == 0
            and th * tw <= WINO_DILATED_MAX_TILES * (-(-H // 2)) * (-(-W // 2)))


def _wino_dilated_applicable(x, weight, d):
    return _wino_dilated_fits(int(x.shape[-2]), int(x.shape[-1]), weight.shape[1], d)


def _polyphase_grid(H, W, d):
    """The map padded to multiples of 2d, or None when that costs more than POLYPHASE_MAX_PAD times the pixels."""
    Hp, Wp = -(-H // (2 * d)) * 2 * d, -(-W // (2 * d)) * 2 * d
    return (Hp, Wp) if Hp * Wp <= POLYPHASE_MAX_PAD * H * W else None


def _dilated_polyphase(x, weight, d):
    B, Cc, H, W = x.shape
    grid = _polyphase_grid(H, W, d)
    if grid is None:
        return None
    Hp, Wp = grid
    xp = torch.nn.functional.pad(x, [0, Wp - W, 0, Hp - H]) if (Hp != H or Wp != W) else x
    xs = xp.reshape(B, Cc, Hp // d, d, Wp // d, d).permute(0, 3, 5, 1, 2, 4).reshape(B * d * d, Cc, Hp // d, Wp // d)
    ys = conv2d(xs, weight, None, 1, 1, 1)
    Co = weight.shape[0]
    y = ys.reshape(B, d, d, Co, Hp // d, Wp // d).permute(0, 3, 4, 1, 5, 2).reshape(B, Co, Hp, Wp)
    return y[:, :, :H, :W]


# -------------------------------------------------------------------------------------------------
# conv routing: which leaf serves a conv3d / conv2d / conv_transpose3d call
# -------------------------------------------------------------------------------------------------
# ONE place decides and ONE place executes, like select_conv_path in csrc/conv_mfma.hip one level down.  `_conv_route` is a pure
# function of shapes and module switches (read at call time: tests and A/B runs assign to them) that states the order of the
# routes top to bottom and returns a `_Route`; `_conv_run` is the only caller of the leaves (_ConvNd, _ConvNd16, _WinoConv,
# _WinoConvDF, linear_cl, _DeconvKS, torch.mm, torch.relu) and of the steps around them.  The entry points normalise their
# arguments (conv2d lifts its shapes to a depth-1 volume) and call the two.  A new route is one kind, one line in `_conv_route` and
# one case in `_conv_run`; tests/test_conv_routes_snapshot.py pins what every layer shape of the workload gets under every switch.
#
# Order.  bf16 storage (GPU tensor, admitted tile hint): wide16 ring (conv3d) | polyphase batch (conv2d) | bf16 Winograd | bf16
# direct (both channel counts % 8 == 0) | fp32 island, cast back.  Otherwise, conv_transpose3d: k == s GEMM (k = s = 1 as a
# linear layer | own kernels | library mm) | direct.  conv3d / conv2d: ReLU fused into the direct kernel unless one of the next
# three or a non-GPU tensor takes the call (then ReLU outside) | pointwise GEMM | dilated 3x3 (conv2d): strided-tile Winograd |
# polyphase batch | Winograd, depth-fused where it applies | direct.
#
# What a route fixes besides the leaf -- each was a detail of a call site once, and is kept as found:
#   * the bias goes INTO the direct / GEMM kernels and is added AFTER the Winograd pipelines and the polyphase batch;
#   * the ReLU is fused into the direct kernels and applied after everything else;
#   * the `fork` gradient slot is taken off the input alias (_slot_of) exactly when the leaf receives it.  A route that took it
#     and returned a fresh gradient would double-count silently.  Quirks: the fp32 islands, conv2d's bf16 direct route (the parent
#     asked the lifted view, which carries no slot) and the whole fp32 side of conv_transpose3d never take it;
#   * which TILE_HINT values admit the bf16 routes differs per entry point (_BF16_HINTS): also a quirk; any hint but 0 takes the
#     fp32 GEMM and Winograd routes away (the hint is a tuning hook of the direct kernels).
_BF16_HINTS = {"conv3d": (0, 7, 9), "conv2d": (0, 9), "conv_transpose3d": (0, 9)}


class _Route(NamedTuple):
    kind: str                         # the case of _conv_run
    geom: tuple                       # (stride, padding, dilation, transposed, output_padding) of the leaf (conv2d: depth-1 volume)
    take_slot: bool = True            # the leaf gets the input's gradient slot (False: it stays on the alias)
    bias_after: bool = False          # added to the leaf's result (False: passed into the leaf)
    relu_fused: bool = False          # in the leaf's epilogue ...
    relu_after: bool = False          # ... or torch.relu on the result
    cast: bool = False                # fp32 island: _to_act on the result
    lift: bool = False                # conv2d on a 5-D leaf: unsqueeze(2) going in, squeeze(2) coming out
    dil: int = 1                      # dilation of the strided-tile Winograd route / of the polyphase batch
    out_fp32: bool = False            # _ConvNd16: fp32 result (no route asks for it yet)


def _pointwise_gemm(wshape, st, pd):
    """A wide 1x1(x1) / stride 1 layer: the plain GEMM of linear_cl (fp32 without a tile hint)."""
    return (GEMM_LAYERS and TILE_HINT == 0 and PRECISION == "fp32" and tuple(wshape[2:]) == (1, 1, 1) and st == (1, 1, 1)
            and pd == (0, 0, 0) and wshape[1] >= GEMM_MIN_CIN)


def _dilated_same_3x3(wshape, st, pd, dl):
    """A wide 2-D 3x3 / stride 1 layer with dilation = padding = d > 1 (lifted to a depth-1 volume): the ASPP branches."""
    return (tuple(wshape[2:]) == (1, 3, 3) and st == (1, 1, 1) and dl[1] == dl[2] and dl[1] > 1 and pd[1:] == dl[1:]
            and min(wshape[0], wshape[1]) >= 64)


def _conv_route(entry, xshape, wshape, stride, padding, dilation, transposed, output_padding, relu, is_cuda):
    st, pd, dl, k = tuple(stride), tuple(padding), tuple(dilation), tuple(wshape[2:])
    B, _, D, H, W = xshape
    cin, cout = (wshape[0], wshape[1]) if transposed else (wshape[1], wshape[0])
    lift = entry == "conv2d"

    def route(kind, **facts):
        return _Route(kind, (st, pd, dl, transposed, tuple(output_padding)), **facts)
    wino = not transposed and WINOGRAD and _wino_applicable(is_cuda, xshape, wshape, st, pd, dl)
    dilated = lift and WINOGRAD and is_cuda and _dilated_same_3x3(wshape, st, pd, dl)
    if storage_bf16() and is_cuda and TILE_HINT in _BF16_HINTS[entry]:
        if entry == "conv3d" and WIDE16 and k == (3, 3, 3) and st == pd == dl == (1, 1, 1) and cin % 8 == 0 and cout % 8 == 0:
            d = _conv_dims((B, D, H, W, cin), tuple(wshape), st, pd, dl, False, (0, 0, 0))
            d.precision = 2
            if capi.load().ssbev_conv_kernel_class(C.byref(d), 0) == 19:          # conv_wide16_kernel takes it
                return route("conv16", relu_fused=relu)
        if dilated and DILATED_POLYPHASE and WINO_BF16S and _polyphase_grid(H, W, dl[1]):
            return route("polyphase", take_slot=False, bias_after=True, dil=dl[1])
        if wino and WINO_BF16S:
            return route("wino", bias_after=True, relu_after=relu, lift=lift)
        if cin % 8 == 0 and cout % 8 == 0:       # 16-byte bf16 voxel-line pieces (the Cout-channel gradient is a bf16 SOURCE in backward)
            return route("conv16", relu_fused=relu, lift=lift, take_slot=not lift)       # (quirk: conv2d leaves the slot on the alias)
        return route("convnd", take_slot=False, relu_fused=relu, cast=True, lift=lift)       # the 1- / 2- / 20-channel layers
    if transposed:
        if GEMM_LAYERS and TILE_HINT == 0 and PRECISION == "fp32" and is_cuda and k == st and pd == (0, 0, 0) and \
                tuple(output_padding) == (0, 0, 0) and cin >= 128:
            # k = s = 1 (SECONDFPN3D's first branch, FPN:53-69) is a pointwise layer: the plain NT / NN / skinny-TN products of
            # linear_cl.  Through the depth-to-space table of the general k == s path its weight gradient ran at 26 TF/s (0.33 ms
            # for 8.6 GF: profiles/r6c layer table) where the skinny TN kernel needs 0.12 ms for the same product.
            if k == (1, 1, 1) and own_gemm_site("deconv") and own_gemm_site("linear") and cout % 4 == 0:
                return route("linear", take_slot=False)
            return route("deconv_ks" if own_gemm_site("deconv") and cout % 64 == 0 and cin % 4 == 0 else "deconv_mm", take_slot=False)
        return route("convnd", take_slot=False)                 # (quirk: no fp32 route of conv_transpose3d takes the slot)
    gemm = is_cuda and _pointwise_gemm(wshape, st, pd)
    wino = wino and TILE_HINT == 0
    if gemm:                                     # wide pointwise conv = plain GEMM on the channels-last buffer
        return route("linear", take_slot=False, relu_after=relu)
    if dilated and TILE_HINT == 0:
        if WINO_DILATED and PRECISION == "fp32" and _wino_dilated_fits(H, W, cin, dl[1]):
            return route("wino", bias_after=True, lift=True, dil=dl[1])
        if DILATED_POLYPHASE and _polyphase_grid(H, W, dl[1]):
            return route("polyphase", take_slot=False, bias_after=True, dil=dl[1])
    if wino:
        df = k == (3, 3, 3) and H % 4 == 0 and W % 4 == 0 and _wino_df_applicable(B, D, H, W, cin, cout)
        return route("wino_df" if df else "wino", bias_after=True, relu_after=relu, lift=lift)
    # epilogue ReLU of the direct kernels (the MIE block's two conv -> ReLU pairs, VT:250-258); elsewhere a norm follows
    return route("convnd", relu_fused=relu and is_cuda, relu_after=relu and not is_cuda, lift=lift)


def _conv_run(r, x, weight, bias):
    slot = _slot_of(x) if r.take_slot else None
    stride, _, _, transposed, _ = r.geom
    x5, w5 = (x.unsqueeze(2), weight.unsqueeze(2)) if r.lift else (x, weight)
    if r.kind == "conv16":
        y = _ConvNd16.apply(x5, w5, bias, *r.geom, slot, r.relu_fused, r.out_fp32)
    elif r.kind == "convnd":
        y = _ConvNd.apply(x5, w5, bias, *r.geom, slot, r.relu_fused)
    elif r.kind == "wino":
        y = _WinoConv.apply(x5, w5, slot, r.dil)
    elif r.kind == "wino_df":
        y = _WinoConvDF.apply(x5, w5, slot)
    elif r.kind == "linear":                     # (a k = s = 1 deconv: weight [Cin, Cout, 1, 1, 1])
        y = linear_cl(x, weight.reshape(weight.shape[0], weight.shape[1]).t() if transposed else weight, bias)
    elif r.kind == "polyphase":                  # d * d sub-images through conv2d again (their route: undilated Winograd)
        y = _dilated_polyphase(x, weight, r.dil)
    elif r.kind == "deconv_ks":
        y = from_cl(_DeconvKS.apply(to_cl(_f32(x, "deconv_gemm")), weight, bias, stride))
    elif r.kind == "deconv_mm":                  # the library's k == s deconv: GEMM, depth-to-space copy, bias
        xcl = to_cl(_f32(x, "deconv_gemm"))
        (B, D, H, W, Ci), Co, (kd, kh, kw) = xcl.shape, weight.shape[1], stride
        w2 = weight.permute(0, 2, 3, 4, 1).reshape(Ci, kd * kh * kw * Co)
        fl = 2.0 * B * D * H * W * Ci * kd * kh * kw * Co
        nby = 4.0 * (xcl.numel() + w2.numel() + B * D * H * W * kd * kh * kw * Co)
        mult = 3.0 if (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)) else 1.0
        with _span("gemm_lib", fl * mult, nby * mult, f"fwd   deconv k=s {Ci}->{Co} k{kd}{kh}{kw}"):
            g = torch.mm(xcl.reshape(-1, Ci), w2).view(B, D, H, W, kd, kh, kw, Co)
        y = g.permute(0, 1, 4, 2, 5, 3, 6, 7).reshape(B, D * kd, H * kh, W * kw, Co)
        y = from_cl(y if bias is None else y + bias)
    else:
        raise capi.SsbevError(f"conv route {r.kind!r} has no executor")
    if r.cast:
        y = _to_act(y)
    if r.lift:
        y = y.squeeze(2)
    if r.bias_after and bias is not None:
        y = y + _like_act(bias, y).view((1, -1) + (1,) * (y.dim() - 2))
    return torch.relu(y) if r.relu_after else y


def conv3d(x, weight, bias=None, stride=1, padding=0, dilation=1, relu=False):
    """F.conv3d replacement (groups=1): the MFMA implicit-GEMM kernels, or Winograd F(2x2x2,3x3x3) for the wide
    stride-1 3x3x3 layers."""
    r = _conv_route("conv3d", x.shape, weight.shape, _triple(stride, 3), _triple(padding, 3), _triple(dilation, 3), False, (0, 0, 0),
                    bool(relu), x.is_cuda)
    return _conv_run(r, x, weight, bias)


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1):
    """F.conv2d replacement: a depth-1 volume through the same kernels (groups=1); wide 3x3 stride-1 layers via
    Winograd F(2x2,3x3)."""
    r = _conv_route("conv2d", (*x.shape[:2], 1, *x.shape[2:]), (*weight.shape[:2], 1, *weight.shape[2:]), (1,) + _triple(stride, 2),
                    (0,) + _triple(padding, 2), (1,) + _triple(dilation, 2), False, (0, 0, 0), False, x.is_cuda)
    return _conv_run(r, x, weight, bias)


def conv_transpose3d(x, weight, bias=None, stride=1, padding=0, output_padding=0):
    """F.conv_transpose3d replacement (weight [Cin, Cout, kd, kh, kw])."""
    r = _conv_route("conv_transpose3d", x.shape, weight.shape, _triple(stride, 3), _triple(padding, 3), (1, 1, 1), True,
                    _triple(output_padding, 3), False, x.is_cuda)
    return _conv_run(r, x, weight, bias)


# -------------------------------------------------------------------------------------------------
# Winograd F(2x2x2, 3x3x3) convolution for the wide stride-1 3x3x3 layers
# -------------------------------------------------------------------------------------------------

_WINO_G = None


def _wino_g(device):
    global _WINO_G
    if _WINO_G is None or _WINO_G.device != device:
        _WINO_G = torch.tensor([[1.0, 0.0, 0.0], [0.5, 0.5, 0.5], [0.5, -0.5, 0.5], [0.0, 0.0, 1.0]], device=device)
    return _WINO_G


# BASELINE configs[3] ("bf16 mixed precision, MFMA 3D-conv path").  Three modes, never switched implicitly:
#   "fp32"           the parity contract of the headline metric (default);
#   "bf16"           (round 4) bf16 STORAGE: activations and activation gradients are bf16 channels-last tensors between the
#                    layers (convolutions on csrc/conv_bf16.hip, normalisations with bf16 I/O, the F(2,3) Winograd pipeline with
#                    bf16 on both sides); fp32 islands: parameters and their gradients (masters), normalisation statistics,
#                    softmaxes, the BRI attention, the scatter, the losses -- what mmcv's Fp16OptimizerHook / auto_fp16 keep
#                    in fp32 (reference mmdet_train.py:131-134), with bf16 in place of fp16;
#   "bf16_operands"  (rounds 1-3) tensors stay fp32 in HBM, the MFMA operands are rounded to bf16 in registers and the
#                    Winograd-domain tensors are stored as bf16: kept for A/B runs.
PRECISION = os.environ.get("SSBEV_PRECISION", "fp32")
_MODES = ("fp32", "bf16", "bf16_operands")


def set_precision(mode):
    global PRECISION
    if mode not in _MODES:
        raise ValueError(f"precision must be one of {_MODES}, got {mode!r}")
    PRECISION = mode


def storage_bf16():
    """Are activations stored as bf16 between layers (precision mode "bf16")?"""
    return PRECISION == "bf16"


def act_dtype():
    return torch.bfloat16 if PRECISION == "bf16" else torch.float32


def _like_act(y, ref):
    """A broadcast parameter (bias) in the dtype of the activation it is added to (bf16 + fp32 would promote the sum)."""
    return y if y.dtype == ref.dtype else y.to(ref.dtype)


def _wino_call(name, src, dims, out_shape, dtype=torch.float32):
    lib = capi.load()
    dst = torch.empty(out_shape, dtype=dtype, device=src.device)
    capi.check(getattr(lib, name)(capi.ptr(src), capi.ptr(dst), C.byref(dims), capi.stream()), name)
    return dst


# Opt-in: (h,w)-only transforms + the depth axis of F(2,3) inside a hand-written MFMA GEMM kernel (half the HBM traffic of
# the batched-GEMM pipeline, but this first version of the kernel runs at 60-75 TF/s and does not beat it yet:
# 128->128 1.34 vs 1.41 ms, 384->192 4.6 vs 3.6 ms; tools/wino_gemm_probe.py)
WINO_DEPTH_FUSED = os.environ.get("SSBEV_WINO_DEPTH_FUSED", "0") != "0"


# Opt-in: hand-written LDS-streaming MFMA kernel for the 64 frequency GEMMs (default: one rocBLAS batched GEMM, which is
# still 20-40 % faster on these shapes: tools/wino_gemm_probe.py)
WINO_OWN_GEMM = os.environ.get("SSBEV_WINO_OWN_GEMM", "0") != "0"


def gemm16_nn(a16, b32, out_fp32=False, tag=None):
    """C[b] = A[b] @ B[b]: a16 [Bt, M, K] bf16, b32 [Bt, K, N] fp32 (rounded to bf16 while it is packed) -> [Bt, M, N] bf16 / fp32,
    fp32 accumulation on conv_igemm16_kernel (csrc/conv_bf16.hip).  None when the shapes do not fit (K % 32, N % 8)."""
    lib = capi.load()
    Bt, M, K = a16.shape
    N = b32.shape[2]
    d = capi.Gemm16Dims(M, N, K, Bt, int(out_fp32))
    n = lib.ssbev_gemm16_packed_elems(C.byref(d))
    if n == 0 or a16.dtype != torch.bfloat16 or b32.dtype != torch.float32 or tuple(b32.shape[:2]) != (Bt, K):
        return None
    a16, b32 = a16.contiguous(), b32.contiguous()
    packed = torch.empty(n, dtype=torch.int16, device=a16.device)
    out = torch.empty(Bt, M, N, dtype=torch.float32 if out_fp32 else torch.bfloat16, device=a16.device)
    with _span("gemm16", 2.0 * Bt * M * K * N, 2.0 * (a16.numel() + out.numel()) + 4.0 * b32.numel(), tag or f"gemm16 {Bt}x[{M}x{K}x{N}]"):
        capi.check(lib.ssbev_gemm16_pack(capi.ptr(b32), capi.ptr(packed), C.byref(d), capi.stream()), "ssbev_gemm16_pack")
        capi.check(lib.ssbev_gemm16_nn(capi.ptr(a16), capi.ptr(packed), capi.ptr(out), C.byref(d), capi.stream()), "ssbev_gemm16_nn")
    return out


# bf16 storage mode: the Winograd frequency products on the own bf16 kernel instead of torch.bmm / rocBLAS (0 = library)
GEMM16_OWN = os.environ.get("SSBEV_GEMM16_OWN", "1") != "0"


def _bmm16(V, U):
    """V [nf, T, K] bf16 x U [nf, K, N] fp32 -> bf16 [nf, T, N]"""
    if GEMM16_OWN and V.is_cuda:
        M = gemm16_nn(V, U, tag=f"wino16 gemm {V.shape[0]}x[{V.shape[1]}x{V.shape[2]}x{U.shape[2]}]")
        if M is not None:
            return M
    return torch.bmm(V, U.to(torch.bfloat16))


def gemm16_tn(a16, b16, tag=None):
    """C[b] = A[b]^T @ B[b] over the row axis: a16 [Bt, M, K], b16 [Bt, M, N] bf16 -> [Bt, K, N] fp32 on gemm16_tn_kernel
    (csrc/conv_bf16.hip: LDS-DMA staging + ds_read_b64_tr_b16 operands).  None when the shapes do not fit (K % 8, N % 8)."""
    lib = capi.load()
    Bt, M, K = a16.shape
    N = b16.shape[2]
    d = capi.Gemm16Dims(M, N, K, Bt, 1)
    if (K % 8 or N % 8 or a16.dtype != torch.bfloat16 or b16.dtype != torch.bfloat16 or tuple(b16.shape[:2]) != (Bt, M)
            or Bt >= 65536):
        return None
    a16, b16 = a16.contiguous(), b16.contiguous()
    out = torch.empty(Bt, K, N, dtype=torch.float32, device=a16.device)
    ws = torch.empty(max(int(lib.ssbev_gemm16_tn_workspace(C.byref(d))), 4), dtype=torch.float32, device=a16.device)
    with _span("gemm16", 2.0 * Bt * M * K * N, 2.0 * (a16.numel() + b16.numel()) + 4.0 * out.numel(), tag or f"gemm16 tn {Bt}x[{K}x{M}x{N}]"):
        capi.check(lib.ssbev_gemm16_tn(capi.ptr(a16), capi.ptr(b16), capi.ptr(out), C.byref(d), capi.ptr(ws), ws.numel(),
                                       capi.stream()), "ssbev_gemm16_tn")
    return out


def _bmm16_tn(V, Z):
    """V [nf, T, K]^T x Z [nf, T, N] (bf16) -> fp32 [nf, K, N]: the weight-gradient frequency products"""
    if GEMM16_OWN and V.is_cuda:
        g = gemm16_tn(V, Z, tag=f"wino16 wgrad gemm {V.shape[0]}x[{V.shape[2]}x{V.shape[1]}x{Z.shape[2]}]")
        if g is not None:
            return g
    return torch.bmm(V.transpose(1, 2), Z, out_dtype=torch.float32)


def _wino_bgemm(V, w, Cout, Cin, mode):
    """M[xi] = V[xi] @ U[xi] for the 64 frequencies on the LDS-streaming MFMA kernel (mode 0 forward, 1 data gradient)."""
    lib = capi.load()
    T, K = V.shape[1], V.shape[2]
    N = Cout if mode == 0 else Cin
    Wp = torch.empty(lib.ssbev_wino_dgemm_packed_elems(Cout, Cin), dtype=torch.float32, device=V.device)
    capi.check(lib.ssbev_wino_dgemm_pack(capi.ptr(w), capi.ptr(Wp), Cout, Cin, mode, capi.stream()), "ssbev_wino_dgemm_pack")
    M = torch.empty(64, T, N, dtype=torch.float32, device=V.device)
    capi.check(lib.ssbev_wino_bgemm(capi.ptr(V), capi.ptr(Wp), capi.ptr(M), T, K, N, capi.stream()), "ssbev_wino_bgemm")
    return M


def _wino_depth_fused(xcl, w, B, D, H, W, K, N, mode):
    """3-D Winograd conv of a channels-last volume with K input / N output channels: (h,w) transform -> depth-fused
    frequency GEMM (HIP MFMA kernel, the depth axis of F(2,3) done in registers) -> (h,w) output transform.
    mode 0: forward (w [N,K,3,3,3]); mode 1: data gradient (w [K,N,3,3,3], mirrored taps)."""
    lib = capi.load()
    Cout, Cin = (N, K) if mode == 0 else (K, N)
    R = B * D * (H // 2) * (W // 2)
    P = _wino_call("ssbev_wino2d_input_transform", xcl, capi.WinoDims(B, D, H, W, K), (16, R, K))
    Wp = torch.empty(lib.ssbev_wino_dgemm_packed_elems(Cout, Cin), dtype=torch.float32, device=xcl.device)
    capi.check(lib.ssbev_wino_dgemm_pack(capi.ptr(w), capi.ptr(Wp), Cout, Cin, mode, capi.stream()), "ssbev_wino_dgemm_pack")
    Mo = torch.empty(16, R, N, dtype=torch.float32, device=xcl.device)
    dims = capi.WinoDims(B, D, H, W, K)
    capi.check(lib.ssbev_wino_dgemm(capi.ptr(P), capi.ptr(Wp), capi.ptr(Mo), C.byref(dims), N, capi.stream()),
               "ssbev_wino_dgemm")
    del P
    return _wino_call("ssbev_wino2d_output_transform", Mo, capi.WinoDims(B, D, H, W, N), (B, D, H, W, N))


# F(4,3) tiles along h and w (F(2,3) along d): 4.5x / 2.25x transformed domain instead of 8x / 4x and 6x / 4x fewer
# multiply-adds instead of 3.375x / 2.25x; used whenever H and W are multiples of 4 (SSBEV_WINO_F43=0: F(2,3) everywhere)
WINO_F43 = os.environ.get("SSBEV_WINO_F43", "1") != "0"
# ... and for the 2-D layers (DepthNet, 640 channels on the 48x160 map) only on request: there F(4,3)^2 saves ~1 ms per step
# but its rounding error (reduction over 640 channels of values scaled by the 4 / 5 / 8 entries) more than doubles the
# gradient noise of the DepthNet parameters in the full-step parity test (L2 1.1 % vs 0.45 %), for no accuracy budget left
WINO_F43_2D = os.environ.get("SSBEV_WINO_F43_2D", "0") != "0"
# ... or, opt-in, inside a `wino_f43_2d_scope()` (r3: DepthNet wraps its own 640 -> 640 layers; SSBEV_WINO_F43_2D_DEPTHNET=1).
# Measured in r3 (profiles/r3p_f43_2d.txt): F(4,3)^2 on every 2-D layer = -1.5 ms per step, forward logits unchanged
# (1.6e-4), but the stereo feature net's 640 -> 128 conv sits in front of the cost volume and its 1e-5 forward change flips
# ReLU decisions in the 20-layer 3-D stack behind it: gradient distance of that stack to the oracle 0.87 % -> 1.85-2.1 %,
# over the 2e-2 gate.  Limited to DepthNet the step is still 1.5 ms faster and every gate passes (worst gradient 1.3e-2),
# but DepthNet's own gradients then sit at 0.9 % where the oracle moves by 0.2 % under a one-ulp input change
# (tests/test_gpu_fullsize.py::test_gradient_gate_vs_oracle_noise_floor fails its 3x criterion): visible rounding, not
# noise floor.  Parity first: off by default.
WINO_F43_2D_DEPTHNET = os.environ.get("SSBEV_WINO_F43_2D_DEPTHNET", "0") != "0"
_F43_2D_SCOPE = 0


class wino_f43_2d_scope:
    """2-D 3x3 layers built inside this scope use F(4,3)^2 tiles (the choice is recorded per call for its backward)."""

    def __enter__(self):
        global _F43_2D_SCOPE
        _F43_2D_SCOPE += 1 if WINO_F43_2D_DEPTHNET else 0
        return self

    def __exit__(self, *exc):
        global _F43_2D_SCOPE
        _F43_2D_SCOPE -= 1 if WINO_F43_2D_DEPTHNET else 0
        return False
# F(4,3) along d as well (F(4x4x4): 216 GEMMs, 8x fewer multiply-adds, 3.375x transformed domain) when D % 4 == 0: opt-in.
# Measured 106.3 vs 108.8 ms/step, but the third non-+-1 axis brings the gradient noise of the full-step parity test back
# to 1.1 % (tools/grad_l2_probe.py), so the default keeps F(2,3) along d.
WINO_F444 = os.environ.get("SSBEV_WINO_F444", "0") != "0"
WINO_F444_MIN_CIN = int(os.environ.get("SSBEV_WINO_F444_MIN_CIN", "0"))     # with F444 on: only layers at least this wide


# Default realisation of the wide 3-D layers (r2): F(4,3)^2 over (h, w) in memory + F(2,3) along d in registers inside the
# hand-written MFMA contraction csrc/winograd_fused.hip (forward, data and weight gradient): no library GEMM, transformed
# tensors 2.25x instead of 4.5x.  SSBEV_WINO_DF=0 restores the F(2x4x4) transforms + 144 batched rocBLAS GEMMs.
WINO_DF = os.environ.get("SSBEV_WINO_DF", "1") != "0"
WINO_DF_MIN_ROWS = int(os.environ.get("SSBEV_WINO_DF_MIN_ROWS", "1024"))


def _wino_df_applicable(B, D, H, W, Cin, Cout):
    if not (WINO_DF and WINO_F43 and PRECISION == "fp32" and not (WINO_DEPTH_FUSED or WINO_OWN_GEMM or WINO_F444)):
        return False
    # Layers with few rows per frequency (512 channels on the 32 x 32 x 4 grid: 256 rows against 4 x 512 x 512 weights per
    # frequency) are weight-streaming problems: 151 MB of transformed weights for 10 GF of MFMA work.  The row-blocked fused
    # kernel re-reads that slab per 32-row block; they stay on the 144-GEMM pipeline (SSBEV_WINO_DF_MIN_ROWS=0: all fused).
    if B * D * (H // 4) * (W // 4) < WINO_DF_MIN_ROWS:
        return False
    lib = capi.load()
    return bool(lib.ssbev_wino43_df_supported(C.byref(capi.WinoDims(B, D, H, W, Cin)), Cout)) and \
        bool(lib.ssbev_wino43_df_supported(C.byref(capi.WinoDims(B, D, H, W, Cout)), Cin)) and Cout % 4 == 0


def _wino_df_gemm(xcl, w, B, D, H, W, K, N, mode, tag, fl, into=None):
    """(h,w) input transform -> depth-fused MFMA contraction -> (h,w) output transform of a channels-last volume with K
    input / N output channels.  mode 0: forward (w [N,K,3,3,3]); mode 1: data gradient (w [K,N,3,3,3], mirrored taps).
    Returns (y_cl, P) -- P [36, B*D*H/4*W/4, K] is what the weight gradient needs."""
    lib = capi.load()
    Cout, Cin = (N, K) if mode == 0 else (K, N)
    R = B * D * (H // 4) * (W // 4)
    with _span("wino_transform", 0.0, 4.0 * xcl.numel() * 3.25, tag + " in"):
        P = _wino_call("ssbev_wino43_2d_input_transform", xcl, capi.WinoDims(B, D, H, W, K), (36, R, K))
    Wp = torch.empty(lib.ssbev_wino43_df_packed_elems(Cout, Cin), dtype=torch.float32, device=xcl.device)
    capi.check(lib.ssbev_wino43_df_pack(capi.ptr(w), capi.ptr(Wp), Cout, Cin, mode, capi.stream()), "ssbev_wino43_df_pack")
    Mo = torch.empty(36, R, N, dtype=torch.float32, device=xcl.device)
    dims = capi.WinoDims(B, D, H, W, K)
    nby = 4.0 * (P.numel() + Mo.numel() + Wp.numel())          # the kernel's own operands: P and Mo are 2.25x the activations
    # span family "conv_wino_fused:<MT><NW>": one entry per template instance of wino_df_kernel (= per kernel symbol)
    with _span(f"conv_wino_fused:{lib.ssbev_wino43_df_instance(C.byref(dims), N)}" if KERNEL_TIMER is not None else "conv_wino_fused",
               fl, nby, tag, fl / 6.0):
        capi.check(lib.ssbev_wino43_df_gemm(capi.ptr(P), capi.ptr(Wp), capi.ptr(Mo), C.byref(dims), N, capi.stream()),
                   "ssbev_wino43_df_gemm")
    with _span("wino_transform", 0.0, 4.0 * B * D * H * W * N * (3.25 + (into is not None)), tag + " out"):
        if into is not None:          # gradient slot: add to the gradient another consumer already left there
            odims = capi.WinoDims(B, D, H, W, N)
            capi.check(lib.ssbev_wino43_2d_output_transform_acc(capi.ptr(Mo), capi.ptr(into), C.byref(odims), capi.stream()),
                       "ssbev_wino43_2d_output_transform_acc")
            y = into
        else:
            y = _wino_call("ssbev_wino43_2d_output_transform", Mo, capi.WinoDims(B, D, H, W, N), (B, D, H, W, N))
    return y, P


class _WinoConvDF(torch.autograd.Function):
    """3x3x3 / stride 1 / pad 1 convolution on the depth-fused Winograd kernels (see WINO_DF)."""

    @staticmethod
    def forward(ctx, x, weight, slot=None):
        ctx.slot = slot
        if ctx.needs_input_grad[1]:
            streams.note_use(weight)
        xcl = to_cl(_f32(x, "wino_conv"))
        B, D, H, W, Cin = xcl.shape
        Cout = weight.shape[0]
        fl = 2.0 * B * D * H * W * Cin * Cout * 27
        w = weight.detach().contiguous()
        y, P = _wino_df_gemm(xcl, w, B, D, H, W, Cin, Cout, 0, f"winoDF fwd {Cin}->{Cout} {D}x{H}x{W}", fl)
        ctx.save_for_backward(P if weight.requires_grad else None, weight)
        ctx.geom = (B, D, H, W, Cin, Cout, fl)
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        P, weight = ctx.saved_tensors
        B, D, H, W, Cin, Cout, fl = ctx.geom
        gcl = to_cl(gy)
        lib = capi.load()
        w = weight.detach().contiguous()

        def weight_gradient():
            R = B * D * (H // 4) * (W // 4)
            with _span("wino_transform", 0.0, 4.0 * gcl.numel() * 3.25, "winoDF wgrad adjoint"):
                Z = _wino_call("ssbev_wino43_2d_output_adjoint", gcl, capi.WinoDims(B, D, H, W, Cout), (36, R, Cout))
            dims = capi.WinoDims(B, D, H, W, Cin)
            ws = _ws(lib.ssbev_wino43_df_wgrad_workspace(C.byref(dims), Cout), gy.device)
            gwt = torch.empty_like(w)
            nby = 4.0 * (P.numel() + Z.numel() + 144 * Cin * Cout)
            with _span("conv_wino_fused_wgrad", fl, nby, f"winoDF wgrad {Cin}->{Cout} {D}x{H}x{W}", fl / 6.0):
                capi.check(lib.ssbev_wino43_df_wgrad(capi.ptr(P), capi.ptr(Z), capi.ptr(gwt), C.byref(dims), Cout, capi.ptr(ws),
                                                     ws.numel(), capi.stream()), "ssbev_wino43_df_wgrad")
            return gwt

        def data_gradient():
            into = _slot_target(ctx.slot, torch.empty((B, D, H, W, Cin), device="meta"))
            gxcl, _ = _wino_df_gemm(gcl, w, B, D, H, W, Cout, Cin, 1, f"winoDF dgrad {Cin}->{Cout} {D}x{H}x{W}", fl, into=into)
            if ctx.slot is not None:
                ctx.slot.buf = gxcl
            return from_cl(gxcl)

        want = (ctx.needs_input_grad[0], ctx.needs_input_grad[1], False)
        return _conv_grads(gy.device, weight, want, False, (gcl, P), weight_gradient, data_gradient)


class _WinoConv(torch.autograd.Function):
    """3x3(x3) / stride 1 / pad 1 convolution in the Winograd domain: HIP transforms + NF plain GEMMs.  x logical
    [B,Cin,D,H,W] channels-last, weight [Cout,Cin,kd,3,3] with kd = 3 (3-D, even D) or kd = 1 (2-D over (H,W); D is a
    batch axis).  Tiles: F(4,3) along h and w when both are multiples of 4 (NF = 144 / 36), else F(2,3) (NF = 64 / 16).
    ``dil`` > 1 (2-D fp32 only): dilation = padding = dil on the strided-tile F(2,3) transforms (see WINO_DILATED); any H, W."""

    @staticmethod
    def _plan(three_d, D, H, W, bf, cin=1 << 30, dil=1):
        # bf16 mode stays on F(2,3): its +-1 transforms add no error of their own, while the F(4,3) matrices amplify the
        # bf16 rounding of V / M by their 4 / 5 / 8 entries (measured: 11 % max error against 1 % for F(2,3))
        f43 = WINO_F43 and (three_d or WINO_F43_2D or _F43_2D_SCOPE > 0) and not bf and H % 4 == 0 and W % 4 == 0 and dil == 1 and \
            not (three_d and (WINO_DEPTH_FUSED or WINO_OWN_GEMM))
        if f43 and three_d and WINO_F444 and D % 4 == 0 and cin >= WINO_F444_MIN_CIN:
            return 4, "ssbev_wino444_", 216, 4, 8.0
        if f43:
            pre = "ssbev_wino43_" if three_d else "ssbev_wino43_2d_"
            nf, th, reduction = (144, 4, 6.0) if three_d else (36, 4, 4.0)
        else:
            pre = "ssbev_wino_" if three_d else "ssbev_wino2d_"
            nf, th, reduction = (64, 2, 3.375) if three_d else (16, 2, 2.25)
        return (1 if f43 else 0), pre, nf, th, reduction

    @staticmethod
    def forward(ctx, x, weight, slot=None, dil=1):
        ctx.slot = slot
        if ctx.needs_input_grad[1]:
            streams.note_use(weight)
        bf = PRECISION != "fp32"
        if dil > 1 and (bf or weight.shape[2] != 1):
            raise capi.SsbevError("dilated Winograd: 2-D fp32 layers only")
        a16 = storage_bf16()              # bf16 tensors on the activation side too (`_bf16a` transforms)
        xcl = to_cl(x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)) if a16 else to_cl(_f32(x, "wino_conv"))
        B, D, H, W, Cin = xcl.shape
        Cout, three_d = weight.shape[0], weight.shape[2] == 3
        f43, pre, nf, th, red = _WinoConv._plan(three_d, D, H, W, bf, Cin, dil)
        T = B * (D // (4 if f43 == 4 else 2) if three_d else D) * (H // th) * (W // th)
        dtag = ""
        if dil > 1:                       # every residue class tiled on its own: more tiles than (H / 2) (W / 2)
            T = B * D * wino2d_axis_tiles(H, dil) * wino2d_axis_tiles(W, dil)
            red *= B * D * H * W / (4.0 * T)
            dtag = f" d{dil}"
        lib = capi.load()
        w = weight.detach().contiguous()
        fl = 2.0 * B * D * H * W * Cin * Cout * (27 if three_d else 9)
        fused = three_d and WINO_DEPTH_FUSED and not bf and not f43
        wt = lib.ssbev_wino43_weight_transform if f43 else lib.ssbev_wino_weight_transform
        wdim = 4 if f43 == 4 else (3 if three_d else 2)
        if not fused:
            U = torch.empty(nf, Cin, Cout, dtype=torch.float32, device=x.device)
            capi.check(wt(capi.ptr(w), capi.ptr(U), Cout, Cin, wdim, 0, capi.stream()), "ssbev_wino_weight_transform")
        tag = f"wino{ {0: '', 1: '43', 4: '444'}[f43]} fwd {Cin}->{Cout} {D}x{H}x{W}{dtag}"
        nby = 4.0 * (B * D * H * W * (Cin + Cout) + (27 if three_d else 9) * Cin * Cout)
        with _span("conv_winograd", fl, nby, tag, fl / red):
            if fused:      # (h,w)-transformed tensors only (4x), the depth axis of F(2,3) inside the GEMM kernel
                y = _wino_depth_fused(xcl, w, B, D, H, W, Cin, Cout, 0)
                V = None
            elif bf:
                sfx = "_bf16a" if a16 else "_bf16"
                V = _wino_call(pre + "input_transform" + sfx, xcl, capi.WinoDims(B, D, H, W, Cin, dil), (nf, T, Cin), torch.bfloat16)
                M = _bmm16(V, U)
                y = _wino_call(pre + "output_transform" + sfx, M, capi.WinoDims(B, D, H, W, Cout, dil), (B, D, H, W, Cout),
                               torch.bfloat16 if a16 else torch.float32)
            else:
                V = _wino_call(pre + "input_transform", xcl, capi.WinoDims(B, D, H, W, Cin, dil), (nf, T, Cin))
                M = _wino_bgemm(V, w, Cout, Cin, 0) if (three_d and WINO_OWN_GEMM and not f43) else (gemm_nn(V, U, tag=tag + " gemm") if own_gemm_site("wino") else torch.bmm(V, U))
                y = _wino_call(pre + "output_transform", M, capi.WinoDims(B, D, H, W, Cout, dil), (B, D, H, W, Cout))
        ctx.save_for_backward(xcl if fused else V, weight)
        ctx.geom = (B, D, H, W, Cin, Cout, T, three_d, fl, fused, bf, f43, pre, nf, red, a16, dil)
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        V, weight = ctx.saved_tensors            # (depth-fused path: V is the channels-last input, transformed below)
        B, D, H, W, Cin, Cout, T, three_d, fl, fused, bf, f43, pre, nf, red, a16, dil = ctx.geom
        dtag = f" d{dil}" if dil > 1 else ""
        sfx, fdt = (("_bf16a" if a16 else "_bf16"), torch.bfloat16) if bf else ("", torch.float32)
        gcl = to_cl(gy)
        if a16 and gcl.dtype != torch.bfloat16:
            gcl = gcl.to(torch.bfloat16)
        adt = torch.bfloat16 if a16 else torch.float32          # dtype of the activation-side tensors
        lib = capi.load()
        w = weight.detach().contiguous()
        nd = 4 if f43 == 4 else (3 if three_d else 2)
        gx = gw = None
        vtag = {0: "", 1: "43", 4: "444"}[f43]
        nby = 4.0 * (B * D * H * W * (Cin + Cout) + (27 if three_d else 9) * Cin * Cout)
        if ctx.needs_input_grad[0] and fused:
            with _span("conv_winograd", fl, nby, f"wino dgrad {Cin}->{Cout} {D}x{H}x{W}", fl / red):
                gx = from_cl(_wino_depth_fused(gcl, w, B, D, H, W, Cout, Cin, 1))
        elif ctx.needs_input_grad[0]:
            Ut = torch.empty(nf, Cout, Cin, dtype=torch.float32, device=gy.device)
            wt = lib.ssbev_wino43_weight_transform if f43 else lib.ssbev_wino_weight_transform
            capi.check(wt(capi.ptr(w), capi.ptr(Ut), Cout, Cin, nd, 1, capi.stream()), "ssbev_wino_weight_transform")
            with _span("conv_winograd", fl, nby, f"wino{vtag} dgrad {Cin}->{Cout} {D}x{H}x{W}{dtag}", fl / red):
                Vg = _wino_call(pre + "input_transform" + sfx, gcl, capi.WinoDims(B, D, H, W, Cout, dil), (nf, T, Cout), fdt)
                Mx = _wino_bgemm(Vg, w, Cout, Cin, 1) if (three_d and WINO_OWN_GEMM and not bf and not f43) \
                    else ((_bmm16(Vg, Ut) if fdt == torch.bfloat16 else torch.bmm(Vg, Ut.to(fdt))) if (bf or not own_gemm_site("wino")) else gemm_nn(Vg, Ut, tag="wino dgrad gemm"))
                del Vg
                acc_fn = {"ssbev_wino2d_": "ssbev_wino2d_output_transform_acc",
                          "ssbev_wino43_2d_": "ssbev_wino43_2d_output_transform_acc"}.get(pre) if not bf else None
                into = _slot_target(ctx.slot, torch.empty((B, D, H, W, Cin), device="meta")) if acc_fn else None
                if into is not None:
                    odims = capi.WinoDims(B, D, H, W, Cin, dil)
                    capi.check(getattr(lib, acc_fn)(capi.ptr(Mx), capi.ptr(into), C.byref(odims), capi.stream()), acc_fn)
                    gxcl = into
                else:
                    gxcl = _wino_call(pre + "output_transform" + sfx, Mx, capi.WinoDims(B, D, H, W, Cin, dil), (B, D, H, W, Cin), adt)
                if ctx.slot is not None:
                    ctx.slot.buf = gxcl
            gx = from_cl(gxcl)
        if ctx.needs_input_grad[1]:
            def weight_gradient(V=V):
                with _span("conv_winograd_wgrad", fl, nby, f"wino{vtag} wgrad {Cin}->{Cout} {D}x{H}x{W}{dtag}", fl / red):
                    if fused:
                        V = _wino_call(pre + "input_transform", V, capi.WinoDims(B, D, H, W, Cin, dil), (nf, T, Cin))
                    Z = _wino_call(pre + "output_adjoint" + sfx, gcl, capi.WinoDims(B, D, H, W, Cout, dil), (nf, T, Cout), fdt)
                    gU = _bmm16_tn(V, Z) if bf else (gemm_tn(V, Z, tag="wino wgrad gemm") if own_gemm_site("wino") else torch.bmm(V.transpose(1, 2), Z))
                gwt = torch.empty_like(w)
                wg = lib.ssbev_wino43_weight_grad if f43 else lib.ssbev_wino_weight_grad
                capi.check(wg(capi.ptr(gU), capi.ptr(gwt), Cout, Cin, nd, capi.stream()), "ssbev_wino_weight_grad")
                return gwt

            if streams.wgrad_on_side(weight):    # after the data gradient here (rocBLAS workspaces are per stream: no reordering)
                with streams.on_side(gy.device, gcl, V) as side:
                    gw = weight_gradient()
                    side.publish(gw)
            else:
                gw = weight_gradient()
        return gx, gw, None, None


def conv_flops_3x3(B, D, H, W, Cin, Cout):
    return 2.0 * B * D * H * W * Cin * Cout * 27


def wino_conv3d_applicable(x, weight, stride, padding, dilation):
    """Wide stride-1 3x3x3 (or 1x3x3) 'same' layers on even grids; narrow ones are memory-bound in the 8x (4x) larger
    transformed domain."""
    return _wino_applicable(x.is_cuda, x.shape, weight.shape, stride, padding, dilation)


def _wino_applicable(is_cuda, xshape, wshape, stride, padding, dilation):
    k = tuple(wshape[2:])
    if k not in ((3, 3, 3), (1, 3, 3)):
        return False
    tiled = xshape[2:] if k[0] == 3 else xshape[3:]                 # kd = 1: the depth axis is a batch axis
    return (is_cuda and tuple(stride) == (1, 1, 1) and tuple(dilation) == (1, 1, 1) and wshape[0] >= 64 and wshape[1] >= 64
            and wshape[1] % 4 == 0 and tuple(padding) == (k[0] // 2, 1, 1) and all(int(n) % 2 == 0 for n in tiled))


# -------------------------------------------------------------------------------------------------
# deformable convolution v1 (DepthNet's DCN)
# -------------------------------------------------------------------------------------------------


class _DcnIm2col(torch.autograd.Function):
    """x [B,C,H,W], offset [B,2*k*k,H,W] -> cols [G, B*H*W, k*k*C/G] (bilinear taps, group-major)."""

    @staticmethod
    def forward(ctx, x, offset, groups, k, pad, dil):
        lib = capi.load()
        xcl, ocl = to_cl(_f32(x, "dcn")), to_cl(_f32(offset, "dcn"))
        B, H, W, Cch = xcl.shape
        d = capi.DcnDims(B, Cch, H, W, groups, k, pad, dil)
        cols = torch.empty(groups, B * H * W, k * k * (Cch // groups), dtype=torch.float32, device=x.device)
        with _span("dcn_sample", 0.0, 4.0 * (xcl.numel() + ocl.numel() + cols.numel()), "fwd   dcn_im2col"):
            capi.check(lib.ssbev_dcn_im2col(capi.ptr(xcl), capi.ptr(ocl), capi.ptr(cols), C.byref(d), capi.stream()),
                       "ssbev_dcn_im2col")
        ctx.save_for_backward(xcl, ocl)
        ctx.d = d
        return cols

    @staticmethod
    def backward(ctx, gcols):
        lib = capi.load()
        xcl, ocl = ctx.saved_tensors
        gx, goff = torch.empty_like(xcl), torch.empty_like(ocl)
        ws = _ws(lib.ssbev_dcn_col2im_workspace(C.byref(ctx.d)), xcl.device)
        with _span("dcn_sample", 0.0, 4.0 * (2 * xcl.numel() + 2 * ocl.numel() + gcols.numel()), "bwd   dcn_col2im"):
            capi.check(lib.ssbev_dcn_col2im(capi.ptr(xcl), capi.ptr(ocl), capi.ptr(gcols.contiguous()), capi.ptr(gx),
                                            capi.ptr(goff), C.byref(ctx.d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_dcn_col2im")
        return from_cl(gx), from_cl(goff), None, None, None, None


def deform_conv2d(x, offset, weight, groups=1, padding=1, dilation=1):
    """mmcv deform_conv2d (v1, stride 1, deform_groups 1, no bias): HIP sampling + one dense MFMA 1x1 conv per group."""
    Cout, Cg, k, _ = weight.shape
    B, _, H, W = x.shape
    cols = _DcnIm2col.apply(x, offset, int(groups), int(k), int(padding), int(dilation))
    Cog = Cout // groups
    Kc = k * k * Cg
    if (x.is_cuda and own_gemm_site("linear") and _gemm_supported(cols) and PRECISION == "fp32" and Cog % 4 == 0 and Kc % 4 == 0):
        # the grouped contraction as ONE batched product per direction, written straight into / read straight out of the
        # channels-last [pixels, Cout] map through the kernels' row and batch strides: no concatenation forward, no 177 MB
        # stack of the column gradients backward (round 6; rounds 2-5: four products + cat / unbind per direction)
        w3 = weight.view(groups, Cog, Cg, k, k).permute(0, 1, 3, 4, 2).reshape(groups, Cog, Kc)
        y2 = _GroupedLinearCL.apply(cols, w3)                              # [B*H*W, Cout]
        return from_cl(y2.view(B, H, W, Cout))
    outs = []
    # unbind, not cols[g]: the backward of four selects is four zero-filled [groups, ...] tensors plus three accumulation adds
    # (0.4 ms per step on the 177 MB column tensor); the backward of unbind is one stack
    for g, cg in enumerate(cols.unbind(0)):
        colg = cg.view(B, H, W, Kc).permute(0, 3, 1, 2)                 # channels-last [B, K*Cg, H, W]
        wg = weight[g * Cog:(g + 1) * Cog].permute(0, 2, 3, 1).reshape(Cog, Kc, 1, 1)
        outs.append(conv2d(colg, wg, None, 1, 0, 1))
    return torch.cat(outs, dim=1) if groups > 1 else outs[0]


class _GroupedLinearCL(torch.autograd.Function):
    """y[r, g * N + n] = sum_k cols[g, r, k] * w[g, n, k]: the group contraction of a grouped pointwise layer (DepthNet's DCN,
    BD:490-498, groups = 4) on the own GEMM kernels, batch element = group.  The group's [R, N] block is a column slice of the
    channels-last [R, G * N] map: leading dimension G * N, batch stride N -- the operand strides of ssbev_gemm_* do the
    concatenation (forward, C side) and the split (backward, A side)."""

    @staticmethod
    def forward(ctx, cols, w3):
        lib = capi.load()
        cols, w3 = cols.contiguous(), w3.contiguous()
        G, R, K = cols.shape
        N = w3.shape[1]
        y = torch.empty(R, G * N, dtype=torch.float32, device=cols.device)
        g = _gdims(R, N, K, G, K, K, G * N, R * K, N * K, N)
        ws = _ws(lib.ssbev_gemm_nt_workspace(C.byref(g)), cols.device)
        with _span("gemm_own", 2.0 * G * R * N * K, 4.0 * (cols.numel() + w3.numel() + y.numel()), f"linear fwd grouped {G}x[{K}->{N}] rows={R}"):
            capi.check(lib.ssbev_gemm_nt(capi.ptr(cols), capi.ptr(w3), None, capi.ptr(y), C.byref(g), capi.ptr(ws), ws.numel(),
                                         capi.stream()), "ssbev_gemm_nt")
        ctx.save_for_backward(cols, w3)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = capi.load()
        cols, w3 = ctx.saved_tensors
        G, R, K = cols.shape
        N = w3.shape[1]
        gy = gy.contiguous()
        gcols = gw = None
        fl = 2.0 * G * R * N * K
        if ctx.needs_input_grad[0]:      # gcols[g] [R, K] = gy[:, g N : (g + 1) N] [R, N] @ w3[g] [N, K]            (NN)
            gcols = torch.empty_like(cols)
            g = _gdims(R, K, N, G, G * N, K, K, N, N * K, R * K)
            ws = _ws(lib.ssbev_gemm_nn_workspace(C.byref(g)), gy.device)
            with _span("gemm_own", fl, 4.0 * (gy.numel() + w3.numel() + gcols.numel()), f"linear dgrad grouped {G}x[{K}->{N}] rows={R}"):
                capi.check(lib.ssbev_gemm_nn(capi.ptr(gy), capi.ptr(w3), None, capi.ptr(gcols), C.byref(g), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_gemm_nn")
        if ctx.needs_input_grad[1]:      # gw[g] [N, K] = gy[:, g N : (g + 1) N]^T [N, R] @ cols[g] [R, K]               (TN)
            gw = torch.empty_like(w3)
            g = _gdims(R, K, N, G, G * N, K, K, N, R * K, N * K)
            ws = _ws(lib.ssbev_gemm_tn_workspace(C.byref(g)), gy.device)
            with _span("gemm_own", fl, 4.0 * (gy.numel() + cols.numel() + gw.numel()), f"linear wgrad grouped {G}x[{K}->{N}] rows={R}"):
                capi.check(lib.ssbev_gemm_tn(capi.ptr(gy), capi.ptr(cols), capi.ptr(gw), C.byref(g), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_gemm_tn")
        return gcols, gw


# -------------------------------------------------------------------------------------------------
# normalisation
# -------------------------------------------------------------------------------------------------


# The fused ReLU's sign pattern travels to backward as a bit mask (1/32 of the tensor) instead of y being re-read twice
GN_RELU_MASK = os.environ.get("SSBEV_GN_RELU_MASK", "1") != "0"


def _norm_ext(device, running=None, n=0):
    """ssbev_norm_ext: (running_mean, running_var, momentum) of a training-mode BatchNorm, updated inside the statistics finalize."""
    e = capi.NormExt(None, None, 0.0, int(n))
    if running is not None:
        e.running_mean, e.running_var, e.momentum = running[0].data_ptr(), running[1].data_ptr(), float(running[2])
    return e


class _GroupNorm(torch.autograd.Function):
    """GroupNorm on a channels-last volume with optional fused residual add and ReLU."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual, groups, eps, relu, as_batch, given_mean, given_rstd, pre_act=0, res_slot=None,
                running=None):
        lib = capi.load()
        ctx.res_slot = res_slot
        ctx.set_materialize_grads(False)           # no zero tensors for the (non-differentiable) statistics outputs
        xcl, io = _act(to_cl(x), "group_norm")
        Cch = xcl.shape[-1]
        B = 1 if as_batch else xcl.shape[0]
        S = xcl.numel() // (B * Cch)
        rcl = to_cl(residual if residual.dtype == xcl.dtype else residual.to(xcl.dtype)) if residual is not None else None
        given = given_mean is not None
        d = capi.NormDims(B, Cch, groups, S, float(eps), int(relu), int(given), int(pre_act), 0, 0, io)
        y = torch.empty_like(xcl)
        mean = given_mean.contiguous() if given else torch.empty(B * groups, dtype=torch.float32, device=x.device)
        rstd = given_rstd.contiguous() if given else torch.empty(B * groups, dtype=torch.float32, device=x.device)
        ws = _ws(lib.ssbev_groupnorm_workspace(C.byref(d)), x.device)
        w, b = weight.detach().contiguous(), bias.detach().contiguous()
        nb = float(xcl.element_size()) * xcl.numel() * (3 + (residual is not None) - 2 * given)      # stats read + apply read/write
        use_mask = bool(relu) and GN_RELU_MASK and not given and any(ctx.needs_input_grad[:4])
        mask = torch.empty(lib.ssbev_groupnorm_mask_words(C.byref(d)), dtype=torch.int64, device=x.device) if use_mask else None
        ext = _norm_ext(x.device, running, B * S)
        with _span("groupnorm", 0.0, nb, f"fwd   N C={Cch} G={groups} S={S} res={int(residual is not None)}"):
            capi.check(lib.ssbev_groupnorm_fwd_ext(capi.ptr(xcl), capi.ptr(w), capi.ptr(b), capi.ptr(rcl), capi.ptr(y),
                                                   capi.ptr(mean), capi.ptr(rstd), capi.ptr(mask) if use_mask else None,
                                                   C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_groupnorm_fwd_ext")
        ctx.save_for_backward(xcl, (mask if use_mask else y) if relu else None, w, mean, rstd)
        ctx.use_mask = use_mask
        ctx.meta = (B, S, Cch, groups, float(eps), int(relu), residual is not None, given, int(pre_act), io)
        ctx.mark_non_differentiable(mean, rstd)
        return from_cl(y), mean, rstd

    @staticmethod
    def backward(ctx, gy, _gm, _gr):
        lib = capi.load()
        xcl, y, w, mean, rstd = ctx.saved_tensors
        B, S, Cch, groups, eps, relu, has_res, given, pre_act, io = ctx.meta
        if given:
            raise capi.SsbevError("eval-mode (given statistics) normalisation has no HIP backward; use torch for it")
        gcl = to_cl(gy if gy.dtype == xcl.dtype else gy.to(xcl.dtype))
        d = capi.NormDims(B, Cch, groups, S, eps, relu, 0, pre_act, 0, 0, io)
        gx = torch.empty_like(xcl)
        gres = torch.empty_like(xcl) if has_res else None
        gg = torch.empty(Cch, dtype=torch.float32, device=gy.device)
        gb = torch.empty(Cch, dtype=torch.float32, device=gy.device)
        ws = _ws(lib.ssbev_groupnorm_workspace(C.byref(d)), gy.device)
        # stats: x, gy (, y); apply: x, gy (, y) -> gx (, gres); the ReLU bit mask replaces both y reads
        nb = float(xcl.element_size()) * xcl.numel() * (5 + (relu and not ctx.use_mask) + has_res)
        ext = _norm_ext(gy.device)
        with _span("groupnorm", 0.0, nb, f"bwd   N C={Cch} G={groups} S={S} res={int(has_res)}"):
            capi.check(lib.ssbev_groupnorm_bwd_ext(capi.ptr(gcl), capi.ptr(xcl), None if ctx.use_mask else capi.ptr(y),
                                                   capi.ptr(y) if ctx.use_mask else None, capi.ptr(w), capi.ptr(mean),
                                                   capi.ptr(rstd), capi.ptr(gx), capi.ptr(gres), capi.ptr(gg), capi.ptr(gb),
                                                   C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_groupnorm_bwd_ext")
        if has_res and ctx.res_slot is not None and ctx.res_slot.buf is None:
            ctx.res_slot.buf = gres        # first gradient of a forked activation: later consumers accumulate into it
        return from_cl(gx), gg, gb, (from_cl(gres) if has_res else None), None, None, None, None, None, None, None, None, None


NORM_CAT = os.environ.get("SSBEV_NORM_CAT", "1") != "0"     # concatenations of normalised branches without torch.cat (0 = cat)


class _NormCat(torch.autograd.Function):
    """``torch.cat([relu?(norm_i(x_i)) for i], dim=1)`` with every normalisation writing straight into its channel slice of
    the concatenated channels-last tensor (``ssbev_norm_dims.ld_y``) and reading its slice of the incoming gradient in place
    (``ld_gy``): no concatenation pass forward, no slice copies backward (SECONDFPN3D, second_fpn3d.py:113-116: 0.4 GB written
    and re-read per step; ASPP, BD:404-410).  ``parts``: (groups, eps, as_batch) per branch; tensors: x_i, weight_i, bias_i."""

    @staticmethod
    def forward(ctx, parts, relu, running, *tensors):
        lib = capi.load()
        ctx.set_materialize_grads(False)
        n = len(parts)
        extra = tensors[3 * n] if len(tensors) > 3 * n else None     # an un-normalised last branch (ASPP's image-level one)
        xs = [to_cl(tensors[3 * i]) for i in range(n)]
        adt = xs[0].dtype if all(x.dtype == xs[0].dtype for x in xs) else torch.float32      # one storage type for the whole cat
        if adt == torch.bfloat16 and (any(x.shape[-1] % 8 for x in xs) or (extra is not None and extra.shape[1] % 8)):
            adt = torch.float32            # 16-byte bf16 lanes need channel slices that start and end on multiples of 8
        xs = [_act(x if x.dtype == adt else x.to(adt), "norm_cat")[0] for x in xs]
        io, esz = (1, 2) if adt == torch.bfloat16 else (0, 4)
        ws_ = [tensors[3 * i + 1].detach().contiguous() for i in range(n)]
        bs_ = [tensors[3 * i + 2].detach().contiguous() for i in range(n)]
        Cs = [x.shape[-1] for x in xs]
        Ctot = sum(Cs) + (extra.shape[1] if extra is not None else 0)
        out = torch.empty(xs[0].shape[:-1] + (Ctot,), dtype=adt, device=xs[0].device)
        if extra is not None:
            out[..., sum(Cs):].copy_(extra.detach().movedim(1, -1))
        saved, stats, metas = [], [], []
        c0 = 0
        for i, (groups, eps, as_batch) in enumerate(parts):
            x = xs[i]
            B = 1 if as_batch else x.shape[0]
            S = x.numel() // (B * Cs[i])
            d = capi.NormDims(B, Cs[i], groups, S, float(eps), int(relu), 0, 0, Ctot, 0, io)
            mean = torch.empty(B * groups, dtype=torch.float32, device=x.device)
            rstd = torch.empty(B * groups, dtype=torch.float32, device=x.device)
            ws = _ws(lib.ssbev_groupnorm_workspace(C.byref(d)), x.device)
            mask = torch.empty(lib.ssbev_groupnorm_mask_words(C.byref(d)), dtype=torch.int64, device=x.device) if relu else None
            run = running[i] if running is not None else None
            ext = _norm_ext(x.device, run, B * S)
            with _span("groupnorm", 0.0, 3.0 * esz * x.numel(), f"fwd   N C={Cs[i]} G={groups} S={S} cat@{c0}/{Ctot}"):
                capi.check(lib.ssbev_groupnorm_fwd_ext(capi.ptr(x), capi.ptr(ws_[i]), capi.ptr(bs_[i]), None,
                                                       C.c_void_p(out.data_ptr() + esz * c0), capi.ptr(mean), capi.ptr(rstd), capi.ptr(mask),
                                                       C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(), capi.stream()),
                           "ssbev_groupnorm_fwd_ext")
            saved += [x, mask, ws_[i], mean, rstd]
            stats += [mean, rstd]
            metas.append((B, S, Cs[i], groups, float(eps), c0))
            c0 += Cs[i]
        ctx.save_for_backward(*[t for t in saved if t is not None])
        ctx.has_mask = bool(relu)
        ctx.metas, ctx.relu, ctx.Ctot, ctx.io = metas, int(relu), Ctot, io
        ctx.extra_at = sum(Cs) if extra is not None else None
        ctx.mark_non_differentiable(*stats)
        return (from_cl(out), *stats)

    @staticmethod
    def backward(ctx, gy, *_):
        lib = capi.load()
        per = 5 if ctx.has_mask else 4
        sv = ctx.saved_tensors
        adt, esz = (torch.bfloat16, 2) if ctx.io else (torch.float32, 4)
        gcl = to_cl(gy if gy.dtype == adt else gy.to(adt))    # the whole concatenated gradient, channels-last
        grads = []
        for i, (B, S, Cch, groups, eps, c0) in enumerate(ctx.metas):
            if ctx.has_mask:
                x, mask, w, mean, rstd = sv[per * i: per * i + 5]
            else:
                (x, w, mean, rstd), mask = sv[per * i: per * i + 4], None
            d = capi.NormDims(B, Cch, groups, S, eps, ctx.relu, 0, 0, 0, ctx.Ctot, ctx.io)
            gx = torch.empty_like(x)
            gg = torch.empty(Cch, dtype=torch.float32, device=gy.device)
            gb = torch.empty(Cch, dtype=torch.float32, device=gy.device)
            ws = _ws(lib.ssbev_groupnorm_workspace(C.byref(d)), gy.device)
            ext = _norm_ext(gy.device)
            with _span("groupnorm", 0.0, 5.0 * esz * x.numel(), f"bwd   N C={Cch} G={groups} S={S} cat@{c0}/{ctx.Ctot}"):
                capi.check(lib.ssbev_groupnorm_bwd_ext(C.c_void_p(gcl.data_ptr() + esz * c0), capi.ptr(x), None, capi.ptr(mask),
                                                       capi.ptr(w), capi.ptr(mean), capi.ptr(rstd), capi.ptr(gx), None, capi.ptr(gg),
                                                       capi.ptr(gb), C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(), capi.stream()),
                           "ssbev_groupnorm_bwd_ext")
            grads += [from_cl(gx), gg, gb]
        if ctx.extra_at is not None:
            grads.append(gcl[..., ctx.extra_at:].movedim(-1, 1))
        return (None, None, None, *grads)


def norm_cat(xs, norms, relu=True, extra=None, running=None):
    """Concatenation along the channel axis of relu?(norm_i(x_i)) (+ ``extra`` as it is, behind them): ``norms`` = (weight, bias,
    groups, eps, as_batch) per branch; ``running``: per branch None or (running_mean, running_var, momentum) of a training-mode
    BatchNorm, updated inside the operator.  Returns (y, [(mean_i, rstd_i)])."""
    parts = tuple((int(g), float(e), bool(ab)) for (_, _, g, e, ab) in norms)
    flat = []
    for x, (w, b, _, _, _) in zip(xs, norms):
        flat += [x, w, b]
    if extra is not None:
        flat.append(extra)
    out = _NormCat.apply(parts, bool(relu), running, *flat)
    return out[0], [(out[1 + 2 * i], out[2 + 2 * i]) for i in range(len(xs))]


def norm_cat_supported(xs):
    return (NORM_CAT and GN_RELU_MASK and all(x.is_cuda and x.dtype in (torch.float32, torch.bfloat16) and x.shape[1] % 4 == 0 for x in xs)
            and all(x.shape[0] == xs[0].shape[0] and x.shape[2:] == xs[0].shape[2:] for x in xs))


def group_norm(x, groups, weight, bias, eps=1e-5, residual=None, relu=False, pre_act=None):
    """relu?(GroupNorm(act?(x)) + residual?) on a channels-last volume (any spatial rank); ``pre_act="gelu"`` normalises
    gelu(x) (exact form) without materialising it."""
    if pre_act not in (None, "gelu"):
        raise ValueError(f"group_norm: unknown pre_act {pre_act!r}")
    return _GroupNorm.apply(x, weight, bias, residual, int(groups), eps, relu, False, None, None, 1 if pre_act else 0,
                            _slot_of(residual))[0]


def batch_norm_train(x, weight, bias, eps=1e-5, residual=None, relu=False, running=None):
    """Training-mode BatchNorm (batch statistics): returns (y, mean[C], rstd[C]).  ``running`` = (running_mean, running_var,
    momentum): nn.BatchNorm's momentum update of the running statistics, done inside the operator (in the finalize tail of
    the statistics kernel; no launch of its own)."""
    return _GroupNorm.apply(x, weight, bias, residual, x.shape[1], eps, relu, True, None, None, 0, _slot_of(residual), running)


def bn_update_running_(running_mean, running_var, mean, rstd, momentum, eps, n):
    """In-place momentum update of BatchNorm running statistics from the batch (mean, rstd): one launch."""
    lib = capi.load()
    capi.check(lib.ssbev_bn_update_running(capi.ptr(mean), capi.ptr(rstd), capi.ptr(running_mean), capi.ptr(running_var),
                                           running_mean.numel(), float(momentum), float(eps), int(n), capi.stream()),
               "ssbev_bn_update_running")


def batch_norm_eval(x, weight, bias, running_mean, running_var, eps=1e-5, residual=None, relu=False):
    """Inference-mode BatchNorm with the running statistics (forward only on the HIP path)."""
    rstd = torch.rsqrt(running_var + eps)
    return _GroupNorm.apply(x, weight, bias, residual, x.shape[1], eps, relu, True, running_mean, rstd)[0]


class _DualNorm(torch.autograd.Function):
    """relu?(N_a(xa) + N_b(xb)) in one operator (csrc/groupnorm.hip, ssbev_groupnorm2_*): each side a per-sample GroupNorm or a
    batch normalisation; returns (y, mean_a, rstd_a, mean_b, rstd_b)."""

    @staticmethod
    def forward(ctx, xa, wa, ba, xb, wb, bb, ga, gb, eps_a, eps_b, relu, a_batch, b_batch, run_a=None, run_b=None):
        lib = capi.load()
        ctx.set_materialize_grads(False)
        acl, io = _act(to_cl(xa), "dual_norm")
        bcl = to_cl(xb if xb.dtype == acl.dtype else xb.to(acl.dtype))
        if acl.shape != bcl.shape:
            raise capi.SsbevError(f"dual_norm: shapes differ, {tuple(acl.shape)} vs {tuple(bcl.shape)}")
        B, Cch = acl.shape[0], acl.shape[-1]
        S = acl.numel() // (B * Cch)
        d = capi.Norm2Dims(B, Cch, int(ga), int(gb), S, float(eps_a), float(eps_b), int(relu), int(a_batch), int(b_batch), io)
        dev = xa.device
        y = torch.empty_like(acl)
        mean_a = torch.empty((1 if a_batch else B) * ga, dtype=torch.float32, device=dev)
        rstd_a = torch.empty_like(mean_a)
        mean_b = torch.empty((1 if b_batch else B) * gb, dtype=torch.float32, device=dev)
        rstd_b = torch.empty_like(mean_b)
        nbytes = lib.ssbev_groupnorm2_workspace(C.byref(d))
        if nbytes == 0:
            raise capi.SsbevError("dual_norm: unsupported dims (C % 4, C <= 1024, C % G)")
        ws = _ws(nbytes, dev)
        nd = capi.NormDims(B, Cch, ga, S, float(eps_a), int(relu), 0, 0, 0, 0, io)
        mask = torch.empty(lib.ssbev_groupnorm_mask_words(C.byref(nd)), dtype=torch.int64, device=dev) if relu else None
        wa_, ba_, wb_, bb_ = (t.detach().contiguous() for t in (wa, ba, wb, bb))
        ext = capi.Norm2Ext(None, None, 0.0, None, None, 0.0)
        if run_a is not None and a_batch:
            ext.running_mean_a, ext.running_var_a, ext.momentum_a = run_a[0].data_ptr(), run_a[1].data_ptr(), float(run_a[2])
        if run_b is not None and b_batch:
            ext.running_mean_b, ext.running_var_b, ext.momentum_b = run_b[0].data_ptr(), run_b[1].data_ptr(), float(run_b[2])
        with _span("groupnorm", 0.0, float(acl.element_size()) * acl.numel() * 5, f"fwd   N2 C={Cch} Ga={ga} Gb={gb} S={S}"):
            capi.check(lib.ssbev_groupnorm2_fwd_ext(capi.ptr(acl), capi.ptr(wa_), capi.ptr(ba_), capi.ptr(mean_a), capi.ptr(rstd_a),
                                                    capi.ptr(bcl), capi.ptr(wb_), capi.ptr(bb_), capi.ptr(mean_b), capi.ptr(rstd_b),
                                                    capi.ptr(y), capi.ptr(mask), C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(),
                                                    capi.stream()),
                       "ssbev_groupnorm2_fwd_ext")
        ctx.save_for_backward(acl, bcl, mask, wa_, wb_, mean_a, rstd_a, mean_b, rstd_b)
        ctx.meta = (B, Cch, int(ga), int(gb), S, float(eps_a), float(eps_b), int(relu), int(a_batch), int(b_batch), io)
        ctx.mark_non_differentiable(mean_a, rstd_a, mean_b, rstd_b)
        return from_cl(y), mean_a, rstd_a, mean_b, rstd_b

    @staticmethod
    def backward(ctx, gy, *_unused):
        lib = capi.load()
        acl, bcl, mask, wa_, wb_, mean_a, rstd_a, mean_b, rstd_b = ctx.saved_tensors
        d = capi.Norm2Dims(*ctx.meta)
        Cch, dev = ctx.meta[1], gy.device
        gcl = to_cl(gy if gy.dtype == acl.dtype else gy.to(acl.dtype))
        gxa, gxb = torch.empty_like(acl), torch.empty_like(bcl)
        gga, gba, ggb, gbb = (torch.empty(Cch, dtype=torch.float32, device=dev) for _ in range(4))
        ws = _ws(lib.ssbev_groupnorm2_workspace(C.byref(d)), dev)
        with _span("groupnorm", 0.0, float(acl.element_size()) * acl.numel() * 8, f"bwd   N2 C={Cch} Ga={ctx.meta[2]} Gb={ctx.meta[3]} S={ctx.meta[4]}"):
            ext = capi.Norm2Ext(None, None, 0.0, None, None, 0.0)
            capi.check(lib.ssbev_groupnorm2_bwd_ext(capi.ptr(gcl), capi.ptr(mask), capi.ptr(acl), capi.ptr(wa_), capi.ptr(mean_a),
                                                    capi.ptr(rstd_a), capi.ptr(bcl), capi.ptr(wb_), capi.ptr(mean_b), capi.ptr(rstd_b),
                                                    capi.ptr(gxa), capi.ptr(gxb), capi.ptr(gga), capi.ptr(gba), capi.ptr(ggb),
                                                    capi.ptr(gbb), C.byref(d), C.byref(ext), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_groupnorm2_bwd_ext")
        return from_cl(gxa), gga, gba, from_cl(gxb), ggb, gbb, None, None, None, None, None, None, None, None, None


DUAL_NORM = os.environ.get("SSBEV_DUAL_NORM", "1") != "0"      # 0: the two-operator residual form (A/B timing)


def dual_norm_supported(xa, xb):
    return xa.is_cuda and xa.shape == xb.shape and xa.dim() >= 3 and xa.shape[1] % 4 == 0 and xa.shape[1] <= 1024


def dual_norm(xa, wa, ba, groups_a, eps_a, xb, wb, bb, groups_b, eps_b, relu=False, a_batch=False, b_batch=False,
              running_a=None, running_b=None):
    """relu?(N_a(xa) + N_b(xb)); ``x_batch`` = statistics over the batch axis too (BatchNorm when groups == channels);
    ``running_x`` = (running_mean, running_var, momentum) of a training-mode BatchNorm side, updated inside the operator.
    Returns (y, (mean_a, rstd_a), (mean_b, rstd_b))."""
    y, ma, ra, mb, rb = _DualNorm.apply(xa, wa, ba, xb, wb, bb, int(groups_a), int(groups_b), eps_a, eps_b, relu,
                                        bool(a_batch), bool(b_batch), running_a, running_b)
    return y, (ma, ra), (mb, rb)


# -------------------------------------------------------------------------------------------------
# softmax along a strided axis
# -------------------------------------------------------------------------------------------------


class _SoftmaxAxis(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dim):
        lib = capi.load()
        x = _f32(x, "softmax").contiguous()
        outer = 1
        for n in x.shape[:dim]:
            outer *= n
        Cn = x.shape[dim]
        inner = x.numel() // (outer * Cn)
        y = torch.empty_like(x)
        with _span("softmax", 0.0, 8.0 * x.numel(), "fwd   softmax_axis"):
            capi.check(lib.ssbev_softmax_axis_fwd(capi.ptr(x), capi.ptr(y), outer, Cn, inner, capi.stream()),
                       "ssbev_softmax_axis_fwd")
        ctx.save_for_backward(y)
        ctx.meta = (outer, Cn, inner)
        return y

    @staticmethod
    def backward(ctx, gy):
        lib = capi.load()
        (y,) = ctx.saved_tensors
        outer, Cn, inner = ctx.meta
        gy = gy.contiguous()
        gx = torch.empty_like(y)
        with _span("softmax", 0.0, 12.0 * y.numel(), "bwd   softmax_axis"):
            capi.check(lib.ssbev_softmax_axis_bwd(capi.ptr(y), capi.ptr(gy), capi.ptr(gx), outer, Cn, inner, capi.stream()),
                       "ssbev_softmax_axis_bwd")
        return gx, None


def softmax_rows_(x):
    """In-place softmax over the innermost axis of a contiguous fp32 tensor with rows of <= 8192 floats (the BRI
    attention matrix, attention.py:66-68): ssbev_softmax_rows_fwd, one read + one write.  No autograd."""
    n = x.shape[-1]
    capi.check(capi.load().ssbev_softmax_rows_fwd(capi.ptr(x), capi.ptr(x), x.numel() // n, n, capi.stream()),
               "ssbev_softmax_rows_fwd")
    return x


def softmax_rows_bwd_(y, gy):
    """gy <- y * (gy - sum(y * gy, -1)) in place (softmax backward along the innermost axis)."""
    n = y.shape[-1]
    capi.check(capi.load().ssbev_softmax_rows_bwd(capi.ptr(y), capi.ptr(gy), capi.ptr(gy), y.numel() // n, n,
                                                  capi.stream()), "ssbev_softmax_rows_bwd")
    return gy


def softmax_rows_ok(x):
    return x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.shape[-1] % 4 == 0 and x.shape[-1] <= 8192


def softmax(x, dim):
    """softmax over ``dim``.  A non-innermost axis of a standard-contiguous tensor runs on the strided-axis HIP kernel;
    an axis that is innermost in memory (channels-last 2-D maps) is already a single fast row kernel in ATen."""
    dim = dim % x.dim()
    if x.is_cuda and x.is_contiguous() and dim != x.dim() - 1:
        return _SoftmaxAxis.apply(x, dim)
    return torch.softmax(x, dim)


# -------------------------------------------------------------------------------------------------
# trilinear x2 upsample of the logits
# -------------------------------------------------------------------------------------------------


class _Trilinear2x(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        lib = capi.load()
        xcl = to_cl(_f32(x, "trilinear2x"))
        B, D, H, W, Cch = xcl.shape
        d = capi.UpsampleDims(B, D, H, W, Cch)
        y = torch.empty(B, 2 * D, 2 * H, 2 * W, Cch, dtype=torch.float32, device=x.device)
        with _span("trilinear", 0.0, 4.0 * (xcl.numel() + y.numel()), "fwd   trilinear2x"):
            capi.check(lib.ssbev_trilinear2x_fwd(capi.ptr(xcl), capi.ptr(y), C.byref(d), capi.stream()),
                       "ssbev_trilinear2x_fwd")
        ctx.dims = (B, D, H, W, Cch)
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        lib = capi.load()
        B, D, H, W, Cch = ctx.dims
        gcl = to_cl(gy)
        d = capi.UpsampleDims(B, D, H, W, Cch)
        gx = torch.empty(B, D, H, W, Cch, dtype=torch.float32, device=gy.device)
        with _span("trilinear", 0.0, 4.0 * (gcl.numel() + gx.numel()), "bwd   trilinear2x"):
            capi.check(lib.ssbev_trilinear2x_bwd(capi.ptr(gcl), capi.ptr(gx), C.byref(d), capi.stream()),
                       "ssbev_trilinear2x_bwd")
        return from_cl(gx)


def upsample_trilinear(x, size):
    """F.interpolate(x, size, mode='trilinear', align_corners=False); the exact-x2 case the path uses
    (logits -> label grid) runs on the HIP kernel, any other ratio on ATen's device kernel."""
    size = tuple(int(v) for v in size)
    if tuple(x.shape[-3:]) == size:
        return x
    if all(o == 2 * i for o, i in zip(size, x.shape[-3:])) and x.shape[1] % 4 == 0:
        return _Trilinear2x.apply(x)
    return torch.nn.functional.interpolate(x.contiguous(), size=size, mode="trilinear", align_corners=False)


# -------------------------------------------------------------------------------------------------
# fused occupancy-head epilogue
# -------------------------------------------------------------------------------------------------


class _OccLossSums(torch.autograd.Function):
    """logits [B,20,D,H,W] (coarse), label uint8 [B,2D,2H,2W] -> (diff [41] f64: ce_num, sum_p[20], nom[20];
    aux [3+20+400] f64: ce_den, M, (unused), cnt[20], conf[20][20]).  Only ``diff`` carries gradient."""

    @staticmethod
    def forward(ctx, logits, label_u8, class_weight):
        lib = capi.load()
        xcl = to_cl(_f32(logits, "occ_loss"))
        B, D, H, W, Cch = xcl.shape
        d = capi.UpsampleDims(B, D, H, W, Cch)
        ns = lib.ssbev_occ_loss_num_sums()
        sums = torch.empty(ns, dtype=torch.float64, device=logits.device)
        cw = class_weight.to(device=logits.device, dtype=torch.float32).contiguous()
        lab = label_u8.contiguous()
        ws = _ws(lib.ssbev_occ_loss_workspace(C.byref(d)), logits.device)
        with _span("occ_loss", 0.0, 4.0 * xcl.numel() + lab.numel(), "fwd   occ_loss"):
            capi.check(lib.ssbev_occ_loss_fwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(cw), capi.ptr(sums), C.byref(d),
                                              capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_occ_loss_fwd")
        ctx.save_for_backward(xcl, lab, cw)
        nc = Cch
        diff = torch.cat((sums[0:1], sums[3:3 + 2 * nc]))
        aux = torch.cat((sums[1:3], sums[3 + 2 * nc:]))
        ctx.mark_non_differentiable(aux)
        return diff, aux

    @staticmethod
    def backward(ctx, gdiff, _gaux):
        lib = capi.load()
        xcl, lab, cw = ctx.saved_tensors
        B, D, H, W, Cch = xcl.shape
        d = capi.UpsampleDims(B, D, H, W, Cch)
        coef = gdiff.to(torch.float32).contiguous()
        gx = torch.empty_like(xcl)
        ws = _ws(lib.ssbev_occ_loss_bwd_workspace(C.byref(d)), xcl.device)
        with _span("occ_loss", 0.0, 8.0 * xcl.numel() + lab.numel(), "bwd   occ_loss"):
            capi.check(lib.ssbev_occ_loss_bwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(cw), capi.ptr(coef), capi.ptr(gx),
                                              C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_occ_loss_bwd")
        return from_cl(gx), None, None


def occ_loss_sums(logits, label_u8, class_weight):
    return _OccLossSums.apply(logits, label_u8, class_weight)


def occ_predict_supported(logits, size=None):
    """The fused inference epilogue serves fp32 20-class logits on the GPU and a label grid of exactly twice their size."""
    return (logits.is_cuda and logits.dim() == 5 and logits.shape[1] == 20 and logits.dtype == torch.float32
            and (size is None or tuple(int(v) for v in size) == tuple(2 * int(v) for v in logits.shape[2:])))


@torch.no_grad()
def occ_predict(logits, gt_occ=None, remap=None):
    """Inference epilogue of the head in one pass (``ssbev_occ_predict``): coarse ``logits`` [B,20,d,h,w] ->
    ``(pred_u8 [B,2d,2h,2w], raw_u16 | None, conf_i64 [B,20,20] | None, n_ignored [B] | None)``.
    ``pred`` is exactly ``upsample_trilinear(logits, 2x).argmax(1)``; ``raw = remap[pred]`` when a 20-entry ``remap`` (training id ->
    raw id) is given; with ``gt_occ`` [B,2d,2h,2w] (255 = ignore) the per-sample confusion counts [gt][pred] over the labelled
    voxels and the number of ignored ones come back too.  The up-sampled logits are never written.  No fallback: CPU tensors, a
    class count other than 20 or a label grid that is not exactly x2 raise ``SsbevError``."""
    if not logits.is_cuda:
        raise capi.SsbevError("occ_predict: ssbev operators run on the MI355X only: got a CPU tensor (no CPU fallback exists)")
    if logits.dim() != 5 or logits.shape[1] != 20:
        raise capi.SsbevError(f"occ_predict: logits [B,20,d,h,w] expected, got {tuple(logits.shape)}")
    lib = capi.load()
    xcl = to_cl(_f32(logits, "occ_predict"))
    B, D, H, W, Cch = xcl.shape
    fine = (B, 2 * D, 2 * H, 2 * W)
    dev = logits.device
    d = capi.UpsampleDims(B, D, H, W, Cch)
    lab = conf = nign = raw = tab = None
    ws_bytes = 0
    if gt_occ is not None:
        if tuple(gt_occ.shape) != fine:
            raise capi.SsbevError(f"occ_predict: label grid {tuple(gt_occ.shape)} is not exactly twice the logits' {tuple(xcl.shape[:4])}")
        lab = gt_occ.to(device=dev, dtype=torch.uint8).contiguous()       # classes 0..19, 255 = ignore
        conf = torch.empty(B, Cch, Cch, dtype=torch.int64, device=dev)
        nign = torch.empty(B, dtype=torch.int64, device=dev)
        ws_bytes = lib.ssbev_occ_predict_workspace(C.byref(d))
    if remap is not None:
        tab = np.ascontiguousarray(np.asarray(remap).reshape(-1), dtype=np.uint16)
        if tab.size != Cch:
            raise capi.SsbevError(f"occ_predict: remap needs {Cch} entries, got {tab.size}")
        raw = torch.empty(fine, dtype=torch.uint16, device=dev)
    pred = torch.empty(fine, dtype=torch.uint8, device=dev)
    ws = _ws(ws_bytes, dev)
    with _span("occ_predict", 0.0, 4.0 * xcl.numel() + pred.numel() * (1 + (lab is not None) + 2 * (raw is not None)), "fwd   occ_predict"):
        capi.check(lib.ssbev_occ_predict(capi.ptr(xcl), capi.ptr(lab), None if tab is None else C.c_void_p(tab.ctypes.data),
                                         capi.ptr(pred), capi.ptr(raw), capi.ptr(conf), capi.ptr(nign), C.byref(d), capi.ptr(ws),
                                         ws.numel(), capi.stream()), "ssbev_occ_predict")
    return pred, raw, conf, nign


LOVASZ = os.environ.get("SSBEV_LOVASZ", "1") != "0"          # fused Lovasz-softmax (0 = the tensor form: softmax + one torch.sort per class)


def lovasz_supported(logits, label):
    """The fused Lovasz-softmax serves fp32 20-class logits on the GPU that sit on the label grid or at exactly half of it."""
    if not (logits.is_cuda and logits.dim() == 5 and logits.shape[1] == 20 and logits.dtype == torch.float32 and label.dim() == 4
            and label.shape[0] == logits.shape[0]):
        return False
    fine, coarse = tuple(int(v) for v in label.shape[1:]), tuple(int(v) for v in logits.shape[2:])
    return fine == coarse or fine == tuple(2 * v for v in coarse)


class _LovaszSoftmax(torch.autograd.Function):
    """logits [B,20,D,H,W], label uint8 [B,D',H',W'] (the same grid or exactly twice it) -> the unweighted Lovasz-softmax loss
    (0-dim fp32), ``ssbev_lovasz_fwd / _bwd``.  Forward keeps dJ per [voxel][class] and the per-class counts on the device;
    nothing is read back."""

    @staticmethod
    def forward(ctx, logits, label_u8, ignore):
        lib = capi.load()
        xcl = to_cl(_f32(logits, "lovasz_softmax"))
        B, D, H, W, Cch = xcl.shape
        lab = label_u8.contiguous()
        up = int(tuple(lab.shape[1:]) != (D, H, W))
        d = capi.LovaszDims(B, D, H, W, Cch, int(ignore), up)
        dev = logits.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        dj = torch.empty(lab.numel(), Cch, dtype=torch.float32, device=dev)
        counts = torch.empty(lib.ssbev_lovasz_num_counts(), dtype=torch.int32, device=dev)
        ws = _ws(lib.ssbev_lovasz_workspace(C.byref(d)), dev)
        with _span("lovasz", 0.0, 4.0 * xcl.numel() + lab.numel() + 4.0 * 37 * dj.numel(), "fwd   lovasz"):
            capi.check(lib.ssbev_lovasz_fwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(loss), capi.ptr(dj), capi.ptr(counts),
                                            C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_lovasz_fwd")
        ctx.save_for_backward(xcl, lab, dj, counts)
        ctx.dims = d
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        xcl, lab, dj, counts = ctx.saved_tensors
        d = ctx.dims
        gl = g.to(torch.float32).reshape(1).contiguous()
        gx = torch.empty_like(xcl)
        ws = _ws(lib.ssbev_lovasz_bwd_workspace(C.byref(d)), xcl.device)
        with _span("lovasz", 0.0, 8.0 * xcl.numel() + lab.numel() + 8.0 * dj.numel(), "bwd   lovasz"):
            capi.check(lib.ssbev_lovasz_bwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(dj), capi.ptr(counts), capi.ptr(gl),
                                            capi.ptr(gx), C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_lovasz_bwd")
        return from_cl(gx), None, None


def lovasz_softmax(logits, label_u8, ignore=255):
    """Unweighted Lovasz-softmax loss of ``softmax(up(logits))`` against ``label_u8`` over the labelled voxels of the whole batch
    (classes present in the labels only; 0 with a zero gradient when no voxel is labelled), fp32, 0-dim.  Supported inputs
    (``lovasz_supported``) with ``LOVASZ`` on run on the fused HIP path; anything else on the tensor form of plugin/losses.py
    after ``upsample_trilinear``."""
    label_u8 = label_u8.to(torch.uint8)
    if LOVASZ and lovasz_supported(logits, label_u8):
        return _LovaszSoftmax.apply(logits, label_u8, int(ignore))
    from .plugin import losses
    if not LOVASZ and logits.is_cuda:
        return losses.lovasz_softmax_tensor(upsample_trilinear(logits, label_u8.shape[-3:]), label_u8, ignore).float()
    return losses.lovasz_softmax_loss(logits, label_u8, ignore).float()


OHEM = os.environ.get("SSBEV_OHEM", "1") != "0"              # fused OHEM cross entropy (0 = the tensor form: CE volume + one stable sort per sample)


def ohem_supported(logits, label):
    """The fused OHEM cross entropy serves what the fused Lovasz-softmax serves: fp32 20-class logits on the GPU that sit on the
    label grid or at exactly half of it."""
    return lovasz_supported(logits, label)


def _ohem_forward(logits, label_u8, class_weight, top_k):
    """``ssbev_ohem_ce_fwd``: (loss [1], mask uint8 [voxels], inv_wsum [1], channels-last logits, labels, weights, dims, ws)."""
    lib = capi.load()
    xcl = to_cl(_f32(logits, "ohem_ce_loss"))
    B, D, H, W, Cch = xcl.shape
    lab = label_u8.contiguous()
    up = int(tuple(lab.shape[1:]) != (D, H, W))
    top_k = float(top_k)
    if not 0.0 < top_k <= 1.0:
        raise capi.SsbevError(f"ohem_ce_loss: top_k must be in (0, 1], got {top_k}")
    d = capi.OhemDims(B, D, H, W, Cch, 255, up, top_k)
    dev = logits.device
    cw = class_weight.detach().to(device=dev, dtype=torch.float32).contiguous()
    if cw.numel() != Cch:
        raise capi.SsbevError(f"ohem_ce_loss: {Cch} class weights expected, got {cw.numel()}")
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    inv = torch.empty(1, dtype=torch.float32, device=dev)
    mask = torch.empty(lab.numel(), dtype=torch.uint8, device=dev)
    ws = _ws(lib.ssbev_ohem_ce_workspace(C.byref(d)), dev)
    # the loss pass reads the logits' taps and writes 4 B per voxel; three histogram passes, the tie count and the selection read them
    with _span("ohem", 0.0, 4.0 * xcl.numel() + 3.0 * lab.numel() + 4.0 * 6 * lab.numel(), "fwd   ohem"):
        capi.check(lib.ssbev_ohem_ce_fwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(cw), capi.ptr(loss), capi.ptr(mask), capi.ptr(inv),
                                         C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_ohem_ce_fwd")
    return loss, mask, inv, xcl, lab, cw, d, ws


def ohem_voxel_losses(logits, label_u8, class_weight, top_k=0.25):
    """Diagnostics: (per-voxel fp32 losses of the fused path, NaN where ignored, in the labels' shape; the selection mask) -- a
    read of the head of the forward workspace, for the accuracy tests and tools/ohem_probe.py."""
    label_u8 = label_u8.to(torch.uint8)
    _, mask, _, _, lab, _, _, ws = _ohem_forward(logits, label_u8, class_weight, top_k)
    bits = ws[:4 * lab.numel()].clone().view(torch.int32)
    l = torch.where(bits == -1, torch.full_like(bits, 0x7FC00000), bits).view(torch.float32)
    return l.view(lab.shape), mask.view(lab.shape).bool()


class _OhemCe(torch.autograd.Function):
    """logits [B,20,D,H,W], label uint8 [B,D',H',W'] (the same grid or exactly twice it), class weights [20] -> the OHEM cross
    entropy (0-dim fp32), ``ssbev_ohem_ce_fwd / _bwd``.  Forward keeps one byte per voxel (the selection) and the reciprocal of
    the clamped weight sum on the device; nothing is read back.  No gradient for the class weights (a buffer of the head)."""

    @staticmethod
    def forward(ctx, logits, label_u8, class_weight, top_k):
        loss, mask, inv, xcl, lab, cw, d, _ = _ohem_forward(logits, label_u8, class_weight, top_k)
        ctx.save_for_backward(xcl, lab, cw, mask, inv)
        ctx.dims = d
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        xcl, lab, cw, mask, inv = ctx.saved_tensors
        d = ctx.dims
        gl = g.to(torch.float32).reshape(1).contiguous()
        gx = torch.empty_like(xcl)
        ws = _ws(lib.ssbev_ohem_ce_bwd_workspace(C.byref(d)), xcl.device)
        with _span("ohem", 0.0, 8.0 * xcl.numel() + 2.0 * lab.numel() + 8.0 * 20 * lab.numel() * d.upsample, "bwd   ohem"):
            capi.check(lib.ssbev_ohem_ce_bwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(cw), capi.ptr(mask), capi.ptr(inv), capi.ptr(gl),
                                             capi.ptr(gx), C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_ohem_ce_bwd")
        return from_cl(gx), None, None, None


def ohem_ce_loss(logits, label_u8, class_weight, top_k=0.25):
    """OHEM cross entropy of ``up(logits)`` against ``label_u8`` (255 = ignore): per sample the ``int(M_b * top_k)`` largest
    class-weighted voxel losses, their sum over the sum of their class weights (clamped at 1e-4) over the batch; 0 with a zero
    gradient when nothing is selected; fp32, 0-dim.  Supported inputs (``ohem_supported``) with ``OHEM`` on run on the fused HIP
    path; anything else on the tensor form of plugin/losses.py after ``upsample_trilinear``."""
    label_u8 = label_u8.to(torch.uint8)
    if OHEM and ohem_supported(logits, label_u8):
        return _OhemCe.apply(logits, label_u8, class_weight, float(top_k))
    from .plugin import losses
    if not OHEM and logits.is_cuda:
        up = upsample_trilinear(logits, label_u8.shape[-3:])
        return losses.ohem_ce_tensor(up, label_u8, class_weight.to(up), top_k).float()
    return losses.ohem_ce_loss(logits, label_u8, class_weight, top_k).float()


FRUSTUM_DIST = os.environ.get("SSBEV_FRUSTUM_DIST", "1") != "0"    # fused frustum-proportion loss (0 = the tensor form: one scatter-add over the up-sampled softmax)
FRUSTUM_NONE = 255                                                 # id of a voxel that lies in no frustum


def frustum_dist_supported(logits, ids, dists):
    """The fused frustum-proportion loss serves what the fused Lovasz-softmax serves (fp32 20-class logits on the GPU that sit on
    the id grid or at exactly half of it) with uint8 ids and counts [B, F, 20] of at most 64 frusta."""
    return (lovasz_supported(logits, ids) and ids.dtype == torch.uint8 and ids.device == logits.device
            and torch.is_tensor(dists) and dists.dim() == 3
            and dists.shape[0] == logits.shape[0] and 1 <= dists.shape[1] <= 64 and dists.shape[2] == 20)


def frustum_ids_from_masks(masks):
    """The reference's dense bool ``frustums_masks`` [B, F, X, Y, Z] (or [F, X, Y, Z]) -> the id volume uint8 [B, X, Y, Z]
    ([X, Y, Z]): the index of the mask that holds the voxel, 255 for none.  ``None`` when two masks overlap somewhere (the masks of
    ``CreateRelationLabels`` never do: a centre projects into one half-open patch) or with more than 255 masks; the caller then
    uses the dense tensor form.  The overlap test reads one scalar back: pass ``frustums_ids`` to avoid it."""
    m = masks.bool()
    dim = m.dim() - 4
    if m.shape[dim] > 255:
        return None
    if bool((m.sum(dim, dtype=torch.int32) > 1).any()):
        return None
    first = m.to(torch.uint8).argmax(dim).to(torch.uint8)
    return torch.where(m.any(dim), first, torch.full_like(first, FRUSTUM_NONE))


class _FrustumDist(torch.autograd.Function):
    """logits [B,20,D,H,W], ids uint8 [B,D',H',W'] (the same grid or exactly twice it), counts [B,F,20] -> the frustum-proportion
    loss (0-dim fp32), ``ssbev_frustum_dist_fwd / _bwd``.  Forward keeps the F x 20 coefficient table d loss / d cum on the device;
    nothing is read back.  No gradient for the counts."""

    @staticmethod
    def forward(ctx, logits, ids_u8, dists):
        lib = capi.load()
        xcl = to_cl(_f32(logits, "frustum_dist_loss"))
        B, D, H, W, Cch = xcl.shape
        ids = ids_u8.contiguous()
        up = int(tuple(ids.shape[1:]) != (D, H, W))
        dev = logits.device
        cnt = dists.detach().to(device=dev, dtype=torch.float32).contiguous()
        d = capi.FrustumDims(B, D, H, W, Cch, cnt.shape[1], up)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        g = torch.empty(cnt.shape[1], Cch, dtype=torch.float32, device=dev)
        ws = _ws(lib.ssbev_frustum_dist_workspace(C.byref(d)), dev)
        # one pass reads the logits' taps and one byte per voxel; the partial tables are small
        with _span("frustum", 0.0, 4.0 * xcl.numel() + ids.numel() + 2.0 * ws.numel(), "fwd   frustum"):
            capi.check(lib.ssbev_frustum_dist_fwd(capi.ptr(xcl), capi.ptr(ids), capi.ptr(cnt), capi.ptr(loss), capi.ptr(g),
                                                  C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_frustum_dist_fwd")
        ctx.save_for_backward(xcl, ids, g)
        ctx.dims = d
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        lib = capi.load()
        xcl, ids, g = ctx.saved_tensors
        d = ctx.dims
        gl = gout.to(torch.float32).reshape(1).contiguous()
        gx = torch.empty_like(xcl)
        ws = _ws(lib.ssbev_frustum_dist_bwd_workspace(C.byref(d)), xcl.device)
        with _span("frustum", 0.0, 8.0 * xcl.numel() + ids.numel() + 8.0 * 20 * ids.numel() * d.upsample, "bwd   frustum"):
            capi.check(lib.ssbev_frustum_dist_bwd(capi.ptr(xcl), capi.ptr(ids), capi.ptr(g), capi.ptr(gl), capi.ptr(gx), C.byref(d),
                                                  capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_frustum_dist_bwd")
        return from_cl(gx), None, None


def frustum_dist_loss(logits, ids_u8, dists):
    """Frustum-proportion loss of ``up(logits)`` against the frustum ids ``ids_u8`` (255 = in no frustum) and the class counts
    ``dists`` [B,F,20]: per frustum, pooled over the batch, the KL divergence (over the classes with a non-zero count) between the
    labelled class mix and the predicted one, averaged over the frusta that hold both voxels and counts; 0 with a zero gradient
    when there is none; fp32, 0-dim; no gradient for ``dists``.  Supported inputs (``frustum_dist_supported``) with
    ``FRUSTUM_DIST`` on run on the fused HIP path; anything else on the tensor form of plugin/losses.py after
    ``upsample_trilinear``."""
    ids_u8 = ids_u8.to(device=logits.device, dtype=torch.uint8)       # (the loader step's output may still live on the host)
    if FRUSTUM_DIST and frustum_dist_supported(logits, ids_u8, dists):
        return _FrustumDist.apply(logits, ids_u8, dists)
    from .plugin import losses
    if not FRUSTUM_DIST and logits.is_cuda:
        up = upsample_trilinear(logits, ids_u8.shape[-3:])
        return losses.frustum_dist_tensor(up, ids_u8, dists.detach().to(up)).float()
    return losses.frustum_dist_loss(logits, ids_u8, dists).float()


def frustum_view_matrix(view):
    """The loader step's camera of one sample of a view (``img_inputs[k]``: imgs, rots, trans, intrins, post_rots, post_trans,
    bda, ...; of one sample, or the first sample of a batch) -> (M float64 [3,4] that takes a point of the (BEV-augmented) label grid to
    (x d, y d, d): inverse BEV matrix (3x3, or 4x4 applied to the homogeneous point), minus ``trans``, inverse ``rots``, the 4x4
    ``intrins``; post-rotation float64 [2,2]; post-translation float64 [2]; (img_h, img_w)), composed on the host in float64."""
    imgs, rots, trans, intrins, post_rots, post_trans, bda = view[:7]

    def mat(t, r, c):
        t = torch.as_tensor(t).detach().double().cpu()
        t = t.reshape(-1, r, c) if t.numel() > r * c else t.reshape(1, r, c)
        return t[0]
    bda = torch.as_tensor(bda)
    n = int(bda.shape[-1])
    inv_bda = torch.eye(4, dtype=torch.float64)
    inv_bda[:n, :n] = torch.inverse(mat(bda, n, n))
    A, a = inv_bda[:3, :3], inv_bda[:3, 3]
    Rinv = torch.inverse(mat(rots, 3, 3))
    K = mat(intrins, 4, 4)
    t = mat(trans, 1, 3).reshape(3)
    KR = K[:3, :3] @ Rinv
    M = torch.cat([KR @ A, (KR @ (a - t) + K[:3, 3]).reshape(3, 1)], dim=1)
    pr = mat(post_rots, 3, 3)[:2, :2].clone()
    pt = mat(post_trans, 1, 3).reshape(3)[:2].clone()
    return M, pr, pt, tuple(int(v) for v in imgs.shape[-2:])


def frustum_labels(labels, view, point_cloud_range, frustum_size=8):
    """The loader step ``CreateRelationLabels`` of one sample: voxel labels [X,Y,Z] (255 = unlabelled) and one view of
    ``img_inputs`` -> (ids uint8 [X,Y,Z]: ``py * frustum_size + px`` of the image patch the voxel centre projects into, 255 for no
    patch, a depth <= 0 or an unlabelled voxel; counts float32 [frustum_size^2, 20]: labelled voxels per frustum and class).  CUDA
    labels run ``ssbev_frustum_labels``; CPU labels the same fp32 arithmetic in tensor ops.  The camera is composed on the host
    in float64 (``frustum_view_matrix``) and rounded to fp32 once.  The image size is that of ``view[0]``."""
    fs = int(frustum_size)
    if not 1 <= fs <= 8:
        raise ValueError(f"frustum_labels: frustum_size must be in 1..8, got {frustum_size}")
    M, pr, pt, (img_h, img_w) = frustum_view_matrix(view)
    X, Y, Z = (int(v) for v in labels.shape)
    r = torch.as_tensor(point_cloud_range, dtype=torch.float64).reshape(6)
    size = (r[3:] - r[:3]) / torch.tensor([X, Y, Z], dtype=torch.float64)
    params = torch.cat([r[:3] + size / 2, size, M.reshape(-1), pr.reshape(-1), pt.reshape(-1)]).float().contiguous()
    if labels.is_cuda:
        lib = capi.load()
        lab = labels.to(torch.uint8).contiguous()
        ids = torch.empty_like(lab)
        counts = torch.empty(fs * fs, 20, dtype=torch.int32, device=lab.device)
        capi.check(lib.ssbev_frustum_labels(capi.ptr(lab), capi.ptr(ids), capi.ptr(counts), X, Y, Z, C.c_void_p(params.data_ptr()),
                                            img_h, img_w, fs, capi.stream()), "ssbev_frustum_labels")
        return ids, counts.float()
    o, s, m = params[0:3], params[3:6], params[6:18].reshape(3, 4)
    cx = (o[0] + torch.arange(X, dtype=torch.float32) * s[0]).view(X, 1, 1)
    cy = (o[1] + torch.arange(Y, dtype=torch.float32) * s[1]).view(1, Y, 1)
    cz = (o[2] + torch.arange(Z, dtype=torch.float32) * s[2]).view(1, 1, Z)
    xd, yd, d = (m[i, 0] * cx + m[i, 1] * cy + m[i, 2] * cz + m[i, 3] for i in range(3))
    u0, v0 = xd / d, yd / d
    pu = params[18] * u0 + params[19] * v0 + params[22]
    pv = params[20] * u0 + params[21] * v0 + params[23]
    ex = torch.tensor([i / fs * img_w for i in range(fs + 1)], dtype=torch.float64).float()
    ey = torch.tensor([i / fs * img_h for i in range(fs + 1)], dtype=torch.float64).float()
    px = torch.bucketize(pu.contiguous(), ex, right=True) - 1                    # ex[px] <= pu < ex[px + 1]
    py = torch.bucketize(pv.contiguous(), ey, right=True) - 1
    lab = labels.long()
    ok = (px >= 0) & (px < fs) & (py >= 0) & (py < fs) & (d > 0) & (lab < 20) & ~torch.isnan(pu) & ~torch.isnan(pv)
    ids = torch.where(ok, py * fs + px, torch.full_like(px, FRUSTUM_NONE)).to(torch.uint8)
    counts = torch.zeros(fs * fs * 20, dtype=torch.float32)
    counts.index_add_(0, (ids.long() * 20 + lab)[ok], torch.ones(int(ok.sum()), dtype=torch.float32))
    return ids, counts.view(fs * fs, 20)


# -------------------------------------------------------------------------------------------------
# BEV augmentation of the voxel labels (csrc/bev_augment.hip)
# -------------------------------------------------------------------------------------------------
SSBEV_BDA = os.environ.get("SSBEV_BDA", "1") != "0"          # loader's BEV label augmentation on the GPU (0 = the host form: scipy, then one upload)


def bev_label_transform(labels_u8, coeffs, flip_dx, flip_dy, inplace=True, fill=255, out_dtype=torch.int64):
    """``pipelines.bev_transform``'s label half on the GPU: uint8 labels [X,Y,Z] rotated in every (X, Y) plane by scipy's
    order-0 ``mode='constant'`` rule (``coeffs`` = scipy's own ``(m00, m01, m10, m11, off0, off1)`` as Python floats, composed
    by the caller in double; ``None`` = no rotation), then flipped along axis 1 (``flip_dy``) and axis 0 (``flip_dx``).
    ``inplace=True`` reproduces the upstream's ``rotate(lab, output=lab)``, which reads voxels it has already overwritten;
    ``inplace=False`` is the out-of-place rotation.  Returns int64 (or uint8 with ``out_dtype=torch.uint8``) [X,Y,Z]."""
    if labels_u8.dtype != torch.uint8 or labels_u8.dim() != 3:
        raise capi.SsbevError(f"bev_label_transform: uint8 [X,Y,Z] labels expected, got {labels_u8.dtype} {tuple(labels_u8.shape)}")
    if out_dtype not in (torch.int64, torch.uint8):
        raise ValueError(f"bev_label_transform: out_dtype must be torch.int64 or torch.uint8, got {out_dtype}")
    lib = capi.load()
    lab = labels_u8.contiguous()
    X, Y, Z = (int(v) for v in lab.shape)
    out = torch.empty(X, Y, Z, dtype=out_dtype, device=lab.device)
    c6 = None if coeffs is None else (C.c_double * 6)(*(float(v) for v in coeffs))
    ws = _ws(lib.ssbev_bev_label_workspace(X, Y, int(c6 is not None), int(bool(inplace))), lab.device)
    fn = lib.ssbev_bev_label_transform if out_dtype == torch.int64 else lib.ssbev_bev_label_transform_u8
    capi.check(fn(capi.ptr(lab), capi.ptr(out), X, Y, Z, c6, int(bool(inplace)), int(bool(flip_dx)), int(bool(flip_dy)), int(fill),
                  capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_bev_label_transform")
    return out


# -------------------------------------------------------------------------------------------------
# Occupancy -> depth map and image-view label map (csrc/occ_depth.hip)
# -------------------------------------------------------------------------------------------------
SSBEV_OCC_DEPTH = os.environ.get("SSBEV_OCC_DEPTH", "1") != "0"   # CreateDepthFromOccupancy on the GPU (0 = the tensor form on the host, then one upload)
SEG_OCCLUDERS = ("reference", "occupied")
_OCC_TABLES = {}                                                  # (range, grid, device) -> the three centre tables, made once


def occ_voxel_tables(point_cloud_range, grid_size, device="cpu"):
    """The voxel centres per axis as ``CreateDepthFromOccupancy.init_voxel_coordinates`` makes them (occ_to_depth.py:32-38: the
    same ``torch.arange`` over float64 bounds, so the fp32 centres carry its bits): one fp32 tensor [X + Y + Z] on ``device``."""
    grid = tuple(int(v) for v in grid_size)
    key = (tuple(float(v) for v in point_cloud_range), grid, str(device))
    t = _OCC_TABLES.get(key)
    if t is None:
        r = np.array(key[0], dtype=np.float64)
        size = (r[3:] - r[:3]) / np.array(grid)
        lo = r[:3] + size / 2
        tabs = [torch.arange(lo[i], r[3 + i], size[i]) for i in range(3)]
        if tuple(int(a.numel()) for a in tabs) != grid:
            raise ValueError(f"occ_voxel_tables: torch.arange gives {[int(a.numel()) for a in tabs]} centres for the grid {grid} "
                             f"(the reference's .view(X, 1, 1) fails the same way)")
        if len(_OCC_TABLES) >= 16:
            _OCC_TABLES.clear()
        t = _OCC_TABLES[key] = torch.cat(tabs).float().contiguous().to(device)
    return t


def occ_camera(view):
    """The 46 camera floats of ``ssbev_occ_depth_map`` from one view of ``img_inputs`` (slots 1..6: rots, trans, intrins,
    post_rots, post_trans, bda), on the host: ``inv(bda)[:3]`` as 3x4 | ``inv(rots)`` | trans | intrins 4x4 | ``post_rots[:2,:2]``
    | ``post_trans[:2]``, both inverses by ``torch.inverse`` in fp32 as the reference takes them (occ_to_depth.py:45, :51).
    Returns (cam [46] fp32 CPU, n = 3 or 4, the size of the BEV matrix)."""
    def host(t):
        return torch.as_tensor(t).detach().float().cpu()
    rots, trans, intrins, post_rots, post_trans, bda = (host(t) for t in view[1:7])
    n = int(bda.shape[-1])
    if n not in (3, 4) or bda.numel() != n * n:
        raise ValueError(f"occupancy_depth_map: one 3x3 or 4x4 BEV matrix expected in slot 6, got {tuple(bda.shape)}")
    inv_bda = torch.zeros(3, 4)
    inv_bda[:, :n] = torch.inverse(bda.reshape(n, n))[:3]
    cam = torch.cat([inv_bda.reshape(-1), torch.inverse(rots.reshape(3, 3)).reshape(-1), trans.reshape(-1)[:3],
                     intrins.reshape(4, 4).reshape(-1), post_rots.reshape(3, 3)[:2, :2].reshape(-1),
                     post_trans.reshape(-1)[:2]]).contiguous()
    assert cam.numel() == 46
    return cam, n


def _occ_depth_tensor(lab, tabs, cam, n, occupied_only, H, W):
    """``ssbev_occ_depth_map`` in elementwise tensor operations on the host, one rounding per operation in the kernel's order,
    the nearest voxel per pixel by the same 64-bit key (depth bits << 32 | flat index) under ``amin``."""
    X, Y, Z = (int(v) for v in lab.shape)
    N = X * Y * Z
    px = tabs[:X].view(X, 1, 1).expand(X, Y, Z).reshape(-1)
    py = tabs[X:X + Y].view(1, Y, 1).expand(X, Y, Z).reshape(-1)
    pz = tabs[X + Y:].view(1, 1, Z).expand(X, Y, Z).reshape(-1)
    A, R, t, K, pr, pt = cam[0:12], cam[12:21], cam[21:24], cam[24:40], cam[40:44], cam[44:46]
    l3 = [(A[4 * i] * px + A[4 * i + 1] * py) + A[4 * i + 2] * pz for i in range(3)]
    if n == 4:
        l3 = [l3[i] + A[4 * i + 3] for i in range(3)]
    x, y, z = (l3[i] - t[i] for i in range(3))
    cx, cy, cz = ((R[3 * i] * x + R[3 * i + 1] * y) + R[3 * i + 2] * z for i in range(3))
    qx, qy, d = (((K[4 * i] * cx + K[4 * i + 1] * cy) + K[4 * i + 2] * cz) + K[4 * i + 3] for i in range(3))
    u0, v0 = qx / d, qy / d
    u = (pr[0] * u0 + pr[1] * v0) + pt[0]
    v = (pr[2] * u0 + pr[3] * v0) + pt[1]
    ok = (u >= 0) & (v >= 0) & (u <= W - 1) & (v <= H - 1) & (d > 0)
    flat = lab.reshape(-1)
    occupied = (flat != 0) & (flat != 255)
    idx = torch.arange(N, dtype=torch.int64)
    none = torch.iinfo(torch.int64).max

    def nearest(mask):
        pix = torch.round(v[mask]).long() * W + torch.round(u[mask]).long()
        key = (d[mask].contiguous().view(torch.int32).long() << 32) | idx[mask]
        return torch.full((H * W,), none, dtype=torch.int64).scatter_reduce_(0, pix, key, "amin")

    zd = nearest(ok & occupied)
    zs = zd if occupied_only else nearest(ok)
    depth = torch.where(zd != none, (zd >> 32).to(torch.int32).view(torch.float32), torch.zeros(()))
    hit = zs != none
    seg = torch.where(hit, flat[torch.where(hit, zs & 0xFFFFFFFF, torch.zeros_like(zs))].float(), torch.full((), 255.0))
    return depth.view(H, W), seg.view(H, W)


def label_map_downsample(seg, downscale=16):
    """``CreateDepthFromOccupancy._downsample_label`` (occ_to_depth.py:67-93): a label map [H,W] (float holding 0..255; any other
    value counts as 255) -> float32 [H // ds, W // ds], trailing rows and columns dropped.  A patch with more than ``0.95 ds^2``
    pixels 0 or 255 (compared in fp32, as the reference's tensor-against-float comparison does) becomes 0 when the zeros outnumber
    the 255s and 255 otherwise (a tie included); any other patch takes its most frequent label in 1..254, the LOWEST on a tie --
    what ``torch.mode`` returns on the CPU.  CUDA maps run ``ssbev_label_map_downsample``; CPU maps the same rule in tensor ops."""
    ds = int(downscale)
    seg = torch.as_tensor(seg)
    if seg.dim() != 2 or not 1 <= ds <= 256:
        raise ValueError(f"label_map_downsample: a [H,W] map and a downscale in 1..256 expected, got {tuple(seg.shape)}, {downscale}")
    H, W = (int(v) for v in seg.shape)
    oh, ow = H // ds, W // ds
    empty_t = float(torch.tensor(0.95 * ds * ds, dtype=torch.float32))
    if seg.is_cuda:
        lib = capi.load()
        src = seg.float().contiguous()
        out = torch.empty(oh, ow, dtype=torch.float32, device=seg.device)
        if H and W:
            capi.check(lib.ssbev_label_map_downsample(capi.ptr(src), capi.ptr(out), H, W, ds, empty_t, capi.stream()),
                       "ssbev_label_map_downsample")
        return out
    if oh == 0 or ow == 0:
        return torch.empty(oh, ow, dtype=torch.float32)
    v = seg.float()[:oh * ds, :ow * ds]
    lab = torch.where((v >= 0) & (v <= 255), v, torch.full((), 255.0)).long()
    patches = lab.reshape(oh, ds, ow, ds).permute(0, 2, 1, 3).reshape(-1, ds * ds)
    hist = torch.zeros(patches.shape[0], 256, dtype=torch.int64).scatter_add_(1, patches, torch.ones_like(patches))
    z0, z255 = hist[:, 0], hist[:, 255]
    empty = (z0 + z255).float() > empty_t
    ids = torch.arange(1, 255)
    cls = ids[(hist[:, 1:255] * 256 + (255 - ids)).argmax(1)]                     # the larger count, then the lower id
    out = torch.where(empty, torch.where(z0 > z255, torch.zeros_like(cls), torch.full_like(cls, 255)), cls)
    return out.float().view(oh, ow)


def occupancy_depth_map(labels, view, point_cloud_range, seg_occluders="reference", downsample=False, downscale=16):
    """The loader step ``CreateDepthFromOccupancy`` of one view (occ_to_depth.py:95-149): voxel labels [X,Y,Z] (0 = empty, 255 =
    ignored) and one view of ``img_inputs`` -> (depth float32 [H,W]: the depth of the nearest voxel centre labelled 1..254 per
    pixel, 0 where none; seg float32 [H,W], or [H // ds, W // ds] with ``downsample``: the label of the nearest centre, 255 where
    none).  The image size is that of ``view[0]``; the grid is the labels' shape.
    ``seg_occluders="reference"``: as upstream, EVERY in-view centre competes for the label map, empty and ignored voxels
    included, so whatever voxel lies in front of a surface along a pixel's ray takes that pixel with its own label.
    ``"occupied"``: only labels 1..254 compete; a pixel shows the first occupied voxel, on the mask the depth map uses.
    Exact fp32 depth ties go to the lowest flat voxel index (upstream leaves them open).
    CUDA labels run ``ssbev_occ_depth_map`` (+ ``ssbev_label_map_downsample``); CPU labels the same fp32 arithmetic in tensor
    ops; with ``SSBEV_OCC_DEPTH`` off CUDA labels take the tensor form on the host and the maps are uploaded once."""
    if seg_occluders not in SEG_OCCLUDERS:
        raise ValueError(f"occupancy_depth_map: seg_occluders must be one of {SEG_OCCLUDERS}, got {seg_occluders!r}")
    labels = torch.as_tensor(labels)
    if labels.dim() != 3 or labels.dtype.is_floating_point:
        raise ValueError(f"occupancy_depth_map: integer labels [X,Y,Z] expected, got {labels.dtype} {tuple(labels.shape)}")
    X, Y, Z = (int(v) for v in labels.shape)
    H, W = (int(v) for v in view[0].shape[-2:])
    if min(X, Y, Z, H, W) < 1:
        raise ValueError(f"occupancy_depth_map: empty grid {(X, Y, Z)} or image {(H, W)}")
    cam, n = occ_camera(view)
    occupied_only = seg_occluders == "occupied"
    dev = labels.device
    if labels.is_cuda and SSBEV_OCC_DEPTH:
        lib = capi.load()
        lab = labels.to(torch.uint8).contiguous()
        tabs = occ_voxel_tables(point_cloud_range, (X, Y, Z), dev)
        depth = torch.empty(H, W, dtype=torch.float32, device=dev)
        seg = torch.empty(H, W, dtype=torch.float32, device=dev)
        ws = _ws(lib.ssbev_occ_depth_workspace(H, W), dev)
        base = tabs.data_ptr()
        capi.check(lib.ssbev_occ_depth_map(capi.ptr(lab), X, Y, Z, C.c_void_p(base), C.c_void_p(base + 4 * X),
                                           C.c_void_p(base + 4 * (X + Y)), C.c_void_p(cam.data_ptr()), n, int(occupied_only),
                                           capi.ptr(depth), capi.ptr(seg), H, W, capi.ptr(ws), ws.numel(), capi.stream()),
                   "ssbev_occ_depth_map")
        return depth, (label_map_downsample(seg, downscale) if downsample else seg)
    tabs = occ_voxel_tables(point_cloud_range, (X, Y, Z))
    depth, seg = _occ_depth_tensor(labels.cpu().to(torch.uint8), tabs, cam, n, occupied_only, H, W)
    if downsample:
        seg = label_map_downsample(seg, downscale)
    return depth.to(dev), seg.to(dev)


# -------------------------------------------------------------------------------------------------
# 3-D context relation prior (csrc/crp.hip): label down-sampling, relation matrix, relation loss, relation gather
# -------------------------------------------------------------------------------------------------
CRP = os.environ.get("SSBEV_CRP", "1") != "0"                # fused relation loss and gather (0 = the tensor forms: sigmoid, bmm, cat, BCEWithLogits)
CRP_RELATIONS = 4


def label_downsample(labels, downscale):
    """``CreateRelationLabels._downsample_label`` (voxel_labels.py:79-122), byte-exact: labels uint8 [X,Y,Z] -> uint8
    [X/ds, Y/ds, Z/ds].  A block with more than ``0.95 * ds**3`` voxels labelled 0 or 255 becomes 0 when the zeros outnumber the
    255s and 255 otherwise (a tie included); any other block takes its most frequent class 1..254, the lowest id on a tie.
    CUDA labels run ``ssbev_label_downsample``; CPU labels the same rule in tensor ops."""
    ds = int(downscale)
    lab = torch.as_tensor(labels)
    if lab.dim() != 3 or lab.dtype != torch.uint8:
        raise ValueError(f"label_downsample: uint8 [X,Y,Z] expected, got {lab.dtype} {tuple(lab.shape)}")
    X, Y, Z = (int(v) for v in lab.shape)
    if not 1 <= ds <= 32 or X % ds or Y % ds or Z % ds:
        raise ValueError(f"label_downsample: downscale {downscale} must be in 1..32 and divide the grid {(X, Y, Z)}")
    if lab.is_cuda:
        lib = capi.load()
        lab = lab.contiguous()
        out = torch.empty(X // ds, Y // ds, Z // ds, dtype=torch.uint8, device=lab.device)
        capi.check(lib.ssbev_label_downsample(capi.ptr(lab), capi.ptr(out), X, Y, Z, ds, capi.stream()), "ssbev_label_downsample")
        return out
    blocks = lab.view(X // ds, ds, Y // ds, ds, Z // ds, ds).permute(0, 2, 4, 1, 3, 5).reshape(-1, ds ** 3).long()
    hist = torch.zeros(blocks.shape[0], 256, dtype=torch.int64).scatter_add_(1, blocks, torch.ones_like(blocks))
    z0, z255 = hist[:, 0], hist[:, 255]
    empty = (z0 + z255).double() > 0.95 * ds * ds * ds
    ids = torch.arange(1, 255)
    cls = ids[(hist[:, 1:255] * 256 + (255 - ids)).argmax(1)]                     # the larger count, then the lower id
    out = torch.where(empty, torch.where(z0 > z255, torch.zeros_like(cls), torch.full_like(cls, 255)), cls)
    return out.to(torch.uint8).view(X // ds, Y // ds, Z // ds)


def relation_matrix(labels):
    """``CreateRelationLabels.compute_CP_mega_matrix(is_binary=False)`` (voxel_labels.py:124-174): the down-sampled label grid
    uint8 [X,Y,Z] (or [B,X,Y,Z]) -> the dense relation matrix uint8 [4, N, Mc] ([B, 4, N, Mc]); N = X Y Z rows in grid order, Mc
    = N / 8 columns, column ``xx (Y/2)(Z/2) + yy (Z/2) + zz`` for the 2x2x2 block at (2xx, 2yy, 2zz).  Entry [r, n, m] is the OR
    over the block's children that are not 255 of: 0 child == row != 0; 1 child != row, both != 0; 2 child == row == 0; 3 child !=
    row and one of them 0; rows labelled 255 are all zero.  Tensor ops on the labels' device."""
    lab = torch.as_tensor(labels)
    g = (lab if lab.dim() == 4 else lab[None]).long()
    B, X, Y, Z = g.shape
    if X % 2 or Y % 2 or Z % 2:
        raise ValueError(f"relation_matrix: the grid {(X, Y, Z)} must be even on every axis")
    row = g.reshape(B, -1, 1, 1)
    kids = g.view(B, X // 2, 2, Y // 2, 2, Z // 2, 2).permute(0, 1, 3, 5, 2, 4, 6).reshape(B, 1, -1, 8)
    ok = (kids != 255) & (row != 255)
    same = kids == row
    rels = (same & (kids != 0), ~same & (kids != 0) & (row != 0), same & (kids == 0), ~same & ((kids == 0) | (row == 0)))
    m = torch.stack([(r & ok).any(-1) for r in rels], dim=1).to(torch.uint8)
    return m if lab.dim() == 4 else m[0]


def relation_loss_tensor(P_logits, matrices):
    """``compute_super_CP_multilabel_loss`` (resnet3d.py:269-290) in tensor ops on any device, in the logits' dtype, without a
    read-back: P_logits [B, 4, Mc, N], matrices [B, 4, N, Mc] (0 / 1).  pos_weight_r = negatives / positives of relation r over
    the batch; for a relation without a positive the reference divides by zero and returns NaN, here the weight is 1 (it
    multiplies nothing)."""
    x = P_logits.permute(0, 1, 3, 2)
    y = matrices.to(device=x.device)
    if tuple(y.shape) != tuple(x.shape):
        raise ValueError(f"relation loss: matrices {tuple(y.shape)} do not match the logits' {tuple(x.shape)} ([B, R, N, Mc])")
    R = x.shape[1]
    pos = y.long().sum(dim=(0, 2, 3))
    neg = y.numel() // R - pos
    pw = torch.where(pos > 0, neg.double() / pos.clamp(min=1).double(), torch.ones_like(pos, dtype=torch.float64))
    return torch.nn.functional.binary_cross_entropy_with_logits(x, y.to(x.dtype), pos_weight=pw.to(x.dtype).view(1, R, 1, 1))


def relation_loss_supported(P_logits, labels):
    """The fused relation loss serves fp32 logits [B, 4, Mc, N] on the GPU with uint8 labels [B, X, Y, Z] on the same device, an
    even grid, N = X Y Z and Mc = N / 8."""
    if not (torch.is_tensor(P_logits) and torch.is_tensor(labels) and P_logits.is_cuda and P_logits.dtype == torch.float32):
        return False
    if P_logits.dim() != 4 or labels.dim() != 4 or labels.dtype != torch.uint8 or labels.device != P_logits.device:
        return False
    B, R, Mc, N = P_logits.shape
    X, Y, Z = (int(v) for v in labels.shape[1:])
    return (R == CRP_RELATIONS and labels.shape[0] == B and X % 2 == 0 and Y % 2 == 0 and Z % 2 == 0 and N == X * Y * Z
            and Mc * 8 == N and N < (1 << 24))


class _RelationLoss(torch.autograd.Function):
    """P_logits [B,4,Mc,N] (a view of the channels-last convolution result [B,N,4,Mc]: no copy), labels uint8 [B,X,Y,Z] -> the
    relation loss (0-dim fp32), ``ssbev_crp_loss_fwd / _bwd``.  The four pos_weights stay on the device for backward."""

    @staticmethod
    def forward(ctx, P_logits, labels):
        lib = capi.load()
        pcl = P_logits.permute(0, 3, 1, 2).contiguous()
        lab = labels.contiguous()
        B, X, Y, Z = lab.shape
        d = capi.CrpDims(B, X, Y, Z)
        dev = pcl.device
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        pw = torch.empty(CRP_RELATIONS, dtype=torch.float32, device=dev)
        ws = _ws(lib.ssbev_crp_loss_workspace(C.byref(d)), dev)
        with _span("crp", 0.0, 4.0 * pcl.numel() + lab.numel(), "fwd   crp_loss"):
            capi.check(lib.ssbev_crp_loss_fwd(capi.ptr(pcl), capi.ptr(lab), capi.ptr(loss), capi.ptr(pw), C.byref(d), capi.ptr(ws),
                                              ws.numel(), capi.stream()), "ssbev_crp_loss_fwd")
        ctx.save_for_backward(pcl, lab, pw)
        ctx.dims = d
        return loss[0]

    @staticmethod
    def backward(ctx, gout):
        lib = capi.load()
        pcl, lab, pw = ctx.saved_tensors
        gl = gout.to(torch.float32).reshape(1).contiguous()
        gp = torch.empty_like(pcl)
        with _span("crp", 0.0, 8.0 * pcl.numel() + lab.numel(), "bwd   crp_loss"):
            capi.check(lib.ssbev_crp_loss_bwd(capi.ptr(pcl), capi.ptr(lab), capi.ptr(pw), capi.ptr(gl), capi.ptr(gp), C.byref(ctx.dims),
                                              capi.stream()), "ssbev_crp_loss_bwd")
        return gp.permute(0, 2, 3, 1), None


def relation_loss(P_logits, labels=None, matrices=None):
    """The context-prior relation loss of ``P_logits`` [B, 4, Mc, N]: the mean over all 4 B N Mc elements of the weighted binary
    cross entropy against the relation matrix, pos_weight pooled over the batch (``relation_loss_tensor``); fp32, 0-dim.
    ``labels``: the down-sampled label grid uint8 [B,X,Y,Z] -- on the GPU with ``CRP`` on the fused kernel derives every matrix
    bit from it and the dense matrix is never built; elsewhere the matrix is expanded (``relation_matrix``) for the tensor form.
    ``matrices``: a dense [B, 4, N, Mc] matrix from the caller takes precedence and always runs the TENSOR form."""
    if matrices is not None:
        return relation_loss_tensor(P_logits, torch.as_tensor(matrices)).float()
    if labels is None:
        raise ValueError("relation_loss needs the down-sampled labels or the dense relation matrices")
    labels = torch.as_tensor(labels).to(device=P_logits.device, dtype=torch.uint8)
    if CRP and relation_loss_supported(P_logits, labels):
        return _RelationLoss.apply(P_logits, labels)
    return relation_loss_tensor(P_logits, relation_matrix(labels)).float()


def relation_gather_tensor(P_logits, context, x=None):
    """The gather of ``CPMegaVoxels.forward`` (crp3d.py:229-253) as the reference writes it: per relation sigmoid, permute and
    ``bmm`` with the mega context, ``cat`` of the results (and of ``x`` in front)."""
    B, R, Mc, N = P_logits.shape
    rels = [torch.bmm(torch.sigmoid(P_logits[:, r].permute(0, 2, 1)), context) for r in range(R)]
    out = torch.cat(rels, dim=2).permute(0, 2, 1)
    return out if x is None else torch.cat([x.reshape(B, -1, N), out], dim=1)


def relation_gather_supported(P_logits, context, x=None):
    ts = [P_logits, context] + ([x] if x is not None else [])
    if not all(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 for t in ts):
        return False
    if P_logits.dim() != 4 or context.dim() != 3 or context.shape[:2] != (P_logits.shape[0], P_logits.shape[2]):
        return False
    B, R, Mc, N = P_logits.shape
    return R <= 16 and max(N, Mc, context.shape[2]) < (1 << 24) and (x is None or (x.shape[0] == B and x[0, 0].numel() == N))


class _RelationGather(torch.autograd.Function):
    """out[b, Cin + r C2 + c, n] = sum_m sigmoid(P[b,r,m,n]) context[b,m,c] behind the Cin channels of ``x``: one MFMA GEMM per
    (b, r) that stages sigmoid(P) into LDS and writes its channel slice of the concatenated channels-last tensor
    (``ssbev_crp_gather_fwd / _bwd``).  sigmoid(P) is never stored; backward recomputes it."""

    @staticmethod
    def forward(ctx, P_logits, context, x):
        lib = capi.load()
        pcl = P_logits.permute(0, 3, 1, 2).contiguous()               # [B,N,R,Mc]: the layout the convolution left
        cx = context.contiguous()
        B, N, R, Mc = pcl.shape
        C2 = cx.shape[2]
        cin = 0 if x is None else x.shape[1]
        ctot = cin + R * C2
        out = torch.empty(B, N, ctot, dtype=torch.float32, device=pcl.device)
        if x is not None:
            out[:, :, :cin].copy_(x.reshape(B, cin, N).permute(0, 2, 1))
        d = capi.CrpGatherDims(B, N, Mc, C2, R, ctot)
        with _span("crp", 2.0 * B * R * N * Mc * C2, 4.0 * (pcl.numel() + B * N * R * C2), "fwd   crp_gather"):
            capi.check(lib.ssbev_crp_gather_fwd(capi.ptr(pcl), capi.ptr(cx), C.c_void_p(out.data_ptr() + 4 * cin), C.byref(d),
                                                capi.stream()), "ssbev_crp_gather_fwd")
        ctx.save_for_backward(pcl, cx)
        ctx.dims, ctx.cin, ctx.xshape = d, cin, (None if x is None else tuple(x.shape))
        return out.permute(0, 2, 1)

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        pcl, cx = ctx.saved_tensors
        d, cin = ctx.dims, ctx.cin
        gcl = g.permute(0, 2, 1).contiguous()                          # [B,N,Ctot]
        gp = torch.empty_like(pcl)
        gc = torch.empty_like(cx)
        ws = _ws(lib.ssbev_crp_gather_bwd_workspace(C.byref(d)), pcl.device)
        with _span("crp", 4.0 * d.B * d.R * d.N * d.Mc * d.C2, 4.0 * (2 * pcl.numel() + 2 * d.B * d.N * d.R * d.C2) + 2.0 * ws.numel(),
                   "bwd   crp_gather"):
            capi.check(lib.ssbev_crp_gather_bwd(capi.ptr(pcl), capi.ptr(cx), C.c_void_p(gcl.data_ptr() + 4 * cin), capi.ptr(gp),
                                                capi.ptr(gc), C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_crp_gather_bwd")
        gx = None if ctx.xshape is None else gcl[:, :, :cin].permute(0, 2, 1).reshape(ctx.xshape)
        return gp.permute(0, 2, 3, 1), gc, gx


def relation_gather(P_logits, context, x=None):
    """Context features gathered through the relation priors: P_logits [B, R, Mc, N], context [B, Mc, C2] (, x [B, Cin, ...] with
    N positions) -> [B, (Cin +) R C2, N] with ``out[b, Cin + r C2 + c, n] = sum_m sigmoid(P[b,r,m,n]) context[b,m,c]`` and ``x`` in
    the first Cin channels.  fp32 GPU tensors with ``CRP`` on run the fused HIP path (the result is a view of a channels-last
    buffer); anything else the tensor form ``relation_gather_tensor``."""
    if CRP and relation_gather_supported(P_logits, context, x):
        return _RelationGather.apply(P_logits, context, x)
    return relation_gather_tensor(P_logits, context, x)


DEPTH_BCE = os.environ.get("SSBEV_DEPTH_BCE", "1") != "0"    # fused depth loss (0 = the ~35 ATen ops of the tensor expression)


class _DepthBce(torch.autograd.Function):
    """weight * BCE(depth_pred, one-hot of the down-sampled LiDAR depth) over the pixels with a return (VT:349-416),
    ``ssbev_depth_bce_fwd / _bwd``: gt_depths [B, N, H, W], depth_pred [B*N, D, H/ds, W/ds] -> 0-dim loss."""

    @staticmethod
    def forward(ctx, gt_depths, depth_pred, ds, dbound, weight):
        lib = capi.load()
        B, N, H, W = gt_depths.shape
        BN, D, fH, fW = depth_pred.shape
        assert BN == B * N and fH * ds == H and fW * ds == W
        gt = _f32(gt_depths, "depth_bce").contiguous()
        pred = _f32(depth_pred, "depth_bce").contiguous()
        c0 = float(dbound[0] - dbound[2] / 2)                      # in double, like the reference's Python expression
        args = (BN, D, fH, fW, int(ds), c0, float(dbound[2]), float(weight))
        ws = torch.empty(lib.ssbev_depth_bce_workspace(BN, fH, fW), dtype=torch.uint8, device=pred.device)   # kept for backward
        out = torch.empty(2, dtype=torch.float32, device=pred.device)
        capi.check(lib.ssbev_depth_bce_fwd(capi.ptr(gt), capi.ptr(pred), capi.ptr(out), *args, capi.ptr(ws), ws.numel(),
                                           capi.stream()), "ssbev_depth_bce_fwd")
        ctx.save_for_backward(pred, out, ws)
        ctx.args = args
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        pred, out, ws = ctx.saved_tensors
        gp = torch.empty_like(pred)
        gl = g.to(torch.float32).reshape(1).contiguous()
        capi.check(lib.ssbev_depth_bce_bwd(capi.ptr(pred), capi.ptr(gl), capi.ptr(out), capi.ptr(gp), *ctx.args, capi.ptr(ws),
                                           capi.stream()), "ssbev_depth_bce_bwd")
        return None, gp, None, None, None


def depth_bce_loss(gt_depths, depth_pred, ds, dbound, weight):
    return _DepthBce.apply(gt_depths, depth_pred, ds, dbound, weight)


DEPTH_KLD = os.environ.get("SSBEV_DEPTH_KLD", "1") != "0"    # fused Gaussian KL depth loss (0 = the tensor expression below)
DEPTH_KLD_UNITS = ("reference", "bins")


def _depth_kld_edge_scale(dbound, units):
    """1 for "reference" (the executed formula: mean in bin units, edges in metres), 1 / dd for "bins" (both in bin units)."""
    if units not in DEPTH_KLD_UNITS:
        raise ValueError(f"units must be one of {DEPTH_KLD_UNITS}, got {units!r}")
    return 1.0 if units == "reference" else 1.0 / float(dbound[2])


class _DepthKld(torch.autograd.Function):
    """weight * KL(Gaussian target of the down-sampled LiDAR depth || depth_pred) over the foreground pixels (VT:390-416 +
    utils/gaussian.py:90-130 with constant_std), ``ssbev_depth_kld_fwd / _bwd``: gt_depths [B, N, H, W], depth_pred
    [B*N, D, H/ds, W/ds] -> 0-dim loss.  Nothing is read back to the host."""

    @staticmethod
    def forward(ctx, gt_depths, depth_pred, ds, dbound, weight, std, edge_scale):
        lib = capi.load()
        B, N, H, W = gt_depths.shape
        BN, D, fH, fW = depth_pred.shape
        assert BN == B * N and fH * ds == H and fW * ds == W
        gt = _f32(gt_depths, "depth_kld").contiguous()
        pred = _f32(depth_pred, "depth_kld").contiguous()
        args = (BN, D, fH, fW, int(ds), float(dbound[0]), float(dbound[1]), float(dbound[2]), float(std), float(edge_scale),
                float(weight))
        ws = torch.empty(lib.ssbev_depth_kld_workspace(BN, fH, fW), dtype=torch.uint8, device=pred.device)   # kept for backward
        out = torch.empty(2, dtype=torch.float32, device=pred.device)
        capi.check(lib.ssbev_depth_kld_fwd(capi.ptr(gt), capi.ptr(pred), capi.ptr(out), *args, capi.ptr(ws), ws.numel(),
                                           capi.stream()), "ssbev_depth_kld_fwd")
        ctx.save_for_backward(pred, out, ws)
        ctx.args = args
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        pred, out, ws = ctx.saved_tensors
        gp = torch.empty_like(pred)
        gl = g.to(torch.float32).reshape(1).contiguous()
        capi.check(lib.ssbev_depth_kld_bwd(capi.ptr(pred), capi.ptr(gl), capi.ptr(out), capi.ptr(gp), *ctx.args, capi.ptr(ws),
                                           ws.numel(), capi.stream()), "ssbev_depth_kld_bwd")
        return None, gp, None, None, None, None, None


def depth_kld_loss_tensor(gt_depths, depth_pred, ds, dbound, weight, std=0.5, units="reference"):
    """The Gaussian KL depth loss in ATen ops, on any device (fp32; float64 when ``depth_pred`` is float64): the reference's
    ``generate_guassian_depth_target(..., constant_std=std)`` + ``get_klv_depth_loss`` operation by operation, except that the
    background rows are masked instead of gathered away with a boolean index (a nonzero() + host synchronisation): their target
    and their prediction are replaced by constants, so their terms and gradients vanish exactly.  A target that rounds below
    zero counts as 0, and no foreground row at all gives 0 instead of the reference's 0 / 0."""
    es = _depth_kld_edge_scale(dbound, units)
    d0, d1, dd = (float(v) for v in dbound)
    if not (dd > 0 and std > 0):
        raise ValueError(f"dbound step and std must be positive, got {dd}, {std}")
    B, N, H, W = gt_depths.shape
    BN, D, fH, fW = depth_pred.shape
    assert BN == B * N and fH * ds == H and fW * ds == W
    dt = torch.float64 if depth_pred.dtype == torch.float64 else torch.float32
    dev = depth_pred.device
    x = torch.arange(d0 - dd / 2, d1, dd, dtype=dt, device=dev)
    if x.numel() != D + 1:
        raise ValueError(f"dbound {tuple(dbound)} gives {x.numel()} edges, depth_pred has {D} bins")
    g = gt_depths.to(dt).reshape(BN, fH, ds, fW, ds).permute(0, 1, 3, 2, 4).reshape(-1, ds * ds)
    m = torch.where(g != 0, g, torch.full_like(g, 1e10)).min(dim=-1).values
    m = torch.where(m == 1e10, torch.zeros_like(m), m)
    fg = (m >= d0) & (m <= (d1 - dd))
    rs = (torch.full((), std, dtype=dt, device=dev) / dd).reciprocal()
    cdf = 0.5 * (1 + torch.erf((x * es - (m / dd).unsqueeze(1)) * rs / math.sqrt(2)))
    mask = fg.unsqueeze(1)
    t = torch.where(mask, (cdf[:, 1:] - cdf[:, :-1]).clamp_min(0), torch.zeros((), dtype=dt, device=dev))
    p = depth_pred.to(dt).permute(0, 2, 3, 1).reshape(-1, D)
    logp = torch.log(torch.where(mask, p, torch.ones_like(p)) + 1e-4)
    kl = torch.xlogy(t, t) - t * logp
    return weight * (kl.sum() / fg.sum().to(dt).clamp(min=1.0))


def depth_kld_loss(gt_depths, depth_pred, ds, dbound, weight, std=0.5, units="reference"):
    """``loss_depth_type="kld"``: fp32 CUDA tensors with ``DEPTH_KLD`` on run on the fused HIP path, anything else (CPU, other
    dtypes, the switch off) on ``depth_kld_loss_tensor``."""
    es = _depth_kld_edge_scale(dbound, units)
    if (DEPTH_KLD and depth_pred.is_cuda and gt_depths.is_cuda and depth_pred.dtype == torch.float32
            and gt_depths.dtype == torch.float32):
        return _DepthKld.apply(gt_depths, depth_pred, ds, dbound, weight, std, es)
    return depth_kld_loss_tensor(gt_depths, depth_pred, ds, dbound, weight, std, units)


IMGSEG = os.environ.get("SSBEV_IMGSEG", "1") != "0"          # fused image-view segmentation loss (0 = the tensor expression below)
IMGSEG_MAX_CLASSES = 32


def imgseg_nearest_index(n_in, n_out):
    """int64 [n_out]: the source index ``F.interpolate(mode="nearest")`` reads for every destination index when ``n_in`` entries
    are resized to ``n_out``: min(floor(i * s), n_in - 1) with s = (float)n_in / n_out and the product in fp32 -- the rule
    ``ssbev_imgseg_ce_fwd`` derives its pixel rectangles from."""
    if n_in < 1 or n_out < 1:
        raise ValueError(f"sizes must be positive, got {n_in}, {n_out}")
    s = torch.tensor(float(n_in), dtype=torch.float32) / torch.tensor(float(n_out), dtype=torch.float32)
    return torch.floor(torch.arange(n_out, dtype=torch.float32) * s).long().clamp_(max=n_in - 1)


def _imgseg_labels(seg_labels, K):
    """int64 labels with everything outside [1, K) sent to 0 (= ignored); floating labels are truncated as ``.long()`` does."""
    lab = seg_labels
    if lab.is_floating_point():
        lab = torch.where(torch.isfinite(lab), lab, torch.zeros_like(lab))
    lab = lab.long()
    return torch.where((lab >= 1) & (lab < K), lab, torch.zeros_like(lab))


class _ImgSegCe(torch.autograd.Function):
    """weight * class-weighted cross entropy of the nearest-up-sampled logits against the label map, ignore_index 0 (VT:418-430),
    ``ssbev_imgseg_ce_fwd / _bwd``: logits fp32 [BN, K, h, w] contiguous, labels fp32 [BN, H, W], class weights fp32 [K] -> 0-dim
    loss.  The [BN, K, H, W] tensor is never formed and nothing is read back to the host."""

    @staticmethod
    def forward(ctx, logits, labels, class_w, weight):
        lib = capi.load()
        BN, K, h, w = logits.shape
        H, W = labels.shape[1:]
        args = (BN, K, h, w, H, W, float(weight))
        ws = torch.empty(lib.ssbev_imgseg_ce_workspace(BN, h, w), dtype=torch.uint8, device=logits.device)   # kept for backward
        out = torch.empty(1, dtype=torch.float32, device=logits.device)
        capi.check(lib.ssbev_imgseg_ce_fwd(capi.ptr(logits), capi.ptr(labels), capi.ptr(class_w), *args, capi.ptr(out),
                                           capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_imgseg_ce_fwd")
        ctx.save_for_backward(logits, labels, class_w, ws)
        ctx.args = args
        return out[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        logits, labels, class_w, ws = ctx.saved_tensors
        gx = torch.empty_like(logits)
        gl = g.to(torch.float32).reshape(1).contiguous()
        capi.check(lib.ssbev_imgseg_ce_bwd(capi.ptr(logits), capi.ptr(labels), capi.ptr(class_w), capi.ptr(gl), *ctx.args,
                                           capi.ptr(gx), capi.ptr(ws), capi.stream()), "ssbev_imgseg_ce_bwd")
        return gx, None, None, None


def _imgseg_check(seg_logits, seg_labels, class_weights):
    if seg_logits.dim() != 4 or seg_labels.dim() != 3 or seg_labels.shape[0] != seg_logits.shape[0]:
        raise ValueError(f"logits [BN, K, h, w] and labels [BN, H, W] expected, got {tuple(seg_logits.shape)}, "
                         f"{tuple(seg_labels.shape)}")
    K = seg_logits.shape[1]
    if not 2 <= K <= IMGSEG_MAX_CLASSES or class_weights.numel() != K:
        raise ValueError(f"2 .. {IMGSEG_MAX_CLASSES} classes with one weight each expected, got {K} and {class_weights.numel()}")


def imgseg_loss_tensor(seg_logits, seg_labels, class_weights, weight=1.0):
    """The image-view segmentation loss in ATen ops, on any device (fp32; float64 when ``seg_logits`` is float64): the
    reference's lines (VT:418-430) -- ``F.interpolate`` (nearest) of the logits to the label map, then the class-weighted
    cross entropy with ``ignore_index=0`` -- as weighted sum over weight sum, so that no valid pixel gives 0 with a zero gradient
    instead of the reference's 0 / 0.  Labels outside [0, K) are ignored (the reference raises on them)."""
    _imgseg_check(seg_logits, seg_labels, class_weights)
    dt = torch.float64 if seg_logits.dtype == torch.float64 else torch.float32
    x = seg_logits.to(dt)
    lab = _imgseg_labels(seg_labels, x.shape[1])
    if x.shape[-2:] != lab.shape[-2:]:
        x = torch.nn.functional.interpolate(x, size=lab.shape[1:])
    cw = class_weights.to(device=x.device, dtype=dt)
    num = torch.nn.functional.cross_entropy(x, lab, weight=cw, ignore_index=0, reduction="sum")
    den = (cw[lab] * (lab > 0).to(dt)).sum()
    return weight * (num / torch.where(den > 0, den, torch.ones_like(den)))


def imgseg_loss(seg_logits, seg_labels, class_weights, weight=1.0):
    """``imgseg=True``: weight * cross entropy of the segmentation head's logits [BN, K, h, w] against the projected LiDAR
    labels [BN, H, W] (fp32 as the loader writes them, or int64).  fp32 CUDA logits with ``IMGSEG`` on and h <= H, w <= W run on
    the fused HIP path (channels-last logits are made contiguous, int64 labels are converted: 154 kB and 2 MB at the model's
    size), anything else (CPU, other dtypes, the switch off) on ``imgseg_loss_tensor``."""
    _imgseg_check(seg_logits, seg_labels, class_weights)
    h, w = seg_logits.shape[-2:]
    H, W = seg_labels.shape[-2:]
    if (IMGSEG and seg_logits.is_cuda and seg_labels.is_cuda and seg_logits.dtype == torch.float32 and h <= H and w <= W
            and seg_logits.numel() > 0 and seg_labels.numel() > 0):
        lab = seg_labels if seg_labels.dtype == torch.float32 else seg_labels.to(torch.float32)
        cw = class_weights.to(device=seg_logits.device, dtype=torch.float32).contiguous()
        return _ImgSegCe.apply(seg_logits.contiguous(), lab.contiguous(), cw, weight)
    return imgseg_loss_tensor(seg_logits, seg_labels, class_weights, weight)


# -------------------------------------------------------------------------------------------------
# lifted-point position encoder (point_xyz_channel, VT:432-476; csrc/point_xyz.hip)
# -------------------------------------------------------------------------------------------------
POINT_XYZ = os.environ.get("SSBEV_POINT_XYZ", "1") != "0"    # fused position encoder (0 = the tensor form: one row per kept point)
POINT_XYZ_MAX_WIDTH = 512                                    # Cxyz: M = Cxyz / 2 channels-last rows of at most 256 floats


def voxel_index_tensor(geom, origin, dx, n):
    """``voxel_index`` in ATen ops, on any device: geom [B, ..., 3] fp32, ``origin`` / ``dx`` / ``n`` = the host lists of
    ``grid_host`` -> vox int32 [B*P] (linear voxel or -1), the same fp32 subtract, divide and truncation (VT:441-451)."""
    B = geom.shape[0]
    g = geom.reshape(B, -1, 3)
    f = (g - torch.tensor(origin, dtype=g.dtype, device=g.device)) / torch.tensor(dx, dtype=g.dtype, device=g.device)
    nn_ = torch.tensor([float(v) for v in n], dtype=g.dtype, device=g.device)
    kept = ((f > -1.0) & (f < nn_)).all(-1)
    i = torch.where(kept.unsqueeze(-1), f, torch.zeros_like(f)).long()
    b = torch.arange(B, device=g.device).view(B, 1)
    v = ((b * n[0] + i[..., 0]) * n[1] + i[..., 1]) * n[2] + i[..., 2]
    return torch.where(kept, v, torch.full_like(v, -1)).to(torch.int32).reshape(-1)


def point_xyz_unit(geom, pc_range):
    """u = ((g - lo) / (hi - lo) - 0.5) * 2 for every point: geom [..., 3] -> [P, 3] in geom's dtype (VT:455-458)."""
    g = geom.reshape(-1, 3)
    lo = torch.tensor([float(v) for v in pc_range[:3]], dtype=g.dtype, device=g.device)
    hi = torch.tensor([float(v) for v in pc_range[3:]], dtype=g.dtype, device=g.device)
    return ((g - lo) / (hi - lo) - 0.5) * 2


def point_xyz_pool_tensor(geom, vox, pc_range, grid, w1, b1, gamma, beta, w2, b2, running_mean=None, running_var=None,
                          num_batches_tracked=None, training=True, eps=1e-5, momentum=0.1):
    """The position encoder in its literal form, on any device: ``u[kept]`` is materialised, ``Linear(3, M) -> BatchNorm1d ->
    ReLU -> Linear(M, Cxyz)`` runs on the [n_kept, .] matrices with plain torch ops (training mode: batch statistics over all
    kept points of all samples, running statistics updated in place), the rows are summed per voxel (``bev_pool`` on the card,
    ``index_add_`` on the CPU).  geom [B, ..., 3], vox int32 [B*P], ``grid`` = (nx, ny, nz) -> [B, Cxyz, nx, ny, nz].
    Fewer than two kept points in training mode (the reference raises): zeros, zero gradients, statistics untouched."""
    B = geom.shape[0]
    nx, ny, nz = (int(v) for v in grid)
    Cx = w2.shape[0]
    kept = vox >= 0
    u = point_xyz_unit(geom, pc_range)[kept]
    n = u.shape[0]
    if n == 0 or (training and n < 2):
        zero = sum((p * 0).sum() for p in (w1, b1, gamma, beta, w2, b2))
        return torch.zeros(B, Cx, nx, ny, nz, dtype=w2.dtype, device=geom.device) + zero
    u = u.to(w1.dtype)
    h = torch.nn.functional.linear(u, w1, b1)
    h = torch.nn.functional.batch_norm(h, running_mean, running_var, gamma, beta, training, momentum, eps)
    if training and num_batches_tracked is not None:
        num_batches_tracked += 1
    f = torch.nn.functional.linear(torch.relu(h), w2, b2)
    idx = vox[kept].long()
    if f.is_cuda and f.dtype == torch.float32:
        iz, r = idx % nz, idx // nz
        iy, r = r % ny, r // ny
        ix, b = r % nx, r // nx
        return bev_pool(f, torch.stack((ix, iy, iz, b), 1), B, nz, nx, ny).permute(0, 1, 3, 4, 2)
    out = torch.zeros(B * nx * ny * nz, Cx, dtype=f.dtype, device=f.device).index_add_(0, idx, f)
    return out.view(B, nx, ny, nz, Cx).permute(0, 4, 1, 2, 3)


def point_xyz_moments_tensor(geom, vox, pc_range):
    """[10] float64: count, sum u, sum u u^T (xx, xy, xz, yy, yz, zz) over the kept points, in ATen ops."""
    u = point_xyz_unit(geom, pc_range)[vox >= 0].double()
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    cols = [torch.ones_like(x), x, y, z, x * x, x * y, x * z, y * y, y * z, z * z]
    return torch.stack([c.sum() for c in cols])


def point_xyz_stats(moments, w1, b1):
    """Batch statistics of h = W1 u + b1 from the ten moments, float64 on the moments' device, nothing read back:
    (n, ubar [3], cov [3, 3] biased, mu [M] = W1 ubar + b1, var [M] = w_m^T cov w_m)."""
    m = moments.double()
    n = m[0]
    ns = torch.clamp(n, min=1.0)
    ubar = m[1:4] / ns
    s2 = torch.stack((m[4], m[5], m[6], m[5], m[7], m[8], m[6], m[8], m[9])).view(3, 3) / ns
    cov = s2 - torch.outer(ubar, ubar)
    w = w1.detach().double()
    mu = w @ ubar + b1.detach().double()
    var = torch.clamp(((w @ cov) * w).sum(1), min=0.0)
    return n, ubar, cov, mu, var


def _point_xyz_dims(B, P, grid, M, pc_range):
    d = capi.PointXyzDims()
    d.B, d.P, d.nx, d.ny, d.nz, d.M = int(B), int(P), int(grid[0]), int(grid[1]), int(grid[2]), int(M)
    for i in range(3):
        d.lo[i] = float(pc_range[i])
        d.hi[i] = float(pc_range[3 + i])
    return d


def point_xyz_moments(geom, vox, pc_range, grid):
    """The ten moments (``point_xyz_moments_tensor``) by ``ssbev_point_xyz_moments``: one pass over geom [B, ..., 3] + vox,
    double sums folded in a fixed order, the result stays on the device.  They depend on the calibration only."""
    if not (POINT_XYZ and geom.is_cuda):
        return point_xyz_moments_tensor(geom, vox, pc_range)
    lib = capi.load()
    B = geom.shape[0]
    g = _f32(geom, "point_xyz_moments").reshape(B, -1, 3).contiguous()
    d = _point_xyz_dims(B, g.shape[1], grid, 4, pc_range)
    out = torch.empty(10, dtype=torch.float64, device=g.device)
    ws = _ws(lib.ssbev_point_xyz_workspace(C.byref(d)), g.device)
    capi.check(lib.ssbev_point_xyz_moments(capi.ptr(g), capi.ptr(vox), capi.ptr(out), C.byref(d), capi.ptr(ws), ws.numel(),
                                           capi.stream()), "ssbev_point_xyz_moments")
    return out


class _PointXyzSum(torch.autograd.Function):
    """S[v] = sum_{p in v} relu(BN(W1 u_p + b1)) as [NV, M] (``ssbev_point_xyz_fwd / _bwd``): the per-point rows are never
    formed.  Training mode normalises with the batch statistics that follow from the moments and updates the running
    statistics on the device; eval mode with the running statistics.  Backward: five sums per channel from one walk, then

        gbeta = sum gz,  ggamma = sum gz hhat,
        gW1[m] = (gamma_m / s_m) (sum gz u - (gbeta_m / n) sum u - (ggamma_m / s_m) Cov(u) w_m),  gb1 = 0        (training)
        gW1[m] = (gamma_m / s_m) sum gz u,  gb1 = (gamma_m / s_m) sum gz                                         (eval)."""

    @staticmethod
    def forward(ctx, w1, b1, gamma, beta, geom, starts, order, moments, running_mean, running_var, num_batches_tracked,
                pc_range, grid, training, eps, momentum):
        lib = capi.load()
        B = geom.shape[0]
        g = geom.detach().reshape(B, -1, 3).contiguous()
        M = w1.shape[0]
        d = _point_xyz_dims(B, g.shape[1], grid, M, pc_range)
        n, ubar, cov, mu, var = point_xyz_stats(moments, w1, b1)
        w64 = w1.detach().double()
        if training:
            valid = n >= 2.0
            s = torch.sqrt(var + eps)
            c3 = -(w64 @ ubar) / s
            if running_mean is not None:
                with torch.no_grad():
                    unb = var * (n / torch.clamp(n - 1.0, min=1.0))
                    running_mean.copy_(torch.where(valid, (1 - momentum) * running_mean.double() + momentum * mu,
                                                   running_mean.double()))
                    running_var.copy_(torch.where(valid, (1 - momentum) * running_var.double() + momentum * unb,
                                                  running_var.double()))
                    if num_batches_tracked is not None:
                        num_batches_tracked += valid.to(num_batches_tracked.dtype)
        else:
            valid = torch.ones((), dtype=torch.bool, device=g.device)
            s = torch.sqrt(running_var.detach().double() + eps)
            c3 = (b1.detach().double() - running_mean.detach().double()) / s
        coef = torch.cat(((w64 / s[:, None]).t(), c3[None], gamma.detach().double()[None], beta.detach().double()[None]), 0)
        coef = (coef * valid).to(torch.float32).contiguous()                 # [6, M]; all zero without statistics: S = 0
        nv = B * d.nx * d.ny * d.nz
        S = torch.empty(nv, M, dtype=torch.float32, device=g.device)
        nby = 4.0 * (4 * g.shape[0] * g.shape[1] + S.numel())
        with _span("point_xyz", 2.0 * 4 * g.shape[0] * g.shape[1] * M, nby, f"fwd   point_xyz M={M} grid={d.nx}x{d.ny}x{d.nz}"):
            capi.check(lib.ssbev_point_xyz_fwd(capi.ptr(g), capi.ptr(starts), capi.ptr(order), capi.ptr(getattr(order, "long_list", None)),
                                               capi.ptr(coef), capi.ptr(S), C.byref(d), capi.stream()), "ssbev_point_xyz_fwd")
        ctx.save_for_backward(g, starts, order.as_subclass(torch.Tensor), coef, w64, gamma.detach().double(), s, n, ubar, cov, moments, valid)
        ctx.d, ctx.training = d, bool(training)
        return S

    @staticmethod
    def backward(ctx, gS):
        lib = capi.load()
        g, starts, order, coef, w64, gam, s, n, ubar, cov, moments, valid = ctx.saved_tensors
        d = ctx.d
        M = d.M
        gS = gS.contiguous()
        sums = torch.empty(5, M, dtype=torch.float64, device=g.device)
        ws = _ws(lib.ssbev_point_xyz_workspace(C.byref(d)), g.device)
        with _span("point_xyz", 2.0 * 9 * g.shape[0] * g.shape[1] * M, 4.0 * (4 * g.shape[0] * g.shape[1] + gS.numel()),
                   f"bwd   point_xyz M={M}"):
            capi.check(lib.ssbev_point_xyz_bwd(capi.ptr(g), capi.ptr(starts), capi.ptr(order), capi.ptr(coef), capi.ptr(gS),
                                               capi.ptr(sums), C.byref(d), capi.ptr(ws), ws.numel(), capi.stream()),
                       "ssbev_point_xyz_bwd")
        gbeta, ggamma, gzu = sums[0], sums[1], sums[2:5].t()                 # [M], [M], [M, 3]
        k = (gam / s)[:, None]
        if ctx.training:
            ns = torch.clamp(n, min=1.0)
            gw1 = k * (gzu - (gbeta / ns)[:, None] * moments[1:4][None] - (ggamma / s)[:, None] * (w64 @ cov))
            gb1 = torch.zeros_like(gbeta)
        else:
            gw1 = k * gzu
            gb1 = (gam / s) * gbeta
        z = torch.zeros((), dtype=torch.float64, device=g.device)
        gw1, gb1, ggamma, gbeta = (torch.where(valid, t, z).to(torch.float32) for t in (gw1, gb1, ggamma, gbeta))
        return (gw1, gb1, ggamma, gbeta) + (None,) * 12


def point_xyz_pool(geom, tables, pc_range, grid, w1, b1, gamma, beta, w2, b2, running_mean=None, running_var=None,
                   num_batches_tracked=None, training=True, eps=1e-5, momentum=0.1, moments=None):
    """``point_xyz_channel``: P[v] = sum_{p in v} Linear(relu(BN(Linear(u_p)))) = W2 S[v] + n_v b2 -> [B, Cxyz, nx, ny, nz]
    (channels-last memory) for geom [B, ..., 3] and ``tables`` = lift_splat_tables of it.  fp32 CUDA tensors with ``POINT_XYZ``
    on take the fused path: statistics from ``moments`` (``point_xyz_moments``; computed here when None), S by
    ``_PointXyzSum``, the second Linear as a row-wise GEMM on the [NV, M] voxel sums (``small_linear``: forward, gS and gW2
    on the own GEMM kernels), the bias term as one addcmul with the list lengths.  Anything else: ``point_xyz_pool_tensor``."""
    vox, starts, order = tables
    M, Cx = w1.shape[0], w2.shape[0]
    fused = POINT_XYZ and geom.is_cuda and geom.dtype == torch.float32 and w1.dtype == torch.float32
    if geom.is_cuda and storage_bf16():
        raise NotImplementedError("point_xyz_channel is built for fp32 only (SSBEV_PRECISION=bf16 is refused)")
    if not fused:
        return point_xyz_pool_tensor(geom, vox, pc_range, grid, w1, b1, gamma, beta, w2, b2, running_mean, running_var,
                                     num_batches_tracked, training, eps, momentum)
    if M % 4 or not 4 <= M <= POINT_XYZ_MAX_WIDTH // 2 or Cx % 4:
        raise capi.SsbevError(f"point_xyz_pool: M = {M} (a multiple of 4 up to {POINT_XYZ_MAX_WIDTH // 2}) and Cxyz = {Cx} refused")
    if not training and (running_mean is None or running_var is None):
        raise ValueError("point_xyz_pool: eval mode needs running statistics")
    B = geom.shape[0]
    nx, ny, nz = (int(v) for v in grid)
    if moments is None:
        with torch.no_grad():
            moments = point_xyz_moments(geom, vox, pc_range, grid)
    S = _PointXyzSum.apply(w1, b1, gamma, beta, geom, starts, order, moments, running_mean, running_var, num_batches_tracked,
                           tuple(float(v) for v in pc_range), (nx, ny, nz), bool(training), float(eps), float(momentum))
    with torch.no_grad():
        cnt = (starts[1:] - starts[:-1]).to(torch.float32)
        if training:
            cnt = cnt * (moments[0] >= 2.0)
    P = torch.addcmul(small_linear(S, w2), cnt[:, None], b2[None])
    return from_cl(P.view(B, nx, ny, nz, Cx))


# -------------------------------------------------------------------------------------------------
# point-level branch of the head (occhead.py:171-236, 363-398; csrc/point_head.hip)
# -------------------------------------------------------------------------------------------------
POINT_HEAD = os.environ.get("SSBEV_POINT_HEAD", "1") != "0"  # fused point sampling and point CE (0 = the tensor forms: grid_sample, cross_entropy)
POINT_AXIS_ORDERS = ("reference", "xyz")
POINT_HEAD_MAX_LEVELS = 4


def point_unit(points, pc_range):
    """g = ((p[:, :3] - lo) / (hi - lo)) * 2 - 1 in the points' dtype, each step rounded as the tensor expression of
    occhead.py:178-183 rounds it: [n, >= 3] -> [n, 3]."""
    p = points[:, :3]
    dt = np.float64 if p.dtype == torch.float64 else np.float32
    lo = np.asarray(pc_range[:3], dtype=dt)
    rng = np.asarray(pc_range[3:], dtype=dt) - lo                 # rounded in the points' dtype, as the tensor subtraction is
    # the six bounds ride as scalar kernel arguments: no host tensor is copied to the device
    return torch.stack([(p[:, i] - float(lo[i])) / float(rng[i]) for i in range(3)], 1) * 2 - 1


def _point_offsets(counts, device):
    """int32 [B + 1] on ``device`` from the host-known sample sizes: pinned staging + an asynchronous copy, nothing read back."""
    offs = torch.tensor([0] + list(np.cumsum(counts)), dtype=torch.int32)
    return offs.pin_memory().to(device, non_blocking=True) if torch.device(device).type == "cuda" else offs


def point_sample_tensor(feats, g, counts, axis_order="reference", per_level=False):
    """``point_sample`` as literal ``grid_sample`` calls, one per sample and level, on any device and in the features' dtype.

    The reference hands g = (x, y, z) to ``grid_sample`` unflipped (occhead.py:186-189), and ``grid_sample``'s first grid
    coordinate addresses the LAST tensor axis.  Seen on the CPU (and asserted by tests/test_point_head.py): on a [1, 1, 2, 3, 5]
    map filled with 100 x + 10 y + z, the centre of cell (x, y, z) = (1, 1, 0), g = (0.5, 0, -0.8), reads 9.275 as given -- its
    x = 0.5 walks the 5-long Z axis to index 3.25, its z = -0.8 the 2-long X axis to index -0.3, so 0.7 * (10 + 3.25) -- and
    110, the cell's value, when given as (z, y, x).  ``axis_order="xyz"`` therefore flips the coordinates before the call."""
    if axis_order not in POINT_AXIS_ORDERS:
        raise ValueError(f"axis_order must be one of {POINT_AXIS_ORDERS}, got {axis_order!r}")
    C_ = feats[0].shape[1]
    g = g.to(feats[0].dtype)
    if axis_order == "xyz":
        g = g.flip(-1)
    levels = []
    for f in feats:
        rows, at = [], 0
        for b, n in enumerate(counts):
            if n:
                s = torch.nn.functional.grid_sample(f[b:b + 1], g[at:at + n].view(1, 1, 1, n, 3), mode="bilinear",
                                                    padding_mode="zeros", align_corners=False)
                rows.append(s.reshape(C_, n).t())
            at += n
        levels.append(torch.cat(rows, 0) if rows else f.new_zeros(0, C_))
    return torch.stack(levels, 0) if per_level else sum(levels[1:], levels[0])


def point_img_mask(uv):
    """feature_sampling's mask (occhead.py:436-440): depth > 1e-5 and u, v strictly inside (-1, 1); uv [n, cams, 3] -> bool."""
    return (uv[..., 2] > 1e-5) & (uv[..., 0] > -1.0) & (uv[..., 0] < 1.0) & (uv[..., 1] > -1.0) & (uv[..., 1] < 1.0)


def point_img_sample_tensor(img_feats, uv, counts):
    """``point_img_sample`` as literal ``grid_sample`` calls (occhead.py:196-206, 428-453): bilinear samples per camera,
    ``nan_to_num``, times the mask, summed over the cameras."""
    C_ = img_feats.shape[2]
    uv = uv.to(img_feats.dtype)
    rows, at = [], 0
    for b, n in enumerate(counts):
        if n:
            p = uv[at:at + n]
            s = torch.nn.functional.grid_sample(img_feats[b], p[..., :2].permute(1, 0, 2).unsqueeze(2), mode="bilinear",
                                                padding_mode="zeros", align_corners=False)
            s = torch.nan_to_num(s.squeeze(-1).permute(2, 0, 1))                     # [n, cams, C]
            rows.append((s * point_img_mask(p).to(s.dtype).unsqueeze(-1)).sum(1))
        at += n
    return torch.cat(rows, 0) if rows else img_feats.new_zeros(0, C_)


def _point_csr(ws, nk, cells):
    """(starts, order) of the keys at the start of a sampling workspace: ``pool_prepare``'s stable sort, which drops the -1 keys
    of skipped corners.  Its long-list output is not used: the gradient kernel walks every list in list order."""
    starts, order = pool_prepare(ws[:4 * nk].view(torch.int32), 1, cells, 1, 1)
    return starts, order.as_subclass(torch.Tensor)


class _PointSample(torch.autograd.Function):
    """``ssbev_point_sample_fwd / _bwd``: g [N, 3], offsets int32 [B + 1], levels [B, C, X, Y, Z] -> rows [L, N, C] or [N, C].
    Forward keeps the (key, weight) pairs and, when a level needs a gradient, the CSR table of the keys; backward writes every
    cell of every level once."""

    @staticmethod
    def forward(ctx, g, offs, axis_xyz, per_level, *feats):
        lib = capi.load()
        xcl = [to_cl(_f32(f, "point_sample")) for f in feats]
        B, C_ = xcl[0].shape[0], xcl[0].shape[-1]
        N = g.shape[0]
        d = capi.PointHeadDims()
        d.B, d.N, d.C, d.L, d.axis_xyz, d.per_level = B, N, C_, len(xcl), int(axis_xyz), int(per_level)
        cells = 0
        for l, x in enumerate(xcl):
            d.X[l], d.Y[l], d.Z[l] = (int(v) for v in x.shape[1:4])
            cells += x.numel() // C_
        nws = lib.ssbev_point_sample_workspace(C.byref(d))
        if not nws:
            raise capi.SsbevError(f"point_sample: dims refused (N = {N}, C = {C_}, levels {[tuple(x.shape) for x in xcl]})")
        ws = torch.empty(nws, dtype=torch.uint8, device=g.device)                   # kept for backward
        rows = torch.empty((len(xcl), N, C_) if per_level else (N, C_), dtype=torch.float32, device=g.device)
        ptrs = [capi.ptr(x) for x in xcl] + [None] * (POINT_HEAD_MAX_LEVELS - len(xcl))
        with _span("point_head", 2.0 * 8 * len(xcl) * N * C_, 4.0 * 9 * len(xcl) * N * C_, f"fwd   point_sample N={N} C={C_}"):
            capi.check(lib.ssbev_point_sample_fwd(capi.ptr(g), capi.ptr(offs), *ptrs, capi.ptr(rows), C.byref(d), capi.ptr(ws),
                                                  ws.numel(), capi.stream()), "ssbev_point_sample_fwd")
        if any(ctx.needs_input_grad[4:]):
            starts, order = _point_csr(ws, len(xcl) * 8 * N, cells)
            ctx.save_for_backward(starts, order, ws)
        ctx.d, ctx.shapes = d, [x.shape for x in xcl]
        return rows

    @staticmethod
    def backward(ctx, grows):
        lib = capi.load()
        starts, order, ws = ctx.saved_tensors
        d = ctx.d
        grows = grows.contiguous()
        gf = [torch.empty(s, dtype=torch.float32, device=grows.device) for s in ctx.shapes]
        ptrs = [capi.ptr(x) for x in gf] + [None] * (POINT_HEAD_MAX_LEVELS - len(gf))
        with _span("point_head", 2.0 * 8 * d.L * d.N * d.C, 4.0 * sum(x.numel() for x in gf), f"bwd   point_sample N={d.N} C={d.C}"):
            capi.check(lib.ssbev_point_sample_bwd(capi.ptr(grows), capi.ptr(starts), capi.ptr(order), capi.ptr(ws), *ptrs,
                                                  C.byref(d), capi.stream()), "ssbev_point_sample_bwd")
        return (None, None, None, None) + tuple(from_cl(x) for x in gf)


class _PointImgSample(torch.autograd.Function):
    """``ssbev_point_img_fwd / _bwd``: img [B, cams, C, H, W], uv [N, cams, 3], offsets -> rows [N, C].  The CSR table and the
    gradient exist only when the image features require a gradient."""

    @staticmethod
    def forward(ctx, img, uv, offs):
        lib = capi.load()
        B, cams, C_, H, W = img.shape
        icl = to_cl(_f32(img, "point_img_sample").reshape(B * cams, C_, H, W))        # [B cams, H, W, C]
        N = uv.shape[0]
        d = capi.PointImgDims(B, N, cams, C_, H, W)
        nws = lib.ssbev_point_img_workspace(C.byref(d))
        if not nws:
            raise capi.SsbevError(f"point_img_sample: dims refused (N = {N}, img {tuple(img.shape)})")
        ws = torch.empty(nws, dtype=torch.uint8, device=img.device)
        rows = torch.empty(N, C_, dtype=torch.float32, device=img.device)
        with _span("point_head", 2.0 * 4 * cams * N * C_, 4.0 * 5 * cams * N * C_, f"fwd   point_img N={N} C={C_}"):
            capi.check(lib.ssbev_point_img_fwd(capi.ptr(icl), capi.ptr(uv), capi.ptr(offs), capi.ptr(rows), C.byref(d),
                                               capi.ptr(ws), ws.numel(), capi.stream()), "ssbev_point_img_fwd")
        if ctx.needs_input_grad[0]:
            starts, order = _point_csr(ws, 4 * cams * N, B * cams * H * W)
            ctx.save_for_backward(starts, order, ws)
        ctx.d = d
        return rows

    @staticmethod
    def backward(ctx, grows):
        lib = capi.load()
        starts, order, ws = ctx.saved_tensors
        d = ctx.d
        grows = grows.contiguous()
        gi = torch.empty(d.B * d.cams, d.H, d.W, d.C, dtype=torch.float32, device=grows.device)
        with _span("point_head", 2.0 * 4 * d.cams * d.N * d.C, 4.0 * gi.numel(), f"bwd   point_img N={d.N} C={d.C}"):
            capi.check(lib.ssbev_point_img_bwd(capi.ptr(grows), capi.ptr(starts), capi.ptr(order), capi.ptr(ws), capi.ptr(gi),
                                               C.byref(d), capi.stream()), "ssbev_point_img_bwd")
        return from_cl(gi).reshape(d.B, d.cams, d.C, d.H, d.W), None, None


def _point_head_fused(*ts):
    if any(t.is_cuda for t in ts) and storage_bf16():
        raise NotImplementedError("the head's point-level branch is built for fp32 only (SSBEV_PRECISION=bf16 is refused)")
    return POINT_HEAD and all(t.is_cuda and t.dtype == torch.float32 for t in ts)


def point_sample(feats, g, counts, axis_order="reference", per_level=False):
    """Trilinear samples of the voxel feature maps at the points of a batch (occhead.py:185-189): ``feats`` = list of L levels
    [B, C, X_l, Y_l, Z_l], g [N, 3] = ``point_unit`` of all samples' points one after the other, ``counts`` = the host list of
    the B sample sizes -> [L, N, C] (``per_level``) or the sum over the levels [N, C].  fp32 CUDA tensors with ``POINT_HEAD`` on,
    up to 4 levels of one width C % 4 == 0 and N > 0 take the fused path (one launch forward, one backward over a CSR table of the
    corners: no float atomics); anything else ``point_sample_tensor``.  bf16 storage is refused."""
    if axis_order not in POINT_AXIS_ORDERS:
        raise ValueError(f"axis_order must be one of {POINT_AXIS_ORDERS}, got {axis_order!r}")
    feats = list(feats)
    if sum(counts) != g.shape[0] or any(f.shape[0] != len(counts) for f in feats):
        raise ValueError("point_sample: counts must name every sample's points")
    C_ = feats[0].shape[1]
    ok = (_point_head_fused(g, *feats) and g.shape[0] > 0 and C_ % 4 == 0 and len(feats) <= POINT_HEAD_MAX_LEVELS
          and all(f.dim() == 5 and f.shape[1] == C_ for f in feats))
    if not ok:
        return point_sample_tensor(feats, g, counts, axis_order, per_level)
    offs = _point_offsets(counts, g.device)
    return _PointSample.apply(g.detach().contiguous(), offs, axis_order == "xyz", bool(per_level), *feats)


def point_img_sample(img_feats, uv, counts):
    """Masked bilinear samples of the image features at the points' projections, summed over the cameras (occhead.py:196-206,
    428-453): img_feats [B, cams, C, H, W], uv [N, cams, 3] = (u, v, depth) -> [N, C].  The fused path (fp32 CUDA, ``POINT_HEAD``
    on, C % 4 == 0, N > 0) never reads a masked pair, so NaN features behind one are not scrubbed (the tensor form's
    ``nan_to_num`` turns NaN samples of kept pairs into 0 as the reference does); the gradient wrt the image features is built
    only when they require one."""
    if sum(counts) != uv.shape[0] or img_feats.shape[0] != len(counts) or uv.shape[1] != img_feats.shape[1]:
        raise ValueError(f"point_img_sample: img_feats {tuple(img_feats.shape)} and uv {tuple(uv.shape)} disagree")
    if not (_point_head_fused(img_feats, uv) and uv.shape[0] > 0 and img_feats.shape[2] % 4 == 0):
        return point_img_sample_tensor(img_feats, uv, counts)
    return _PointImgSample.apply(img_feats, uv.detach().contiguous(), _point_offsets(counts, uv.device))


def point_ce_loss_tensor(logits, labels):
    """Unweighted ``CrossEntropyLoss(ignore_index=0)`` of logits [N, K] against labels [N] in ATen ops, as sum over count, so that
    no labelled point gives 0 with a zero gradient (the reference: NaN).  Labels outside [1, K) are ignored."""
    lab = _imgseg_labels(labels, logits.shape[1])
    num = torch.nn.functional.cross_entropy(logits, lab, ignore_index=0, reduction="sum")
    den = (lab > 0).sum().to(logits.dtype)
    return num / torch.where(den > 0, den, torch.ones_like(den))


def point_ce_loss(logits, labels):
    """``loss_point_ce_`` before its weight (occhead.py:384-386).  On the fused path the [N, K] logits are the [1, K, N, 1] map of
    the image-view segmentation kernel with unit class weights (``ssbev_imgseg_ce_fwd``: one wave per point, log-softmax, pick,
    the partial sums folded in a fixed order by the shared ``block_fold256``): one deterministic pass, nothing read back."""
    N, K = logits.shape
    if (_point_head_fused(logits) and IMGSEG and labels.is_cuda and 2 <= K <= IMGSEG_MAX_CLASSES and 0 < N < 2 ** 24):
        lab = labels.to(torch.float32).reshape(1, N, 1).contiguous()
        cw = torch.ones(K, dtype=torch.float32, device=logits.device)
        return _ImgSegCe.apply(logits.t().contiguous().view(1, K, N, 1), lab, cw, 1.0)
    if N == 0:
        return logits.sum() * 0.0
    return point_ce_loss_tensor(logits, labels)


def point_lovasz_loss(logits, labels):
    """``loss_point_lovasz_`` before its weight (occhead.py:389-394): ``lovasz_softmax(softmax(logits), labels, ignore=0)`` on
    the [1, K, N, 1, 1] view.  fp32 CUDA logits of 20 classes run on the fused Lovasz kernels (``lovasz_softmax``; the view is
    already channels-last, so nothing is copied); anything else on ``losses.lovasz_softmax_tensor``.  0 with a zero gradient
    when no point is labelled."""
    N, K = logits.shape
    if N == 0:
        return logits.sum() * 0.0
    lab = _imgseg_labels(labels, K).view(1, N, 1, 1)
    x5 = logits.contiguous().view(1, N, 1, 1, K).permute(0, 4, 1, 2, 3)
    if _point_head_fused(logits):
        return lovasz_softmax(x5, lab, ignore=0)
    from .plugin import losses
    return losses.lovasz_softmax_tensor(x5, lab, 0)


OCC_TAIL =os.environ.get("SSBEV_OCC_TAIL", "1") != "0"     # scalar loss algebra in one launch (0 = ~110 tiny ATen ops)


class _OccLossTail(torch.autograd.Function):
    """(diff [41] f64, aux f64) from _OccLossSums -> the three weighted losses + the two metric scalars (five 0-dim float
    tensors), ``ssbev_occ_loss_tail``: forward also returns the Jacobian, backward scales its three rows."""

    @staticmethod
    def forward(ctx, diff, aux, w_ce, w_sem, w_geo):
        lib = capi.load()
        ctx.set_materialize_grads(False)
        nd = diff.numel()
        nc = (nd - 1) // 2
        # back to the kernel's layout: ce_num, ce_den, M, sum_p, nom, cnt, conf
        sums = torch.cat((diff[0:1], aux[0:2], diff[1:], aux[2:])).contiguous()
        assert sums.numel() == lib.ssbev_occ_loss_num_sums() and nc * 2 + 1 == nd
        out = torch.empty(5, dtype=torch.float32, device=diff.device)
        jac = torch.empty(3, nd, dtype=torch.float64, device=diff.device)
        capi.check(lib.ssbev_occ_loss_tail(capi.ptr(sums), float(w_ce), float(w_sem), float(w_geo), capi.ptr(out), capi.ptr(jac),
                                           capi.stream()), "ssbev_occ_loss_tail")
        ctx.save_for_backward(jac)
        outs = tuple(out[i] for i in range(5))
        ctx.mark_non_differentiable(outs[3], outs[4])
        return outs

    @staticmethod
    def backward(ctx, g_ce, g_sem, g_geo, _g3, _g4):
        (jac,) = ctx.saved_tensors
        gd = None
        for k, g in enumerate((g_ce, g_sem, g_geo)):
            if g is not None:
                term = jac[k] * g.to(torch.float64)
                gd = term if gd is None else gd + term
        return gd, None, None, None, None


def occ_loss_tail(diff, aux, w_ce, w_sem, w_geo):
    return _OccLossTail.apply(diff, aux, w_ce, w_sem, w_geo)


class _OccDiceTail(torch.autograd.Function):
    """(diff [41] f64, aux f64) from _OccLossSums -> the soft-Dice loss of the occupied probability (0-dim float),
    ``ssbev_occ_dice_tail``: forward also returns the Jacobian row over ``diff``, backward scales it."""

    @staticmethod
    def forward(ctx, diff, aux, smooth):
        lib = capi.load()
        nd = diff.numel()
        sums = torch.cat((diff[0:1], aux[0:2], diff[1:], aux[2:])).contiguous()      # the kernel's layout, as in _OccLossTail
        assert sums.numel() == lib.ssbev_occ_loss_num_sums()
        out = torch.empty(1, dtype=torch.float32, device=diff.device)
        jac = torch.empty(nd, dtype=torch.float64, device=diff.device)
        capi.check(lib.ssbev_occ_dice_tail(capi.ptr(sums), float(smooth), capi.ptr(out), capi.ptr(jac), capi.stream()),
                   "ssbev_occ_dice_tail")
        ctx.save_for_backward(jac)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (jac,) = ctx.saved_tensors
        return jac * g.to(torch.float64), None, None


def occ_dice_tail(diff, aux, smooth=1.0):
    """Soft-Dice voxel loss (SoftDiceLossWithProb of ``1 - p_0`` against ``t > 0`` over the labelled voxels) from the sums of
    ``occ_loss_sums``: one launch; its gradient joins the coefficient vector of ``ssbev_occ_loss_bwd``."""
    return _OccDiceTail.apply(diff, aux, float(smooth))


LGA = os.environ.get("SSBEV_LGA", "1") != "0"                # fused LGA-weighted cross entropy (0 = the tensor form: up-sampled volume + CE + label shifts)


def lga_weights(label):
    """Twice the local geometric anisotropy of ``PositionAwareLoss.get_lga`` for labels [B,X,Y,Z] (255 = ignore), uint8 in 0..12,
    exact.  CUDA labels run ``ssbev_lga_weights``; CPU labels the same rule in tensor ops (``losses.lga_weights_tensor``).  An
    axis shorter than 2 is a ``ValueError`` (``torch.gradient`` raises there too)."""
    if label.dim() != 4 or min(label.shape[1:]) < 2:
        raise ValueError(f"lga_weights: labels [B,X,Y,Z] with every axis >= 2 expected, got {tuple(label.shape)}")
    if not label.is_cuda:
        from .plugin import losses
        return losses.lga_weights_tensor(label)
    lib = capi.load()
    lab = label.to(torch.uint8).contiguous()
    out = torch.empty_like(lab)
    B, X, Y, Z = lab.shape
    with _span("occ_lga", 0.0, 2.0 * lab.numel(), "fwd   lga_weights"):
        capi.check(lib.ssbev_lga_weights(capi.ptr(lab), capi.ptr(out), B, X, Y, Z, capi.stream()), "ssbev_lga_weights")
    return out


def occ_lga_supported(logits, gt_occ):
    """The fused LGA-weighted cross entropy serves fp32 20-class logits on the GPU and a label grid of exactly twice their size."""
    return (logits.is_cuda and logits.dim() == 5 and logits.shape[1] == 20 and logits.dtype == torch.float32
            and gt_occ.dim() == 4 and gt_occ.shape[0] == logits.shape[0]
            and tuple(int(v) for v in gt_occ.shape[1:]) == tuple(2 * int(v) for v in logits.shape[2:]))


class _OccLga(torch.autograd.Function):
    """logits [B,20,D,H,W] (coarse), label uint8 [B,2D,2H,2W], lga2 uint8 (``lga_weights``), class weights [20] -> the
    LGA-weighted cross entropy (0-dim fp32), ``ssbev_occ_lga_fwd / _bwd``.  Forward keeps (num, den) on the device; nothing is read
    back.  No gradient for the class weights (a buffer of the head)."""

    @staticmethod
    def forward(ctx, logits, label_u8, lga2, class_weight, alpha, beta):
        lib = capi.load()
        xcl = to_cl(_f32(logits, "occ_lga_loss"))
        B, D, H, W, Cch = xcl.shape
        d = capi.UpsampleDims(B, D, H, W, Cch)
        dev = logits.device
        lab, lga2 = label_u8.contiguous(), lga2.contiguous()
        cw = class_weight.detach().to(device=dev, dtype=torch.float32).contiguous()
        if cw.numel() != Cch:
            raise capi.SsbevError(f"occ_lga_loss: {Cch} class weights expected, got {cw.numel()}")
        numden = torch.empty(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = _ws(lib.ssbev_occ_lga_workspace(C.byref(d)), dev)
        with _span("occ_lga", 0.0, 4.0 * xcl.numel() + 2.0 * lab.numel(), "fwd   occ_lga"):
            capi.check(lib.ssbev_occ_lga_fwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(lga2), capi.ptr(cw), alpha, beta,
                                             capi.ptr(numden), capi.ptr(loss), C.byref(d), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_occ_lga_fwd")
        ctx.save_for_backward(xcl, lab, lga2, cw, numden)
        ctx.ab = (alpha, beta)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        lib = capi.load()
        xcl, lab, lga2, cw, numden = ctx.saved_tensors
        B, D, H, W, Cch = xcl.shape
        d = capi.UpsampleDims(B, D, H, W, Cch)
        alpha, beta = ctx.ab
        gl = g.to(torch.float32).reshape(1).contiguous()
        gx = torch.empty_like(xcl)
        ws = _ws(lib.ssbev_occ_lga_bwd_workspace(C.byref(d)), xcl.device)
        with _span("occ_lga", 0.0, 8.0 * xcl.numel() + 2.0 * lab.numel() + 8.0 * 20 * lab.numel(), "bwd   occ_lga"):
            capi.check(lib.ssbev_occ_lga_bwd(capi.ptr(xcl), capi.ptr(lab), capi.ptr(lga2), capi.ptr(cw), alpha, beta,
                                             capi.ptr(numden), capi.ptr(gl), capi.ptr(gx), C.byref(d), capi.ptr(ws), ws.numel(),
                                             capi.stream()), "ssbev_occ_lga_bwd")
        return from_cl(gx), None, None, None, None, None


def occ_lga_loss(logits, gt_occ, class_weights, alpha=1.0, beta=1.0):
    """LGA-weighted cross entropy (PositionAwareLoss) of ``up(logits)`` against ``gt_occ`` (255 = ignore): the sum over the labelled
    voxels of w[t] (alpha + beta lga) (-log p_t) over the sum of w[t]; 0 with a zero gradient when nothing is labelled; fp32, 0-dim.
    Supported inputs (``occ_lga_supported``) with ``LGA`` on run on the fused HIP path; anything else on the tensor form of
    plugin/losses.py after ``upsample_trilinear``."""
    label_u8 = gt_occ.to(torch.uint8)
    if LGA and occ_lga_supported(logits, label_u8):
        return _OccLga.apply(logits, label_u8, lga_weights(label_u8), class_weights, float(alpha), float(beta))
    from .plugin import losses
    if not LGA and logits.is_cuda:
        up = upsample_trilinear(logits, label_u8.shape[-3:])
        return losses.pal_tensor(up, label_u8, class_weights.to(up), alpha, beta).float()
    return losses.occ_lga_loss(logits, label_u8, class_weights, alpha, beta).float()


# -------------------------------------------------------------------------------------------------
# Image branch: depthwise conv with "same" padding, Swish, squeeze-excitation pieces
# -------------------------------------------------------------------------------------------------

def same_padding(size, k, stride):
    """mmcv Conv2dAdaptivePadding (the conv_cfg of CustomEfficientNet, efficientnet.py:373): output = ceil(size/stride),
    total padding max((out-1)*stride + k - size, 0), the odd element goes to the bottom/right.  Returns (out, before, after)."""
    out = -(-size // stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2, total - total // 2


def linear_cl(x, weight, bias=None):
    """1x1 / stride-1 convolution of a channels-last map as the plain GEMM it is -- [pixels, Cin] x [Cin, Cout] on the
    channels-last buffer, no layout change -- on the own GEMM kernels (csrc/gemm.hip: forward, data and weight gradient) whenever
    Cout % 4 == 0, else on the library through autograd's mm.
    Used by the image branch, whose pointwise convs range from 2 rows (SE gates) to 245 k rows x 32..3840 channels."""
    xcl = to_cl(_f32(x, "linear_cl"))
    shp = xcl.shape
    w2 = weight.reshape(weight.shape[0], -1)
    x2 = xcl.reshape(-1, shp[-1])
    if own_gemm_site("linear") and x2.is_cuda and w2.shape[0] % 4 == 0:
        y = small_linear(x2, w2, bias)                 # (any row count; Cin zero-padded to a multiple of 4 when it is not one)
        return from_cl(y.view(*shp[:-1], w2.shape[0]))
    fl = 2.0 * x2.shape[0] * x2.shape[1] * w2.shape[0]
    nby = 4.0 * (x2.numel() + w2.numel() + x2.shape[0] * w2.shape[0])
    mult = 3.0 if (torch.is_grad_enabled() and (x.requires_grad or weight.requires_grad)) else 1.0
    with _span("gemm_lib", fl * mult, nby * mult, f"fwd   linear_cl {x2.shape[1]}->{w2.shape[0]} rows={x2.shape[0]}"):
        y = torch.addmm(bias, x2, w2.t()) if bias is not None else torch.mm(x2, w2.t())
    return from_cl(y.view(*shp[:-1], w2.shape[0]))


def small_linear(x2, weight2, bias=None):
    """nn.functional.linear for the few-row products of the path (camera MLPs, squeeze-excite gates, CA3D's channel MLP:
    [B, K] x [N, K]^T): on the own GEMM kernels (N a multiple of 4; K is zero-padded to one), so that no rocBLAS kernel is launched
    for them either."""
    if x2.is_cuda and x2.dtype != torch.float32:
        x2 = x2.float()              # (a bf16 pooled vector in the storage mode: the few-row products stay fp32, like their weights)
    if (x2.is_cuda and x2.dim() == 2 and own_gemm_site("linear") and weight2.shape[0] % 4 == 0
            and weight2.shape[1] == x2.shape[1]):
        pad = -x2.shape[1] % 4
        if pad:                      # (the 27-feature camera vector: zero columns on both operands, 16-byte rows)
            x2, weight2 = torch.nn.functional.pad(x2, (0, pad)), torch.nn.functional.pad(weight2, (0, pad))
        return _LinearCL.apply(x2.contiguous(), weight2.contiguous(), bias)
    fl = 2.0 * x2.shape[0] * x2.shape[-1] * weight2.shape[0]
    with _span("gemm_lib", fl, 4.0 * (x2.numel() + weight2.numel()), f"fwd   linear (library) {x2.shape[-1]}->{weight2.shape[0]} rows={x2.shape[0]}"):
        return torch.nn.functional.linear(x2, weight2, bias)


class _DwConv2d(torch.autograd.Function):
    """Depthwise k x k conv (groups = channels), TF-"same" padding; x logical [B,C,H,W], weight [C,1,k,k]."""

    @staticmethod
    def forward(ctx, x, weight, stride):
        xcl = to_cl(_f32(x, "dwconv2d"))
        B, H, W, Cc = xcl.shape
        k = weight.shape[-1]
        Ho, pt, _ = same_padding(H, k, stride)
        Wo, pl, _ = same_padding(W, k, stride)
        d = capi.DwDims(B, Cc, H, W, Ho, Wo, k, stride, pt, pl)
        wt = weight.detach().reshape(Cc, k * k).t().contiguous()
        y = torch.empty(B, Ho, Wo, Cc, dtype=torch.float32, device=x.device)
        lib = capi.load()
        with _span("dwconv", 2.0 * y.numel() * k * k, 4.0 * (xcl.numel() + y.numel()), f"dw fwd C={Cc} {H}x{W} k{k} s{stride}"):
            capi.check(lib.ssbev_dwconv2d_fwd(capi.ptr(xcl), capi.ptr(wt), capi.ptr(y), C.byref(d), capi.stream()),
                       "ssbev_dwconv2d_fwd")
        ctx.save_for_backward(xcl, wt)
        ctx.d = d
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        xcl, wt = ctx.saved_tensors
        d = ctx.d
        gcl = to_cl(gy)
        lib = capi.load()
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gxcl = torch.empty_like(xcl)
            with _span("dwconv", 2.0 * gcl.numel() * d.k * d.k, 4.0 * (xcl.numel() + gcl.numel()), f"dw dgrad C={d.C} k{d.k} s{d.stride}"):
                capi.check(lib.ssbev_dwconv2d_bwd_data(capi.ptr(gcl), capi.ptr(wt), capi.ptr(gxcl), C.byref(d), capi.stream()),
                           "ssbev_dwconv2d_bwd_data")
            gx = from_cl(gxcl)
        if ctx.needs_input_grad[1]:
            n = lib.ssbev_dwconv2d_bwd_weight_workspace(C.byref(d))
            ws = torch.empty(max(n, 4), dtype=torch.float32, device=gy.device)
            gwt = torch.empty_like(wt)
            with _span("dwconv", 2.0 * gcl.numel() * d.k * d.k, 4.0 * (xcl.numel() + gcl.numel()), f"dw wgrad C={d.C} k{d.k} s{d.stride}"):
                capi.check(lib.ssbev_dwconv2d_bwd_weight(capi.ptr(xcl), capi.ptr(gcl), capi.ptr(gwt), C.byref(d), capi.ptr(ws),
                                                         ws.numel(), capi.stream()), "ssbev_dwconv2d_bwd_weight")
            gw = gwt.t().reshape(d.C, 1, d.k, d.k).contiguous()
        return gx, gw, None


def depthwise_conv2d_same(x, weight, stride=1):
    return _DwConv2d.apply(x, weight, int(stride))


class _Swish(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        x = _f32(x, "swish")
        ctx.cl = x.dim() >= 3
        xc = to_cl(x) if ctx.cl else x.contiguous()       # no copy for the channels-last activations of the branch
        n = xc.numel()
        ctx.torch_path = n % 4 != 0
        ctx.save_for_backward(xc)
        if ctx.torch_path:
            y = xc * torch.sigmoid(xc)
        else:
            y = torch.empty_like(xc)
            capi.check(capi.load().ssbev_swish_fwd(capi.ptr(xc), capi.ptr(y), n, capi.stream()), "ssbev_swish_fwd")
        return from_cl(y) if ctx.cl else y

    @staticmethod
    def backward(ctx, gy):
        (xc,) = ctx.saved_tensors
        g = to_cl(gy) if ctx.cl else gy.contiguous()
        if ctx.torch_path:
            s = torch.sigmoid(xc)
            gx = g * (s + xc * s * (1 - s))
        else:
            gx = torch.empty_like(xc)
            capi.check(capi.load().ssbev_swish_bwd(capi.ptr(xc), capi.ptr(g), capi.ptr(gx), xc.numel(), capi.stream()),
                       "ssbev_swish_bwd")
        return from_cl(gx) if ctx.cl else gx


def swish(x):
    """mmcv ``Swish``: x * sigmoid(x)."""
    return _Swish.apply(x)


def _chan_sum(a, bmul, B, S, Cc, scale):
    lib = capi.load()
    out = torch.empty(B, Cc, dtype=torch.float32, device=a.device)
    ws = torch.empty(max(lib.ssbev_chan_sum_workspace(B, S, Cc), 4), dtype=torch.float32, device=a.device)
    capi.check(lib.ssbev_chan_sum(capi.ptr(a), capi.ptr(bmul), capi.ptr(out), B, S, Cc, float(scale), capi.ptr(ws),
                                  ws.numel(), capi.stream()), "ssbev_chan_sum")
    return out


class _GlobalAvgPool(torch.autograd.Function):
    """nn.AdaptiveAvgPool2d(1) of mmdet's SELayer: logical [B,C,H,W] -> [B,C,1,1]."""

    @staticmethod
    def forward(ctx, x):
        xcl = to_cl(_f32(x, "global_avg_pool"))
        B, H, W, Cc = xcl.shape
        ctx.shape = (B, H, W, Cc)
        return _chan_sum(xcl, None, B, H * W, Cc, 1.0 / (H * W)).view(B, Cc, 1, 1)

    @staticmethod
    def backward(ctx, g):
        B, H, W, Cc = ctx.shape
        gx = torch.empty(B, H, W, Cc, dtype=torch.float32, device=g.device)
        capi.check(capi.load().ssbev_chan_scale(None, capi.ptr(g.reshape(B, Cc).contiguous()), capi.ptr(gx), B, H * W, Cc,
                                                1.0 / (H * W), capi.stream()), "ssbev_chan_scale")
        return from_cl(gx)


class _ChanScale(torch.autograd.Function):
    """x * gate with gate [B,C,1,1] (the SE rescale, mmdet SELayer.forward)."""

    @staticmethod
    def forward(ctx, x, gate):
        xcl = to_cl(_f32(x, "chan_scale"))
        B, H, W, Cc = xcl.shape
        gt = gate.reshape(B, Cc).contiguous()
        y = torch.empty_like(xcl)
        capi.check(capi.load().ssbev_chan_scale(capi.ptr(xcl), capi.ptr(gt), capi.ptr(y), B, H * W, Cc, 1.0, capi.stream()),
                   "ssbev_chan_scale")
        ctx.save_for_backward(xcl, gt)
        return from_cl(y)

    @staticmethod
    def backward(ctx, gy):
        xcl, gt = ctx.saved_tensors
        B, H, W, Cc = xcl.shape
        gcl = to_cl(gy)
        gx = ggate = None
        if ctx.needs_input_grad[0]:
            gxcl = torch.empty_like(xcl)
            capi.check(capi.load().ssbev_chan_scale(capi.ptr(gcl), capi.ptr(gt), capi.ptr(gxcl), B, H * W, Cc, 1.0,
                                                    capi.stream()), "ssbev_chan_scale")
            gx = from_cl(gxcl)
        if ctx.needs_input_grad[1]:
            ggate = _chan_sum(gcl, xcl, B, H * W, Cc, 1.0).view(B, Cc, 1, 1)
        return gx, ggate


def global_avg_pool(x):
    return _GlobalAvgPool.apply(x)


def chan_scale(x, gate):
    return _ChanScale.apply(x, gate)
