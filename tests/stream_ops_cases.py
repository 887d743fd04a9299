"""The shapes of test_gpu_stream_ops.py and what each of them reaches in csrc/image_ops.hip, csrc/softmax.hip and csrc/trilinear.hip.

The streaming operators take different paths with the geometry of a launch.  The mirrors below restate the launch arithmetic in
plain Python; every constant in them is read from the .hip source by hand:

  image_ops.hip
    dw_layout            `*Q = quads <= 256 ? quads : 64`  -> DW_Q_ALL = 256 (C <= 1024), DW_Q_WIDE = 64; `*L = 256 / *Q` -> NT = 256
    dw_chunks            `2048L / qblocks` -> DW_WANT = 2048 workgroups; `std::max(64L, ...)` -> CHUNK_FLOOR = 64 pixels
    dw_reduce_kernel,    `for (int ch = lane; ch < nchunks; ch += 64)` -> FOLD_LANES = 64 chunk slabs per trip of a wave
    chan_fold_kernel
    chan_sum_kernel      `blockIdx.x * 64 + ql` -> CHAN_Q = 64 quads per workgroup; `s += 4` -> CHAN_LANES = 4 pixel lanes
    chan_chunks          `1024L / blocks` -> CHAN_WANT = 1024; `std::max(64L, ...)` -> CHUNK_FLOOR = 64
    stream_blocks        `std::min<long>((n4 + 255) / 256, 256L * 32)` -> STREAM_CAP = 8192 workgroups of NT threads
  softmax.hip
    axis_slices          `C >= 64 && inner >= 32 ? 8 : 1` -> SM_MIN_C = 64, SM_MIN_INNER = 32, SM_SLICES = 8
    softmax_axis_*       `COLS = 256 / SL`; slice sl walks `C * sl / SL .. C * (sl + 1) / SL`
  trilinear.hip
    ssbev_trilinear2x_*  one thread per channel quad of the output (forward) / input (backward), workgroups of NT

The library answers for the numbers only it knows: ssbev_dwconv2d_bwd_weight_layout (Q, L, qblocks), ssbev_stream_blocks,
ssbev_softmax_axis_slices, and the chunk counts through ssbev_dwconv2d_bwd_weight_workspace / ssbev_chan_sum_workspace;
test_stream_ops_plan.py holds the mirrors to those answers and to each case's hand-written `expect` on a box without a GPU, and
test_gpu_stream_ops.py runs the cases against a float64 reference."""
from collections import namedtuple

NT = 256               # threads of every workgroup here
DW_Q_ALL = 256         # channel quads up to which one workgroup of the depthwise weight gradient takes all of them (C <= 1024)
DW_Q_WIDE = 64         # quads per workgroup above that
DW_WANT = 2048         # workgroups a depthwise weight-gradient launch aims at
CHAN_Q = 64            # quads per workgroup of chan_sum_kernel
CHAN_LANES = 4         # its pixel lanes
CHAN_WANT = 1024       # workgroups a chan_sum launch aims at
CHUNK_FLOOR = 64       # pixels a chunk never goes below (both reductions)
FOLD_LANES = 64        # chunk slabs a wave of the fold kernels takes per trip
STREAM_CAP = 8192      # workgroups of a grid-stride pass
SM_MIN_C, SM_MIN_INNER, SM_SLICES = 64, 32, 8


def cdiv(a, b):
    return -(-a // b)


# ---- mirrors of the launch arithmetic ---------------------------------------------------------------------------------------------
def same_padding(size, k, stride):
    """(out, before, after): out = ceil(size / stride), the odd element of padding after."""
    out = cdiv(size, stride)
    total = max((out - 1) * stride + k - size, 0)
    return out, total // 2, total - total // 2


def dw_layout(Cch):
    """dw_layout -> Q quads x L pixel lanes per workgroup, qblocks workgroups over the channels."""
    quads = Cch // 4
    Q = quads if quads <= DW_Q_ALL else DW_Q_WIDE
    return dict(Q=Q, L=NT // Q, qblocks=cdiv(quads, Q))


def dw_chunks(npix, qblocks):
    """dw_chunks -> pixels per chunk, chunks, pixels of the last chunk."""
    want = max(1, DW_WANT // qblocks)
    per = max(CHUNK_FLOOR, cdiv(npix, want))
    n = cdiv(npix, per)
    return dict(ppc=per, nchunks=n, last_chunk=npix - (n - 1) * per)


def chan_chunks(B, S, Cch):
    """chan_chunks -> pixels per chunk, chunks, pixels of the last chunk."""
    blocks = B * cdiv(Cch // 4, CHAN_Q)
    want = max(1, CHAN_WANT // blocks)
    per = max(CHUNK_FLOOR, cdiv(S, want))
    n = cdiv(S, per)
    return dict(per=per, nchunks=n, last_chunk=S - (n - 1) * per)


def stream_blocks(n4):
    """stream_blocks -> workgroups, grid-stride trips, quads taken on the second trip."""
    blocks = min(cdiv(n4, NT), STREAM_CAP)
    stride = blocks * NT
    return dict(blocks=blocks, trips=cdiv(n4, stride), trip2=max(0, min(n4 - stride, stride)))


def softmax_plan(outer, Cn, inner):
    """The instance the launchers pick and what its last workgroup and its slices look like."""
    SL = SM_SLICES if Cn >= SM_MIN_C and inner >= SM_MIN_INNER else 1
    cols = NT // SL
    ncol = outer * inner
    blocks = cdiv(ncol, cols)
    lens = [Cn * (sl + 1) // SL - Cn * sl // SL for sl in range(SL)]
    return dict(SL=SL, blocks=blocks, last_cols=ncol - (blocks - 1) * cols, slice_min=min(lens), slice_max=max(lens))


def softmax_view(shape, dim):
    """(outer, C, inner) of softmax over `dim` of a contiguous tensor."""
    outer = 1
    for n in shape[:dim]:
        outer *= n
    inner = 1
    for n in shape[dim + 1:]:
        inner *= n
    return outer, shape[dim], inner


def fold_trips(nchunks):
    """Trips of a lane of dw_reduce_kernel / chan_fold_kernel over the chunk slabs."""
    return cdiv(nchunks, FOLD_LANES)


def clipped_taps(c):
    """Taps (a, e) of a depthwise case that fall outside the input at one output pixel at least.  (The centre tap of a "same"
    padded odd kernel never does: pad_before <= (k - 1) / 2 <= pad_before + what the last output needs.)"""
    Ho, pt, _ = same_padding(c.Hi, c.k, c.s)
    Wo, pl, _ = same_padding(c.Wi, c.k, c.s)
    rows = {a for a in range(c.k) for ho in range(Ho) if not 0 <= ho * c.s - pt + a < c.Hi}
    cols = {e for e in range(c.k) for wo in range(Wo) if not 0 <= wo * c.s - pl + e < c.Wi}
    return sum(1 for a in range(c.k) for e in range(c.k) if a in rows or e in cols)


# ---- depthwise convolution: (B, C, Hi, Wi, k, s) ---------------------------------------------------------------------------------
# expectations, by hand from the code:
#   Q, L, qblocks, active, last_quads   thread layout of dw_bwd_weight_kernel, threads with work, quads of the last quad block
#   ppc, nchunks, last_chunk            pixel chunks of the weight gradient
#   out, pad_h, pad_w                   (Ho, Wo), (top, bottom), (left, right)
#   fwd_quads, dgrad_quads              threads with work in dw_fwd_kernel / dw_bwd_data_kernel
DwCase = namedtuple("DwCase", "id B C Hi Wi k s expect")
DW_CASES = [
    # wide layout: 6 quad blocks, the last with 16 quads; 2 chunks, the second of 6 pixels
    DwCase("W1", 2, 1344, 5, 7, 5, 1,
           dict(Q=64, L=4, qblocks=6, active=256, last_quads=16, ppc=64, nchunks=2, last_chunk=6, out=(5, 7), pad_h=(2, 2),
                pad_w=(2, 2), fwd_quads=23520, dgrad_quads=23520)),
    # 5 quad blocks, the last with one quad; stride 2 on odd H; the one chunk is exactly L pixels
    DwCase("W2", 1, 1028, 3, 4, 3, 2,
           dict(Q=64, L=4, qblocks=5, active=256, last_quads=1, ppc=64, nchunks=1, last_chunk=4, out=(2, 2), pad_h=(1, 1),
                pad_w=(0, 1), fwd_quads=1028, dgrad_quads=3084)),
    # the boundary C = 1024: every thread a quad, one pixel lane
    DwCase("W3", 1, 1024, 4, 4, 3, 1,
           dict(Q=256, L=1, qblocks=1, active=256, last_quads=256, ppc=64, nchunks=1, last_chunk=16, out=(4, 4), pad_h=(1, 1),
                pad_w=(1, 1), fwd_quads=4096, dgrad_quads=4096)),
    # 128 pixel lanes over 64-pixel chunks (half the lanes idle), 68 chunks: a second trip of the reduce lanes; last chunk of 2
    DwCase("W4", 1, 8, 66, 65, 3, 1,
           dict(Q=2, L=128, qblocks=1, active=256, last_quads=2, ppc=64, nchunks=68, last_chunk=2, out=(66, 65), pad_h=(1, 1),
                pad_w=(1, 1), fwd_quads=8580, dgrad_quads=8580)),
    # Q = 5: 255 active threads; even W with k = 5, s = 2: the odd padding column on the right; totals no multiple of 256
    DwCase("W5", 1, 20, 9, 6, 5, 2,
           dict(Q=5, L=51, qblocks=1, active=255, last_quads=5, ppc=64, nchunks=1, last_chunk=15, out=(5, 3), pad_h=(2, 2),
                pad_w=(1, 2), fwd_quads=75, dgrad_quads=270)),
    # a map smaller than the kernel: every tap but the centre is clipped at some output pixel (stride 2 has one output column,
    # which keeps the two taps of the centre row that lie on the map)
    DwCase("W6-s1", 2, 12, 1, 2, 5, 1,
           dict(Q=3, L=85, qblocks=1, active=255, last_quads=3, ppc=64, nchunks=1, last_chunk=4, out=(1, 2), pad_h=(2, 2),
                pad_w=(2, 2), fwd_quads=12, dgrad_quads=12)),
    DwCase("W6-s2", 2, 12, 1, 2, 5, 2,
           dict(Q=3, L=85, qblocks=1, active=255, last_quads=3, ppc=64, nchunks=1, last_chunk=2, out=(1, 1), pad_h=(2, 2),
                pad_w=(1, 2), fwd_quads=6, dgrad_quads=12)),
]


def dw_properties(c):
    """What `expect` lists, from the mirrors."""
    Ho, pt, pb = same_padding(c.Hi, c.k, c.s)
    Wo, pl, pr = same_padding(c.Wi, c.k, c.s)
    lay = dw_layout(c.C)
    quads = c.C // 4
    p = dict(lay, active=lay["Q"] * lay["L"], last_quads=quads - (lay["qblocks"] - 1) * lay["Q"])
    p.update(dw_chunks(c.B * Ho * Wo, lay["qblocks"]))
    p.update(out=(Ho, Wo), pad_h=(pt, pb), pad_w=(pl, pr), fwd_quads=c.B * Ho * Wo * quads, dgrad_quads=c.B * c.Hi * c.Wi * quads)
    return p


# ---- squeeze-excitation pieces: (B, C, H, W) --------------------------------------------------------------------------------------
#   qblocks, last_quads                 quad blocks of chan_sum_kernel (blockIdx.x), quads of the last
#   per, nchunks, last_chunk            pixel chunks (blockIdx.z); fold_trips: trips of a chan_fold_kernel lane over them
#   scale_trips, scale_trip2            grid-stride trips of chan_scale_kernel and the quads on the second
SeCase = namedtuple("SeCase", "id B C H W expect")
SE_CASES = [
    # two quad blocks, the second with one quad; 3 chunks, the last of 2 pixels, with B = 3: the [chunk][B][C] slab index
    SeCase("S1", 3, 260, 10, 13, dict(qblocks=2, last_quads=1, per=64, nchunks=3, last_chunk=2, fold_trips=1, scale_trips=1,
                                      scale_trip2=0)),
    # 68 chunks: a second trip of the fold lanes
    SeCase("S2", 1, 4, 66, 65, dict(qblocks=1, last_quads=1, per=64, nchunks=68, last_chunk=2, fold_trips=2, scale_trips=1,
                                    scale_trip2=0)),
    # one pixel
    SeCase("S3", 2, 40, 1, 1, dict(qblocks=1, last_quads=10, per=64, nchunks=1, last_chunk=1, fold_trips=1, scale_trips=1,
                                   scale_trip2=0)),
    # the one large case (8 396 800 floats): the 8192-workgroup cap, 2048 quads on a second trip, all in sample 1; chunks above
    # the 64-pixel floor (512 of 1025 pixels, 8 fold trips)
    SeCase("G1", 2, 8, 1025, 512, dict(qblocks=1, last_quads=2, per=1025, nchunks=512, last_chunk=1025, fold_trips=8,
                                       scale_trips=2, scale_trip2=2048)),
]


def se_properties(c):
    quads, S = c.C // 4, c.H * c.W
    qb = cdiv(quads, CHAN_Q)
    p = dict(qblocks=qb, last_quads=quads - (qb - 1) * CHAN_Q)
    p.update(chan_chunks(c.B, S, c.C))
    p["fold_trips"] = fold_trips(p["nchunks"])
    sb = stream_blocks(c.B * S * quads)
    p.update(scale_trips=sb["trips"], scale_trip2=sb["trip2"])
    return p


# ---- Swish: shape -> workgroups, trips, quads on the second trip (None: n % 4 != 0, the tensor-op route of the wrapper) -----------
SwishCase = namedtuple("SwishCase", "id shape expect")
SWISH_CASES = [
    SwishCase("G1", (2, 8, 1025, 512), dict(blocks=8192, trips=2, trip2=2048)),
    SwishCase("G2", (3, 7), None),
    SwishCase("G3", (2, 12, 5, 7), dict(blocks=1, trips=1, trip2=0)),          # 210 quads: a partial workgroup
]
BIG = "G1"          # the case whose inputs are drawn with one hashed uniform per element instead of four


def numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n


def swish_properties(c):
    n = numel(c.shape)
    return stream_blocks(n // 4) if n % 4 == 0 else None


# ---- softmax along a strided axis: (shape, dim) -----------------------------------------------------------------------------------
#   SL, blocks, last_cols               slices per column, workgroups, columns of the last workgroup
#   slice_min, slice_max                shortest and longest slice of the axis
#   special                             X6: columns given a mask, an offset or a constant (see test_gpu_stream_ops.softmax_input)
#   direct                              X7: through the C entry points only
SmCase = namedtuple("SmCase", "id shape dim expect special direct", defaults=(False, False))
SOFTMAX_CASES = [
    # uneven slices of 8 and 9, outer = 3, inner = 45, a last workgroup of 7 columns
    SmCase("X1", (3, 67, 5, 9), 1, dict(SL=8, blocks=5, last_cols=7, slice_min=8, slice_max=9)),
    # both boundaries, full workgroups
    SmCase("X2", (2, 64, 32), 1, dict(SL=8, blocks=2, last_cols=32, slice_min=8, slice_max=8)),
    # one below the boundary of C: unsliced
    SmCase("X3", (2, 63, 40), 1, dict(SL=1, blocks=1, last_cols=80, slice_min=63, slice_max=63)),
    # one below the boundary of inner: unsliced, with a long walk
    SmCase("X4", (2, 200, 31), 1, dict(SL=1, blocks=1, last_cols=62, slice_min=200, slice_max=200)),
    # the kitti_d112 depth axis: a last workgroup of one column
    SmCase("X5", (1, 1, 112, 3, 11), 2, dict(SL=8, blocks=2, last_cols=1, slice_min=14, slice_max=14)),
    # X1 with a masked column, columns far off either way and a constant one
    SmCase("X6", (3, 67, 5, 9), 1, dict(SL=8, blocks=5, last_cols=7, slice_min=8, slice_max=9), special=True),
    # inner = 1 and an uneven sliced axis with outer = 1
    SmCase("X7-a", (4, 5, 1), 1, dict(SL=1, blocks=1, last_cols=4, slice_min=5, slice_max=5), direct=True),
    SmCase("X7-b", (1, 70, 33), 1, dict(SL=8, blocks=2, last_cols=1, slice_min=8, slice_max=9), direct=True),
]


def softmax_properties(c):
    return softmax_plan(*softmax_view(c.shape, c.dim))


# ---- trilinear x2: (B, C, (D, H, W)) -> quads of the forward and of the backward launch ------------------------------------------
TriCase = namedtuple("TriCase", "id B C sp expect")
TRILINEAR_CASES = [
    TriCase("T1", 1, 8, (1, 1, 1), dict(fwd_quads=16, bwd_quads=2, unit_axes=3)),
    TriCase("T2", 2, 12, (1, 4, 3), dict(fwd_quads=576, bwd_quads=72, unit_axes=1)),
    TriCase("T3", 1, 4, (5, 1, 2), dict(fwd_quads=80, bwd_quads=10, unit_axes=1)),
    TriCase("T4", 3, 4, (3, 3, 3), dict(fwd_quads=648, bwd_quads=81, unit_axes=0)),
]


def trilinear_properties(c):
    vox = c.sp[0] * c.sp[1] * c.sp[2]
    return dict(fwd_quads=c.B * 8 * vox * (c.C // 4), bwd_quads=c.B * vox * (c.C // 4), unit_axes=sum(1 for s in c.sp if s == 1))


def case_id(c):
    return c.id


def by_id(table):
    return {c.id: c for c in table}
