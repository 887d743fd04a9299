"""Case table of the bf16 storage convolutions' path tests (test_conv_bf16_plan.py on the CPU, test_gpu_conv_bf16_paths.py on the GPU).

csrc/conv_bf16.hip serves ssbev_conv_fwd_bf16 (mode 0), ssbev_conv_bwd_data_bf16 (mode 1) and ssbev_conv_bwd_weight_bf16 (mode 2)
with six kernels and about forty template instances.  Each case below is a small ssbev_conv_dims that reaches one instance with
the tails and borders it is listed for; the expected plan is what ``ssbev_conv_bf16_plan_query`` -- the plan functions the
launchers read -- answers, so test_conv_bf16_plan.py notices on a box without a GPU when a threshold moves a case to another
kernel, and the GPU tests cannot lose this coverage quietly.

A case's dims carry precision 2; ``precisions`` names the result types it is run with (2 bf16, 3 fp32: the plan does not depend
on it, which test_conv_bf16_plan.py asserts).  The weight gradient exists for precision 2 only.

The 256 x 32 and 128 x 32 tiles of conv_igemm16_kernel (32 destination channels need SSBEV_IGEMM16_MIN_COUT) and forced stage
depths (SSBEV_IGEMM16_BKC) are reachable in a tuning build only and have no case."""
import collections
import ctypes as C

from stereoscene_amd import capi

FWD, DGRAD, WGRAD = 0, 1, 2
MODE_NAMES = {FWD: "fwd", DGRAD: "dgrad", WGRAD: "wgrad"}
GATHER16, TAP16, WGRAD16, WIDE16, WGRING16, IGEMM16 = 16, 17, 18, 19, 20, 21

# ---- what the product build can reach (the coverage assertions of test_conv_bf16_plan.py enumerate these)
GATHER16_TILINGS = {11, 12, 14, 21, 22, 24, 26}                                    # 10 MT + NT
IGEMM16_TILES = {(bm, bn, bkc) for bm, bn in ((128, 128), (128, 64), (64, 128), (64, 64)) for bkc in (32, 64)}
WIDE16_INSTANCES = {(2, 1), (3, 1), (3, 2), (4, 1), (4, 2)}                         # (ntl, ntn): N = 64; 96, 192; 128, 256
WGRAD16_CONFIGS = {(1, 1, 3, 3), (2, 2, 1, 3), (2, 2, 1, 1), (1, 1, 1, 1)}          # <MQ, MP, TH, TW>
WGRING16_INSTANCES = {0, 1}                                                        # narrow

# ---- property tags: all of them follow from the dims and the plan (plan_props below recomputes them from the query)
RAGGED_M = "ragged_m_tile"             # 16 / 21: the voxels (of a parity class) are no multiple of the workgroup's rows
COUT_TAIL = "cout_tail"                # 16 / 21: the destination channels are no multiple of the tile's columns
COUT_PAD = "cout_pad"                  # 16 / 21: the packed weights are padded past the destination channels (CoutPad > Cout)
PARITY = "parity_classes"              # 16 / 21: transposed gather with more than one parity class
NCHUNKS_MOD4 = "nchunks_mod4"          # 18: the last workgroup has idle waves (nchunks % 4 != 0)
SHORT_VOXEL_CHUNK = "short_voxel_chunk"  # 18: the last voxel chunk is shorter than the others
RAGGED_TAP = "ragged_tap_tile"         # 18: kh or kw is no multiple of the tap tile (kw = 2 or 4 under TW = 3)
CQ_TAIL = "cq_tail"                    # 18: Cq is no multiple of 32 MQ
CP_TAIL = "cp_tail"                    # 18: Cp is no multiple of 32 MP
SHORT_TILE_CHUNK = "short_tile_chunk"  # 20: the last chunk of tiles is shorter than tpc
RAGGED_H = "ragged_h"                  # 19: H % 16 != 0; 20: H % 8 != 0
D1, D2 = "d1", "d2"                    # 19: one / two depth planes (both outer planes of the three-plane ring are border)
NCQT_RAGGED = "ncqt_ragged"            # 20 wide: the last 32-channel Q tile is ragged
CP_RAGGED = "cp_ragged"                # 20 wide: the last group of four 32-channel P tiles is ragged
BATCH2 = "batch2"                      # B = 2
ALL_PROPS = {RAGGED_M, COUT_TAIL, COUT_PAD, PARITY, NCHUNKS_MOD4, SHORT_VOXEL_CHUNK, RAGGED_TAP, CQ_TAIL, CP_TAIL, SHORT_TILE_CHUNK,
             RAGGED_H, D1, D2, NCQT_RAGGED, CP_RAGGED, BATCH2}

FIELDS = tuple(n for n, _ in capi.ConvDims._fields_)
Case = collections.namedtuple("Case", "name dims mode precisions plan props")
# plan: (16, mt, nt) | (17, nseg, gpc) | (18, mq, mp, th, tw, chunk, nchunks) | (19, ntl, nth, ntw, ntn) |
#       (20, narrow, tpc, nchunks, ncqt) | (21, bm, bn, bkc)


def case_id(c):
    return f"{c.name}-{MODE_NAMES[c.mode]}"


def _t3(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v, v)


def conv(B, cin, cout, size, k, s=1, p=0, dil=1, hint=0, transposed=False, op=0):
    """The 26 ints of ssbev_conv_dims (precision 2) of a convolution over the input grid size = (D, H, W); a 2-D layer has D = 1
    and k = (1, kh, kw).  Transposed: output extent (i - 1) s - 2 p + dil (k - 1) + op + 1."""
    k, s, p, dil, op = _t3(k), _t3(s), _t3(p), _t3(dil), _t3(op)
    if transposed:
        out = tuple((i - 1) * st - 2 * pd + dl * (kk - 1) + o + 1 for i, kk, st, pd, dl, o in zip(size, k, s, p, dil, op))
    else:
        out = tuple((i + 2 * pd - dl * (kk - 1) - 1) // st + 1 for i, kk, st, pd, dl in zip(size, k, s, p, dil))
    return (B, cin, cout) + tuple(size) + out + k + s + p + dil + (int(transposed), 0, 0, hint, 2)


def dims_of(case, precision=2, relu=0, accumulate=0, B=None):
    d = capi.ConvDims(*case.dims)
    d.precision, d.relu, d.accumulate = precision, relu, accumulate
    if B is not None:
        d.B = B
    return d


def query(d, mode):
    """ssbev_conv_bf16_plan of dims d, or the error code."""
    p = capi.ConvBf16Plan()
    rc = capi.load().ssbev_conv_bf16_plan_query(C.byref(d), mode, C.byref(p))
    return p if rc == capi.OK else rc


PLAN_FIELDS = tuple(n for n, _ in capi.ConvBf16Plan._fields_)
GROUPS = {GATHER16: ("mt", "nt"), TAP16: ("nseg", "gpc"), WGRAD16: ("mq", "mp", "th", "tw", "chunk", "nchunks"),
          WIDE16: ("ntl", "nth", "ntw", "ntn"), WGRING16: ("narrow", "tpc", "nchunks", "ncqt"), IGEMM16: ("bm", "bn", "bkc")}


def plan_tuple(p):
    """The group of the plan's kernel class, in the order of Case.plan."""
    return (p.kernel,) + tuple(getattr(p, n) for n in GROUPS[p.kernel])


def full_tuple(p):
    return tuple(getattr(p, n) for n in PLAN_FIELDS)


def _cdiv(a, b):
    return -(-a // b)


def gather_geom(d, mode):
    """(K, N, form, classes, rows of the largest parity class, out grid) of the gather a forward / data-gradient call runs."""
    fwd = mode == FWD
    K, N = (d.Cin, d.Cout) if fwd else (d.Cout, d.Cin)
    out = (d.Do, d.Ho, d.Wo) if fwd else (d.Di, d.Hi, d.Wi)
    form = int(bool(d.transposed) == fwd)
    st = (d.sd, d.sh, d.sw) if form == 1 else (1, 1, 1)
    classes = st[0] * st[1] * st[2]
    rows = d.B * _cdiv(out[0], st[0]) * _cdiv(out[1], st[1]) * _cdiv(out[2], st[2])
    return K, N, form, classes, rows, out


def expected_grid(d, mode, p):
    """Workgroups of the launch, from the kernels' own tile sizes (not from the library)."""
    if p.kernel in (GATHER16, IGEMM16):
        K, N, form, classes, rows, out = gather_geom(d, mode)
        bm, bn = (128 * p.mt, 32 * p.nt) if p.kernel == GATHER16 else (p.bm, p.bn)
        return _cdiv(rows, bm) * _cdiv(N, bn) * classes
    if p.kernel == TAP16:
        return _cdiv(d.B * d.Do * d.Ho, p.gpc) * p.nseg
    if p.kernel == WIDE16:
        return d.B * d.Do * p.nth * p.ntw * p.ntn
    if p.kernel == WGRAD16:
        cp, cq = (d.Cin, d.Cout) if d.transposed else (d.Cout, d.Cin)
        return _cdiv(p.nchunks, 4) * _cdiv(cq, 32 * p.mq) * _cdiv(cp, 32 * p.mp) * d.kd * _cdiv(d.kh, p.th) * _cdiv(d.kw, p.tw)
    return p.nchunks if p.narrow else p.nchunks * p.ncqt * _cdiv(d.Cout, 128) * 3


def expected_workspace(d, mode, p):
    if mode != WGRAD:
        return 0
    return p.nchunks * d.kd * d.kh * d.kw * d.Cin * d.Cout * 4


def plan_props(d, mode, p):
    """The property tags a launch of dims d with plan p has, from the definitions in words."""
    props = set()
    if d.B == 2:
        props.add(BATCH2)
    if p.kernel in (GATHER16, IGEMM16):
        K, N, form, classes, rows, out = gather_geom(d, mode)
        bm, bn = (128 * p.mt, 32 * p.nt) if p.kernel == GATHER16 else (p.bm, p.bn)
        if rows % bm:
            props.add(RAGGED_M)
        if N % bn:
            props.add(COUT_TAIL)
        if N % 32:
            props.add(COUT_PAD)
        if form == 1 and classes > 1:
            props.add(PARITY)
    elif p.kernel == WIDE16:
        if d.Ho % 16:
            props.add(RAGGED_H)
        if d.Do in (1, 2):
            props.add(D1 if d.Do == 1 else D2)
    elif p.kernel == WGRAD16:
        cp, cq = (d.Cin, d.Cout) if d.transposed else (d.Cout, d.Cin)
        small = (d.Di, d.Hi, d.Wi) if d.transposed else (d.Do, d.Ho, d.Wo)
        M = d.B * small[0] * small[1] * small[2]
        if p.nchunks % 4:
            props.add(NCHUNKS_MOD4)
        if M % p.chunk:
            props.add(SHORT_VOXEL_CHUNK)
        if d.kh % p.th or d.kw % p.tw:
            props.add(RAGGED_TAP)
        if cq % (32 * p.mq):
            props.add(CQ_TAIL)
        if cp % (32 * p.mp):
            props.add(CP_TAIL)
    elif p.kernel == WGRING16:
        ntiles = d.B * d.Do * _cdiv(d.Ho, 8) * (d.Wo // 16)
        if ntiles % p.tpc:
            props.add(SHORT_TILE_CHUNK)
        if d.Ho % 8:
            props.add(RAGGED_H)
        if not p.narrow and d.Cin % 32:
            props.add(NCQT_RAGGED)
        if not p.narrow and d.Cout % 128:
            props.add(CP_RAGGED)
    return props


def flops(d):
    """Multiply-adds x 2 of the operator (the float64 reference costs this much, once per operand pair)."""
    small = (d.Di, d.Hi, d.Wi) if d.transposed else (d.Do, d.Ho, d.Wo)
    return 2 * d.B * small[0] * small[1] * small[2] * d.Cin * d.Cout * d.kd * d.kh * d.kw


def _c(name, dims, modes, plans, props, precisions=None):
    out = []
    for mode, plan, pr in zip(modes, plans, props):
        out.append(Case(name, dims, mode, precisions or ((2,) if mode == WGRAD else (2, 3)), plan, frozenset(pr)))
    return out


_TAILS = {BATCH2, COUT_PAD, COUT_TAIL, RAGGED_M}
_H = (11, 12, 14, 21, 22, 24, 26)
_W18 = {BATCH2, CP_TAIL, CQ_TAIL, NCHUNKS_MOD4, SHORT_VOXEL_CHUNK}

CASES = tuple(
    # ------------------------------------------------------------------------------------------------ conv_gather16_kernel
    # 24 -> 40 on 3 x 5 x 20, B = 2 (600 voxels: ragged under every row tile; 40 channels: a column tail under every column tile,
    # weights padded to 64) under each tiling: form 0 forward, form 1 (one class) as the data gradient
    sum((_c(f"g16-24to40-h{h}", conv(2, 24, 40, (3, 5, 20), 3, 1, 1, hint=h), (FWD, DGRAD), [(16, h // 10, h % 10)] * 2, [_TAILS] * 2)
         for h in _H), [])
    # stride 2 with odd extents 5 x 7 x 9 -> 3 x 4 x 5: the data gradient walks eight parity classes of different sizes
    + sum((_c(f"g16-s2-32to64-h{h}", conv(2, 32, 64, (5, 7, 9), 3, 2, 1, hint=h), (FWD, DGRAD), [(16, h // 10, h % 10)] * 2,
              [{BATCH2, RAGGED_M} | ({COUT_TAIL} if h % 10 > 2 else set()),
               {BATCH2, RAGGED_M, PARITY} | ({COUT_TAIL} if h % 10 > 1 else set())]) for h in _H), [])
    # ... and what the heuristic picks on small grids
    + _c("g16-s2-32to64", conv(2, 32, 64, (5, 7, 9), 3, 2, 1), (FWD, DGRAD), [(16, 1, 2), (16, 1, 1)],
         [{BATCH2, RAGGED_M}, {BATCH2, RAGGED_M, PARITY}])
    + _c("g16-24to40", conv(2, 24, 40, (3, 5, 20), 3, 1, 1), (FWD, DGRAD), [(16, 1, 2), (16, 1, 1)], [_TAILS] * 2)
    + _c("g16-deconv-64to32", conv(2, 64, 32, (4, 4, 8), 3, 2, 1, transposed=True, op=1), (FWD, DGRAD), [(16, 1, 1), (16, 1, 2)],
         [{BATCH2, PARITY}, {BATCH2}])
    + _c("g16-2d-dil-64to48", conv(2, 64, 48, (1, 12, 20), (1, 3, 3), 1, (0, 2, 2), (1, 2, 2)), (FWD, DGRAD), [(16, 1, 2)] * 2,
         [_TAILS, {BATCH2, RAGGED_M}])
    # ------------------------------------------------------------------------------------------------ conv_igemm16_kernel
    # 64 x 64: the shapes of test_conv_igemm16_is_bit_identical_to_the_gather_kernel (the third with a ragged last row tile)
    + _c("ig16-s2-64to128", conv(2, 64, 128, (16, 16, 32), 3, 2, 1), (FWD, DGRAD), [(21, 64, 64, 64)] * 2, [{BATCH2}, {BATCH2, PARITY}])
    + _c("ig16-deconv-128to64", conv(2, 128, 64, (8, 8, 16), 3, 2, 1, transposed=True, op=1), (FWD, DGRAD), [(21, 64, 64, 64)] * 2,
         [{BATCH2, PARITY}, {BATCH2}])
    + _c("ig16-96to64", conv(2, 96, 64, (4, 15, 41), 3, 1, 1), (FWD, DGRAD), [(21, 64, 64, 32), (21, 64, 64, 64)],
         [{BATCH2, RAGGED_M}, {BATCH2, RAGGED_M, COUT_TAIL}])
    + _c("ig16-pw-128to160", conv(2, 128, 160, (4, 20, 16), 1), (FWD, DGRAD), [(21, 64, 64, 64), (21, 64, 64, 32)],
         [{BATCH2, COUT_TAIL}, {BATCH2}])
    # 64 x 128, 128 x 64 and 128 x 128 are chosen only where they still give 512 workgroups (1024 transposed)
    + _c("ig16-s2-32to128", conv(1, 32, 128, (32, 64, 128), 3, 2, 1), (FWD,), [(21, 64, 128, 32)], [set()])
    + _c("ig16-s2-32to64", conv(2, 32, 64, (32, 64, 128), 3, 2, 1), (FWD,), [(21, 128, 64, 32)], [{BATCH2}])
    + _c("ig16-2d-dil-32to128", conv(1, 32, 128, (1, 256, 256), (1, 3, 3), 1, (0, 2, 2), (1, 2, 2)), (FWD,), [(21, 128, 128, 32)], [set()])
    + _c("ig16-deconv-64to128", conv(1, 64, 128, (16, 32, 32), 3, 2, 1, transposed=True, op=1), (FWD,), [(21, 128, 128, 64)], [{PARITY}])
    # pointwise and k == s layers reach the same tiles at a fraction of the reference's cost, with the other stage depth and
    # ragged rows / columns; their data gradients reach the wide tiles in mode 1 (and conv_gather16_kernel<2, 2> by the heuristic)
    + _c("ig16-pw-64to128", conv(1, 64, 128, (8, 64, 64), 1), (FWD, DGRAD), [(21, 64, 128, 64), (21, 64, 64, 64)], [set(), set()])
    + _c("ig16-pw-64to72", conv(2, 64, 72, (8, 63, 65), 1), (FWD, DGRAD), [(21, 128, 64, 64), (16, 2, 2)],
         [{BATCH2, RAGGED_M, COUT_TAIL, COUT_PAD}, {BATCH2, RAGGED_M}])
    + _c("ig16-pw-128to128", conv(2, 128, 128, (8, 64, 64), 1), (FWD, DGRAD), [(21, 128, 128, 64), (21, 64, 128, 64)], [{BATCH2}] * 2)
    + _c("ig16-pw-128to96", conv(2, 128, 96, (8, 63, 65), 1), (FWD, DGRAD), [(21, 128, 64, 64), (21, 64, 128, 32)],
         [{BATCH2, RAGGED_M, COUT_TAIL}, {BATCH2, RAGGED_M}])
    + _c("ig16-deconv-k2-64to96", conv(2, 64, 96, (8, 32, 34), 2, 2, 0, transposed=True), (FWD, DGRAD),
         [(21, 128, 64, 64), (21, 64, 64, 32)], [{BATCH2, COUT_TAIL, PARITY}, {BATCH2}])
    + _c("ig16-deconv-k2-128to32", conv(2, 128, 32, (16, 32, 32), 2, 2, 0, transposed=True), (FWD, DGRAD),
         [(16, 1, 1), (21, 64, 128, 32)], [{BATCH2, PARITY}, {BATCH2}])
    + _c("ig16-pw-64to32", conv(2, 64, 32, (16, 64, 64), 1), (FWD, DGRAD), [(16, 2, 1), (21, 128, 64, 32)], [{BATCH2}] * 2)
    # ------------------------------------------------------------------------------------------------ conv_wide16_kernel (hint 7)
    + _c("w16-64to64", conv(2, 64, 64, (3, 16, 32), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 2, 1, 2, 1)] * 2, [{BATCH2}] * 2)
    + _c("w16-96to96", conv(1, 96, 96, (1, 5, 16), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 3, 1, 1, 1)] * 2, [{D1, RAGGED_H}] * 2)
    + _c("w16-64to192", conv(1, 64, 192, (2, 20, 16), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 3, 2, 1, 2), (19, 2, 2, 1, 1)],
         [{D2, RAGGED_H}] * 2)
    + _c("w16-160to128", conv(2, 160, 128, (2, 5, 16), 3, 1, 1, hint=7), (FWD,), [(19, 4, 1, 1, 1)], [{BATCH2, D2, RAGGED_H}])
    + _c("w16-64to256", conv(1, 64, 256, (1, 16, 32), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 4, 1, 2, 2), (19, 2, 1, 2, 1)], [{D1}] * 2)
    + _c("w16-192to64", conv(1, 192, 64, (2, 20, 16), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 2, 2, 1, 1), (19, 3, 2, 1, 2)],
         [{D2, RAGGED_H}] * 2)
    + _c("w16-256to96", conv(1, 256, 96, (1, 5, 16), 3, 1, 1, hint=7), (FWD, DGRAD), [(19, 3, 1, 1, 1), (19, 4, 1, 1, 2)],
         [{D1, RAGGED_H}] * 2)
    + _c("w16-128to160", conv(1, 128, 160, (3, 20, 16), 3, 1, 1, hint=7), (DGRAD,), [(19, 4, 2, 1, 1)], [{RAGGED_H}])
    # ------------------------------------------------------------------------------------------------ conv_tap16_kernel (hint 9)
    + _c("t16-24to16", conv(2, 24, 16, (4, 6, 32), 3, 1, 1, hint=9), (FWD, DGRAD), [(17, 1, 1)] * 2, [{BATCH2}] * 2)
    # ------------------------------------------------------------------------------------------------ wgrad16_kernel
    # 600 voxels in chunks of 256: three chunks (one workgroup with an idle wave), the last one 88 voxels
    + _c("wg16-24to16-k3", conv(2, 24, 16, (3, 5, 20), 3, 1, 1), (WGRAD,), [(18, 1, 1, 3, 3, 256, 3)], [_W18])
    + _c("wg16-24to40-k3", conv(2, 24, 40, (3, 5, 20), 3, 1, 1), (WGRAD,), [(18, 2, 2, 1, 3, 256, 3)], [_W18])
    + _c("wg16-24to16-big", conv(2, 24, 16, (7, 9, 20), 3, 1, 1), (WGRAD,), [(18, 1, 1, 3, 3, 256, 10)], [_W18])
    + _c("wg16-16to24-k2s2", conv(2, 16, 24, (6, 10, 40), 2, 2, 0), (WGRAD,), [(18, 1, 1, 3, 3, 256, 3)], [_W18 | {RAGGED_TAP}])
    + _c("wg16-deconv-24to16-k2s2", conv(2, 24, 16, (3, 5, 20), 2, 2, 0, transposed=True), (WGRAD,), [(18, 1, 1, 3, 3, 256, 3)],
         [_W18 | {RAGGED_TAP}])
    + _c("wg16-40to72-k4s4", conv(1, 40, 72, (8, 20, 44), 4, 4, 0), (WGRAD,), [(18, 2, 2, 1, 3, 256, 1)],
         [(_W18 | {RAGGED_TAP}) - {BATCH2}])
    + _c("wg16-deconv-72to40-k4s4", conv(2, 72, 40, (2, 5, 29), 4, 4, 0, transposed=True), (WGRAD,), [(18, 2, 2, 1, 3, 256, 3)],
         [_W18 | {RAGGED_TAP}])
    + _c("wg16-pw-24to32", conv(2, 24, 32, (3, 5, 41), 1), (WGRAD,), [(18, 1, 1, 1, 1, 256, 5)], [_W18 - {CP_TAIL}])
    + _c("wg16-pw-72to40", conv(2, 72, 40, (3, 5, 41), 1), (WGRAD,), [(18, 2, 2, 1, 1, 256, 5)], [_W18])
    + _c("wg16-s2-32to64", conv(2, 32, 64, (5, 7, 9), 3, 2, 1), (WGRAD,), [(18, 2, 2, 1, 3, 256, 1)], [_W18 - {CP_TAIL}])
    + _c("wg16-2d-dil-64to48", conv(2, 64, 48, (1, 12, 20), (1, 3, 3), 1, (0, 2, 2), (1, 2, 2)), (WGRAD,), [(18, 2, 2, 1, 3, 256, 2)],
         [_W18 - {CQ_TAIL}])
    # ------------------------------------------------------------------------------------------------ wgrad_ring16_kernel (hint 7 / 9)
    # 3, 6 and 26 tiles of 8 rows x 16 voxels: one chunk of three, 4 + 2, six chunks of 4 + 2
    + _c("wr16-16to24-t3", conv(1, 16, 24, (3, 8, 16), 3, 1, 1, hint=9), (WGRAD,), [(20, 1, 3, 1, 1)], [set()])
    + _c("wr16-16to24-t6", conv(1, 16, 24, (3, 12, 16), 3, 1, 1, hint=9), (WGRAD,), [(20, 1, 4, 2, 1)], [{RAGGED_H, SHORT_TILE_CHUNK}])
    + _c("wr16-16to24-t26", conv(2, 16, 24, (13, 8, 16), 3, 1, 1, hint=7), (WGRAD,), [(20, 1, 4, 7, 1)], [{BATCH2, SHORT_TILE_CHUNK}])
    + _c("wr16-40to160-t3", conv(1, 40, 160, (3, 8, 16), 3, 1, 1, hint=7), (WGRAD,), [(20, 0, 3, 1, 2)], [{CP_RAGGED, NCQT_RAGGED}])
    + _c("wr16-40to160-t6", conv(2, 40, 160, (3, 8, 16), 3, 1, 1, hint=7), (WGRAD,), [(20, 0, 4, 2, 2)],
         [{BATCH2, CP_RAGGED, NCQT_RAGGED, SHORT_TILE_CHUNK}])
    + _c("wr16-40to160-t26", conv(1, 40, 160, (13, 12, 16), 3, 1, 1, hint=9), (WGRAD,), [(20, 0, 4, 7, 2)],
         [{CP_RAGGED, NCQT_RAGGED, RAGGED_H, SHORT_TILE_CHUNK}])
)

# the three shapes of test_gpu_bf16_storage.py::test_conv_igemm16_is_bit_identical_to_the_gather_kernel (B = 2): all on the 64 x 64 tile
LEGACY_IGEMM16 = (conv(2, 64, 128, (16, 16, 32), 3, 2, 1), conv(2, 128, 64, (8, 8, 16), 3, 2, 1, transposed=True, op=1),
                  conv(2, 96, 64, (4, 16, 40), 3, 1, 1))
