"""Case table of the depth-fused Winograd stage tests (test_wino_df_plan.py on the CPU, test_gpu_wino_df.py on the GPU).

csrc/winograd_fused.hip runs the contraction on one of six instances wino_df_kernel<MT, NW> (``10 MT + NW``) and the weight
gradient on one of three instances wino_dfw_kernel<KW, NT, BR> with a row split into chunks (wino_dfw_sum_kernel adds the
chunks).  Each case below is the smallest shape found that reaches one instance with the tails, dead waves and chunk shapes it
is listed for; the expected plan is what ``ssbev_wino43_df_plan_query`` -- which reads the plan functions the launchers read --
answers, so test_wino_df_plan.py notices on a box without a GPU when a threshold moves a case, and the GPU tests cannot lose
this coverage quietly.

Shapes are ``(B, K, N, D, H, W)``: ssbev_wino_dims (B, D, H, W, C = K) and N columns; Thw = (H / 4)(W / 4) rows per plane.

Instances 22 and 23 are reachable through the tuning-build hooks only (nw == 3 and nw == 2 force mt = 1 in the product build):
they have no case and nothing here forces them.

``reference_plan`` is a transcription of the launch geometry as the launchers computed it inline before the query existed;
test_wino_df_plan.py compares the query with it on random dims."""
import collections
import ctypes as C

from stereoscene_amd import capi

FWD, WGRAD = "fwd", "wgrad"
ALL_INSTANCES = {12, 13, 14, 24}                       # 22 / 23: tuning builds only
ALL_WGRAD_KERNELS = {(2, 1, 16), (4, 3, 8), (4, 2, 16)}

# ---- contraction properties (fwd_props recomputes them from the query)
ROW_TAIL = "row_tail"                # Thw is no multiple of the workgroup's 32 MT rows: rows of the last row group do not exist
ROW_GROUPS = "row_groups"            # more than one row group per plane (then ROW_TAIL = a ragged last group)
COL_GROUPS = "col_groups"            # more than one column group of 32 NW columns
NST_1 = "one_k_stage"                # K = 32: the pipeline is the single stage(..., false_type) call
NST_ODD = "odd_k_stages"             # odd nst > 1: the last stage sits in buffer 0
N_TAIL = "n_tail"                    # N % 32 != 0: NPad > N, a wave stores fewer than 8 float4 columns per row
IDLE_WAVES = "idle_waves"            # waves whose 32 columns lie beyond NPad (the nw = 4 fallback of odd tile counts)
HALO_BOTH = "both_halo_planes_out"   # D = 2: planes -1 and D of the only depth tile are out of range
DEPTH_TILES = "depth_tiles"          # more than one depth tile
BATCHED = "batched"                  # B > 1
XCD_TAIL = "grid_not_multiple_of_8"  # the XCD renumbering has a remainder
FWD_PROPS = {ROW_TAIL, ROW_GROUPS, COL_GROUPS, NST_1, NST_ODD, N_TAIL, IDLE_WAVES, HALO_BOTH, DEPTH_TILES, BATCHED, XCD_TAIL}

# ---- weight-gradient properties (wgrad_props)
SPLIT = "split"                      # nchunk > 1: wino_dfw_sum_kernel runs
CHUNKS_3 = "three_chunks"            # the sum pass adds more than two chunks
SHORT_LAST = "short_last_chunk"      # the last chunk has fewer stages than the others
DEAD_KWAVE = "dead_k_wave"           # a k-wave whose 32 channels lie beyond K (tile_active false, kk < K zero fill)
K_BLOCKS = "k_blocks"                # more than one block of 32 KW channels
N_BLOCKS = "n_blocks"                # more than one column block
THW_BELOW = "thw_below_stage"        # Thw < BR: every stage is mostly zero fill
THW_ONE_PAST = "thw_one_past_stage"  # Thw % BR == 1 with Thw > BR: a stage of one live row
ROW_STAGES = "row_stages"            # more than one row stage per plane
WGRAD_PROPS = {SPLIT, CHUNKS_3, SHORT_LAST, DEAD_KWAVE, K_BLOCKS, N_BLOCKS, N_TAIL, THW_BELOW, THW_ONE_PAST, ROW_STAGES}

Case = collections.namedtuple("Case", "stage shape plan props")
# plan: fwd -> instance; wgrad -> ((kw, nt, br), nchunk, stages_per_chunk)


def _f(shape, instance, *props):
    return Case(FWD, shape, instance, frozenset(props))


def _w(shape, kernel, nchunk, per, *props):
    return Case(WGRAD, shape, (kernel, nchunk, per), frozenset(props))


CASES = (
    # ------------------------------------------------------------------------------------------------------- contraction
    # <2, 4>, the instance of the production grids: Thw = 60 (4 rows of the 64-row tile missing), 2 column groups, 2 k-stages,
    # 15 depth tiles x 2 batch elements, grid 2160 (nothing smaller gets past the `< 2048` threshold)
    _f((2, 64, 256, 30, 24, 40), 24, ROW_TAIL, COL_GROUPS, DEPTH_TILES, BATCHED),
    # one k-stage, one row, one depth tile, three waves without columns, grid 36
    _f((1, 32, 32, 2, 4, 4), 14, ROW_TAIL, NST_1, IDLE_WAVES, HALO_BOTH, XCD_TAIL),
    # N = 36: the second wave stores one float4 column per row
    _f((1, 32, 36, 2, 8, 20), 12, ROW_TAIL, NST_1, N_TAIL, HALO_BOTH, XCD_TAIL),
    # N = 100: the fourth wave is partially live
    _f((1, 32, 100, 2, 4, 36), 14, ROW_TAIL, NST_1, N_TAIL, HALO_BOTH, XCD_TAIL),
    # three k-stages; 5 column tiles: the second column group has one live wave
    _f((1, 96, 160, 4, 12, 12), 14, ROW_TAIL, COL_GROUPS, NST_ODD, IDLE_WAVES, DEPTH_TILES),
    # three waves, 9 depth tiles
    _f((1, 96, 96, 18, 4, 12), 13, ROW_TAIL, NST_ODD, DEPTH_TILES, XCD_TAIL),
    _f((1, 64, 64, 6, 8, 8), 12, ROW_TAIL, DEPTH_TILES, XCD_TAIL),
    # mt = 1 with two row groups, the second one ragged (Thw = 33)
    _f((1, 32, 64, 2, 12, 44), 12, ROW_TAIL, ROW_GROUPS, NST_1, HALO_BOTH),
    # --------------------------------------------------------------------------------------------------- weight gradient
    _w((1, 64, 64, 34, 4, 4), (2, 1, 16), 2, 9, SPLIT, SHORT_LAST, THW_BELOW),                  # 17 stages = 9 + 8
    _w((1, 64, 64, 50, 4, 4), (2, 1, 16), 3, 9, SPLIT, CHUNKS_3, SHORT_LAST, THW_BELOW),        # 25 = 9 + 9 + 7
    # K = 32: the second k-wave is dead; N = 36; Thw = 3 against 16-row stages
    _w((1, 32, 36, 34, 4, 12), (2, 1, 16), 2, 9, SPLIT, SHORT_LAST, DEAD_KWAVE, N_TAIL, THW_BELOW),
    _w((1, 96, 96, 34, 4, 4), (4, 3, 8), 2, 9, SPLIT, SHORT_LAST, DEAD_KWAVE, THW_BELOW),       # the fourth k-wave is dead
    _w((1, 96, 96, 50, 4, 12), (4, 3, 8), 3, 9, SPLIT, CHUNKS_3, SHORT_LAST, DEAD_KWAVE, THW_BELOW),
    # K = 160: 2 K blocks, the second with one live k-wave; N = 100: 2 column blocks; 21 stages = 11 + 10
    _w((1, 160, 100, 42, 4, 20), (4, 2, 16), 2, 11, SPLIT, SHORT_LAST, DEAD_KWAVE, K_BLOCKS, N_BLOCKS, N_TAIL, THW_BELOW),
    _w((1, 192, 64, 18, 4, 20), (4, 2, 16), 1, 9, DEAD_KWAVE, K_BLOCKS, THW_BELOW),             # one chunk
    # one row past a full stage: Thw = 17 against 16 rows, Thw = 9 against 8
    _w((1, 64, 64, 2, 4, 68), (2, 1, 16), 1, 2, THW_ONE_PAST, ROW_STAGES),
    _w((1, 96, 96, 2, 12, 12), (4, 3, 8), 1, 2, DEAD_KWAVE, THW_ONE_PAST, ROW_STAGES),
)

# whole-conv cases of test_gpu_wino_df.py (B, Cin, Cout, D, H, W): the smallest with both channel counts multiples of 32 whose
# weight gradient splits
CONV_CASES = ((1, 64, 64, 34, 4, 4), (1, 96, 96, 34, 4, 4))

# the nine cases of test_gpu_kernels.py::test_winograd_depth_fused_f43, (B, Cin, Cout, D, H, W)
LEGACY_CONV_CASES = ((2, 128, 96, 6, 4, 4), (1, 96, 96, 4, 8, 12), (1, 384, 192, 2, 4, 8), (1, 64, 64, 6, 8, 8),
                     (1, 128, 128, 16, 8, 8), (2, 512, 256, 4, 4, 8), (1, 192, 384, 2, 36, 40), (1, 128, 160, 8, 32, 36),
                     (1, 256, 64, 4, 20, 16))


def case_id(c):
    return c.stage + "-" + "x".join(map(str, c.shape))


def wino_dims(shape):
    B, K, N, D, H, W = shape
    return capi.WinoDims(B, D, H, W, K), N


def query(shape):
    """ssbev_wino43_df_plan of a shape, or the error code."""
    d, N = wino_dims(shape)
    p = capi.Wino43DfPlan()
    rc = capi.load().ssbev_wino43_df_plan_query(C.byref(d), N, C.byref(p))
    return p if rc == capi.OK else rc


def plan_tuple(p):
    return tuple(getattr(p, f) for f, _ in capi.Wino43DfPlan._fields_)


def case_plan(c, p):
    """The part of the plan a case pins."""
    if c.stage == FWD:
        return 10 * p.mt + p.nw
    return ((p.w_kw, p.w_nt, p.w_br), p.w_nchunk, p.w_stages_per_chunk)


def fwd_props(shape, p):
    """The FWD_PROPS a contraction launch with plan p has, from the definitions in words."""
    B, K, N, D, H, W = shape
    Thw, npad = (H // 4) * (W // 4), -(-N // 32) * 32
    props = set()
    if Thw % (32 * p.mt):
        props.add(ROW_TAIL)
    if p.nrowgrp > 1:
        props.add(ROW_GROUPS)
    if p.ncolgrp > 1:
        props.add(COL_GROUPS)
    if p.nst == 1:
        props.add(NST_1)
    elif p.nst % 2:
        props.add(NST_ODD)
    if N % 32:
        props.add(N_TAIL)
    if p.ncolgrp * p.nw * 32 > npad:
        props.add(IDLE_WAVES)
    if D == 2:
        props.add(HALO_BOTH)
    if D > 2:
        props.add(DEPTH_TILES)
    if B > 1:
        props.add(BATCHED)
    if p.grid % 8:
        props.add(XCD_TAIL)
    return props


def chunk_stages(p):
    """Stages of every weight-gradient chunk."""
    return [max(0, min(p.w_total_stages, (c + 1) * p.w_stages_per_chunk) - c * p.w_stages_per_chunk) for c in range(p.w_nchunk)]


def wgrad_props(shape, p):
    """The WGRAD_PROPS a weight-gradient launch with plan p has."""
    B, K, N, D, H, W = shape
    Thw = (H // 4) * (W // 4)
    props = set()
    if p.w_nchunk > 1:
        props.add(SPLIT)
    if p.w_nchunk > 2:
        props.add(CHUNKS_3)
    if p.w_nchunk > 1 and chunk_stages(p)[-1] < p.w_stages_per_chunk:
        props.add(SHORT_LAST)
    if p.w_nkb * p.w_kw * 32 - K >= 32:
        props.add(DEAD_KWAVE)
    if p.w_nkb > 1:
        props.add(K_BLOCKS)
    if p.w_nnb > 1:
        props.add(N_BLOCKS)
    if N % 32:
        props.add(N_TAIL)
    if Thw < p.w_br:
        props.add(THW_BELOW)
    if Thw > p.w_br and Thw % p.w_br == 1:
        props.add(THW_ONE_PAST)
    if Thw > p.w_br:
        props.add(ROW_STAGES)
    return props


# ------------------------------------------------------------------------------------------------------------------------
# transcription of the launch geometry before ssbev_wino43_df_plan_query (every `/` of the C source is on non-negative ints)
def reference_plan(shape):
    B, K, N, D, H, W = shape
    Thw, ND = (H // 4) * (W // 4), D // 2
    ntile = -(-N // 32)
    nw = 4 if ntile % 4 == 0 else (3 if ntile % 3 == 0 else (2 if ntile % 2 == 0 else 4))
    ncolgrp = -(-ntile // nw)
    mt = 2
    if 36 * B * ND * -(-Thw // 64) * ncolgrp < 2048:
        mt = 1
    if -(-Thw // 64) * 64 * 10 > -(-Thw // 32) * 32 * 11:
        mt = 1
    if nw in (2, 3):
        mt = 1
    nrowgrp = -(-Thw // (32 * mt))
    fwd = (mt, nw, ncolgrp, nrowgrp, K // 32, 36 * B * ND * nrowgrp * ncolgrp, 2 * 4 * 32 * mt * 32 * 4)
    if K <= 64:
        kw, nt, br = 2, 1, 16
    elif N % 96 == 0:
        kw, nt, br = 4, 3, 8
    else:
        kw, nt, br = 4, 2, 16
    pc, zc = kw * 32, (4 // kw) * nt * 32
    nkb, nnb = -(-K // pc), -(-N // zc)
    total = B * ND * -(-Thw // br)
    per = 36 * nkb * nnb
    nchunk = max(1, 1024 // per)
    best, best_n = -1.0, nchunk
    for n in range(max(1, nchunk * 2 // 3), nchunk * 2 + 1):
        tot = per * n
        rounds = (tot + 511) // 512
        eff = tot / (rounds * 512) - 0.002 * abs(n - nchunk)
        if eff > best:
            best, best_n = eff, n
    nchunk = min(best_n, max(1, total // 8))
    wgrad = (kw, nt, br, nkb, nnb, nchunk, -(-total // nchunk), total, 36 * nchunk * nkb * nnb,
             2 * (4 * br * pc + 2 * br * zc) * 4, nchunk * 144 * K * N * 4)
    return fwd + wgrad


FAKE = 256           # a non-null pointer for host-side refusals: never dereferenced


def check_return_codes():
    """Every refusal of the depth-fused entry points comes before any device work (placeholder pointers, never dereferenced):
    SSBEV_EINVAL for odd D, H % 4 != 0, W % 4 != 0, K % 32 != 0, N % 4 != 0 and null pointers -- from the query, the launchers,
    and 0 from _supported / _instance / _wgrad_workspace; SSBEV_EWORKSPACE for a workspace one byte short."""
    lib = capi.load()
    fake = C.c_void_p(FAKE)
    good = (1, 64, 64, 34, 4, 4)
    p = query(good)
    assert not isinstance(p, int) and p.w_nchunk == 2 and p.w_workspace == 2 * 144 * 64 * 64 * 4
    d, N = wino_dims(good)
    assert lib.ssbev_wino43_df_supported(C.byref(d), N) == 1
    assert lib.ssbev_wino43_df_wgrad_workspace(C.byref(d), N) == p.w_workspace
    plan = capi.Wino43DfPlan()
    assert lib.ssbev_wino43_df_plan_query(None, N, C.byref(plan)) == capi.EINVAL
    assert lib.ssbev_wino43_df_plan_query(C.byref(d), N, None) == capi.EINVAL
    bad = {"odd D": (1, 64, 64, 33, 4, 4), "H % 4": (1, 64, 64, 34, 6, 4), "W % 4": (1, 64, 64, 34, 4, 6),
           "K % 32": (1, 48, 64, 34, 4, 4), "N % 4": (1, 64, 62, 34, 4, 4), "B = 0": (0, 64, 64, 34, 4, 4),
           "N = 0": (1, 64, 0, 34, 4, 4)}
    for why, shape in bad.items():
        bd, bn = wino_dims(shape)
        assert query(shape) == capi.EINVAL, why
        assert lib.ssbev_wino43_df_supported(C.byref(bd), bn) == 0, why
        assert lib.ssbev_wino43_df_instance(C.byref(bd), bn) == 0, why
        assert lib.ssbev_wino43_df_wgrad_workspace(C.byref(bd), bn) == 0, why
        assert lib.ssbev_wino43_df_gemm(fake, fake, fake, C.byref(bd), bn, None) == capi.EINVAL, why
        assert lib.ssbev_wino43_df_wgrad(fake, fake, fake, C.byref(bd), bn, fake, 1 << 40, None) == capi.EINVAL, why
    # null operands, each on its own
    for null in range(3):
        a = [None if i == null else fake for i in range(3)]
        assert lib.ssbev_wino43_df_gemm(*a, C.byref(d), N, None) == capi.EINVAL, null
        assert lib.ssbev_wino43_df_wgrad(*a, C.byref(d), N, fake, p.w_workspace, None) == capi.EINVAL, null
    assert lib.ssbev_wino43_df_gemm(fake, fake, fake, None, N, None) == capi.EINVAL
    assert lib.ssbev_wino43_df_wgrad(fake, fake, fake, C.byref(d), N, None, p.w_workspace, None) == capi.EINVAL
    for mode, args in {"w": (None, fake, 64, 64, 0), "Wp": (fake, None, 64, 64, 0), "mode": (fake, fake, 64, 64, 2),
                       "Cout": (fake, fake, 0, 64, 0), "Cin": (fake, fake, 64, 0, 1)}.items():
        assert lib.ssbev_wino43_df_pack(*args, None) == capi.EINVAL, mode
    # workspace: one byte short, or none at all
    assert lib.ssbev_wino43_df_wgrad(fake, fake, fake, C.byref(d), N, fake, p.w_workspace - 1, None) == capi.EWORKSPACE
    assert lib.ssbev_wino43_df_wgrad(fake, fake, fake, C.byref(d), N, fake, 0, None) == capi.EWORKSPACE
    # 32-bit slab offsets: the weight gradient alone refuses B D Thw max(K, N) >= 2^31 (the query answers: the contraction runs)
    huge = (64, 512, 512, 64, 128, 128)
    hd, hn = wino_dims(huge)
    assert not isinstance(query(huge), int)
    assert lib.ssbev_wino43_df_wgrad(fake, fake, fake, C.byref(hd), hn, fake, 1 << 62, None) == capi.EINVAL
