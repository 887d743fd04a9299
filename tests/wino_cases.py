"""Case table of the stage tests of csrc/winograd.hip (test_wino_ref.py on the CPU, test_gpu_wino_transforms.py on the GPU).

Four stage kinds: the streaming transforms (one thread per (tile, channel)), the weight transforms, the depth-fused-in-registers
GEMM ``ssbev_wino_dgemm`` (with ``ssbev_wino_dgemm_pack``) and the batched frequency GEMM ``ssbev_wino_bgemm``.  Every case is the
smallest shape found with the properties it is listed for.  test_wino_ref.py recomputes every case's properties from its dims
and, for the GEMMs, from ``ssbev_wino_gemm_plan_query`` -- which answers from the plan functions the two launchers read -- so a
moved threshold, a deleted case or an entry point without a case fails on a box without a GPU.

``wino_dgemm_kernel`` has six template instances; the product build launches <1, 2> only.  The other five (14, 13, 22, 21, 11)
are selected by SSBEV_WINO_TILE, which goes through ``ssbev_tune`` (csrc/common.h): a null constant in the product build, so the
switch is compiled out.  They have no case and nothing here forces them; test_wino_ref.py asserts that the query answers <1, 2>.

The dilated instances of the 2-D F(2,3) kernels (``ssbev_wino_dims.dil`` > 1) belong to test_gpu_wino2d_dilated.py, and the
depth-fused F(4,3) contraction (``ssbev_wino43_df_*``) to test_gpu_wino_df.py."""
import collections
import ctypes as C

import wino_ref as R
from stereoscene_amd import capi

# ---- transform properties (transform_props recomputes them from the dims)
ONE_TILE = "one_tile"                    # one tile per map: every halo plane, row and column of it lies outside the map
DISTINCT_EXTENTS = "distinct_extents"    # B, D, H, W all different, more than one tile (plane) on every axis: a swapped axis shows
GRID_TAIL = "grid_tail"                  # more than 256 threads and no multiple of 256: a second, partial workgroup
ODD_C = "odd_c"                          # `_bf16a`: NV = 1, one channel per thread
EVEN_C = "even_c"                        # `_bf16a`: NV = 2, packed 4-byte accesses
PACKED_MIN = "packed_min"                # `_bf16a`: C = 2, one packed access per position
BATCH_AXIS_D = "batch_axis_d"            # a 2-D tiling with odd D > 1: D is a batch axis
ACC = "acc"                              # the output transform adds to y
TRANSFORM_PROPS = {ONE_TILE, DISTINCT_EXTENTS, GRID_TAIL, ODD_C, EVEN_C, PACKED_MIN, BATCH_AXIS_D, ACC}
FP32, BF16, BF16A = "fp32", "bf16", "bf16a"      # storage: all fp32 / transformed domain bf16 / both sides bf16
INPUT, OUTPUT, ADJOINT, OUTPUT_ACC = "input", "output", "adjoint", "output_acc"

PREFIX = {"w3d": "ssbev_wino_", "w2d": "ssbev_wino2d_", "w43_2d": "ssbev_wino43_2d_", "w43": "ssbev_wino43_", "w444": "ssbev_wino444_"}
STORAGES = {"w3d": (FP32, BF16, BF16A), "w2d": (FP32, BF16, BF16A), "w43_2d": (FP32, BF16), "w43": (FP32, BF16), "w444": (FP32,)}
ACC_TILINGS = ("w2d", "w43_2d")
TWO_D = ("w2d", "w43_2d")

# ---- weight properties
RECT = "rect"                            # Cout != Cin
W_GRID_TAIL = "weight_grid_tail"         # Cout Cin above 256 and no multiple of 256
MODE_1 = "mode_1"                        # mirrored taps, swapped channel roles
WEIGHT_PROPS = {RECT, W_GRID_TAIL, MODE_1}
W_TRANSFORM, W_GRAD = "weight_transform", "weight_grad"
WEIGHT_TILINGS = {("ssbev_wino_", 2): "w2d", ("ssbev_wino_", 3): "w3d", ("ssbev_wino43_", 2): "w43_2d", ("ssbev_wino43_", 3): "w43",
                  ("ssbev_wino43_", 4): "w444"}

# ---- ssbev_wino_dgemm properties (dgemm_props, from the query)
ROW_TAIL = "row_tail"                    # Thw < 32: the only row group is partial
ROW_GROUPS = "row_groups"                # more than one row group, the last with one live row; waves return at tg >= tgroups
X_WORKGROUPS = "x_workgroups"            # more than four row groups: a second workgroup along x per (b, depth tile)
HALO_BOTH = "both_halo_planes_out"       # D = 2
DEPTH_TILES = "depth_tiles"              # D > 2
BATCHED = "batched"                      # B > 1
D_K_HALF = "k_half"                      # Cin % 8 == 4: the second half of the last k-step is zero fill (cok)
D_N_TAIL = "n_tail"                      # N % 32 != 0
N_ONE_TILE = "n_one_tile"                # N = 32 with nt = 2: the second column tile lies beyond CoutPad
COL_GROUPS = "col_groups"                # grid y > 1
DGEMM_PROPS = {ROW_TAIL, ROW_GROUPS, X_WORKGROUPS, HALO_BOTH, DEPTH_TILES, BATCHED, D_K_HALF, D_N_TAIL, N_ONE_TILE, COL_GROUPS}

# ---- ssbev_wino_bgemm properties (bgemm_props, from the query)
ONE_PARTIAL_BLOCK = "one_partial_block"  # T < 64
TWO_BLOCKS = "two_blocks"                # one workgroup walks two row blocks: the LDS ring crosses a row-block boundary
TWO_WORKGROUPS = "two_workgroups"        # gx = 2, both with work, the last row block partial
IDLE_WORKGROUP = "idle_workgroup"        # the last workgroup along x gets no row block (total <= 0)
K_ONE_QUAD = "k_one_quad"                # K = 4
K_STAGE_TAIL = "k_stage_tail"            # two k-stages, the second with one float4 column
K_RING_WRAP = "k_ring_wrap"              # three k-stages: every ring buffer is used once per row block
K_RING_REUSE = "k_ring_reuse"            # four k-stages: a ring buffer is reused within one row block
B_K_HALF = "k_half"                      # K % 8 == 4
K_WHOLE = "k_whole_stages"               # K % 64 == 0
IDLE_WAVES = "idle_waves"                # N <= 32 NT: three of the four waves have no columns
B_N_TAIL = "n_tail"                      # N % 32 != 0
NT2 = "nt2"                              # nt = 2 and a wave whose second tile lies beyond NPad
COL_GROUPS_NT2 = "col_groups_nt2"        # nt = 2 and ycols = 2
BGEMM_PROPS = {ONE_PARTIAL_BLOCK, TWO_BLOCKS, TWO_WORKGROUPS, IDLE_WORKGROUP, K_ONE_QUAD, K_STAGE_TAIL, K_RING_WRAP, K_RING_REUSE,
               B_K_HALF, K_WHOLE, IDLE_WAVES, B_N_TAIL, NT2, COL_GROUPS_NT2}

TRANSFORM, WEIGHT, DGEMM, BGEMM = "transform", "weight", "dgemm", "bgemm"
Case = collections.namedtuple("Case", "stage names shape plan props what")
# transform: what = (tiling, role, storage), shape = (B, D, H, W, C), plan = thread count
# weight:    what = (tiling, role, prefix, ndim, mode), shape = (Cout, Cin), plan = thread count
# dgemm:     shape = (B, D, H, W, K, N), plan = (mt, nt, tgroups, (grid x, y, z), Q, CoutPad)
# bgemm:     shape = (T, K, N), plan = (nt, ycols, gx, nrb, rb_per, nstage)


def transform_entry(tiling, role, storage):
    if role == OUTPUT_ACC:
        return PREFIX[tiling] + "output_transform_acc"
    stem = {INPUT: "input_transform", OUTPUT: "output_transform", ADJOINT: "output_adjoint"}[role]
    return PREFIX[tiling] + stem + {FP32: "", BF16: "_bf16", BF16A: "_bf16a"}[storage]


# (shape, threads, properties) per tiling and storage; every role of the tiling runs every shape
_SHAPES = {
    "w3d": {
        FP32: (((1, 2, 2, 2, 3), 3, {ONE_TILE}), ((2, 4, 6, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL})),
        BF16: (((1, 2, 2, 2, 3), 3, {ONE_TILE}), ((2, 4, 6, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL})),
        BF16A: (((1, 2, 2, 2, 2), 1, {ONE_TILE, EVEN_C, PACKED_MIN}), ((2, 4, 6, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL, ODD_C}),
                ((2, 4, 6, 16, 6), 288, {DISTINCT_EXTENTS, GRID_TAIL, EVEN_C})),
    },
    "w2d": {
        FP32: (((1, 1, 2, 2, 3), 3, {ONE_TILE}), ((2, 3, 4, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D})),
        BF16: (((1, 1, 2, 2, 3), 3, {ONE_TILE}), ((2, 3, 4, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D})),
        BF16A: (((1, 1, 2, 2, 2), 1, {ONE_TILE, EVEN_C, PACKED_MIN}),
                ((2, 3, 4, 16, 3), 288, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D, ODD_C}),
                ((2, 3, 4, 16, 6), 288, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D, EVEN_C})),
    },
    "w43_2d": {
        FP32: (((1, 1, 4, 4, 3), 3, {ONE_TILE}), ((2, 3, 8, 12, 9), 324, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D})),
        BF16: (((1, 1, 4, 4, 3), 3, {ONE_TILE}), ((2, 3, 8, 12, 9), 324, {DISTINCT_EXTENTS, GRID_TAIL, BATCH_AXIS_D})),
    },
    "w43": {
        FP32: (((1, 2, 4, 4, 3), 3, {ONE_TILE}), ((2, 4, 8, 12, 11), 264, {DISTINCT_EXTENTS, GRID_TAIL})),
        BF16: (((1, 2, 4, 4, 3), 3, {ONE_TILE}), ((2, 4, 8, 12, 11), 264, {DISTINCT_EXTENTS, GRID_TAIL})),
    },
    "w444": {
        FP32: (((1, 4, 4, 4, 3), 3, {ONE_TILE}), ((2, 8, 12, 16, 6), 288, {DISTINCT_EXTENTS, GRID_TAIL})),
    },
}


def _transform_cases():
    out = []
    for tiling, by_storage in _SHAPES.items():
        for storage, shapes in by_storage.items():
            roles = (INPUT, OUTPUT, ADJOINT) + ((OUTPUT_ACC,) if storage == FP32 and tiling in ACC_TILINGS else ())
            for role in roles:
                for shape, threads, props in shapes:
                    props = frozenset(props | ({ACC} if role == OUTPUT_ACC else set()))
                    out.append(Case(TRANSFORM, (transform_entry(tiling, role, storage),), shape, threads, props, (tiling, role, storage)))
    return out


def _weight_cases():
    out = []
    for (prefix, ndim), tiling in WEIGHT_TILINGS.items():
        for (cout, cin), threads, props in (((3, 5), 15, {RECT}), ((20, 17), 340, {RECT, W_GRID_TAIL})):
            for mode in (0, 1):
                out.append(Case(WEIGHT, (prefix + "weight_transform",), (cout, cin), threads,
                                frozenset(props | ({MODE_1} if mode else set())), (tiling, W_TRANSFORM, prefix, ndim, mode)))
            out.append(Case(WEIGHT, (prefix + "weight_grad",), (cout, cin), threads, frozenset(props), (tiling, W_GRAD, prefix, ndim, 0)))
    return out


DGEMM_NAMES = ("ssbev_wino_dgemm", "ssbev_wino_dgemm_pack", "ssbev_wino_dgemm_packed_elems", "ssbev_wino_gemm_plan_query")
BGEMM_NAMES = ("ssbev_wino_bgemm", "ssbev_wino_dgemm_pack", "ssbev_wino_dgemm_packed_elems", "ssbev_wino_gemm_plan_query")


def _d(shape, plan, *props):
    return Case(DGEMM, DGEMM_NAMES, shape, plan, frozenset(props), None)


def _b(shape, plan, *props):
    return Case(BGEMM, BGEMM_NAMES, shape, plan, frozenset(props), None)


GEMM_CASES = (
    # ------------------------------------------------------------------------------------ ssbev_wino_dgemm (B, D, H, W, K, N)
    # Thw = 6: one partial row group; 3 depth tiles x 2 batch elements; K = 12: q = 1 is half zero fill; N = 100: 2 column groups,
    # the second with 36 live columns
    _d((2, 6, 4, 6, 12, 100), (1, 2, 1, (6, 2, 16), 2, 128), ROW_TAIL, DEPTH_TILES, BATCHED, D_K_HALF, D_N_TAIL, COL_GROUPS),
    # Thw = 33: two row groups, the second with one live row, waves 2 and 3 return; N = 40: the second tile has 8 live columns
    _d((1, 2, 6, 22, 12, 40), (1, 2, 2, (1, 1, 16), 2, 64), ROW_GROUPS, HALO_BOTH, D_K_HALF, D_N_TAIL),
    # Thw = 129: five row groups, the second workgroup along x carries one live wave; N = 32: the second tile is beyond CoutPad
    _d((1, 2, 6, 86, 8, 32), (1, 2, 5, (2, 1, 16), 1, 32), ROW_GROUPS, X_WORKGROUPS, HALO_BOTH, N_ONE_TILE),
    # ------------------------------------------------------------------------------------------- ssbev_wino_bgemm (T, K, N)
    _b((1, 4, 20), (1, 1, 1, 1, 1, 1), ONE_PARTIAL_BLOCK, K_ONE_QUAD, B_K_HALF, IDLE_WAVES, B_N_TAIL),
    _b((63, 68, 100), (1, 1, 1, 1, 1, 2), ONE_PARTIAL_BLOCK, K_STAGE_TAIL, B_K_HALF, B_N_TAIL),
    # T = 65: the second row block has one live row; N = 132: nt = 2, wave 2 holds columns 128 .. 131 and a tile beyond NPad = 160
    _b((65, 132, 132), (2, 1, 1, 2, 2, 3), TWO_BLOCKS, K_RING_WRAP, B_K_HALF, B_N_TAIL, NT2),
    # N = 300: two column groups of 256, the second with 44 live columns on one wave (NPad = 320: both of its tiles are loaded)
    _b((65, 196, 300), (2, 2, 1, 2, 2, 4), TWO_BLOCKS, K_RING_REUSE, B_K_HALF, B_N_TAIL, COL_GROUPS_NT2),
    # T = 513: 9 row blocks, 5 + 4 on two workgroups, the last one with one live row
    _b((513, 64, 100), (1, 1, 2, 9, 5, 1), TWO_WORKGROUPS, K_WHOLE, B_N_TAIL),
    # T = 1537: 25 row blocks on gx = 6 workgroups of 5: the sixth gets nothing
    _b((1537, 4, 20), (1, 1, 6, 25, 5, 1), IDLE_WORKGROUP, K_ONE_QUAD, B_K_HALF, IDLE_WAVES, B_N_TAIL),
)

CASES = tuple(_transform_cases()) + tuple(_weight_cases()) + GEMM_CASES

# whole-path cases of test_gpu_wino_transforms.py: route -> (B, Cin, Cout, D, H, W); D = 0: a conv2d
CONV_CASES = {
    "f23_2d": (2, 64, 64, 0, 4, 6),              # 2-D F(2,3), the default of the wide conv2d layers
    "f244_gemm_nn": (1, 64, 64, 2, 4, 8),        # F(2x4x4) + gemm_nn: the wide 3-D layers below WINO_DF_MIN_ROWS
    "own_gemm": (1, 64, 64, 4, 6, 22),           # F(2,3)^3 + ssbev_wino_bgemm at T = 66 >= 65: two row blocks
}

# names of capi.SIGNATURES that other tables own
FOREIGN_PREFIXES = ("ssbev_wino43_df_",)
FOREIGN_NAMES = {"ssbev_wino2d_axis_tiles"}


def case_id(c):
    head = c.names[0][len("ssbev_"):]
    if c.stage == WEIGHT:
        head += f"-nd{c.what[3]}-m{c.what[4]}"
    return head + "-" + "x".join(map(str, c.shape))


def threads(c):
    """Threads of a transform or weight launch, from the dims."""
    if c.stage == WEIGHT:
        return c.shape[0] * c.shape[1]
    tiling, role, storage = c.what
    B, D, H, W, Cc = c.shape
    nv = 2 if storage == BF16A and Cc % 2 == 0 else 1
    return R.ntiles(tiling, B, D, H, W) * (Cc // nv)


def transform_props(c):
    tiling, role, storage = c.what
    B, D, H, W, Cc = c.shape
    counts = R.tile_counts(tiling, D, H, W)
    total = threads(c)
    props = set()
    if B == 1 and all(n == 1 for n in counts):
        props.add(ONE_TILE)
    if len({B, D, H, W}) == 4 and B > 1 and all(n > 1 for n in counts):
        props.add(DISTINCT_EXTENTS)
    if total > 256 and total % 256:
        props.add(GRID_TAIL)
    if storage == BF16A:
        props.add(ODD_C if Cc % 2 else EVEN_C)
        if Cc == 2:
            props.add(PACKED_MIN)
    if tiling in TWO_D and D > 1 and D % 2:
        props.add(BATCH_AXIS_D)
    if role == OUTPUT_ACC:
        props.add(ACC)
    return props


def weight_props(c):
    cout, cin = c.shape
    props = set()
    if cout != cin:
        props.add(RECT)
    if cout * cin > 256 and (cout * cin) % 256:
        props.add(W_GRID_TAIL)
    if c.what[4] == 1:
        props.add(MODE_1)
    return props


def query(c):
    """ssbev_wino_gemm_plan of a GEMM case, or the error code."""
    p = capi.WinoGemmPlan()
    lib = capi.load()
    if c.stage == BGEMM:
        T, K, N = c.shape
        rc = lib.ssbev_wino_gemm_plan_query(T, K, N, None, C.byref(p))
    else:
        B, D, H, W, K, N = c.shape
        d = capi.WinoDims(B, D, H, W, K)
        rc = lib.ssbev_wino_gemm_plan_query(0, 0, N, C.byref(d), C.byref(p))
    return p if rc == capi.OK else rc


def case_plan(c, p):
    if c.stage == BGEMM:
        return (p.b_nt, p.b_ycols, p.b_gx, p.b_nrb, p.b_rb_per, p.b_nstage)
    return (p.d_mt, p.d_nt, p.d_tgroups, (p.d_grid_x, p.d_grid_y, p.d_grid_z), p.d_Q, p.d_CoutPad)


def dgemm_props(shape, p):
    B, D, H, W, K, N = shape
    Thw = (H // 2) * (W // 2)
    rows = 32 * p.d_mt
    props = set()
    if Thw < rows:
        props.add(ROW_TAIL)
    if p.d_tgroups > 1 and Thw % rows == 1 and p.d_tgroups % 4:
        props.add(ROW_GROUPS)
    if p.d_grid_x > B * (D // 2):
        props.add(X_WORKGROUPS)
    if D == 2:
        props.add(HALO_BOTH)
    if D > 2:
        props.add(DEPTH_TILES)
    if B > 1:
        props.add(BATCHED)
    if K % 8 == 4 and 8 * (p.d_Q - 1) + 4 == K:
        props.add(D_K_HALF)
    if N % 32:
        props.add(D_N_TAIL)
    if p.d_nt > 1 and p.d_grid_y * p.d_nt * 32 > p.d_CoutPad and N % 32 == 0:
        props.add(N_ONE_TILE)
    if p.d_grid_y > 1:
        props.add(COL_GROUPS)
    return props


def bgemm_props(shape, p):
    T, K, N = shape
    npad = -(-N // 32) * 32
    owned = [max(0, min(p.b_nrb, (x + 1) * p.b_rb_per) - x * p.b_rb_per) for x in range(p.b_gx)]      # row blocks per workgroup
    props = set()
    if p.b_nrb == 1 and T < 64:
        props.add(ONE_PARTIAL_BLOCK)
    if p.b_gx == 1 and p.b_nrb == 2:
        props.add(TWO_BLOCKS)
    if p.b_gx == 2 and min(owned) > 0 and T % 64:
        props.add(TWO_WORKGROUPS)
    if owned[-1] == 0:
        props.add(IDLE_WORKGROUP)
    if K == 4:
        props.add(K_ONE_QUAD)
    if p.b_nstage == 2 and K % 64 == 4:
        props.add(K_STAGE_TAIL)
    if p.b_nstage == 3:
        props.add(K_RING_WRAP)
    if p.b_nstage == 4:
        props.add(K_RING_REUSE)
    if K % 8 == 4:
        props.add(B_K_HALF)
    if K % 64 == 0:
        props.add(K_WHOLE)
    if N <= 32 * p.b_nt:
        props.add(IDLE_WAVES)
    if N % 32:
        props.add(B_N_TAIL)
    # a wave with live columns whose second 32-column tile starts at or beyond NPad
    if p.b_nt == 2 and any(n0 < N and n0 + 32 >= npad for n0 in range(0, p.b_ycols * 256, 64)):
        props.add(NT2)
    if p.b_nt == 2 and p.b_ycols == 2:
        props.add(COL_GROUPS_NT2)
    return props


# ------------------------------------------------------------------------------------------------------------------------
# transcription of the launch geometry as the two launchers computed it inline before ssbev_wino_gemm_plan_query existed
def reference_bgemm_plan(T, K, N):
    nt = 2 if N > 128 else 1
    nrb = -(-T // 64)
    ycols = -(-N // (4 * nt * 32))
    gx = max(1, (768 + 64 * ycols - 1) // (64 * ycols))
    gx = min(gx, max(1, nrb // 4))
    return (nt, ycols, gx, nrb, -(-nrb // gx), -(-K // 64))


def reference_dgemm_plan(B, D, H, W, K, N):
    Thw = (H // 2) * (W // 2)
    mt, nt = 1, 2
    tgroups = -(-Thw // (32 * mt))
    return (mt, nt, tgroups, (B * (D // 2) * ((tgroups + 3) >> 2), -(-N // (nt * 32)), 16), (K + 7) >> 3, (N + 31) & ~31)
