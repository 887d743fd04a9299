"""The shapes of test_gpu_norm_paths.py and what each of them reaches in csrc/groupnorm.hip.

The normalisation kernels take different paths with the geometry of a launch: the statistics kernel (gn_partial_kernel) walks a
chunk of voxels four trips at a time and finishes in a tail loop, per channel slab of at most 8 lanes; the finalize kernels take
16384 chunk records per outer trip and keep the pivots of up to 1024 channels per group in LDS; the apply kernels are grid-stride
loops whose grid is rounded to a multiple of q / gcd(q, 256) (q = C / 4 lanes per voxel) and capped at 16384 workgroups, so
threads make later trips that land in another sample.  Which of these a shape reaches follows from numbers only the library
knows (ssbev_groupnorm_plan_query, which reads the functions the launchers read); the helpers below derive the walk properties
from its answer, test_norm_plan.py asserts them per case on a box without a GPU, and test_gpu_norm_paths.py runs the cases
against a float64 reference."""
import ctypes as C
from collections import namedtuple

from stereoscene_amd import capi

NT = 256                 # threads of a statistics / apply workgroup
FIN_BATCH = 16 * 1024    # records a finalize workgroup takes per outer trip (kFinBatch * FT)
FIN_LDS_PIVOTS = 1024    # channels per group whose pivots the forward finalize keeps in LDS (FT)
STAT_BLOCKS = 768        # workgroups a statistics launch aims at (kStatBlocks)
UB = 4                   # voxels per trip of the statistics kernel's main loop

# expectations, by hand from the code (test_norm_plan.py holds the query to them):
#   vw, slab_q, slabs                 lane width, lanes per slab, channel slabs of the statistics passes
#   chunks, chunk_len, last_len       chunks per sample, voxels per chunk, voxels of the last chunk
#   main                              per distinct slab width q: rows of the workgroup whose FIRST chunk reaches the main loop
#   fin_batches                       outer trips of the group finalize kernels
#   lds_piv                           pivots of the forward finalize in LDS
#   blocks, fixed, trips              apply grid, stride a multiple of q, grid-stride trips
#   trip2                             (vectors on the second trip, smallest .. largest sample distance of a thread's second trip)
Case = namedtuple("Case", "id dtype B C G sp pre_act expect")


def _c(id, dtype, B, Cch, G, sp, expect, pre_act=None):
    return Case(id, dtype, B, Cch, G, sp, pre_act, expect)


CASES = [
    # A: 20 slabs, 19 chunks of 130 with a short last one: main loop and tail in every slab, every row; 320 vectors on a second
    # apply trip one sample ahead
    _c("A", "fp32", 2, 640, 2, (5, 17, 29),
       dict(vw=4, slab_q=8, slabs=20, chunks=19, chunk_len=130, last_len=125, main={8: 32}, fin_batches=1, lds_piv=True,
            blocks=3080, fixed=1, trips=2, trip2=(320, 1, 1))),
    # A with one channel per group: the per-channel (flat) finalize kernels on the same walk
    _c("A-gc", "fp32", 2, 640, 640, (5, 17, 29),
       dict(vw=4, slab_q=8, slabs=20, chunks=19, chunk_len=130, last_len=125, main={8: 32}, fin_batches=1, lds_piv=True,
            blocks=3080, fixed=1, trips=2, trip2=(320, 1, 1))),
    # B: 768 chunks of 100 voxels, 32 rows: rows 0..3 make one main-loop trip, the others only the tail; G = 1: 24576 records
    _c("B-g1", "fp32", 1, 32, 1, (8, 96, 100),
       dict(vw=4, slab_q=8, slabs=1, chunks=768, chunk_len=100, last_len=100, main={8: 4}, fin_batches=2, lds_piv=True,
            blocks=2400, fixed=1, trips=1, trip2=None)),
    _c("B-g2", "fp32", 1, 32, 2, (8, 96, 100),
       dict(vw=4, slab_q=8, slabs=1, chunks=768, chunk_len=100, last_len=100, main={8: 4}, fin_batches=1, lds_piv=True,
            blocks=2400, fixed=1, trips=1, trip2=None)),
    # C: 12 lanes = a slab of 8 and one of 4 (64 rows): 195-voxel chunks reach the main loop in both; 18432 records
    _c("C", "fp32", 1, 48, 1, (6, 96, 130),
       dict(vw=4, slab_q=8, slabs=2, chunks=384, chunk_len=195, last_len=195, main={8: 32, 4: 3}, fin_batches=2, lds_piv=True,
            blocks=3510, fixed=1, trips=1, trip2=None)),
    # D: 1028 channels per group: pivots read from memory; 65 slabs, the last of 2 lanes; chunks of 64 + 6 voxels; q = 514 is
    # more than the 141 workgroups, so the grid is not rounded and every thread looks its channels up per trip
    _c("D", "fp32", 1, 2056, 2, (1, 70, 1),
       dict(vw=4, slab_q=8, slabs=65, chunks=2, chunk_len=64, last_len=6, main={8: 0, 2: 0}, fin_batches=1, lds_piv=False,
            blocks=141, fixed=0, trips=1, trip2=None)),
    _c("D-gelu", "fp32", 1, 2056, 2, (1, 70, 1),
       dict(vw=4, slab_q=8, slabs=65, chunks=2, chunk_len=64, last_len=6, main={8: 0, 2: 0}, fin_batches=1, lds_piv=False,
            blocks=141, fixed=0, trips=1, trip2=None), pre_act="gelu"),
    # E1: q = 3: grid 7 -> 6, 114 vectors on a second trip four samples ahead, partial last wave
    _c("E1", "fp32", 5, 12, 3, (1, 110, 1),
       dict(vw=4, slab_q=3, slabs=1, chunks=2, chunk_len=64, last_len=46, main={3: 0}, fin_batches=1, lds_piv=True,
            blocks=6, fixed=1, trips=2, trip2=(114, 4, 4))),
    _c("E1-gc", "fp32", 5, 12, 12, (1, 110, 1),
       dict(vw=4, slab_q=3, slabs=1, chunks=2, chunk_len=64, last_len=46, main={3: 0}, fin_batches=1, lds_piv=True,
            blocks=6, fixed=1, trips=2, trip2=(114, 4, 4))),
    # E2: q = 48: grid 61 -> 60, second trip two samples ahead
    _c("E2", "fp32", 3, 192, 32, (1, 107, 1),
       dict(vw=4, slab_q=8, slabs=6, chunks=2, chunk_len=64, last_len=43, main={8: 0}, fin_batches=1, lds_piv=True,
            blocks=60, fixed=1, trips=2, trip2=(48, 2, 2))),
    # E3: q = 5: 51 rows, 255 active threads in the statistics pass
    _c("E3-g1", "fp32", 1, 20, 1, (3, 5, 7),
       dict(vw=4, slab_q=5, slabs=1, chunks=2, chunk_len=64, last_len=41, main={5: 0}, fin_batches=1, lds_piv=True,
            blocks=3, fixed=0, trips=1, trip2=None)),
    _c("E3-g5", "fp32", 1, 20, 5, (3, 5, 7),
       dict(vw=4, slab_q=5, slabs=1, chunks=2, chunk_len=64, last_len=41, main={5: 0}, fin_batches=1, lds_piv=True,
            blocks=3, fixed=0, trips=1, trip2=None)),
    # F: the 16384-workgroup cap: 65536 vectors on a second trip, which starts in sample 0 and lands in sample 1; chunks of 694
    _c("F", "fp32", 2, 32, 2, (16, 128, 130),
       dict(vw=4, slab_q=8, slabs=1, chunks=384, chunk_len=694, last_len=438, main={8: 32}, fin_batches=1, lds_piv=True,
            blocks=16384, fixed=1, trips=2, trip2=(65536, 1, 1))),
    # G: bf16 with 8 channels per lane: main loop, 24576 records
    _c("G", "bf16", 1, 64, 2, (8, 96, 100),
       dict(vw=8, slab_q=8, slabs=1, chunks=768, chunk_len=100, last_len=100, main={8: 4}, fin_batches=2, lds_piv=True,
            blocks=4800, fixed=1, trips=1, trip2=None)),
    # H: bf16 with C % 8 != 0: 4 channels per lane
    _c("H-20", "bf16", 2, 20, 5, (3, 5, 7),
       dict(vw=4, slab_q=5, slabs=1, chunks=2, chunk_len=64, last_len=41, main={5: 0}, fin_batches=1, lds_piv=True,
            blocks=5, fixed=1, trips=1, trip2=None)),
    _c("H-12", "bf16", 2, 12, 3, (1, 43, 1),
       dict(vw=4, slab_q=3, slabs=1, chunks=1, chunk_len=64, last_len=43, main={3: 0}, fin_batches=1, lds_piv=True,
            blocks=2, fixed=0, trips=1, trip2=None)),
]
BY_ID = {c.id: c for c in CASES}

# the bf16 norm_cat of H: branches of 32 and 12 channels over (B, spatial); ld_y = ld_gy = 44 is no multiple of 8, so the
# 32-channel branch (gn_vw = 8) falls back to 4 channels per lane on the slabs of 8-channel lanes: 4 lanes per slab, 2 slabs
CAT_CHANNELS, CAT_GROUPS, CAT_B, CAT_SP = (32, 12), (2, 3), 2, (3, 5, 7)

# dual norm: (id, B, C, Ga, Gb, spatial, a_batch, b_batch, relu) -> lanes q and rows of gn2_partial_bwd_kernel, chunks x chunk_len
DualCase = namedtuple("DualCase", "id B C Ga Gb sp a_batch b_batch relu expect")
DUAL_CASES = [
    # one voxel row per workgroup, threads 160..255 idle
    DualCase("I-640", 2, 640, 2, 640, (1, 130, 1), False, True, True, dict(q=160, rows=1, chunks2=3, chunk_len2=64)),
    # q = 256: every thread a lane of the one row
    DualCase("I-1024", 1, 1024, 32, 32, (1, 70, 1), False, False, True, dict(q=256, rows=1, chunks2=2, chunk_len2=64)),
    # q = 3: 85 rows, thread 255 idle
    DualCase("I-12", 5, 12, 3, 12, (1, 110, 1), False, True, True, dict(q=3, rows=85, chunks2=2, chunk_len2=64)),
    DualCase("I-12-norelu", 5, 12, 3, 12, (1, 110, 1), False, True, False, dict(q=3, rows=85, chunks2=2, chunk_len2=64)),
]
DUAL_REFUSED = (1, 1028, 2, 1028, (1, 20, 1))          # C > 1024: dual_norm_supported refuses, the layer entry point falls back


def case_id(c):
    return c.id


def numel(c):
    n = c.B * c.C
    for s in c.sp:
        n *= s
    return n


def spatial(c):
    return numel(c) // (c.B * c.C)


def dims(c, relu=0, as_batch=False, ld_y=0, ld_gy=0):
    """ssbev_norm_dims of a case (as_batch: train-mode BatchNorm, the batch folded into S and one channel per group)."""
    B, S = (1, c.B * spatial(c)) if as_batch else (c.B, spatial(c))
    return capi.NormDims(B, c.C, c.C if as_batch else c.G, S, 1e-5, int(relu), 0, 1 if c.pre_act else 0, ld_y, ld_gy,
                         1 if c.dtype == "bf16" else 0)


def dual_dims(c, io=0):
    S = 1
    for s in c.sp:
        S *= s
    return capi.Norm2Dims(c.B, c.C, c.Ga, c.Gb, S, 1e-5, 1e-5, int(c.relu), int(c.a_batch), int(c.b_batch), io)


def query(d, aligned16=1):
    """The library's plan of a ssbev_norm_dims / ssbev_norm2_dims, or its error code."""
    p = capi.GroupnormPlan()
    single = isinstance(d, capi.NormDims)
    rc = capi.load().ssbev_groupnorm_plan_query(C.byref(d) if single else None, None if single else C.byref(d), aligned16, C.byref(p))
    return p if rc == capi.OK else rc


def plan_tuple(p):
    return tuple(getattr(p, n) for n, _ in capi.GroupnormPlan._fields_)


# ---- walk properties from the query's numbers ------------------------------------------------------------------------------------
def slab_widths(p, Cch):
    """Lanes of each channel slab (blockIdx.z of the statistics kernels)."""
    lanes = Cch // p.vw
    return [min(p.slab_q, lanes - z * p.slab_q) for z in range(p.slabs)]


def rows(q):
    return max(NT // q, 1)


def last_len(p, S):
    return S - (p.chunks - 1) * p.chunk_len


def main_loop_rows(length, q):
    """Rows r of a statistics workgroup that make at least one trip of the main loop on a chunk of `length` voxels: the loop
    runs while s0 + r + (UB - 1) * rows < s1."""
    return max(0, min(rows(q), length - (UB - 1) * rows(q)))


def finalize_batches(p, cpg):
    return -(-p.chunks * cpg // FIN_BATCH)


def trips(p, totalv):
    return -(-totalv // (p.blocks * NT))


def second_trip(p, totalv, per):
    """(vectors on the second trip, smallest, largest number of samples a thread moves ahead on it); per = vectors per sample."""
    stride = p.blocks * NT
    n = max(0, min(totalv - stride, stride))
    if n == 0:
        return None
    # sample(i + stride) - sample(i) is a step function of i: look at i = 0, n - 1 and at both sides of every sample boundary
    marks = {0, n - 1}
    for k in range(1, totalv // per + 2):
        for edge in (k * per, k * per - stride):
            marks.update(i for i in (edge - 1, edge) if 0 <= i < n)
    dist = [(i + stride) // per - i // per for i in marks]
    return n, min(dist), max(dist)


def properties(c, p, as_batch=False):
    """What `expect` lists, from a plan."""
    B, S = (1, c.B * spatial(c)) if as_batch else (c.B, spatial(c))
    G = c.C if as_batch else c.G
    totalv, q = B * S * (c.C // 4), c.C // 4
    first = min(S, p.chunk_len)
    return dict(vw=p.vw, slab_q=p.slab_q, slabs=p.slabs, chunks=p.chunks, chunk_len=p.chunk_len, last_len=last_len(p, S),
                main={w: main_loop_rows(first, w) for w in sorted(set(slab_widths(p, c.C)), reverse=True)},
                fin_batches=finalize_batches(p, c.C // G), lds_piv=c.C // G <= FIN_LDS_PIVOTS, blocks=p.blocks, fixed=p.fixed,
                trips=trips(p, totalv), trip2=second_trip(p, totalv, q * S))


# ---- a transcription of the geometry functions as they stood before the query was added ----------------------------------------
def _cdiv(a, b):
    return -(-a // b)


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def reference_apply_blocks(total4, q):
    blocks = min(_cdiv(total4, NT), 16384)
    m = q // _gcd(NT, q)
    if blocks >= m:
        blocks -= blocks % m
    return blocks if blocks > 0 else 1


def reference_plan(io, B, Cch, G, S, ld_y=0, ld_gy=0, aligned16=1):
    """gn_vw / gn_rows16 / make_geom / gn_slabs / apply_blocks of a single norm -> the fields of ssbev_groupnorm_plan."""
    vw_geom = 8 if io == 1 and Cch % 8 == 0 else 4
    rows16 = not ((ld_y != 0 and ld_y % 8 != 0) or (ld_gy != 0 and ld_gy % 8 != 0)) and bool(aligned16)
    vw = 8 if vw_geom == 8 and rows16 else 4
    slab_q = min(Cch // vw_geom, 8)
    slabs_geom = _cdiv(Cch // vw_geom, slab_q)
    chunks = max(STAT_BLOCKS // (B * slabs_geom), 1)
    length = max(_cdiv(S, chunks), 64)
    chunks = _cdiv(S, length)
    blocks = reference_apply_blocks(B * S * (Cch // 4), Cch // 4)
    return dict(vw=vw, slab_q=slab_q, slabs=_cdiv(Cch // vw, slab_q), chunks=chunks, chunk_len=length, blocks=blocks,
                fixed=int(blocks * NT % (Cch // 4) == 0))


def reference_plan2(io, B, Cch, Ga, Gb, S, a_batch, b_batch, aligned16=1):
    """The two-norm operator: side a's statistics as a single norm (gn2_side), side b's chunks, make_geom2's backward chunks."""
    sides = [reference_plan(io, 1 if batch else B, Cch, G, S * B if batch else S) for G, batch in ((Ga, a_batch), (Gb, b_batch))]
    vw = 8 if io == 1 and Cch % 8 == 0 and aligned16 else 4
    p = dict(sides[0], vw=vw, slabs=_cdiv(Cch // vw, sides[0]["slab_q"]))
    p["blocks"] = reference_apply_blocks(B * S * (Cch // 4), Cch // 4)
    p["fixed"] = int(p["blocks"] * NT % (Cch // 4) == 0)
    p["chunks_b"], p["chunk_len_b"] = sides[1]["chunks"], sides[1]["chunk_len"]
    chunks = max(STAT_BLOCKS // B, 1)
    length = max(_cdiv(S, chunks), 64)
    p["chunk_len2"], p["chunks2"] = length, _cdiv(S, length)
    return p
