"""The shapes of test_gpu_wgrad_paths.py and what each of them reaches in ssbev_conv_bwd_weight (csrc/conv_mfma.hip,
csrc/conv_thin_mfma.hip).

select_wgrad picks one of eight kinds; seven of them leave partial slabs [nchunks][taps][Cq][Cp] that launch_wgrad_reduce folds
with the stage, tiled or plain kernel, the thin-side kind has a fold of its own.  The mirrors below restate the planners'
arithmetic in plain Python where that is short; every constant in them is read from the .hip source by hand:

  conv_mfma.hip
    plan_wgrad_1x1       `(long)p.Cp * p.Cq > 128L * 128L` -> P1_MAX_CC; `std::max(16L, 8192 / tiles)` -> P1_WAVES_MIN, P1_WAVES;
                         `p.N / 256` -> P1_VOX; `(64L << 20)` -> P1_WS_CAP bytes; `(chunk + 15) & ~15L`; 16 waves per workgroup
    wgrad_1x1_kernel     `v0 += 2 * U`, U = 8 -> P1_STEP = 16 voxels per k-step group
    wgrad_cfg            the four <MQ, MP, TH, TW> tilings
    make_wgrad_geom      `3072 / tiles` -> DIRECT_WANT; `chunk < 256` -> DIRECT_MIN; `(chunk + 1) & ~1L`
    make_wgrad_cf_geom   `256L * (acc_regs > 128 ? 1 : (acc_regs > 64 ? 2 : 3))`; rounds 8 .. 1; `>= 512` -> CF_MIN; `(chunk + 31) & ~31L`;
                         `((Wi + 2 pw + 3) & ~3) + 4` -> padded row; `+ 16` floats of slack
    plan_wgrad_thin      kTapWseg = 32 -> TAP_WSEG; `1024L / g.nseg` -> THIN_WANT
    plan_wgrad_reduce    `nchunks >= 64 && total % 4 == 0`; `cdiv(2048, bx)`, bx = cdiv(total / 4, 256); `nchunks / 8`;
                         `taps <= 32 && cdiv(Cp, 32) * cdiv(Cq, 8) >= 128`
  conv_thin_mfma.hip
    make_wg_geom         `(nrows + 4607) / 4608` -> TS_ROWS; workspace slabs of mt = cdiv(27 nt, 32) tiles of 1024 floats
    wgrad_thinside_reduce_kernel   32 slices, two accumulators: `c + 32 < nchunks; c += 64`, then `if (c < nchunks)`

plan_wgrad_lds's search and chunk_groups_by_rounds (the Dh kind's gpc) are not mirrored: their answers come from
ssbev_conv_wgrad_plan_query and are pinned as each case's hand-written `expect`.  test_wgrad_plan.py holds the query to `expect`,
to the mirrors and to ssbev_conv_bwd_weight_workspace on a box without a GPU, and asserts that the properties listed in REQUIRED
are reached, as a set equality; test_gpu_wgrad_paths.py runs the cases against a float64 reference.

Size cap: no tensor of a case (x, gy, gw, the workspace) is larger than CAP = 4 M floats.  CAP_ONE = 9 M is allowed to at most
one case, listed in BIG_CASES, should a 1x1 shape need it to reach the stage fold (nchunks >= 64 needs 64 x 16 waves of >= 256
voxels); with 12 x 8 channels pw_stage stays within CAP, so BIG_CASES is empty.

Stage followed by the tiled fold (dir_stage_tiled): the tiled fold needs cdiv(Cp, 32) * cdiv(Cq, 8) >= 128, the stage fold 64
slabs.  A 1x1 layer of 124 -> 228 channels is too wide for the pointwise kernel, W % 4 != 0 keeps it off the channels-first one,
and on the Direct kind 3072 / 8 tiles = 384 wanted chunks of at least 256 voxels make 64 chunks of 16 129 voxels: 3.7 M floats
of gy.  Both channel counts are multiples of 4, so the wrappers hand the same dims to the library."""
import ctypes as C
from collections import namedtuple

from stereoscene_amd import capi

CAP = 4 << 20
CAP_ONE = 9 << 20
KINDS = ("Bf16Storage", "ThinSide", "Thin", "Pointwise", "Dh", "Lds", "ChannelsFirst", "Direct")
P1_MAX_CC, P1_WAVES_MIN, P1_WAVES, P1_VOX, P1_WS_CAP, P1_STEP = 128 * 128, 16, 8192, 256, 64 << 20, 16
DIRECT_WANT, DIRECT_MIN = 3072, 256
CF_MIN, CF_STEP = 512, 32
TAP_WSEG, THIN_WANT = 32, 1024
TS_ROWS = 4608


def cdiv(a, b):
    return -(-a // b)


def align256(n):
    return (n + 255) & ~255


# kd kh kw / stride / pad / dilation are triples; grid = input grid (D, H, W); op = output_padding (transposed only)
Case = namedtuple("Case", "id B Cin Cout grid k s p dl tr op hint lim props expect")


def out_grid(c):
    if c.tr:
        return tuple((n - 1) * s - 2 * p + dl * (k - 1) + op + 1 for n, k, s, p, dl, op in zip(c.grid, c.k, c.s, c.p, c.dl, c.op))
    return tuple((n + 2 * p - dl * (k - 1) - 1) // s + 1 for n, k, s, p, dl in zip(c.grid, c.k, c.s, c.p, c.dl))


def dims(c, precision=0):
    return capi.ConvDims(c.B, c.Cin, c.Cout, *c.grid, *out_grid(c), *c.k, *c.s, *c.p, *c.dl, c.tr, 0, 0, c.hint, precision)


PLAN_FIELDS = tuple(n for n, _ in capi.ConvWgradPlan._fields_)


def query(d):
    """ssbev_conv_wgrad_plan_query as a dict of its fields (host only)."""
    p = capi.ConvWgradPlan()
    rc = capi.load().ssbev_conv_wgrad_plan_query(C.byref(d), C.byref(p))
    assert rc == 0, rc
    return {n: int(getattr(p, n)) for n in PLAN_FIELDS}


def wshape(c):
    return ((c.Cin, c.Cout) if c.tr else (c.Cout, c.Cin)) + tuple(c.k)


def voxels(c):
    """(input voxels, output voxels) with the batch."""
    o = out_grid(c)
    return c.B * c.grid[0] * c.grid[1] * c.grid[2], c.B * o[0] * o[1] * o[2]


def largest_tensor(c, workspace_bytes):
    vi, vo = voxels(c)
    taps = c.k[0] * c.k[1] * c.k[2]
    return max(vi * c.Cin, vo * c.Cout, c.Cin * c.Cout * taps, workspace_bytes // 4)


# ---- mirrors ----------------------------------------------------------------------------------------------------------------------
def plan_wgrad_reduce(nchunks, taps, Cq, Cp):
    total = taps * Cq * Cp
    r = dict(two_stage=0, nsl=0, per=0)
    if nchunks >= 64 and total % 4 == 0:
        bx = cdiv(total // 4, 256)
        nsl = min(max(cdiv(2048, bx), 1), nchunks // 8)
        per = cdiv(nchunks, nsl)
        r = dict(two_stage=1, nsl=cdiv(nchunks, per), per=per)
    r["final"] = int(taps <= 32 and cdiv(Cp, 32) * cdiv(Cq, 8) >= 128)
    return r


def wgrad_cfg(Cp, Cq, kh, kw):
    if kh * kw == 1:
        return dict(MQ=2, MP=2, TH=1, TW=1)
    if Cp > 32 and Cq > 32:
        return dict(MQ=2, MP=2, TH=1, TW=3)
    if Cp <= 32 and Cq <= 32:
        return dict(MQ=1, MP=1, TH=3, TW=3)
    return dict(MQ=1, MP=1, TH=1, TW=3)


def _tiles(Cp, Cq, k, t):
    return cdiv(Cp, 32 * t["MP"]) * cdiv(Cq, 32 * t["MQ"]) * k[0] * cdiv(k[1], t["TH"]) * cdiv(k[2], t["TW"])


def plan_wgrad_1x1(c):
    Cp, Cq = (c.Cin, c.Cout) if c.tr else (c.Cout, c.Cin)
    N = voxels(c)[1]
    MQ, MP = (2 if Cq > 32 else 1), (2 if Cp > 32 else 1)
    tiles = cdiv(Cq, 32 * MQ) * cdiv(Cp, 32 * MP)
    waves = max(P1_WAVES_MIN, P1_WAVES // tiles)
    waves = min(waves, max(1, N // P1_VOX))
    waves = min(waves, max(1, P1_WS_CAP // (Cq * Cp * 4)))
    chunk = (cdiv(N, waves) + 15) & ~15
    return dict(MQ=MQ, MP=MP, chunk=chunk, nchunks=cdiv(cdiv(N, chunk), 16), Cq=Cq, Cp=Cp, taps=1)


def make_wgrad_geom(c):
    """The Direct kind: P is the tensor on the coarse grid."""
    Cp, Cq = (c.Cin, c.Cout) if c.tr else (c.Cout, c.Cin)
    M = voxels(c)[0] if c.tr else voxels(c)[1]
    t = wgrad_cfg(Cp, Cq, c.k[1], c.k[2])
    want = max(1, DIRECT_WANT // _tiles(Cp, Cq, c.k, t))
    chunk = (max(DIRECT_MIN, cdiv(M, want)) + 1) & ~1
    return dict(t, chunk=chunk, nchunks=cdiv(M, chunk), Cq=Cq, Cp=Cp, taps=c.k[0] * c.k[1] * c.k[2])


def make_wgrad_cf_geom(c):
    Cp, Cq = c.Cout, c.Cin
    N = voxels(c)[1]
    t = wgrad_cfg(Cp, Cq, c.k[1], c.k[2])
    tiles = _tiles(Cp, Cq, c.k, t)
    acc_regs = 16 * t["MQ"] * t["MP"] * t["TH"] * t["TW"]
    resident = 256 * (1 if acc_regs > 128 else (2 if acc_regs > 64 else 3))
    best = min(max(N // (4 * 512), 1), resident)
    for rounds in range(8, 0, -1):
        cb = resident * rounds // tiles
        if cb >= 1 and cdiv(N, 4 * cb) >= CF_MIN:
            best = cb
            break
    chunk = (max(CF_MIN, cdiv(N, 4 * best)) + 31) & ~31
    return dict(t, chunk=chunk, nchunks=cdiv(N, chunk), Cq=Cq, Cp=Cp, taps=c.k[0] * c.k[1] * c.k[2])


def cf_workspace(c, nchunks):
    D, H, W = c.grid
    taps = c.k[0] * c.k[1] * c.k[2]
    Wp = ((W + 2 * c.p[2] + 3) & ~3) + 4
    pt = align256(c.Cout * voxels(c)[1] * 4)
    qp = (c.Cin * c.B * (D + 2 * c.p[0]) * (H + 2 * c.p[1]) * Wp + 16) * 4
    return align256(nchunks * taps * c.Cin * c.Cout * 4) + pt + align256(qp)


def plan_wgrad_thin(c):
    D, H, W = c.grid
    nseg, NG = cdiv(W, TAP_WSEG), c.B * D * H
    nranges = min(max(1, THIN_WANT // nseg), NG)
    gpc = cdiv(NG, nranges)
    return dict(gpc=gpc, nseg=nseg, nchunks=cdiv(NG, gpc) * nseg, Cq=c.Cin, Cp=c.Cout, taps=27)


def make_wg_geom(c):
    """The thin-side kind."""
    nrows = c.B * c.grid[0] * c.grid[1]
    rpw = max(1, cdiv(nrows, TS_ROWS))
    return dict(rows_per_wave=rpw, nchunks=cdiv(nrows, rpw), nt=c.Cout if (c.Cin == 32 and c.Cout != 32) else c.Cin,
                Cq=c.Cin, Cp=c.Cout, taps=27)


def mirror(c, kind):
    """What the mirrored planners say about a case of `kind` (None for the kinds whose planner is a search)."""
    m = {"ThinSide": make_wg_geom, "Thin": plan_wgrad_thin, "Pointwise": plan_wgrad_1x1, "ChannelsFirst": make_wgrad_cf_geom,
         "Direct": make_wgrad_geom}.get(kind)
    return m(c) if m else None


def implied_workspace(c, plan):
    """Bytes ssbev_conv_bwd_weight_workspace must answer, from the plan's own numbers."""
    kind = KINDS[plan["kind"]]
    tile = c.Cin * c.Cout * 4
    slabs = plan["nchunks"] * plan["taps"] * tile
    if kind == "ThinSide":
        return plan["nchunks"] * cdiv(27 * plan["nt"], 32) * 1024 * 4
    if kind == "Dh":
        return align256(slabs) + align256(48 * tile)
    if kind == "ChannelsFirst":
        return cf_workspace(c, plan["nchunks"])
    return slabs if kind == "Direct" else align256(slabs)


# ---- what a plan reaches ----------------------------------------------------------------------------------------------------------
def reached(c, plan):
    """The property names of REQUIRED a case reaches, from its dims and its plan alone."""
    kind = KINDS[plan["kind"]]
    got = {kind}
    Cq, Cp, n = plan["Cq"], plan["Cp"], plan["nchunks"]
    vi, vo = voxels(c)
    if kind == "ThinSide":
        got.add("ThinSide:%d->%d" % (c.Cin, c.Cout))
        got.add("thinside_fold<=32" if n <= 32 else ("thinside_fold33..64" if n <= 64 else "thinside_fold>64"))
        if n > 64 and n % 2 == 1:
            got.add("thinside_fold>64_odd")
        if n % 4 != 0:
            got.add("thinside_early_return")
        if plan["rows_per_wave"] > 1:
            got.add("thinside_rows_per_wave>1")
            if (c.B * c.grid[0] * c.grid[1]) % plan["rows_per_wave"]:
                got.add("short_last_chunk")
        return got
    if kind == "Thin":
        got.add("Thin:Cin%d" % c.Cin if c.Cout != 3 else "Thin:Cin%d,Cout3" % c.Cin)
        NG = c.B * c.grid[0] * c.grid[1]
        if NG % plan["gpc"]:
            got.add("short_last_chunk")
    if kind == "Pointwise":
        got.add("Pointwise<%d,%d>%s" % (plan["MQ"], plan["MP"], "t" if c.tr else ""))
        waves = cdiv(vo, plan["chunk"])
        last = vo - (waves - 1) * plan["chunk"]
        if waves > 1 and last < plan["chunk"]:
            got.add("short_last_chunk")
        if last < P1_STEP:
            got.add("1x1_last_chunk<kstep")
        if waves % 16:
            got.add("1x1_empty_ranges")
        if Cp % 32 or Cq % 32:
            got.add("1x1_channel_clamp")
    if kind == "Dh":
        NG = c.B * (c.grid[0] // 2) * (c.grid[1] // 2)
        if NG % plan["gpc"]:
            got.add("short_last_chunk")
    if kind == "Lds":
        got.add("Lds:cfg%d" % plan["cfg"] + ({0: "", 1: "/wino", 2: "/wino_nks4"}[plan["instance"]] if plan["cfg"] == 1 else ""))
        got.add("Lds:kd%d" % c.k[0])
        if c.s[1] == 2:
            got.add("Lds:stride2t" if c.tr else "Lds:stride2")
        if plan["cfg"] == 1 and plan["instance"] == 0:
            got.add("Lds:plain_by_hint6" if c.hint == 6 else "Lds:plain_by_odd_RG")
        Dp, Hp = (c.grid if c.tr else out_grid(c))[:2]
        if (c.B * Dp * (Hp // plan["RG"])) % plan["gpc"]:
            got.add("short_last_chunk")
    if kind in ("ChannelsFirst", "Direct"):
        got.add("%s<%d,%d,%d,%d>" % (kind, plan["MQ"], plan["MP"], plan["TH"], plan["TW"]))
        got.add("tiling<%d,%d,%d,%d>" % (plan["MQ"], plan["MP"], plan["TH"], plan["TW"]))
        M = vi if c.tr else vo
        last = M - (n - 1) * plan["chunk"]
        if n > 1 and last < plan["chunk"]:
            got.add("short_last_chunk")
        if kind == "ChannelsFirst" and last < CF_STEP:
            got.add("cf_last_chunk<kstep")
        if max(c.dl) == 2:
            got.add("dilation2")
        if c.tr and c.k == (2, 2, 2) and c.s == (2, 2, 2):
            got.add("k2s2_transposed")
        if c.k == (1, 1, 1) and Cp * Cq > P1_MAX_CC:
            got.add("wide_1x1")
        if kind == "Direct" and out_grid(c)[2] % 4 and not c.tr and c.s == (1, 1, 1):
            got.add("W%4_keeps_off_Lds_and_ChannelsFirst")
        if Cq % (32 * plan["MQ"]) and Cp % (32 * plan["MP"]):
            got.add("tiled_kernel_row_and_column_guards")
    if Cq % 32 and Cq > 32 or Cp % 32 and Cp > 32 or Cq in (20, 36, 100, 132) or Cp in (20, 36, 100, 132):
        got.add("channels_fill_no_whole_tile")
    # the fold
    if plan["two_stage"]:
        got.add("fold_stage")
        if n % plan["per"]:
            got.add("fold_stage_short_last_slice")
        if plan["per"] % 8:
            got.add("fold_stage_per%8")
        if plan["final"]:
            got.add("fold_stage_then_tiled")
    elif n >= 64:
        got.add("fold_stage_skipped_total%4")
    got.add("fold_tiled" if plan["final"] else "fold_plain")
    if plan["final"] and Cp % 32 and Cq % 8:
        got.add("fold_tiled_edges")
    return got


REQUIRED = {
    # kinds and instances
    "ThinSide", "ThinSide:32->1", "ThinSide:32->2", "ThinSide:32->4", "ThinSide:1->32", "ThinSide:2->32", "ThinSide:4->32",
    "Thin", "Thin:Cin16", "Thin:Cin20", "Thin:Cin32,Cout3",
    "Pointwise", "Pointwise<1,1>", "Pointwise<1,2>", "Pointwise<2,1>", "Pointwise<2,2>", "Pointwise<1,1>t", "Pointwise<2,2>t",
    "Dh",
    "Lds", "Lds:cfg0", "Lds:cfg2", "Lds:cfg3", "Lds:cfg1", "Lds:cfg1/wino", "Lds:cfg1/wino_nks4", "Lds:plain_by_hint6",
    "Lds:kd1", "Lds:kd3", "Lds:stride2", "Lds:stride2t",
    "ChannelsFirst", "Direct", "tiling<2,2,1,1>", "tiling<2,2,1,3>", "tiling<1,1,3,3>", "tiling<1,1,1,3>",
    "dilation2", "k2s2_transposed", "wide_1x1", "W%4_keeps_off_Lds_and_ChannelsFirst",
    # channel edges
    "channels_fill_no_whole_tile", "1x1_channel_clamp", "tiled_kernel_row_and_column_guards",
    # chunk edges
    "short_last_chunk", "1x1_last_chunk<kstep", "cf_last_chunk<kstep", "1x1_empty_ranges", "thinside_early_return",
    "thinside_rows_per_wave>1",
    # folds
    "fold_plain", "fold_tiled", "fold_stage", "fold_stage_short_last_slice", "fold_stage_per%8", "fold_tiled_edges",
    "fold_stage_skipped_total%4", "fold_stage_then_tiled", "thinside_fold<=32", "thinside_fold33..64", "thinside_fold>64_odd",
}
# reached by cases, asked for by nobody: tolerated by the set equality of test_wgrad_plan.py
EXTRA_OK_PREFIXES = ("ChannelsFirst<", "Direct<", "thinside_fold>64", "Lds:plain_by_odd_RG")
UNREACHABLE = set()         # every path the coverage list names has a case

# lim: the exact regime draws x and gy from the integers -lim .. lim (test_wgrad_plan.py checks that this keeps every sum exact).
# props: what the case is there for -- test_wgrad_plan.py requires it to equal reached(case, plan).  expect: every non-zero field
# of the plan, written down from the query when the case was chosen.
CASES = [
    Case("ts_32to1", 1, 32, 1, (2, 5, 9), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:32->1 thinside_early_return thinside_fold<=32",
         dict(kind=1, nchunks=10, taps=27, Cq=32, Cp=1, rows_per_wave=1, nt=1, workspace=40960)),
    Case("ts_32to2", 1, 32, 2, (3, 15, 7), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:32->2 thinside_early_return thinside_fold33..64",
         dict(kind=1, nchunks=45, taps=27, Cq=32, Cp=2, rows_per_wave=1, nt=2, workspace=368640)),
    Case("ts_32to4", 1, 32, 4, (3, 33, 5), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:32->4 thinside_early_return thinside_fold>64 thinside_fold>64_odd",
         dict(kind=1, nchunks=99, taps=27, Cq=32, Cp=4, rows_per_wave=1, nt=4, workspace=1622016)),
    Case("ts_1to32", 1, 1, 32, (2, 6, 33), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:1->32 thinside_fold<=32",
         dict(kind=1, nchunks=12, taps=27, Cq=1, Cp=32, rows_per_wave=1, nt=1, workspace=49152)),
    Case("ts_2to32", 2, 2, 32, (3, 7, 6), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:2->32 thinside_early_return thinside_fold33..64",
         dict(kind=1, nchunks=42, taps=27, Cq=2, Cp=32, rows_per_wave=1, nt=2, workspace=344064)),
    Case("ts_4to32", 1, 4, 32, (5, 13, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:4->32 thinside_early_return thinside_fold>64 thinside_fold>64_odd",
         dict(kind=1, nchunks=65, taps=27, Cq=4, Cp=32, rows_per_wave=1, nt=4, workspace=1064960)),
    Case("ts_rows2", 1, 32, 1, (97, 48, 4), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ThinSide ThinSide:32->1 thinside_fold>64 thinside_rows_per_wave>1",
         dict(kind=1, nchunks=2328, taps=27, Cq=32, Cp=1, rows_per_wave=2, nt=1, workspace=9535488)),
    Case("thin_16", 1, 16, 4, (3, 5, 40), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 9, 2,
         "Thin Thin:Cin16 fold_plain",
         dict(kind=2, nchunks=30, taps=27, Cq=16, Cp=4, nseg=2, gpc=1, workspace=207360)),
    Case("thin_20", 1, 20, 2, (4, 7, 33), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 9, 2,
         "Thin Thin:Cin20 channels_fill_no_whole_tile fold_plain",
         dict(kind=2, nchunks=56, taps=27, Cq=20, Cp=2, nseg=2, gpc=1, workspace=241920)),
    Case("thin_32to3", 2, 32, 3, (3, 5, 70), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 9, 2,
         "Thin Thin:Cin32,Cout3 fold_plain fold_stage fold_stage_per%8",
         dict(kind=2, nchunks=90, taps=27, Cq=32, Cp=3, two_stage=1, nsl=10, per=9, nseg=3, gpc=1, workspace=933120)),
    Case("pw_11", 1, 32, 20, (5, 25, 37), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "1x1_channel_clamp 1x1_empty_ranges 1x1_last_chunk<kstep Pointwise Pointwise<1,1> channels_fill_no_whole_tile "
         "fold_plain short_last_chunk",
         dict(kind=3, nchunks=2, taps=1, Cq=32, Cp=20, MQ=1, MP=1, chunk=272, workspace=5120)),
    Case("pw_12", 1, 16, 36, (2, 9, 29), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "1x1_channel_clamp 1x1_empty_ranges Pointwise Pointwise<1,2> channels_fill_no_whole_tile fold_plain "
         "short_last_chunk",
         dict(kind=3, nchunks=1, taps=1, Cq=16, Cp=36, MQ=1, MP=2, chunk=272, workspace=2304)),
    Case("pw_21", 1, 100, 32, (3, 11, 17), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "1x1_channel_clamp 1x1_empty_ranges Pointwise Pointwise<2,1> channels_fill_no_whole_tile fold_plain "
         "short_last_chunk",
         dict(kind=3, nchunks=1, taps=1, Cq=100, Cp=32, MQ=2, MP=1, chunk=288, workspace=12800)),
    Case("pw_22", 2, 36, 100, (5, 9, 31), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "1x1_channel_clamp 1x1_empty_ranges Pointwise Pointwise<2,2> channels_fill_no_whole_tile fold_plain "
         "short_last_chunk",
         dict(kind=3, nchunks=1, taps=1, Cq=36, Cp=100, MQ=2, MP=2, chunk=288, workspace=14592)),
    Case("pw_11t", 1, 8, 24, (3, 7, 37), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 1, (0, 0, 0), 0, 2,
         "1x1_channel_clamp 1x1_empty_ranges Pointwise Pointwise<1,1>t fold_plain short_last_chunk",
         dict(kind=3, nchunks=1, taps=1, Cq=24, Cp=8, MQ=1, MP=1, chunk=272, workspace=768)),
    Case("pw_22t", 1, 128, 128, (4, 8, 33), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 1, (0, 0, 0), 0, 2,
         "1x1_empty_ranges Pointwise Pointwise<2,2>t fold_plain short_last_chunk",
         dict(kind=3, nchunks=1, taps=1, Cq=128, Cp=128, MQ=2, MP=2, chunk=272, workspace=65536)),
    Case("pw_stage", 1, 12, 8, (91, 23, 131), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 1,
         "1x1_channel_clamp 1x1_empty_ranges 1x1_last_chunk<kstep Pointwise Pointwise<1,1> fold_plain fold_stage "
         "short_last_chunk",
         dict(kind=3, nchunks=64, taps=1, Cq=12, Cp=8, two_stage=1, nsl=8, per=8, MQ=1, MP=1, chunk=272, workspace=24576)),
    Case("dh_small", 2, 16, 8, (6, 10, 40), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 9, 2,
         "Dh fold_plain",
         dict(kind=4, nchunks=60, taps=48, Cq=16, Cp=8, nseg=2, gpc=1, workspace=1499136)),
    Case("dh_stage", 1, 20, 28, (6, 26, 33), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 9, 2,
         "Dh channels_fill_no_whole_tile fold_plain fold_stage fold_stage_per%8 fold_stage_short_last_slice",
         dict(kind=4, nchunks=78, taps=48, Cq=20, Cp=28, two_stage=1, nsl=9, per=9, nseg=2, gpc=1, workspace=8494080)),
    Case("lds_cfg0", 1, 64, 36, (3, 6, 8), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg0 Lds:kd3 channels_fill_no_whole_tile fold_plain",
         dict(kind=5, nchunks=18, taps=27, Cq=64, Cp=36, Wseg=4, RG=2, nseg=2, gpc=1, nranges=9, ksplit=1, workspace=4478976)),
    Case("lds_cfg0_2d", 1, 100, 64, (1, 6, 12), (1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg0 Lds:kd1 channels_fill_no_whole_tile fold_plain",
         dict(kind=5, nchunks=9, taps=9, Cq=100, Cp=64, Wseg=4, RG=2, nseg=3, gpc=1, nranges=3, ksplit=1, workspace=2073600)),
    Case("lds_wino", 1, 32, 32, (2, 4, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg1/wino Lds:kd3 fold_plain",
         dict(kind=5, nchunks=8, taps=27, Cq=32, Cp=32, cfg=1, Wseg=16, RG=4, nseg=1, gpc=1, nranges=2, ksplit=4, instance=1, workspace=884736)),
    Case("lds_wino_nks4", 1, 32, 32, (1, 8, 32), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg1/wino_nks4 Lds:kd3 fold_plain",
         dict(kind=5, nchunks=8, taps=27, Cq=32, Cp=32, cfg=1, Wseg=32, RG=4, nseg=1, gpc=1, nranges=2, ksplit=4, instance=2, workspace=884736)),
    Case("lds_plain_hint6", 1, 32, 32, (2, 4, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 6, 2,
         "Lds Lds:cfg1 Lds:kd3 Lds:plain_by_hint6 fold_plain",
         dict(kind=5, nchunks=8, taps=27, Cq=32, Cp=32, cfg=1, Wseg=16, RG=4, nseg=1, gpc=1, nranges=2, ksplit=4, workspace=884736)),
    Case("lds_plain_oddrg", 1, 20, 28, (2, 5, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg1 Lds:kd3 Lds:plain_by_odd_RG channels_fill_no_whole_tile fold_plain",
         dict(kind=5, nchunks=40, taps=27, Cq=20, Cp=28, cfg=1, Wseg=16, RG=1, nseg=1, gpc=1, nranges=10, ksplit=4, workspace=2419200)),
    Case("lds_s2_cfg2", 1, 32, 64, (4, 8, 16), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg2 Lds:kd3 Lds:stride2 fold_plain",
         dict(kind=5, nchunks=4, taps=27, Cq=32, Cp=64, cfg=2, Wseg=8, RG=4, nseg=1, gpc=1, nranges=2, ksplit=2, workspace=884736)),
    Case("lds_s2_cfg3", 1, 64, 32, (4, 8, 16), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg3 Lds:kd3 Lds:stride2 fold_plain",
         dict(kind=5, nchunks=4, taps=27, Cq=64, Cp=32, cfg=3, Wseg=8, RG=2, nseg=1, gpc=1, nranges=4, ksplit=1, workspace=884736)),
    Case("lds_s2t_cfg2", 1, 64, 32, (2, 4, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 1, (1, 1, 1), 0, 2,
         "Lds Lds:cfg2 Lds:kd3 Lds:stride2t fold_plain",
         dict(kind=5, nchunks=4, taps=27, Cq=32, Cp=64, cfg=2, Wseg=8, RG=4, nseg=1, gpc=1, nranges=2, ksplit=2, workspace=884736)),
    Case("lds_s2t_cfg3", 1, 32, 64, (2, 4, 8), (3, 3, 3), (2, 2, 2), (1, 1, 1), (1, 1, 1), 1, (1, 1, 1), 0, 2,
         "Lds Lds:cfg3 Lds:kd3 Lds:stride2t fold_plain",
         dict(kind=5, nchunks=4, taps=27, Cq=64, Cp=32, cfg=3, Wseg=8, RG=2, nseg=1, gpc=1, nranges=4, ksplit=1, workspace=884736)),
    Case("lds_s2_2d", 2, 16, 36, (1, 8, 16), (1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Lds Lds:cfg2 Lds:kd1 Lds:stride2 channels_fill_no_whole_tile fold_plain",
         dict(kind=5, nchunks=4, taps=9, Cq=16, Cp=36, cfg=2, Wseg=8, RG=4, nseg=1, gpc=1, nranges=2, ksplit=2, workspace=82944)),
    Case("cf_1133", 1, 20, 28, (13, 5, 8), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 7, 2,
         "ChannelsFirst ChannelsFirst<1,1,3,3> cf_last_chunk<kstep channels_fill_no_whole_tile fold_plain short_last_chunk "
         "tiled_kernel_row_and_column_guards tiling<1,1,3,3>",
         dict(kind=6, nchunks=2, taps=27, Cq=20, Cp=28, MQ=1, MP=1, TH=3, TW=3, chunk=512, workspace=314112)),
    Case("cf_1113", 1, 36, 20, (5, 13, 8), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 7, 2,
         "ChannelsFirst ChannelsFirst<1,1,1,3> cf_last_chunk<kstep channels_fill_no_whole_tile fold_plain short_last_chunk "
         "tiled_kernel_row_and_column_guards tiling<1,1,1,3>",
         dict(kind=6, nchunks=2, taps=27, Cq=36, Cp=20, MQ=1, MP=1, TH=1, TW=3, chunk=512, workspace=439552)),
    Case("cf_2213", 1, 36, 100, (3, 11, 16), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 7, 2,
         "ChannelsFirst ChannelsFirst<2,2,1,3> cf_last_chunk<kstep channels_fill_no_whole_tile fold_plain short_last_chunk "
         "tiled_kernel_row_and_column_guards tiling<2,2,1,3>",
         dict(kind=6, nchunks=2, taps=27, Cq=36, Cp=100, MQ=2, MP=2, TH=1, TW=3, chunk=512, workspace=1213696)),
    Case("cf_dil2", 1, 16, 48, (6, 8, 12), (3, 3, 3), (1, 1, 1), (2, 2, 2), (2, 2, 2), 0, (0, 0, 0), 0, 2,
         "ChannelsFirst ChannelsFirst<1,1,1,3> channels_fill_no_whole_tile dilation2 fold_plain short_last_chunk "
         "tiled_kernel_row_and_column_guards tiling<1,1,1,3>",
         dict(kind=6, nchunks=2, taps=27, Cq=16, Cp=48, MQ=1, MP=1, TH=1, TW=3, chunk=512, workspace=430336)),
    Case("cf_wide1x1", 1, 252, 100, (2, 8, 16), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "ChannelsFirst ChannelsFirst<2,2,1,1> channels_fill_no_whole_tile fold_tiled fold_tiled_edges "
         "tiled_kernel_row_and_column_guards tiling<2,2,1,1> wide_1x1",
         dict(kind=6, nchunks=1, taps=1, Cq=252, Cp=100, final=1, MQ=2, MP=2, TH=1, TW=1, chunk=512, workspace=526080)),
    Case("dir_1133", 1, 20, 12, (3, 9, 31), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<1,1,3,3> W%4_keeps_off_Lds_and_ChannelsFirst channels_fill_no_whole_tile fold_plain "
         "short_last_chunk tiled_kernel_row_and_column_guards tiling<1,1,3,3>",
         dict(kind=7, nchunks=4, taps=27, Cq=20, Cp=12, MQ=1, MP=1, TH=3, TW=3, chunk=256, workspace=103680)),
    Case("dir_1113", 2, 36, 8, (3, 7, 29), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<1,1,1,3> W%4_keeps_off_Lds_and_ChannelsFirst channels_fill_no_whole_tile fold_plain "
         "short_last_chunk tiled_kernel_row_and_column_guards tiling<1,1,1,3>",
         dict(kind=7, nchunks=5, taps=27, Cq=36, Cp=8, MQ=1, MP=1, TH=1, TW=3, chunk=256, workspace=155520)),
    Case("dir_2213", 1, 36, 100, (3, 7, 13), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<2,2,1,3> W%4_keeps_off_Lds_and_ChannelsFirst channels_fill_no_whole_tile fold_plain "
         "short_last_chunk tiled_kernel_row_and_column_guards tiling<2,2,1,3>",
         dict(kind=7, nchunks=2, taps=27, Cq=36, Cp=100, MQ=2, MP=2, TH=1, TW=3, chunk=256, workspace=777600)),
    Case("dir_wide1x1", 1, 252, 100, (2, 8, 15), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<2,2,1,1> W%4_keeps_off_Lds_and_ChannelsFirst channels_fill_no_whole_tile fold_tiled "
         "fold_tiled_edges tiled_kernel_row_and_column_guards tiling<2,2,1,1> wide_1x1",
         dict(kind=7, nchunks=1, taps=1, Cq=252, Cp=100, final=1, MQ=2, MP=2, TH=1, TW=1, chunk=256, workspace=100800)),
    Case("dir_k2s2t", 2, 32, 16, (3, 4, 6), (2, 2, 2), (2, 2, 2), (0, 0, 0), (1, 1, 1), 1, (0, 0, 0), 0, 2,
         "Direct Direct<1,1,3,3> fold_plain k2s2_transposed tiling<1,1,3,3>",
         dict(kind=7, nchunks=1, taps=8, Cq=16, Cp=32, MQ=1, MP=1, TH=3, TW=3, chunk=256, workspace=16384)),
    Case("dir_stage", 1, 4, 8, (9, 41, 45), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<1,1,3,3> W%4_keeps_off_Lds_and_ChannelsFirst fold_plain fold_stage fold_stage_per%8 "
         "fold_stage_short_last_slice short_last_chunk tiled_kernel_row_and_column_guards tiling<1,1,3,3>",
         dict(kind=7, nchunks=65, taps=27, Cq=4, Cp=8, two_stage=1, nsl=8, per=9, MQ=1, MP=1, TH=3, TW=3, chunk=256, workspace=224640)),
    Case("dir_total_odd", 1, 3, 5, (9, 41, 45), (3, 3, 3), (1, 1, 1), (1, 1, 1), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<1,1,3,3> W%4_keeps_off_Lds_and_ChannelsFirst fold_plain fold_stage_skipped_total%4 "
         "short_last_chunk tiled_kernel_row_and_column_guards tiling<1,1,3,3>",
         dict(kind=7, nchunks=65, taps=27, Cq=3, Cp=5, MQ=1, MP=1, TH=3, TW=3, chunk=256, workspace=105300)),
    Case("dir_stage_tiled", 1, 124, 228, (1, 127, 127), (1, 1, 1), (1, 1, 1), (0, 0, 0), (1, 1, 1), 0, (0, 0, 0), 0, 2,
         "Direct Direct<2,2,1,1> W%4_keeps_off_Lds_and_ChannelsFirst channels_fill_no_whole_tile fold_stage "
         "fold_stage_then_tiled fold_tiled fold_tiled_edges short_last_chunk tiled_kernel_row_and_column_guards "
         "tiling<2,2,1,1> wide_1x1",
         dict(kind=7, nchunks=64, taps=1, Cq=124, Cp=228, two_stage=1, nsl=8, per=8, final=1, MQ=2, MP=2, TH=1, TW=1, chunk=256,
              workspace=7237632)),
]
# What the autograd wrappers hand to the library where a channel count is no multiple of 4 (they pad it; the thin-side kind takes
# the tensors as they are): id -> (Cin, Cout, kind, two_stage) of the padded problem.
AUTOGRAD_PADDED = {
    "thin_20": (20, 4, "Thin", 0),
    "thin_32to3": (32, 4, "Thin", 1),
    "dir_total_odd": (4, 8, "Direct", 1),
}
BIG_CASES = set()          # no case needs CAP_ONE: the stage fold is reached by a 1x1 layer of 12 x 8 channels within CAP
BY_ID = {c.id: c for c in CASES}


# ---- inputs and the float64 reference (shared by the CPU plan test and the GPU parity test) ---------------------------------------
def shapes(c):
    """Logical shapes of x [B, Cin, D, H, W] and gy [B, Cout, Do, Ho, Wo]."""
    return (c.B, c.Cin) + tuple(c.grid), (c.B, c.Cout) + out_grid(c)


def exact_inputs(c):
    """x, gy as fp32 tensors of hashed integers in -lim .. lim: every product and partial sum is an integer in any order."""
    import torch
    from stereoscene_amd import synthetic as S
    xs, gs = shapes(c)
    lim = c.lim + 0.4999
    return (torch.round(S.hash_uniform(f"wg/{c.id}/xi", xs, -lim, lim)), torch.round(S.hash_uniform(f"wg/{c.id}/gi", gs, -lim, lim)))


def boundary_voxels(c, plan):
    """(b, d, h, w) on the coarse grid (the grid of P: gy, or x of a transposed layer) of four voxels: the first, the last, the
    last of the first chunk and the first of the last chunk, in the order the kind of `plan` deals its chunks out.

    Pointwise (per wave), ChannelsFirst, Direct: `chunk` consecutive voxels.  ThinSide: rows_per_wave whole rows.  Thin, Lds, Dh:
    chunk = (row range, w-segment), chunk id = range * nseg + segment; a range is gpc consecutive row groups in (b, d, h) order,
    a group one row (Thin), RG rows along h (Lds) or a 2 x 2 block of rows in d and h (Dh); a segment is 32 (Thin, Dh) or Wseg
    (Lds) voxels wide."""
    kind = KINDS[plan["kind"]]
    D, H, W = c.grid if c.tr else out_grid(c)
    N = c.B * D * H * W
    first, last = (0, 0, 0, 0), (c.B - 1, D - 1, H - 1, W - 1)
    if kind in ("Pointwise", "ChannelsFirst", "Direct", "ThinSide"):
        ch = plan["rows_per_wave"] * W if kind == "ThinSide" else plan["chunk"]
        lin = lambda v: (v // (W * H * D), v // (W * H) % D, v // W % H, v % W)
        return [first, last, lin(min(ch, N) - 1), lin((N - 1) // ch * ch)]
    rd, rh, segw = {"Thin": (1, 1, TAP_WSEG), "Dh": (2, 2, TAP_WSEG), "Lds": (1, plan["RG"], plan["Wseg"])}[kind]
    Dg, Hg = D // rd, H // rh
    NG, gpc = c.B * Dg * Hg, plan["gpc"]
    group = lambda g: (g // (Hg * Dg), g // Hg % Dg, g % Hg)
    b0, d0, h0 = group(min(gpc, NG) - 1)
    b1, d1, h1 = group((cdiv(NG, gpc) - 1) * gpc)
    return [first, last, (b0, d0 * rd + rd - 1, h0 * rh + rh - 1, min(segw, W) - 1), (b1, d1 * rd, h1 * rh, (plan["nseg"] - 1) * segw)]


def indicator_inputs(c, plan):
    """The exact inputs with the coarse-grid tensor (gy; x of a transposed layer, whose chunks run over x) non-zero (1 .. lim, by
    channel, alternating sign) at the four boundary_voxels only.  Taps that fall into the padding there must come out exactly 0."""
    import torch
    x, gy = exact_inputs(c)
    src = x if c.tr else gy
    ind = torch.zeros_like(src)
    vals = (torch.arange(src.shape[1]) % c.lim + 1).float()
    for i, (b, d, h, w) in enumerate(sorted(set(boundary_voxels(c, plan)))):
        ind[b, :, d, h, w] = vals if i % 2 == 0 else -vals
    return (ind, gy) if c.tr else (x, ind)


def reference(c, x, gy):
    """float64 weight gradient in the torch layout: autograd of TF.conv3d / TF.conv_transpose3d on the CPU."""
    import torch
    import torch.nn.functional as TF
    w = torch.zeros(wshape(c), dtype=torch.float64, requires_grad=True)
    xd = x.double()
    y = TF.conv_transpose3d(xd, w, None, c.s, c.p, c.op, 1, c.dl) if c.tr else TF.conv3d(xd, w, None, c.s, c.p, c.dl)
    y.backward(gy.double())
    return w.grad.detach()


def summed_voxels(c):
    """Terms of one element of the weight gradient: the voxels of the coarse grid (taps in the padding contribute zeros)."""
    vi, vo = voxels(c)
    return vi if c.tr else vo


def wino_axes(c, plan):
    """Axes (2 = d, 3 = h of a [B, C, D, H, W] tensor) along which the kind accumulates in the F(2,3) domain."""
    kind = KINDS[plan["kind"]]
    if kind == "Dh":
        return (2, 3)
    if kind == "Lds" and plan["instance"] in (1, 2):
        return (3,)
    return ()


def wino_abs_bound(c, x, gy, axes):
    """A of the Winograd-domain kinds: the expression those kernels evaluate, on absolute values, in float64.

    F(2,3) along one axis: gw = G^T sum_tiles (A dy) * (B^T d), with A dy = (y0, y0 + y1, y0 - y1, -y1) of an output pair,
    B^T d = (d0 - d2, d1 + d2, d2 - d1, d1 - d3) of the four input rows around it and G^T = ((1, 1/2, 1/2, 0), (0, 1/2, -1/2, 0),
    (0, 1/2, 1/2, 1)).  With |.| on every operand and + for every sign this bounds the magnitude of everything the kernel adds
    up: (|y0|, |y0| + |y1|, |y0| + |y1|, |y1|) x (|d0| + |d2|, |d1| + |d2|, |d1| + |d2|, |d1| + |d3|), summed over the tiles by a
    weight gradient with a 1-tap kernel along the transformed axis, then |G^T|.  Two axes nest."""
    import itertools
    import torch
    import torch.nn.functional as TF
    xa, ga = x.double().abs(), gy.double().abs()

    def tf_y(t, ax):
        y0, y1 = t.index_select(ax, torch.arange(0, t.shape[ax], 2)), t.index_select(ax, torch.arange(1, t.shape[ax], 2))
        return [y0, y0 + y1, y0 + y1, y1]

    def tf_d(t, ax):
        pad = [0, 0] * (4 - ax) + [1, 1]
        tp = TF.pad(t, pad)
        n = t.shape[ax] // 2
        d = [tp.index_select(ax, torch.arange(j, j + 2 * n, 2)) for j in range(4)]
        return [d[0] + d[2], d[1] + d[2], d[1] + d[2], d[1] + d[3]]

    ys, ds = {(): ga}, {(): xa}
    for ax in axes:
        ys = {k + (i,): v for k, t in ys.items() for i, v in enumerate(tf_y(t, ax))}
        ds = {k + (i,): v for k, t in ds.items() for i, v in enumerate(tf_d(t, ax))}
    kk = tuple(1 if a + 2 in axes else 3 for a in range(3))
    pp = tuple(0 if a + 2 in axes else 1 for a in range(3))
    U = {}
    for key in itertools.product(range(4), repeat=len(axes)):
        w = torch.zeros((c.Cout, c.Cin) + kk, dtype=torch.float64, requires_grad=True)
        TF.conv3d(ds[key], w, None, 1, pp).backward(ys[key])
        U[key] = w.grad.detach()
    # |G^T| along every transformed axis: [..., 4, ...] -> [..., 3, ...]
    out = torch.stack([U[key] for key in itertools.product(range(4), repeat=len(axes))], 0)
    out = out.view((4,) * len(axes) + (c.Cout, c.Cin) + kk)
    for _ in axes:
        u0, u1, u2, u3 = out[0], out[1], out[2], out[3]
        h = 0.5 * (u1 + u2)
        out = torch.stack([u0 + h, h, h + u3], -1)             # the finished axis goes last; the next axis is now in front
    # out: [Cout, Cin, kd', kh', kw', (k of each axis, in order)] -> torch layout [Cout, Cin, 3, 3, 3]
    if axes == (3,):
        return out[:, :, :, 0, :, :].permute(0, 1, 2, 4, 3).contiguous()      # [co, ci, kd, kw, kh] -> [co, ci, kd, kh, kw]
    return out[:, :, 0, 0, :, :, :].permute(0, 1, 3, 4, 2).contiguous()      # [co, ci, kw, kd, kh] -> [co, ci, kd, kh, kw]
