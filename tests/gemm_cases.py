"""Case table of the GEMM family's path tests (test_gemm_plan.py on the CPU, test_gpu_gemm_paths.py on the GPU).

csrc/gemm.hip chooses among five tile configurations of gemm_nn_kernel (each with or without split-K and its gemm_sum_kernel
pass), three instantiations of gemm_tn_kernel and five of gemm_tn_skinny_kernel.  Each case below is the smallest shape found
that reaches one of those paths with the tails, chunk shapes and strides it is listed for; the expected plan is what
``ssbev_gemm_plan_query`` -- the plan function the launchers read -- answers, so test_gemm_plan.py notices on a box without a GPU
when a cost constant moves a case to another kernel, and the GPU tests cannot lose this coverage quietly.

Shapes are ``(batch, M, K, N)``; for TN, M is the number of reduction rows R and the result is ``[batch][K][N]``.  cfg 4 of
gemm_nn_kernel (16-deep k stages) is reachable in a tuning build only and has no case.

``reference_plan`` is a transcription of the dispatch as it stood before the plan functions existed (pick_wn, pick_bm,
nn_cfg_cost, nn_chunks, tn_chunks, tn_chunks_model, tn_wide, tn_skinny*): test_gemm_plan.py compares the query with it on random
problems."""
import collections
import ctypes as C

from stereoscene_amd import capi

NN, NT, TN = 0, 1, 2
FORM_NAMES = {NN: "nn", NT: "nt", TN: "tn"}

# kernel codes of ssbev_gemm_plan.kernel (include/ssbev.h)
CFG_128x128, CFG_128x64, CFG_192x128, CFG_128x160, CFG_BK16 = 0, 1, 2, 3, 4
TN_1, TN_2, TN_WIDE = 10, 11, 12
SK_11, SK_12, SK_21, SK_22, SK_QUAD = 20, 21, 22, 23, 24
ALL_KERNELS = {NN: {0, 1, 2, 3}, NT: {0, 1, 2, 3}, TN: {10, 11, 12, 20, 21, 22, 23, 24}}       # cfg 4: tuning builds only

# ---- property tags.  The first group follows from the plan and the shape (plan_props below recomputes it from the query) ...
SPLIT = "split"                    # nchunk > 1: partials + gemm_sum_kernel (NN / NT split-K, TN row chunks)
SHORT_LAST = "short_last_chunk"    # NN / NT: the last split-K chunk has fewer k stages than the others
CAP16 = "chunk_cap_16"             # NN / NT: nchunk is the cap of 16
EMPTY_CHUNK = "empty_chunk"        # TN: a row chunk lies entirely beyond the last row
EMPTY_RUN = "empty_run"            # skinny TN: the last wave run lies entirely beyond the last row
ROW_TAIL = "row_tail"              # NN / NT: M is no multiple of the tile's rows; TN: K is no multiple of 128
COL_TAIL = "col_tail"              # N is no multiple of the tile's columns
K_TAIL = "k_tail"                  # NN / NT: K % 32 != 0; TN: rows per chunk / run do not divide into whole stages
BATCHED = "batched"                # batch > 1
PLAN_PROPS = {SPLIT, SHORT_LAST, CAP16, EMPTY_CHUNK, EMPTY_RUN, ROW_TAIL, COL_TAIL, K_TAIL, BATCHED}
# ... the second group says how the case is run
SHARED_B = "shared_b"              # sb = 0: one B for every batch element (the BRI products)
SUM_EPILOGUE = "bias_relu_in_sum"  # split-K with bias and ReLU: both are applied by gemm_sum_kernel
STRIDED = "strided_operands"       # lda, ldb larger than the dense row
STRIDED_C = "strided_c"            # NN / NT: ldc > N and sc > M * ldc, into a NaN-filled buffer
EP_MUL = "ep_mul"                  # TN: fused C = ep_mul * (A^T B - ep_rowsub) epilogue
BOUNDARY = "skinny_boundary"       # TN: 32768 rows (skinny) next to 32767 (tiled)
RUN_PROPS = {SHARED_B, SUM_EPILOGUE, STRIDED, STRIDED_C, EP_MUL, BOUNDARY}

Case = collections.namedtuple("Case", "form shape pad kernel nchunk per_chunk props")
# pad = (lda - dense, ldb - dense, ldc - N, sc - M * ldc): all zero for dense operands


def case_id(c):
    b, m, k, n = c.shape
    tags = "".join("-" + t for t in sorted(c.props & RUN_PROPS))
    return f"{FORM_NAMES[c.form]}-{b}x{m}x{k}x{n}{tags}"


def _both(shape_mnkb, kernel, nchunk, per_chunk, props=(), pad=(0, 0, 0, 0)):
    M, N, K, batch = shape_mnkb
    return [Case(f, (batch, M, K, N), pad, kernel, nchunk, per_chunk, frozenset(props)) for f in (NN, NT)]


def _tn(shape_rknb, kernel, nchunk, per_chunk, props=(), pad=(0, 0, 0, 0)):
    R, K, N, batch = shape_rknb
    return [Case(TN, (batch, R, K, N), pad, kernel, nchunk, per_chunk, frozenset(props))]


PADS = (8, 12, 5, 7)         # lda + 8, ldb + 12, ldc = N + 5 (odd: C is stored float by float), sc = M * ldc + 7

CASES = (
    # ---------------------------------------------------------------------------------------------- NN / NT, (M, N, K, batch)
    # cfg 0, 128 x 128: row tail (1900 = 14 x 128 + 108) and k tail (36 = 32 + 4), two stages, no split
    _both((1900, 640, 36, 2), CFG_128x128, 1, 2, {ROW_TAIL, K_TAIL, BATCHED})
    + _both((1900, 640, 36, 2), CFG_128x128, 1, 2, {ROW_TAIL, K_TAIL, BATCHED, STRIDED, STRIDED_C}, PADS)
    # cfg 0 split-K: 49 stages in 3 chunks of 17 (last 15, ending in a 4-wide k tail); bias + ReLU land in the sum pass
    + _both((1900, 640, 1540, 2), CFG_128x128, 3, 17, {ROW_TAIL, K_TAIL, BATCHED, SPLIT, SHORT_LAST, SUM_EPILOGUE})
    + _both((1900, 640, 1540, 2), CFG_128x128, 3, 17,
            {ROW_TAIL, K_TAIL, BATCHED, SPLIT, SHORT_LAST, SUM_EPILOGUE, STRIDED, STRIDED_C}, PADS)
    # cfg 2, 192 x 128 (MW = 3): the row tail (190) falls inside the third 32-row tile of the second wave row; shared and own B
    + _both((190, 7680, 36, 3), CFG_192x128, 1, 2, {ROW_TAIL, K_TAIL, BATCHED, SHARED_B})
    + _both((190, 7680, 36, 3), CFG_192x128, 1, 2, {ROW_TAIL, K_TAIL, BATCHED})
    + _both((190, 7680, 2052, 1), CFG_192x128, 4, 17, {ROW_TAIL, K_TAIL, SPLIT, SHORT_LAST, SUM_EPILOGUE})
    # cfg 3, 128 x 160 (four waves stacked along M): row tail, column tail inside a 160-wide tile (636 = 3 x 160 + 156)
    + _both((1541, 636, 36, 4), CFG_128x160, 1, 2, {ROW_TAIL, COL_TAIL, K_TAIL, BATCHED})
    + _both((1541, 636, 2052, 2), CFG_128x160, 4, 17, {ROW_TAIL, COL_TAIL, K_TAIL, BATCHED, SPLIT, SHORT_LAST, SUM_EPILOGUE})
    # cfg 1, 128 x 64: a column tail narrower than one 32-column fragment
    + _both((130, 20, 36, 1), CFG_128x64, 1, 2, {ROW_TAIL, COL_TAIL, K_TAIL})
    # cfg 1 split in two: 33 stages = 17 + 16, the last one 4 wide
    + _both((190, 100, 1028, 1), CFG_128x64, 2, 17, {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT, SHORT_LAST, SUM_EPILOGUE})
    + _both((190, 100, 1028, 1), CFG_128x64, 2, 17,
            {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT, SHORT_LAST, SUM_EPILOGUE, STRIDED, STRIDED_C}, PADS)
    # cfg 1 at the chunk cap: 257 stages in 16 chunks of 17, the last chunk two stages
    + _both((100, 128, 8200, 1), CFG_128x64, 16, 17, {ROW_TAIL, K_TAIL, SPLIT, SHORT_LAST, CAP16, SUM_EPILOGUE})
    # ---------------------------------------------------------------------------------------------- TN, (R, K, N, batch)
    + _tn((520, 200, 72, 1), TN_2, 2, 288, {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT})
    + _tn((4100, 36, 8, 3), TN_1, 16, 288, {ROW_TAIL, COL_TAIL, K_TAIL, BATCHED, SPLIT, EMPTY_CHUNK})       # chunk 15 starts at row 4320
    + _tn((5000, 128, 128, 1), TN_2, 19, 288, {K_TAIL, SPLIT, EMPTY_CHUNK})
    + _tn((1030, 260, 320, 8), TN_WIDE, 4, 288, {ROW_TAIL, K_TAIL, BATCHED, SPLIT})
    + _tn((700, 128, 160, 9), TN_WIDE, 2, 352, {K_TAIL, BATCHED, SPLIT})
    + _tn((700, 128, 160, 9), TN_WIDE, 2, 352, {K_TAIL, BATCHED, SPLIT, STRIDED}, (8, 12, 0, 0))
    # fused epilogue (one chunk): K and N tails on the 128 x 64 and on the 128 x 128 tile
    + _tn((1000, 100, 40, 2), TN_1, 1, 1024, {ROW_TAIL, COL_TAIL, K_TAIL, BATCHED, EP_MUL})
    + _tn((1000, 200, 100, 1), TN_2, 1, 1024, {ROW_TAIL, COL_TAIL, K_TAIL, EP_MUL})
    # ---------------------------------------------------------------------------------------------- skinny TN
    + _tn((33000, 32, 32, 1), SK_11, 32, 258, {K_TAIL, SPLIT})
    + _tn((32771, 32, 64, 1), SK_12, 32, 258, {K_TAIL, SPLIT})
    + _tn((32770, 36, 20, 2), SK_21, 32, 258, {ROW_TAIL, COL_TAIL, K_TAIL, BATCHED, SPLIT})                 # K N = 720: no multiple of 64
    + _tn((33001, 64, 36, 1), SK_22, 32, 258, {COL_TAIL, K_TAIL, SPLIT})
    + _tn((33001, 64, 36, 1), SK_22, 32, 258, {COL_TAIL, K_TAIL, SPLIT, STRIDED}, (8, 12, 0, 0))
    + _tn((33001, 100, 36, 1), SK_QUAD, 128, 258, {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT})
    + _tn((40001, 128, 128, 2), SK_QUAD, 156, 258, {K_TAIL, BATCHED, SPLIT})
    # the boundary: 32768 rows stream through the skinny kernel, one row fewer runs the tiled one (127 chunks of 288, 13 empty)
    + _tn((32768, 64, 32, 1), SK_21, 32, 256, {SPLIT, BOUNDARY})
    + _tn((32767, 64, 32, 1), TN_1, 127, 288, {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT, EMPTY_CHUNK, BOUNDARY})
    + _tn((131073, 68, 68, 1), SK_QUAD, 512, 258, {ROW_TAIL, COL_TAIL, K_TAIL, SPLIT, EMPTY_RUN})           # run 511 starts at row 131838
)

# the ten shapes of test_gpu_kernels.py::test_gemm_nn_nt_tn_vs_torch, (batch, M, K, N)
LEGACY_SHAPES = ((1, 300, 128, 96), (1, 7680, 3200, 640), (3, 200, 64, 160), (1, 130, 36, 20), (2, 1920, 640, 640),
                 (1, 64, 192, 7680), (1, 40000, 32, 64), (2, 33000, 64, 36), (1, 34000, 128, 100), (1, 33000, 96, 128))


def dense_ld(form, shape):
    """(lda, ldb) of dense operands."""
    _, M, K, N = shape
    return (K, K if form == NT else N)


FAKE = 256           # a non-null pointer for host-side queries: never dereferenced


def dims(form, shape, pad=(0, 0, 0, 0), shared_b=False, relu=0, ep=None):
    """ssbev_gemm_dims of a case (operand layouts as the kernels read them: NN b [K][ldb], NT w [N][ldb], TN a [R][lda] b [R][ldb]);
    ep = (ep_mul, ep_rowsub) device addresses of the fused TN epilogue."""
    batch, M, K, N = shape
    lda, ldb = (x + p for x, p in zip(dense_ld(form, shape), pad[:2]))
    b_rows = N if form == NT else (M if form == TN else K)
    if form == TN:
        ldc, sc = N, K * N
    else:
        ldc = N + pad[2]
        sc = M * ldc + pad[3]
    sa = M * lda + (pad[0] and 8)
    sb = 0 if shared_b else b_rows * ldb + (pad[1] and 4)
    ep_mul, ep_rowsub = ep or (None, None)
    return capi.GemmDims(M, N, K, batch, lda, ldb, ldc, sa, sb, sc, relu, 0, 0, 0, 0, 0, 0, 0, None, ep_mul, ep_rowsub)


def case_dims(c, relu=0, ep=None):
    if EP_MUL in c.props and ep is None:
        ep = (FAKE, FAKE)
    return dims(c.form, c.shape, c.pad, SHARED_B in c.props, relu, ep)


def query(d, form):
    """ssbev_gemm_plan of dims d, or the error code."""
    p = capi.GemmPlan()
    rc = capi.load().ssbev_gemm_plan_query(C.byref(d), form, C.byref(p))
    return p if rc == capi.OK else rc


def workspace(d, form):
    lib = capi.load()
    fn = (lib.ssbev_gemm_nn_workspace, lib.ssbev_gemm_nt_workspace, lib.ssbev_gemm_tn_workspace)[form]
    return fn(C.byref(d))


def plan_tuple(p):
    return (p.kernel, p.bm, p.bn, p.bk, p.nchunk, p.per_chunk, p.grid, p.workspace)


def plan_props(form, shape, p):
    """The PLAN_PROPS a launch with plan p has, from the definitions in words."""
    batch, M, K, N = shape
    props = set()
    if batch > 1:
        props.add(BATCHED)
    if p.nchunk > 1:
        props.add(SPLIT)
    if form != TN:
        nst = -(-K // p.bk)
        if p.nchunk > 1 and nst - (p.nchunk - 1) * p.per_chunk < p.per_chunk:
            props.add(SHORT_LAST)
        if p.nchunk == 16:
            props.add(CAP16)
        if M % p.bm:
            props.add(ROW_TAIL)
        if N % p.bn:
            props.add(COL_TAIL)
        if K % p.bk:
            props.add(K_TAIL)
        return props
    skinny = p.kernel >= SK_11
    runs = p.nchunk * (4 if SK_11 <= p.kernel <= SK_22 else 1)
    rows = [min(M, (i + 1) * p.per_chunk) - i * p.per_chunk for i in range(runs)]       # rows of every chunk / wave run
    if any(r <= 0 for r in rows):
        props.add(EMPTY_RUN if skinny else EMPTY_CHUNK)
    if any(r > 0 and r % p.bk for r in rows):        # a last stage (32 rows; skinny: 16 rows per step) that is not full
        props.add(K_TAIL)
    if K % p.bm:
        props.add(ROW_TAIL)
    if N % p.bn:
        props.add(COL_TAIL)
    return props


# ------------------------------------------------------------------------------------------------------------------------
# transcription of the dispatch before ssbev_gemm_plan_query (every `/` of the C source is on non-negative ints: `//`)
def _pick_wn(N, tap_width=0):
    pad2, pad1 = (N + 127) // 128 * 128 - N, (N + 63) // 64 * 64 - N
    if tap_width and tap_width % 128 != 0:
        return 1
    return 2 if pad2 <= pad1 else 1


def _tn_chunks_model(M, batch, tiles):
    cmax = min(16, max(1, M // 256))
    best, best_cost = 1, 1e300
    for c in range(1, cmax + 1):
        per_cu = max(2, (tiles * batch * c + 255) // 256)
        rows = float((M + c - 1) // c) + 64.0
        cost = per_cu * rows + (12.0 * (c + 1) if c > 1 else 0.0)
        if cost < best_cost * 0.999:
            best_cost, best = cost, c
    return best


def _tn_chunks(M, batch, tiles):
    return min(max(1, 1024 // max(1, tiles * batch)), max(1, M // 256))


def _nn_chunks(K, batch, tiles):
    nst = (K + 31) // 32
    nchunk = max(1, 512 // max(1, tiles * batch))
    nchunk = min(nchunk, max(1, nst // 16))
    return min(nchunk, 16)


def _pick_bm(M, wn, d2s):
    if d2s or wn != 2:
        return 128
    p128, p192 = (M + 127) // 128 * 128, (M + 191) // 192 * 192
    return 192 if p192 * 8 <= p128 * 7 else 128


_NN_CFGS = ((128, 128, 32), (128, 64, 32), (192, 128, 32), (128, 160, 32), (128, 128, 16))


def _nn_cfg_cost(M, N, K, batch, c, nchunk):
    bm, bn, _ = c
    tiles = ((M + bm - 1) // bm) * ((N + bn - 1) // bn) * batch * nchunk
    per_cu = (tiles + 255) // 256
    stages = float((K + 31) // 32) / nchunk + 2.0
    return float(per_cu) * bm * bn * stages * (0.93 if bn == 160 else 1.0)


def reference_plan(form, M, N, K, batch, d2s_Co=0, ep_mul=False):
    """(kernel, bm, bn, bk, nchunk, per_chunk, grid, workspace) as the launchers computed them; d2s_Co > 0: a d2s problem."""
    d2s = d2s_Co > 0
    if form in (NN, NT):
        ntiles = lambda c: ((M + c[0] - 1) // c[0]) * ((N + c[1] - 1) // c[1])
        if d2s:
            cfg = 0 if _pick_wn(N, 0 if form == NT else d2s_Co) == 2 else 1
        else:
            wn = _pick_wn(N)
            cfg = (2 if _pick_bm(M, wn, d2s) == 192 else 0) if wn == 2 else 1
            c0 = _NN_CFGS[cfg]
            best = base = _nn_cfg_cost(M, N, K, batch, c0, _nn_chunks(K, batch, ntiles(c0)))
            for k in (1, 3):
                c = _NN_CFGS[k]
                cost = _nn_cfg_cost(M, N, K, batch, c, _nn_chunks(K, batch, ntiles(c)))
                if cost < 0.95 * base and cost < best:
                    best, cfg = cost, k
        c = _NN_CFGS[cfg]
        nchunk = 1 if (form == NN and d2s) else _nn_chunks(K, batch, ntiles(c))
        nst = (K + c[2] - 1) // c[2]
        return (cfg, c[0], c[1], c[2], nchunk, (nst + nchunk - 1) // nchunk, batch * nchunk * ntiles(c),
                nchunk * batch * M * N * 4 if nchunk > 1 else 0)
    if K <= 128 and N <= 128 and M >= 32768 and not d2s:
        quad = K > 64 or N > 64
        w = min(512 if quad else 2048, max(4, M // 256))
        wgs = w if quad else (w + 3) // 4
        runs = wgs if quad else wgs * 4
        kt, nt = (2, 2) if quad else ((K + 31) // 32, (N + 31) // 32)
        kernel = SK_QUAD if quad else {(1, 1): SK_11, (1, 2): SK_12, (2, 1): SK_21, (2, 2): SK_22}[(kt, nt)]
        tile = 64 if quad else 32
        return (kernel, tile * kt, tile * nt, 16, wgs, ((M + runs - 1) // runs + 1) // 2 * 2, wgs * batch, wgs * batch * K * N * 4)
    wn = _pick_wn(N, d2s_Co)
    wide = batch >= 8 and N % 160 == 0 and not d2s and not ep_mul
    BN = 160 if wide else 64 * wn
    tiles = ((K + 127) // 128) * ((N + BN - 1) // BN)
    nchunk = 1 if ep_mul else (_tn_chunks_model(M, batch, tiles) if wide else _tn_chunks(M, batch, tiles))
    return (TN_WIDE if wide else (TN_2 if wn == 2 else TN_1), 128, BN, 32, nchunk, ((M + nchunk - 1) // nchunk + 31) // 32 * 32,
            batch * nchunk * tiles, nchunk * batch * K * N * 4 if nchunk > 1 else 0)
