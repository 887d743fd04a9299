"""Case table of the multi-block ring-walk tests (test_conv_walk_plan.py on the CPU, test_gpu_conv_walks.py on the GPU).

The row-walking convolution kernels give a workgroup a CHUNK of ``gpc`` consecutive row groups of one w-segment
(``g_begin = range * g.gpc``) and walk them through an LDS ring that lives across the blocks of the chunk.  The launchers choose
``gpc`` in whole rounds of 256 workgroups, so every problem with ``NG * nseg <= 256`` runs with gpc = 1: one block per chunk, no
ring reuse.  The cases below are the smallest shapes at which the library's own plan (``ssbev_conv_chunk_groups``) walks two or
more blocks per chunk, each listed for the walk properties it is there for; test_conv_walk_plan.py asserts class, gpc and
properties through the library on a box without a GPU, so the GPU tests cannot lose this coverage quietly.

Shapes are (B, D, H, W) of the stride-1 grid (3x3x3, pad 1); for the stride-2 kernels the destination grid of conv_tap2_kernel,
which is the coarse grid of conv_tap2up_kernel."""
import collections
import ctypes as C

from stereoscene_amd import capi

# walk properties (computed from gpc, NG, H2, B by walk_properties below)
PLANE = "plane_straddle"      # a chunk holds row groups of two planes (plane pairs for tapdh): ring restage inside a chunk
BATCH = "batch_straddle"      # a chunk holds row groups of two batch samples
SHORT = "short_last_chunk"    # NG % gpc != 0
GRID8 = "grid_not_multiple_of_8"   # remainder branch of the XCD remap of blockIdx.x

Case = collections.namedtuple("Case", "kernel B D H W Cin Cout props epilogues")

# kernel -> (tile hint that forces it, ssbev_conv_dims.precision, kernel class, weight gradient on wgrad_tapdh_kernel)
KERNELS = {
    "tapdh": (9, 0, 9, True),       # conv_tapdh_kernel + wgrad_tapdh_kernel: D and H even
    "taph": (9, 0, 2, False),       # conv_taph_kernel: odd D, even H
    "tap": (6, 0, 1, False),        # conv_tap_kernel
    "tap2": (5, 0, 7, False),       # conv_tap2_kernel (class 7) and conv_tap2up_kernel (class 8): see CALLS
    "tap16": (9, 2, 17, False),     # conv_tap16_kernel, bf16 storage
}


def _c(kernel, shape, props=(), chans=(32, 32), epilogues=False):
    B, D, H, W = shape
    return Case(kernel, B, D, H, W, chans[0], chans[1], frozenset(props), epilogues)


CASES = [
    # conv_tapdh + wgrad_tapdh: H2 = 13 and D2 * H2 = 65 odd -> chunks straddle plane pairs and the batch boundary; ragged segment
    _c("tapdh", (2, 10, 26, 33), {PLANE, BATCH, GRID8}, epilogues=True),
    _c("tapdh", (2, 10, 26, 33), {PLANE, BATCH, GRID8}, chans=(16, 32)),
    _c("tapdh", (2, 18, 10, 70), {PLANE, BATCH, GRID8}, epilogues=True),              # 3 segments; grid 135 (7 mod 8)
    _c("tapdh", (2, 18, 10, 70), {PLANE, BATCH, GRID8}, chans=(32, 20)),
    _c("tapdh", (3, 44, 4, 33), {GRID8}),                                            # gpc = H2: one whole plane pair per chunk
    _c("tapdh", (3, 58, 4, 70), {PLANE, BATCH, GRID8}),                               # gpc 3 > H2 = 2: every chunk crosses
    _c("tapdh", (2, 86, 4, 70), {PLANE, BATCH, SHORT, GRID8}),                        # ... and NG = 172: short last chunk
    _c("tapdh", (3, 58, 2, 70), {PLANE, BATCH, SHORT, GRID8}),                        # H2 = 1: every block is a crossing
    _c("tapdh", (2, 26, 30, 33), {PLANE, BATCH, SHORT, GRID8}),                       # gpc 4: the longest walk that stays small
    _c("taph", (2, 5, 26, 33), {PLANE, BATCH, GRID8}, epilogues=True),
    _c("taph", (2, 5, 26, 33), {PLANE, BATCH, GRID8}, chans=(24, 32)),
    _c("taph", (1, 35, 22, 33), {PLANE, SHORT, GRID8}),
    _c("taph", (3, 43, 6, 33), {PLANE, BATCH, SHORT, GRID8}),                         # gpc 4 > H2 = 3
    _c("tap", (1, 9, 61, 32), {PLANE, SHORT, GRID8}, epilogues=True),
    _c("tap", (1, 9, 61, 32), {PLANE, SHORT, GRID8}, chans=(32, 20)),
    _c("tap", (2, 7, 41, 33), {PLANE, BATCH, SHORT}),
    _c("tap", (1, 5, 105, 40), {GRID8}),                                             # gpc 3 divides H: whole chunks per plane
    _c("tap2", (2, 9, 30, 20), {GRID8}, chans=(32, 64), epilogues=True),              # gpc 3 divides H2 = 15; odd sources too
    _c("tap2", (2, 9, 30, 20), {GRID8}, chans=(16, 48)),
    _c("tap2", (2, 11, 13, 33), {PLANE, BATCH, GRID8}, chans=(32, 64)),               # grid 231 (7 mod 8)
    _c("tap16", (2, 7, 41, 33), {PLANE, BATCH, GRID8}),
    _c("tap16", (2, 7, 41, 33), {PLANE, BATCH, GRID8}, chans=(24, 16)),
    _c("tap16", (1, 25, 31, 32), {PLANE, SHORT, GRID8}),
]


def case_id(c):
    return f"{c.kernel}-{c.B}x{c.D}x{c.H}x{c.W}-{c.Cin}to{c.Cout}"


# The operator calls of a case: name -> (transposed, source grid of x as a function of the table grid, expected kernel class of
# the forward (mode 0) and of the data gradient (mode 1); None = not a walking kernel, not asserted)
def calls(c):
    g = (c.D, c.H, c.W)
    if c.kernel != "tap2":
        cls = KERNELS[c.kernel][2]
        return {"conv": dict(transposed=False, stride=1, grid=g, cin=c.Cin, cout=c.Cout, classes=(cls, cls))}
    even, odd = tuple(2 * n for n in g), tuple(2 * n - 1 for n in g)
    return {
        # stride-2 conv K -> N from the fine grid: forward on the "down" kernel, data gradient on the "up" kernel
        "down": dict(transposed=False, stride=2, grid=even, cin=c.Cin, cout=c.Cout, classes=(7, 8)),
        # ... from an odd fine grid with the same destination: the "down" kernel's ragged source edges (no "up" counterpart)
        "down_odd": dict(transposed=False, stride=2, grid=odd, cin=c.Cin, cout=c.Cout, classes=(7, None)),
        # transposed conv N -> K from the coarse grid (output_padding 1): forward on the "up" kernel, data gradient on "down"
        "up": dict(transposed=True, stride=2, grid=g, cin=c.Cout, cout=c.Cin, classes=(8, 7)),
    }


def conv_dims(c, call):
    """ssbev_conv_dims of one call of a case, as functional._conv_dims fills it under the case's tile hint."""
    hint, precision = KERNELS[c.kernel][:2]
    Di, Hi, Wi = call["grid"]
    s = call["stride"]
    if call["transposed"]:
        Do, Ho, Wo = 2 * Di, 2 * Hi, 2 * Wi                   # (i - 1) * 2 - 2 + 2 + output_padding 1 + 1
    else:
        Do, Ho, Wo = ((n + 2 - 3) // s + 1 for n in (Di, Hi, Wi))
    return capi.ConvDims(c.B, call["cin"], call["cout"], Di, Hi, Wi, Do, Ho, Wo, 3, 3, 3, s, s, s, 1, 1, 1, 1, 1, 1,
                         int(call["transposed"]), 0, 0, hint, precision)


def walk_geometry(c, cls):
    """(NG, H2, nseg) of the walk of kernel class ``cls`` over the case's table grid: row groups in all, row groups per plane
    (per plane pair for class 9), w-segments.  Plain restatement of the kernels' block decomposition."""
    if cls == 9:
        return c.B * (c.D // 2) * (c.H // 2), c.H // 2, (c.W + 31) // 32
    if cls == 2:
        return c.B * c.D * (c.H // 2), c.H // 2, (c.W + 31) // 32
    if cls in (1, 17):
        return c.B * c.D * c.H, c.H, (c.W + 31) // 32
    assert cls in (7, 8)
    return c.B * c.D * ((c.H + 1) // 2), (c.H + 1) // 2, (c.W + 15) // 16


def walk_properties(gpc, NG, H2, nseg, B):
    """The walk properties of a launch, by enumerating its chunks [k * gpc, min(NG, (k + 1) * gpc))."""
    props = set()
    per_sample = NG // B
    for g0 in range(0, NG, gpc):
        g1 = min(NG, g0 + gpc) - 1
        if g0 // H2 != g1 // H2:
            props.add(PLANE)
        if g0 // per_sample != g1 // per_sample:
            props.add(BATCH)
    if NG % gpc:
        props.add(SHORT)
    if (((NG + gpc - 1) // gpc) * nseg) % 8:
        props.add(GRID8)
    return props


def query(c, call, mode):
    """(kernel class, gpc) of one call of a case from the library (host only)."""
    lib = capi.load()
    d = conv_dims(c, call)
    return lib.ssbev_conv_kernel_class(C.byref(d), mode), lib.ssbev_conv_chunk_groups(C.byref(d), mode)
