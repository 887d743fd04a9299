"""Record the host-side conv dispatch of a built library into tests/golden/conv_dispatch.json (CPU only, no device call).

    python tools/make_golden_conv_dispatch.py --lib PATH/libssbev_hip.so --commit SHA [--out FILE]

The snapshot is the guard of tests/test_conv_dispatch_snapshot.py: it pins which kernel every ssbev_conv_* entry point picks,
so it is recorded from the library of the commit BEFORE a dispatch change and never regenerated from the changed code.  `--lib`
is therefore mandatory and `--commit` names the commit that library was built from (stored in the file).

Rows ("cols" names the fields): the 26 ints of ssbev_conv_dims, ssbev_conv_kernel_class and ssbev_conv_chunk_groups for modes
0 / 1 / 2, ssbev_conv_packed_weight_elems, ssbev_conv_bwd_weight_workspace and the weight-gradient kind as a label: the `kind` of
ssbev_conv_wgrad_plan_query (libraries older than ssbev_version() 123 do not have it).
"igemm_off" holds the rows whose class is 11 or 0 once more under SSBEV_IGEMM=0 (recorded by a child process; this process sets
no SSBEV_* variable), "retcodes" the SSBEV_EINVAL answers of the fp32 entry points that return before any device call."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import capi  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_dispatch.json")
FIELDS = [n for n, _ in capi.ConvDims._fields_]
COLS = FIELDS + ["class0", "class1", "class2", "groups0", "groups1", "groups2", "packed_elems", "wgrad_workspace", "wgrad_kind"]
WGRAD_KINDS = ("bf16", "thinside", "thin", "1x1", "dh", "lds", "cf", "generic")

CHANNELS = (3, 4, 8, 12, 16, 30, 32, 48, 64, 128, 192, 640)
# (B, D, H, W) of the coarse / stride-1 grid: tiny, odd and even D / H, W % 4 != 0, the workload's cost volume, a 2-D grid both
# ways round, and two grids past the size thresholds of the ring walks without a hint
GRIDS = ((1, 5, 6, 40), (2, 7, 41, 33), (2, 10, 26, 33), (1, 9, 30, 70), (1, 8, 8, 8), (1, 192, 48, 160), (1, 48, 160, 1),
         (1, 1, 48, 160), (1, 64, 64, 128), (1, 96, 24, 80))
HINTS = (0, 4, 5, 6, 7, 8, 9, 114)
# the full CHANNELS x CHANNELS product runs unhinted on FULL; CORE pairs run on every grid and configuration (the first five
# on the grids outside HINT_GRIDS), and with the hint, precision and relu / accumulate combinations on HINT_GRIDS
CORE = ((32, 32), (16, 32), (32, 64), (64, 32), (32, 4), (4, 32), (30, 32), (64, 128))
FULL = {(1, 192, 48, 160): ("k3", "k3s2_even"), (1, 5, 6, 40): ("k3",)}
HINT_GRIDS = ((1, 5, 6, 40), (2, 10, 26, 33), (1, 192, 48, 160))
HINTED = ("k1", "k3", "k3s2_even", "k3s2_odd", "k3s2t_even")     # the configurations whose kernels read hints 4 .. 9


def configs(grid):
    """name -> (kernel, stride, pad, dilation, transposed, input grid, output grid) on one coarse grid."""
    B, D, H, W = grid
    g = (D, H, W)
    even, odd = tuple(2 * n for n in g), tuple(2 * n - 1 for n in g)
    k3, s1, s2, p0, p1, p2, d1, d2 = (3, 3, 3), (1, 1, 1), (2, 2, 2), (0, 0, 0), (1, 1, 1), (2, 2, 2), (1, 1, 1), (2, 2, 2)
    return {
        "k1": ((1, 1, 1), s1, p0, d1, 0, g, g),
        "k3": (k3, s1, p1, d1, 0, g, g),
        "k3s2_even": (k3, s2, p1, d1, 0, even, g),              # fine = 2 x coarse
        "k3s2_odd": (k3, s2, p1, d1, 0, odd, g),                # coarse = (fine - 1) / 2 + 1 only
        "k3s2t_even": (k3, s2, p1, d1, 1, g, even),             # output_padding 1
        "k3s2t_odd": (k3, s2, p1, d1, 1, g, odd),               # output_padding 0
        "k3d2": (k3, s1, p2, d2, 0, g, g),
        "k2s2t": ((2, 2, 2), s2, p0, d1, 1, g, even),
        "k133": ((1, 3, 3), s1, (0, 1, 1), d1, 0, g, g),
        "k133s2": ((1, 3, 3), (1, 2, 2), (0, 1, 1), d1, 0, (D, 2 * H, 2 * W), g),
        "k133d2": ((1, 3, 3), s1, (0, 2, 2), (1, 2, 2), 0, g, g),
    }


def dims_grid():
    seen, rows = set(), []

    def add(grid, cfg, cin, cout, hint=0, precision=0, relu=0, acc=0):
        k, s, p, dl, tr, gi, go = cfg
        row = (grid[0], cin, cout, *gi, *go, *k, *s, *p, *dl, tr, relu, acc, hint, precision)
        if row not in seen:
            seen.add(row)
            rows.append(row)

    for grid in GRIDS:
        hinted_grid = grid in HINT_GRIDS
        for name, cfg in configs(grid).items():
            if name in FULL.get(grid, ()):
                for cin in CHANNELS:
                    for cout in CHANNELS:
                        add(grid, cfg, cin, cout)
            for cin, cout in (CORE if hinted_grid else CORE[:5]):
                add(grid, cfg, cin, cout)
            if not hinted_grid:
                continue
            for cin, cout in CORE[:3]:
                for hint in (HINTS[1:] if name in HINTED else (7, 114)):
                    add(grid, cfg, cin, cout, hint)
            if grid == HINT_GRIDS[1]:
                continue
            for cin, cout in CORE[:4]:
                for precision in (1, 2, 3):
                    add(grid, cfg, cin, cout, 0, precision)
            if name not in HINTED:
                continue
            for cin, cout in ((32, 32), (32, 64), (32, 4)):
                for relu, acc in ((1, 0), (0, 1), (1, 1)):
                    add(grid, cfg, cin, cout, 0, 0, relu, acc)
            for cin, cout in CORE[:2]:
                for hint in (5, 9, 114):
                    for precision in (1, 2):
                        add(grid, cfg, cin, cout, hint, precision)
                add(grid, cfg, cin, cout, 9, 0, 1, 1)
    # the thin heads: 32 -> 3 and 24 -> 2 take wgrad_thin_kernel / conv_thin_kernel rather than the thin-side MFMA kernels
    for grid in HINT_GRIDS:
        cfg = configs(grid)["k3"]
        for cin, cout in ((32, 3), (24, 2), (3, 32), (2, 32), (32, 2), (32, 1), (16, 4)):
            for hint in (0, 7, 8, 9):
                add(grid, cfg, cin, cout, hint)
        # wide layers in bf16 storage (the fp32 entry points must keep refusing them; classes 19 / 20 live in conv_bf16.hip)
        for cin, cout in ((64, 64), (64, 128), (128, 64)):
            for hint in (0, 7):
                for precision in (2, 3):
                    add(grid, cfg, cin, cout, hint, precision)
    return rows


def open_lib(path):
    lib = C.CDLL(path)
    for name in ("ssbev_conv_kernel_class", "ssbev_conv_chunk_groups", "ssbev_conv_packed_weight_elems",
                 "ssbev_conv_bwd_weight_workspace", "ssbev_conv_fwd", "ssbev_conv_bwd_data", "ssbev_conv_pack_weight",
                 "ssbev_conv_bwd_weight"):
        getattr(lib, name).restype, getattr(lib, name).argtypes = capi.SIGNATURES[name]
    return lib


def wgrad_kind(lib, d):
    """The kind select_wgrad takes, as ssbev_conv_wgrad_plan_query numbers it, under the labels of the snapshot."""
    plan = capi.ConvWgradPlan()
    q = lib.ssbev_conv_wgrad_plan_query
    q.restype, q.argtypes = capi.SIGNATURES["ssbev_conv_wgrad_plan_query"]
    rc = q(C.byref(d), C.byref(plan))
    assert rc == 0, rc
    return WGRAD_KINDS[plan.kind]


def record(lib, row):
    d = capi.ConvDims(*row)
    ref = C.byref(d)
    return list(row) + [lib.ssbev_conv_kernel_class(ref, m) for m in (0, 1, 2)] + \
        [lib.ssbev_conv_chunk_groups(ref, m) for m in (0, 1, 2)] + \
        [lib.ssbev_conv_packed_weight_elems(ref), lib.ssbev_conv_bwd_weight_workspace(ref), wgrad_kind(lib, d)]


# (entry point, dims, which pointer arguments are null): calls that answer SSBEV_EINVAL before any device call.  Non-null
# pointers are host dummies that are never dereferenced on these paths.
def retcode_cases():
    k3 = lambda cin, cout, precision=0, tr=0: (1, cin, cout, 5, 6, 40, 5, 6, 40, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, tr, 0, 0, 0, precision)
    bad = (1, 32, 32, 5, 6, 40, 5, 6, 40, 0, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)          # kd = 0
    return [
        ("ssbev_conv_fwd", k3(32, 32), "x"), ("ssbev_conv_fwd", k3(32, 32), "w"), ("ssbev_conv_fwd", k3(32, 32), "y"),
        ("ssbev_conv_bwd_data", k3(32, 32), "x"), ("ssbev_conv_bwd_data", k3(32, 32), "y"),
        ("ssbev_conv_pack_weight", k3(32, 32), "x"), ("ssbev_conv_pack_weight", k3(32, 32), "w"),
        ("ssbev_conv_pack_weight", k3(32, 32), "mode"),                                          # mode 2
        ("ssbev_conv_fwd", k3(32, 32, 2), ""), ("ssbev_conv_fwd", k3(32, 32, 3), ""), ("ssbev_conv_bwd_data", k3(32, 32, 2), ""),
        ("ssbev_conv_fwd", k3(30, 32), ""), ("ssbev_conv_fwd", k3(3, 64), ""), ("ssbev_conv_fwd", k3(30, 32, 0, 1), ""),
        ("ssbev_conv_bwd_data", k3(32, 30), ""), ("ssbev_conv_bwd_data", k3(64, 3), ""),
        ("ssbev_conv_bwd_weight", k3(32, 32), "x"), ("ssbev_conv_bwd_weight", k3(32, 32), "ws"), ("ssbev_conv_bwd_weight", k3(32, 32, 2), ""),
        ("ssbev_conv_fwd", bad, ""), ("ssbev_conv_bwd_data", bad, ""), ("ssbev_conv_pack_weight", bad, ""),
    ]


def retcode(lib, fn, row, null):
    d = capi.ConvDims(*row)
    buf = (C.c_float * 16)()
    ptr = lambda tag: None if tag == null else C.cast(buf, C.c_void_p)
    if fn == "ssbev_conv_fwd":
        return lib.ssbev_conv_fwd(ptr("x"), ptr("w"), None, ptr("y"), C.byref(d), None)
    if fn == "ssbev_conv_bwd_data":
        return lib.ssbev_conv_bwd_data(ptr("x"), ptr("w"), ptr("y"), C.byref(d), None)
    if fn == "ssbev_conv_bwd_weight":
        return lib.ssbev_conv_bwd_weight(ptr("x"), ptr("y"), ptr("w"), C.byref(d), ptr("ws"), 64, None)
    return lib.ssbev_conv_pack_weight(ptr("x"), ptr("w"), C.byref(d), 2 if null == "mode" else 0, None)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True, help="libssbev_hip.so built from the commit the snapshot pins")
    ap.add_argument("--commit", required=True, help="that commit (recorded in the file)")
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--igemm-off-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    lib = open_lib(a.lib)
    if a.igemm_off_child:        # stdin: rows; stdout: their records under the SSBEV_IGEMM=0 this child was started with
        print(json.dumps([record(lib, tuple(r)) for r in json.load(sys.stdin)]))
        return
    assert not [k for k in os.environ if k.startswith("SSBEV_")], "the snapshot is recorded with no SSBEV_* variable set"
    rows = [record(lib, r) for r in dims_grid()]
    c0, c1 = COLS.index("class0"), COLS.index("class1")
    # every row the implicit-GEMM kernel serves, and one in sixteen of those already on the generic gather
    generic = [r[:len(FIELDS)] for i, r in enumerate(rows) if 11 in (r[c0], r[c1]) or (0 in (r[c0], r[c1]) and i % 16 == 0)]
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--lib", a.lib, "--commit", a.commit, "--igemm-off-child"],
                           input=json.dumps(generic), capture_output=True, text=True, check=True,
                           env=dict(os.environ, SSBEV_IGEMM="0"))
    off = json.loads(child.stdout)
    ret = [[fn, list(row), null, retcode(lib, fn, row, null)] for fn, row, null in retcode_cases()]
    line = lambda r: json.dumps(r, separators=(",", ":"))
    with open(a.out, "w") as f:
        f.write('{"commit":%s,\n"cols":%s,\n"rows":[\n%s\n],\n"igemm_off":[\n%s\n],\n"retcodes":[\n%s\n]}\n' % (
            json.dumps(a.commit), line(COLS), ",\n".join(map(line, rows)), ",\n".join(map(line, off)), ",\n".join(map(line, ret))))
    print(f"{a.out}: {len(rows)} rows, {len(off)} SSBEV_IGEMM=0 rows, {len(ret)} return codes, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
