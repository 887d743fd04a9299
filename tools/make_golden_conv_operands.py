"""Record which operands functional._ConvNd hands to the library into tests/golden/conv_operands.json (CPU only).

    python tools/make_golden_conv_operands.py --commit SHA [--out FILE]

The snapshot is the guard of tests/test_conv_operands_snapshot.py: it pins, for the fp32 direct leaf, which entry points of the
library a forward and a backward call, in which order, with which ssbev_conv_dims and with tensors of which shape: the channel
padding of x, gy and the weight, the thin-side kernels that take their operands unpadded, the skinny TN shortcut of the pointwise
weight gradient, the crop of the results and whether the `fork` gradient slot is taken.  It is recorded from the commit BEFORE a
change of the leaf and never regenerated from the changed code; `--commit` names that commit (stored in the file).  Needs the built
library: the class, workspace and packed-size queries stay real (they are host code).

How a call is observed without a device: the recorder watches the C boundary.  For one observation the launching entry points
(ssbev_conv_pack_weight, _fwd, _bwd_data, _bwd_weight, ssbev_conv_thin_pack / _run) on the loaded library object are no-ops that
note their arguments and return OK, capi.ptr hands the tensor itself on, capi.stream answers None, gemm_tn (a leaf) is noted, the
side stream is off, and _ConvNd.apply plus one backward run on CPU tensors whose contents nobody reads.  ssbev_conv_kernel_class is
counted, forward and backward apart.

File: "dims", "calls" and "records" hold every distinct ssbev_conv_dims, call and observation once; "cases"[geometry] is the record
index of each variant, in the order of "variants"[tier].  In a recorded ssbev_conv_dims "h" / "p" stand for "the case's TILE_HINT"
/ "the case's precision code": what the wrapper must forward, so that cases that differ in nothing else share their records."""
import argparse
import contextlib
import importlib.util
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import capi, functional as F, streams  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_operands.json")
DIM_FIELDS = tuple(n for n, _ in capi.ConvDims._fields_)
_DT = {torch.float32: "f32", torch.uint8: "u8"}


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, *path))
    mod = importlib.util.module_from_spec(spec)
    sys.modules.setdefault(name, mod)
    spec.loader.exec_module(mod)
    return mod


ROUTES = _load(("tools", "make_golden_conv_routes.py"), "make_golden_conv_routes")
WGRAD = _load(("tests", "wgrad_cases.py"), "wgrad_cases")


# ---- the grid ------------------------------------------------------------------------------------------------------------------------
# (name, transposed, Cin, Cout, input grid, kernel, stride, padding, dilation, output_padding, tier); batch 1
def _geom(cin, cout, tr, k, s, tier, grid=(3, 4, 6)):
    p, op = k // 2, (s - 1 if tr and k == 3 else 0)
    return (f"{cin}->{cout} {'T' if tr else 'C'} k{k} s{s}" + ("" if grid == (3, 4, 6) else " on %dx%dx%d" % grid), int(tr), cin, cout,
            grid, (k,) * 3, (s,) * 3, (p,) * 3, (1,) * 3, (op,) * 3, tier)


THIN_PAIRS = [(1, 32), (2, 32), (4, 32), (32, 1), (32, 2), (32, 4)]             # the thin sides of wgrad_cases.py against 32
OFF4_PAIRS = [(3, 5), (5, 7), (33, 31), (20, 2), (32, 3), (7, 32)]              # Cin, Cout just off multiples of 4
CASE_PAIRS = sorted({(c.Cin, c.Cout) for c in WGRAD.CASES})                    # every channel pair of wgrad_cases.py


def _small(n):
    return min(n, 6 if n % 2 == 0 else 5)


def geometries():
    out, seen = [], set()

    def add(g):
        key = g[1:10]
        if key not in seen:
            seen.add(key)
            out.append(g)
    for cin, cout in THIN_PAIRS + OFF4_PAIRS:                     # where the thin-side classes live: every variant
        add(_geom(cin, cout, False, 3, 1, "full"))
    for cin, cout in ((3, 5), (32, 2), (2, 32)):
        add(_geom(cin, cout, True, 3, 2, "full"))
    for cin, cout in ((32, 32), (128, 128)):                      # the TN kind: 32768 rows
        add(_geom(cin, cout, False, 1, 1, "full", (32, 32, 32)))
    add(_geom(132, 32, False, 1, 1, "some", (32, 32, 32)))       # ... refused: more than 128 channels
    add(_geom(32, 32, False, 1, 1, "some", (32, 32, 31)))        # ... refused: 31744 rows
    for cin, cout in ((3, 5), (32, 2), (2, 32), (20, 2), (4, 32), (32, 4)):       # both transposed values, k 1 and 3, stride 1 and 2
        for tr in (False, True):
            for k in (1, 3):
                for s in (1, 2):
                    add(_geom(cin, cout, tr, k, s, "some"))
    for cin, cout in CASE_PAIRS:
        add(_geom(cin, cout, False, 3, 1, "few"))
    for name, entry, cin, cout, grid, k, s, p, d, op in ROUTES.LAYERS:           # the layers _conv_route sends to "convnd" under some switch
        if entry == "conv2d":
            grid, k, s, p, d, op = (1,) + tuple(grid), (1,) + tuple(k), (1,) + tuple(s), (0,) + tuple(p), (1,) + tuple(d), (0, 0, 0)
        add((f"routes: {name}", int(entry == "conv_transpose3d"), cin, cout, tuple(_small(n) for n in grid), tuple(k), tuple(s), tuple(p),
             tuple(d), tuple(op), "few"))
    return out


SWITCHES = [(h, prec, 1) for prec in ("fp32", "bf16_operands") for h in (0, 5, 7, 9)] + [(0, "fp32", 0), (0, "bf16_operands", 0)]


def variants(tier):
    """(name, relu, needs_input_grad of x / weight, slot, TILE_HINT, PRECISION, OWN_GEMM) of every case of one geometry, in file order."""
    if tier == "full":
        core = [(r, nig, slot) for r in (0, 1) for nig in ("x", "w", "xw") for slot in ("none", "empty", "filled")]
        sw = SWITCHES
    elif tier == "some":
        core = [(0, nig, slot) for nig in ("x", "w", "xw") for slot in ("none", "filled")]
        sw = [(0, "fp32", 1), (9, "fp32", 1)]
    else:
        core = [(0, "xw", "filled")]
        sw = [(0, "fp32", 1), (9, "fp32", 1), (0, "bf16_operands", 1)]
    return [(f"r{r} {nig} slot-{slot} hint{h} {prec} own{own}", r, nig, slot, h, prec, own) for r, nig, slot in core for h, prec, own in sw]


# ---- one observation ------------------------------------------------------------------------------------------------------------------
class Recorder:
    """The stubs of one case: `calls` in order, `queries` the class queries so far."""

    def __init__(self, hint, precision):
        self.calls, self.queries, self.hint, self.precision = [], 0, hint, precision

    def _call(self, name, mode, dref, *tensors):
        d = dref._obj
        dims = [getattr(d, n) for n in DIM_FIELDS]
        for field, sym, want in (("tile_hint", "h", self.hint), ("precision", "p", self.precision)):
            i = DIM_FIELDS.index(field)
            dims[i] = sym if dims[i] == want else dims[i]
        self.calls.append([name, mode, dims, [None if t is None else list(t.shape) + [_DT[t.dtype]] for t in tensors]])
        return capi.OK

    def pack_weight(self, w, wp, d, mode, st):
        return self._call("pack_weight", mode, d, w, wp)

    def fwd(self, x, wp, b, y, d, st):
        return self._call("fwd", 0, d, x, wp, b, y)

    def bwd_data(self, gy, wp, gx, d, st):
        return self._call("bwd_data", 1, d, gy, wp, gx)

    def bwd_weight(self, x, gy, gw, d, ws, n, st):
        return self._call("bwd_weight", 2, d, x, gy, gw, ws)

    def thin_pack(self, w, wp, d, mode, st):
        return self._call("thin_pack", mode, d, w, wp)

    def thin_run(self, src, wp, b, out, d, mode, ws, n, st):
        return self._call("thin_run", mode, d, src, wp, b, out, ws)

    def gemm_tn(self, a, b, tag=None, ep_mul=None, ep_rowsub=None):
        self.calls.append(["gemm_tn", -1, None, [list(a.shape) + [_DT[a.dtype]], list(b.shape) + [_DT[b.dtype]]]])
        return torch.empty(a.shape[1], b.shape[1])


_ABSENT = object()


@contextlib.contextmanager
def patched(rec, hint, prec, own):
    lib = capi.load()
    real_class = lib.ssbev_conv_kernel_class

    def counted(*a):
        rec.queries += 1
        return real_class(*a)
    stubs = [(lib, "ssbev_conv_pack_weight", rec.pack_weight), (lib, "ssbev_conv_fwd", rec.fwd), (lib, "ssbev_conv_bwd_data", rec.bwd_data),
             (lib, "ssbev_conv_bwd_weight", rec.bwd_weight), (lib, "ssbev_conv_thin_pack", rec.thin_pack),
             (lib, "ssbev_conv_thin_run", rec.thin_run), (lib, "ssbev_conv_kernel_class", counted),
             (capi, "ptr", lambda t: t), (capi, "stream", lambda: None), (F, "gemm_tn", rec.gemm_tn), (streams, "WGRAD_STREAM", False),
             (F, "TILE_HINT", hint), (F, "PRECISION", prec), (F, "OWN_GEMM", bool(own)), (F, "KERNEL_TIMER", None)]
    saved = []
    try:
        for obj, name, new in stubs:
            saved.append((obj, name, obj.__dict__.get(name, _ABSENT)))
            setattr(obj, name, new)
        yield
    finally:
        for obj, name, old in reversed(saved):
            if old is _ABSENT:
                delattr(obj, name)
            else:
                setattr(obj, name, old)


def observe(geom, variant):
    """Run one case against the stubs and return its record."""
    _name, tr, cin, cout, grid, k, s, p, dl, op, _tier = geom
    _vname, relu, nig, slot_state, hint, prec, own = variant
    x = F.from_cl(torch.empty(1, *grid, cin)).requires_grad_("x" in nig)           # channels-last memory: to_cl makes no copy
    w = torch.empty(((cin, cout) if tr else (cout, cin)) + tuple(k)).requires_grad_("w" in nig)
    b = torch.empty(cout).requires_grad_("w" in nig)
    slot = None if slot_state == "none" else F.GradSlot()
    if slot_state == "filled":                                                      # another consumer's gradient is already there
        slot.buf = torch.empty(1, *grid, cin)
    before = slot.buf if slot is not None else None
    rec = Recorder(hint, 1 if prec == "bf16_operands" else 0)
    with patched(rec, hint, prec, own):
        y = F._ConvNd.apply(x, w, b, tuple(s), tuple(p), tuple(dl), bool(tr), tuple(op), slot, bool(relu))
        asked_fwd = rec.queries
        ins = [t for t in (x, w, b) if t.requires_grad]
        grads = iter(torch.autograd.grad(y, ins, torch.empty_like(y)))
    out = [list(next(grads).shape) if t.requires_grad else None for t in (x, w, b)]
    return {"calls": rec.calls, "y": list(y.shape), "out": out, "slot_set": int(slot is not None and slot.buf is not before),
            "queries": [asked_fwd, rec.queries - asked_fwd]}


def cases():
    for g in geometries():
        for v in variants(g[10]):
            yield g, v


def expand(snap, rec):
    """A record of the file with its calls and dims written out again."""
    calls = []
    for ci in rec[0]:
        name, mode, di, tensors = snap["calls"][ci]
        calls.append([name, mode, None if di is None else snap["dims"][di], tensors])
    return {"calls": calls, "y": rec[1], "out": rec[2], "slot_set": rec[3], "queries": rec[4]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose operand handling the snapshot pins (recorded in the file)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert not [k for k in os.environ if k.startswith("SSBEV_")], "the snapshot is recorded with no SSBEV_* variable set"
    line = lambda r: json.dumps(r, separators=(",", ":"))
    tables = {"dims": ([], {}), "calls": ([], {}), "records": ([], {})}

    def intern(table, value):
        rows, index = tables[table]
        key = line(value)
        if key not in index:
            index[key] = len(rows)
            rows.append(key)
        return index[key]
    by_geom, n = {}, 0
    for g, v in cases():
        r = observe(g, v)
        calls = [intern("calls", [name, mode, None if dims is None else intern("dims", dims), tensors]) for name, mode, dims, tensors in r["calls"]]
        by_geom.setdefault(g[0], []).append(intern("records", [calls, r["y"], r["out"], r["slot_set"], r["queries"]]))
        n += 1
    vnames = {t: [v[0] for v in variants(t)] for t in ("full", "some", "few")}
    with open(a.out, "w") as f:
        f.write('{"commit":%s,\n"dim_fields":%s,\n"geometries":%s,\n"variants":%s,\n"dims":[\n%s\n],\n"calls":[\n%s\n],\n"records":[\n%s\n],\n"cases":{\n%s\n}}\n' % (
            json.dumps(a.commit), line(list(DIM_FIELDS)), line([list(g) for g in geometries()]), line(vnames),
            ",\n".join(tables["dims"][0]), ",\n".join(tables["calls"][0]), ",\n".join(tables["records"][0]),
            ",\n".join(f"{json.dumps(name)}:{line(ix)}" for name, ix in by_geom.items())))
    print(f"{a.out}: {n} cases, {len(tables['records'][0])} distinct records, {len(tables['calls'][0])} calls, {len(tables['dims'][0])} dims, "
          f"{os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
