"""Record which route functional.conv3d / conv2d / conv_transpose3d take into tests/golden/conv_routes.json (CPU only).

    python tools/make_golden_conv_routes.py --commit SHA [--out FILE]

The snapshot is the guard of tests/test_conv_routes_snapshot.py: it pins, for every layer shape of the workload under every
precision mode, tile hint and routing switch, which leaf the Python layer calls with which arguments and what it does to the
result afterwards.  It is recorded from the commit BEFORE a routing change and never regenerated from the changed code;
`--commit` names that commit (stored in the file).  Needs the built library: routing asks it two host-side questions
(ssbev_conv_kernel_class, ssbev_wino43_df_supported) and nothing else.

How a call is observed without a device: inputs are `device="meta"` tensors (a torch.Tensor subclass answers is_cuda = True for
the GPU cases), the leaves -- _ConvNd, _ConvNd16, _WinoConv, _WinoConvDF, _DeconvKS (.apply), linear_cl, torch.mm, torch.relu --
are replaced by stubs that note their arguments and return a meta tensor of the right shape and dtype that requires grad, and
the autograd nodes between the result and the last stub output are the epilogue (bias added after, ReLU after, cast, squeeze).

File: "layers" and "variants" name the two axes of the case grid, "records" holds every distinct observation once and
"routes"[layer] the record index of each variant, in the order of "variants"."""
import argparse
import inspect
import json
import os
import re
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stereoscene_amd import capi, functional as F  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "conv_routes.json")
QUERIES = ("ssbev_conv_kernel_class", "ssbev_wino43_df_supported")

# every module switch routing reads, at the value it has with no SSBEV_* variable set
DEFAULTS = dict(PRECISION="fp32", TILE_HINT=0, WINOGRAD=True, WINO_BF16S=True, WIDE16=True, GEMM_LAYERS=True, GEMM_MIN_CIN=512,
                DILATED_POLYPHASE=True, POLYPHASE_MAX_PAD=1.35, WINO_DILATED=True, WINO_DILATED_MAX_TILES=1.35 + 0.05,
                WINO_DILATED_AXIS_CAP=128, WINO_DF=True, WINO_F43=True, WINO_DF_MIN_ROWS=1024, WINO_DEPTH_FUSED=False,
                WINO_OWN_GEMM=False, WINO_F444=False, OWN_GEMM=True, OWN_GEMM_SITES={"deconv", "bri", "linear", "wino"})
SWITCHES = {
    "WINOGRAD=0": dict(WINOGRAD=False), "WINO_BF16S=0": dict(WINO_BF16S=False), "WIDE16=0": dict(WIDE16=False),
    "GEMM_LAYERS=0": dict(GEMM_LAYERS=False), "GEMM_MIN_CIN=64": dict(GEMM_MIN_CIN=64),
    "DILATED_POLYPHASE=0": dict(DILATED_POLYPHASE=False), "WINO_DILATED=0": dict(WINO_DILATED=False),
    "WINO_DF=0": dict(WINO_DF=False), "WINO_F43=0": dict(WINO_F43=False), "WINO_DF_MIN_ROWS=0": dict(WINO_DF_MIN_ROWS=0),
    "OWN_GEMM_SITES-deconv": dict(OWN_GEMM_SITES={"bri", "linear", "wino"}),
    "OWN_GEMM_SITES-linear": dict(OWN_GEMM_SITES={"deconv", "bri", "wino"}),
}
PRECISIONS = ("fp32", "bf16", "bf16_operands")
HINTS = (0, 5, 7, 9)


def _c3(name, cin, cout, grid, k=3, s=1, p=1):
    return (name, "conv3d", cin, cout, grid, (k,) * 3, (s,) * 3, (p,) * 3, (1,) * 3, (0,) * 3)


def _c2(name, cin, cout, grid, k=3, s=1, p=1, d=1):
    return (name, "conv2d", cin, cout, grid, (k,) * 2, (s,) * 2, (p,) * 2, (d,) * 2, (0,) * 2)


def _ct(name, cin, cout, grid, k, s, p=0, op=0):
    return (name, "conv_transpose3d", cin, cout, grid, (k,) * 3, (s,) * 3, (p,) * 3, (1,) * 3, (op,) * 3)


# (name, entry point, Cin, Cout, input grid, kernel, stride, padding, dilation, output_padding); batch 1
LAYERS = [
    _c3("cost-volume 32->32", 32, 32, (192, 48, 160)),
    _c3("wide 64->64 W%16==0", 64, 64, (16, 128, 128)),
    _c3("wide 64->64 W%16!=0", 64, 64, (16, 32, 40)),
    _c3("wide 64->64 W%4!=0", 64, 64, (8, 30, 42)),
    _c3("wide 128->128", 128, 128, (16, 128, 128)),
    _c3("wide 256->256", 256, 256, (8, 64, 64)),
    _c3("wide 384->192", 384, 192, (8, 64, 64)),
    _c3("wide 512->512 few rows", 512, 512, (4, 32, 32)),
    _c3("wide 64->64 odd D", 64, 64, (9, 32, 32)),
    _c3("thin 32->1", 32, 1, (16, 24, 40)),
    _c3("thin 32->4", 32, 4, (16, 24, 40)),
    _c3("thin 2->32", 2, 32, (16, 24, 40)),
    _c3("20 channels", 20, 20, (16, 24, 40)),
    _c3("1x1x1 256->128", 256, 128, (8, 16, 16), 1, 1, 0),
    _c3("1x1x1 640->128", 640, 128, (8, 16, 16), 1, 1, 0),
    _c3("3x3x3 stride 2", 32, 64, (16, 32, 32), 3, 2, 1),
    _c2("2d 640->640 d1", 640, 640, (48, 160)),
    _c2("2d 640->640 d6", 640, 640, (48, 160), p=6, d=6),
    _c2("2d 640->640 d12", 640, 640, (48, 160), p=12, d=12),
    _c2("2d 640->640 d18", 640, 640, (48, 160), p=18, d=18),
    _c2("2d 640->128", 640, 128, (48, 160)),
    _c2("2d 640->640 d18 on 12x40", 640, 640, (12, 40), p=18, d=18),
    _c2("2d 640->640 d3 on 48x1000", 640, 640, (48, 1000), p=3, d=3),
    _c2("2d 64->64 odd H", 64, 64, (47, 160)),
    _c2("2d 20 channels", 20, 20, (48, 160)),
    _c2("2d 20->64", 20, 64, (48, 160)),
    _c2("2d 3x3 stride 2 32->64", 32, 64, (48, 160), 3, 2, 1),
    _c2("1x1 256->128", 256, 128, (48, 160), 1, 1, 0),
    _c2("1x1 640->256", 640, 256, (48, 160), 1, 1, 0),
    _c2("1x1 512->2", 512, 2, (48, 160), 1, 1, 0),
    _ct("3x3x3 stride 2 transposed", 64, 32, (8, 16, 16), 3, 2, 1, 1),
    _ct("20 channels transposed", 20, 20, (4, 16, 16), 2, 2),
    _ct("20->32 transposed", 20, 32, (4, 16, 16), 2, 2),
    _ct("deconv k1 128->30", 128, 30, (4, 16, 16), 1, 1),
] + [_ct(f"deconv k{k} {cin}->{cout}", cin, cout, (4, 16, 16), k, k) for k in (1, 2, 4) for cin in (128, 64) for cout in (128, 96)]


def variants(entry):
    """(name, bias, relu, is_cuda, switch overrides) of every case of one layer, in file order."""
    out = []
    for bias in (1, 0):
        for relu in ((0, 1) if entry == "conv3d" else (0,)):
            for prec in PRECISIONS:
                for hint in HINTS:
                    out.append((f"b{bias} r{relu} {prec} hint{hint}", bias, relu, True, dict(PRECISION=prec, TILE_HINT=hint)))
                for sw, over in SWITCHES.items():
                    out.append((f"b{bias} r{relu} {prec} {sw}", bias, relu, True, dict(over, PRECISION=prec)))
                out.append((f"b{bias} r{relu} {prec} cpu", bias, relu, False, dict(PRECISION=prec)))
    return out


class _OnGpu(torch.Tensor):
    """A meta tensor that says it lives on the GPU."""
    is_cuda = property(lambda self: True)


def _meta(shape, dtype=torch.float32, cuda=True, grad=False):
    t = torch.empty(tuple(int(v) for v in shape), dtype=dtype, device="meta")
    t = t.as_subclass(_OnGpu) if cuda else t
    return t.requires_grad_() if grad else t


SLOT = object()          # sentinel _ssbev_grad_slot of every input
_DT = {torch.float32: "f32", torch.bfloat16: "bf16"}


def _conv_out(x, weight, stride, padding, dilation, transposed, output_padding):
    k = weight.shape[2:]
    if transposed:
        sp = [(i - 1) * s - 2 * p + d * (kk - 1) + op + 1 for i, s, p, d, kk, op in zip(x.shape[2:], stride, padding, dilation, k, output_padding)]
        return (x.shape[0], weight.shape[1], *sp)
    sp = [(i + 2 * p - d * (kk - 1) - 1) // s + 1 for i, s, p, d, kk in zip(x.shape[2:], stride, padding, dilation, k)]
    return (x.shape[0], weight.shape[0], *sp)


class Recorder:
    """The stubs of one case: `calls` in order, `made` the tensors they returned."""

    def __init__(self):
        self.calls, self.made = [], []

    def _note(self, leaf, fn, args, kwargs, shape, dtype):
        b = inspect.signature(fn).bind(*args, **kwargs)
        b.apply_defaults()
        plain, tensors, first = {}, [], None
        for name, v in b.arguments.items():
            if name in ("bias", "slot"):
                continue
            if isinstance(v, torch.Tensor):
                first = v if first is None else first
                tensors.append([list(v.shape), _DT[v.dtype]])
            else:
                plain[name] = list(v) if isinstance(v, tuple) else v
        self.calls.append([leaf, plain, tensors, int(b.arguments.get("bias") is not None), int(b.arguments.get("slot") is SLOT)])
        assert b.arguments.get("slot") in (None, SLOT)
        y = _meta(shape, dtype, first.is_cuda, grad=True)
        self.made.append(y)
        return y

    def conv_nd(self, x, weight, bias, stride, padding, dilation, transposed, output_padding, slot=None, relu=False):
        return self._note("_ConvNd", self.conv_nd, (x, weight, bias, stride, padding, dilation, bool(transposed), output_padding, slot, bool(relu)), {},
                          _conv_out(x, weight, stride, padding, dilation, transposed, output_padding), torch.float32)

    def conv_nd16(self, x, weight, bias, stride, padding, dilation, transposed, output_padding, slot=None, relu=False, out_fp32=False):
        return self._note("_ConvNd16", self.conv_nd16, (x, weight, bias, stride, padding, dilation, bool(transposed), output_padding, slot, bool(relu), bool(out_fp32)), {},
                          _conv_out(x, weight, stride, padding, dilation, transposed, output_padding), torch.float32 if out_fp32 else torch.bfloat16)

    def wino(self, x, weight, slot=None, dil=1):
        return self._note("_WinoConv", self.wino, (x, weight, slot, int(dil)), {}, (x.shape[0], weight.shape[0], *x.shape[2:]),
                          torch.bfloat16 if F.PRECISION == "bf16" else torch.float32)

    def wino_df(self, x, weight, slot=None):
        return self._note("_WinoConvDF", self.wino_df, (x, weight, slot), {}, (x.shape[0], weight.shape[0], *x.shape[2:]), torch.float32)

    def linear_cl(self, x, weight, bias=None):
        return self._note("linear_cl", self.linear_cl, (x, weight, bias), {}, (x.shape[0], weight.shape[0], *x.shape[2:]), torch.float32)

    def deconv_ks(self, xcl, weight, bias, k):
        B, D, H, W, _ = xcl.shape
        return self._note("_DeconvKS", self.deconv_ks, (xcl, weight, bias, tuple(k)), {}, (B, D * k[0], H * k[1], W * k[2], weight.shape[1]), torch.float32)

    def mm(self, a, b):
        return self._note("torch.mm", self.mm, (a, b), {}, (a.shape[0], b.shape[1]), a.dtype)

    def relu(self, y):
        self.calls.append(["torch.relu", {}, [[list(y.shape), _DT[y.dtype]]], 0, 0])
        return _REAL_RELU(y)


_REAL_RELU = torch.relu


class patched:
    """Leaves stubbed by `rec`, switches set to DEFAULTS + `over`, the two host queries counted in `self.queries`."""

    def __init__(self, rec, over):
        self.rec, self.over, self.queries = rec, over, [0, 0]

    def __enter__(self):
        r = self.rec
        self.saved = []
        stubs = [(F._ConvNd, "apply", r.conv_nd), (F._ConvNd16, "apply", r.conv_nd16), (F._WinoConv, "apply", r.wino),
                 (F._WinoConvDF, "apply", r.wino_df), (F._DeconvKS, "apply", r.deconv_ks), (F, "linear_cl", r.linear_cl),
                 (torch, "mm", r.mm), (torch, "relu", r.relu)]
        stubs += [(F, k, v) for k, v in dict(DEFAULTS, **self.over).items()]
        lib = capi.load()
        for i, q in enumerate(QUERIES):
            stubs.append((lib, q, self._counted(getattr(lib, q), i)))
        for obj, name, new in stubs:
            self.saved.append((obj, name, obj.__dict__.get(name, _ABSENT)))
            setattr(obj, name, new)
        return self

    def _counted(self, fn, i):
        def call(*a):
            self.queries[i] += 1
            return fn(*a)
        return call

    def __exit__(self, *exc):
        for obj, name, old in reversed(self.saved):
            if old is _ABSENT:
                delattr(obj, name)          # (an inherited `apply`: uncover it again)
            else:
                setattr(obj, name, old)
        return False


_ABSENT = object()


def _epilogue(y, made):
    """Autograd nodes from the result back to a stub output, as names without the 'Backward<n>' tail; last entry: which output."""
    if y.grad_fn is None:
        return [f"leaf{[id(m) for m in made].index(id(y))}"]
    names, fn = [], y.grad_fn
    while True:
        if type(fn).__name__ == "AccumulateGrad":
            return names + [f"leaf{[id(m) for m in made].index(id(fn.variable))}"]
        n = re.sub(r"Backward\d*$", "", type(fn).__name__)
        if n != "Alias":                    # (the tensor subclass's own wrapper nodes)
            names.append(n)
        nxt = [g for g, _ in fn.next_functions if g is not None]
        assert len(nxt) == 1, (names, nxt)
        fn = nxt[0]


def observe(layer, variant):
    """Run one case against the stubs and return its record."""
    _name, entry, cin, cout, grid, k, s, p, d, op = layer
    _vname, has_bias, relu, cuda, over = variant
    act = torch.bfloat16 if (over["PRECISION"] == "bf16" and cin % 8 == 0) else torch.float32      # what a bf16 chain hands on
    x = _meta((1, cin, *grid), act, cuda)
    x._ssbev_grad_slot = SLOT
    w = _meta(((cin, cout) if entry == "conv_transpose3d" else (cout, cin)) + tuple(k), cuda=cuda)
    b = _meta((cout,), cuda=cuda) if has_bias else None
    rec = Recorder()
    with patched(rec, over) as pt:
        if entry == "conv3d":
            y = F.conv3d(x, w, b, s, p, d, relu=bool(relu))
        elif entry == "conv2d":
            y = F.conv2d(x, w, b, s, p, d)
        else:
            y = F.conv_transpose3d(x, w, b, s, p, op)
    return {"calls": rec.calls, "out": [list(y.shape), _DT[y.dtype]], "slot_kept": int(getattr(x, "_ssbev_grad_slot", None) is SLOT),
            "epilogue": _epilogue(y, rec.made), "queries": pt.queries}


def cases():
    for layer in LAYERS:
        for v in variants(layer[1]):
            yield layer, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose routing the snapshot pins (recorded in the file)")
    ap.add_argument("--out", default=OUT)
    a = ap.parse_args()
    assert not [k for k in os.environ if k.startswith("SSBEV_")], "the snapshot is recorded with no SSBEV_* variable set"
    assert all(getattr(F, k) == v for k, v in DEFAULTS.items()), "DEFAULTS must restate the module's defaults"
    line = lambda r: json.dumps(r, separators=(",", ":"))
    records, index, routes = [], {}, {}
    for layer, v in cases():
        key = line(observe(layer, v))
        if key not in index:
            index[key] = len(records)
            records.append(key)
        routes.setdefault(layer[0], []).append(index[key])
    vnames = {e: [v[0] for v in variants(e)] for e in ("conv3d", "conv2d", "conv_transpose3d")}
    with open(a.out, "w") as f:
        f.write('{"commit":%s,\n"layers":%s,\n"variants":%s,\n"records":[\n%s\n],\n"routes":{\n%s\n}}\n' % (
            json.dumps(a.commit), line([list(l) for l in LAYERS]), line(vnames), ",\n".join(records),
            ",\n".join(f"{json.dumps(n)}:{line(ix)}" for n, ix in routes.items())))
    print(f"{a.out}: {sum(map(len, routes.values()))} cases, {len(records)} distinct records, {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
