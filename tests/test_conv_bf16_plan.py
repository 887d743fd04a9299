"""CPU: the case table of test_gpu_conv_bf16_paths.py really reaches every product instance of csrc/conv_bf16.hip.

Every case of conv_bf16_cases.CASES is asked of the library itself (ssbev_conv_bf16_plan_query, which reads plan_gather16,
plan_igemm16, plan_wide16, plan_tap16 and plan_wgrad16, the functions the launchers read): it reports the kernel, instance and
chunking the case is listed for, for both result types, and the plan gives the case exactly the properties it is listed for.  A
threshold that moves a GPU case to another kernel or tile, or takes its ragged tile, short chunk or border plane away, fails
here on a box without a GPU.

The 256 x 32 and 128 x 32 tiles of conv_igemm16_kernel and forced stage depths are reachable in a tuning build only: nothing
here forces or tests them."""
import ctypes as C
import random

import pytest

import conv_bf16_cases as T
from stereoscene_amd import capi


@pytest.mark.parametrize("case", T.CASES, ids=T.case_id)
def test_case_runs_its_plan_with_its_properties(case):
    lib = capi.load()
    d = T.dims_of(case)
    p = T.query(d, case.mode)
    assert not isinstance(p, int), p
    assert T.plan_tuple(p) == case.plan, T.full_tuple(p)
    assert T.plan_props(d, case.mode, p) == case.props, T.full_tuple(p)
    assert p.kernel == lib.ssbev_conv_kernel_class(C.byref(d), case.mode)
    assert p.grid == T.expected_grid(d, case.mode, p) and 0 < p.grid < 2 ** 31
    assert p.workspace == T.expected_workspace(d, case.mode, p)
    assert p.workspace == (lib.ssbev_conv_bwd_weight_workspace(C.byref(d)) if case.mode == T.WGRAD else 0)
    assert p.gpc == lib.ssbev_conv_chunk_groups(C.byref(d), case.mode)               # (0 unless class 17)
    # only the group of the reported class (and the two totals) is filled in
    named = set(T.GROUPS[p.kernel]) | {"kernel", "grid", "workspace"}
    assert all(getattr(p, n) == 0 for n in T.PLAN_FIELDS if n not in named), T.full_tuple(p)
    assert case.precisions == ((2,) if case.mode == T.WGRAD else (2, 3))
    for prec in case.precisions:                                                     # the result type changes no choice,
        for relu, acc in ((0, 0), (1, 0), (0, 1)):                                   # nor does the epilogue
            assert T.full_tuple(T.query(T.dims_of(case, prec, relu, acc), case.mode)) == T.full_tuple(p)
    assert T.flops(d) <= 10e9                                                        # the float64 reference stays cheap


def test_table_covers_every_instance_and_property():
    by = lambda k: [c for c in T.CASES if c.plan[0] == k]
    for k in (T.GATHER16, T.TAP16, T.WIDE16, T.IGEMM16):          # every forward kernel in mode 0 and in mode 1, both result types
        assert {c.mode for c in by(k)} == {T.FWD, T.DGRAD}, k
        assert all(c.precisions == (2, 3) for c in by(k))
    assert {c.mode for c in by(T.WGRAD16) + by(T.WGRING16)} == {T.WGRAD}
    g16 = by(T.GATHER16)
    form1 = lambda c: T.gather_geom(T.dims_of(c), c.mode)[2] == 1
    assert {10 * c.plan[1] + c.plan[2] for c in g16 if not form1(c)} == T.GATHER16_TILINGS
    assert {10 * c.plan[1] + c.plan[2] for c in g16 if form1(c) and T.PARITY in c.props} == T.GATHER16_TILINGS
    for tag in (T.RAGGED_M, T.COUT_TAIL, T.COUT_PAD):             # under every tiling
        assert {10 * c.plan[1] + c.plan[2] for c in g16 if tag in c.props} == T.GATHER16_TILINGS, tag
    assert any(c.dims[T.FIELDS.index("transposed")] and T.PARITY in c.props for c in g16)
    assert any(c.dims[T.FIELDS.index("dh")] == 2 for c in g16)
    ig = by(T.IGEMM16)
    assert {c.plan[1:] for c in ig} == T.IGEMM16_TILES
    assert {c.plan[1:3] for c in ig if c.mode == T.DGRAD} >= {(64, 64), (64, 128), (128, 64)}
    assert any(c.plan[1] == 128 and T.PARITY in c.props for c in ig)                 # transposed form on a 128-row tile
    assert {c.plan[1] for c in ig if T.RAGGED_M in c.props} == {64, 128}
    assert {c.plan[2] for c in ig if T.COUT_TAIL in c.props} == {64} and any(T.COUT_PAD in c.props for c in ig)
    for t in ((128, 128), (128, 64), (64, 128), (64, 64)):                           # every tile with a 3-tap axis (halo masks)
        assert any(c.dims[T.FIELDS.index("kw")] == 3 and c.plan[1:3] == t for c in ig), t
    w16 = by(T.WIDE16)
    assert {(c.plan[1], c.plan[4]) for c in w16} == T.WIDE16_INSTANCES
    assert {(c.plan[1], c.plan[4]) for c in w16 if c.mode == T.DGRAD} >= {(2, 1), (3, 2), (4, 1), (4, 2)}
    assert {c.dims[T.FIELDS.index("Do")] for c in w16} == {1, 2, 3}
    assert {c.dims[T.FIELDS.index("Ho")] for c in w16} == {5, 16, 20} and {c.dims[T.FIELDS.index("Wo")] for c in w16} == {16, 32}
    assert {c.dims[T.FIELDS.index("Cin")] for c in w16 if c.mode == T.FWD} >= {64, 96, 160}
    assert len(by(T.TAP16)) == 2
    assert {c.plan[1:5] for c in by(T.WGRAD16)} == T.WGRAD16_CONFIGS
    assert {c.dims[T.FIELDS.index("kw")] for c in by(T.WGRAD16) if T.RAGGED_TAP in c.props} == {2, 4}
    assert {c.dims[T.FIELDS.index("transposed")] for c in by(T.WGRAD16) if T.RAGGED_TAP in c.props} == {0, 1}
    assert any(c.plan[6] > 4 for c in by(T.WGRAD16))                                 # more than one workgroup along the chunks
    assert {c.plan[1] for c in by(T.WGRING16)} == T.WGRING16_INSTANCES
    for narrow in (0, 1):
        mine = [c for c in by(T.WGRING16) if c.plan[1] == narrow]
        tiles = lambda c: c.dims[0] * c.dims[T.FIELDS.index("Do")] * -(-c.dims[T.FIELDS.index("Ho")] // 8) * (c.dims[T.FIELDS.index("Wo")] // 16)
        assert {tiles(c) for c in mine} == {3, 6, 26}
        assert {c.dims[T.FIELDS.index("Ho")] for c in mine} == {8, 12}
        assert {c.dims[T.FIELDS.index("tile_hint")] for c in mine} == {7, 9}
        assert any(T.SHORT_TILE_CHUNK in c.props for c in mine) and any(T.RAGGED_H in c.props for c in mine)
    assert set().union(*(c.props for c in T.CASES)) == T.ALL_PROPS
    for tag, k in ((T.RAGGED_H, T.WIDE16), (T.RAGGED_H, T.WGRING16), (T.D1, T.WIDE16), (T.D2, T.WIDE16), (T.BATCH2, T.GATHER16),
                   (T.BATCH2, T.IGEMM16), (T.BATCH2, T.WIDE16), (T.BATCH2, T.TAP16), (T.BATCH2, T.WGRAD16), (T.BATCH2, T.WGRING16)):
        assert any(tag in c.props for c in by(k)), (tag, k)
    assert len({T.case_id(c) for c in T.CASES}) == len(T.CASES)


def test_plans_of_the_existing_bit_identity_cases():
    """test_conv_igemm16_is_bit_identical_to_the_gather_kernel proves its claim on the 64 x 64 tile alone, which is why the table
    above has the three other tiles."""
    got = {T.plan_tuple(T.query(capi.ConvDims(*dims), mode))[:3] for dims in T.LEGACY_IGEMM16 for mode in (T.FWD, T.DGRAD)}
    assert got == {(21, 64, 64)}


# ------------------------------------------------------------------------------------------------------------------------
# transcription of the choices as they stood inline in dispatch_gather16, launch_igemm16, make_wg_geom / backward_weight and
# make_wr_geom before the plan functions existed (every `/` of the C source is on non-negative ints: `//`)
def _cdiv(a, b):
    return -(-a // b)


def reference_plan(d, mode, kernel):
    if kernel in (T.GATHER16, T.IGEMM16):
        K, N, form, classes, rows, out = T.gather_geom(d, mode)
        if kernel == T.IGEMM16:
            wide = (N + 31) // 32 * 32 % 128 == 0
            need = 1024 if form == 1 else 512
            bm, bn = 64, 64
            for cm, cn in ((128, 128 if wide else 64), (64, 128 if wide else 64), (64, 64)):
                if _cdiv(rows, cm) * _cdiv(N, cn) * classes >= need:
                    bm, bn = cm, cn
                    break
            return (21, bm, bn, 64 if K % 64 == 0 else 32)
        blocks = lambda mt, nt: _cdiv(rows, 128 * mt) * _cdiv(N, 32 * nt) * classes
        if d.tile_hint >= 10:
            return (16, d.tile_hint // 10, d.tile_hint % 10)
        nt = 6 if (N % 192 == 0 and blocks(2, 6) >= 256) else 4 if N % 128 == 0 else (2 if N > 32 else 1)
        if nt == 4 and blocks(2, 4) < 256:
            nt = 2
        mt = 2 if blocks(2, nt) >= 160 else 1
        if form == 1 and classes > 1:
            mt, nt = 1, min(nt, 2)
        return (16, mt, nt)
    if kernel == T.WGRAD16:
        cp, cq = (d.Cin, d.Cout) if d.transposed else (d.Cout, d.Cin)
        small = (d.Di, d.Hi, d.Wi) if d.transposed else (d.Do, d.Ho, d.Wo)
        narrow = cp <= 32 and cq <= 32
        if d.kh * d.kw == 1:
            cfg = (1, 1, 1, 1) if narrow else (2, 2, 1, 1)
        else:
            cfg = (1, 1, 3, 3) if narrow else (2, 2, 1, 3)
        M = d.B * small[0] * small[1] * small[2]
        tiles = _cdiv(cp, 32 * cfg[1]) * _cdiv(cq, 32 * cfg[0]) * d.kd * _cdiv(d.kh, cfg[2]) * _cdiv(d.kw, cfg[3])
        want = max(1, 4096 // max(1, tiles))
        want = min(want, max(1, (256 << 20) // (d.kd * d.kh * d.kw * cp * cq * 4)))
        chunk = (max(_cdiv(M, want), 256) + 15) // 16 * 16
        return (18,) + cfg + (chunk, _cdiv(M, chunk))
    if kernel == T.WGRING16:
        ntiles = d.B * d.Do * _cdiv(d.Ho, 8) * (d.Wo // 16)
        narrow = d.Cin <= 32 and d.Cout <= 32
        ncqt = 1 if narrow else _cdiv(d.Cin, 32)
        types = 1 if narrow else ncqt * _cdiv(d.Cout, 128) * 3
        want = min(max(1, 1024 // types), max(1, (256 << 20) // (27 * d.Cin * d.Cout * 4)))
        tpc = _cdiv(ntiles, want)
        if tpc < 4:
            tpc = min(4, ntiles)
        return (20, int(narrow), tpc, _cdiv(ntiles, tpc), ncqt)
    if kernel == T.WIDE16:
        N = d.Cout if mode == T.FWD else d.Cin
        ntl = 4 if N % 128 == 0 else (3 if N % 96 == 0 else 2)
        return (19, ntl, _cdiv(d.Ho, 16), d.Wo // 16, N // (32 * ntl))
    return None


def test_query_matches_a_transcription_of_the_previous_choices_on_random_dims():
    """The choices that stood inline in the launchers moved into plan functions without changing: random bf16-storage dims get the
    plan that reference_plan, a transcription of the code before the move, computes (class 17's chunking already had its plan
    function: ssbev_conv_chunk_groups and the dispatch snapshot pin it)."""
    rng = random.Random(20261019)
    lib = capi.load()
    seen = set()
    n = 0
    for i in range(30000):
        kind = rng.choice(("k3s1", "k3s1", "k3s2", "deconv3", "pw", "kes", "2d"))
        B = rng.choice((1, 1, 2, 3))
        cin, cout = (8 * rng.choice((1, 2, 3, 4, 4, 5, 8, 8, 12, 16, 24, 32, 48)) for _ in range(2))
        size = tuple(int(2 ** rng.uniform(0, e)) for e in (4.5, 6.5, 7.2))
        if rng.random() < 0.5:
            size = size[:2] + (16 * max(1, size[2] // 16),)
        hint = rng.choice((0, 0, 0, 0, 7, 8, 9, 11, 12, 14, 21, 22, 24, 26))
        if kind == "k3s1":
            dims = T.conv(B, cin, cout, size, 3, 1, 1, hint=hint)
        elif kind == "k3s2":
            dims = T.conv(B, cin, cout, size, 3, 2, 1, hint=hint)
        elif kind == "deconv3":
            dims = T.conv(B, cin, cout, size, 3, 2, 1, hint=hint, transposed=True, op=1)
        elif kind == "pw":
            dims = T.conv(B, cin, cout, size, 1, hint=hint)
        elif kind == "kes":
            k = rng.choice((2, 4))
            dims = T.conv(B, cin, cout, size, k, k, 0, hint=hint, transposed=rng.random() < 0.5)
        else:
            dl = rng.choice((1, 2, 6))
            dims = T.conv(B, cin, cout, (1,) + size[1:], (1, 3, 3), 1, (0, dl, dl), (1, dl, dl), hint=hint)
        if min(dims[6:9]) < 1:
            continue
        for mode in (T.FWD, T.DGRAD, T.WGRAD):
            d = capi.ConvDims(*dims)
            d.precision = 2 if mode == T.WGRAD else rng.choice((2, 3))
            p = T.query(d, mode)
            assert not isinstance(p, int), (i, dims, mode, p)
            assert p.kernel == lib.ssbev_conv_kernel_class(C.byref(d), mode)
            ref = reference_plan(d, mode, p.kernel)
            if ref is not None:
                assert T.plan_tuple(p) == ref, (i, dims, mode)
            assert p.grid == T.expected_grid(d, mode, p), (i, dims, mode)
            assert p.workspace == (lib.ssbev_conv_bwd_weight_workspace(C.byref(d)) if mode == T.WGRAD else 0)
            seen.add(T.plan_tuple(p)[:5] if p.kernel == T.WGRAD16 else T.plan_tuple(p)[:4] if p.kernel == T.IGEMM16 else
                     T.plan_tuple(p)[:3] if p.kernel in (T.GATHER16, T.WGRING16) else (p.kernel, p.ntl))
            n += 1
    assert n >= 60000
    assert {s[1:] for s in seen if s[0] == T.IGEMM16} == T.IGEMM16_TILES
    assert {10 * s[1] + s[2] for s in seen if s[0] == T.GATHER16} == T.GATHER16_TILINGS
    assert {s[1:] for s in seen if s[0] == T.WGRAD16} == T.WGRAD16_CONFIGS
    assert {s[1] for s in seen if s[0] == T.WIDE16} == {2, 3, 4} and {s[1] for s in seen if s[0] == T.WGRING16} == {0, 1}


def test_refusals_come_before_any_device_work():
    lib = capi.load()
    assert lib.ssbev_version() >= 113
    good = lambda prec=2: capi.ConvDims(*T.conv(2, 24, 40, (3, 5, 20), 3, 1, 1)[:-1], prec)
    plan = capi.ConvBf16Plan()
    q = lib.ssbev_conv_bf16_plan_query
    assert q(C.byref(good()), 0, C.byref(plan)) == capi.OK and plan.kernel == 16
    assert q(None, 0, C.byref(plan)) == capi.EINVAL
    assert q(C.byref(good()), 0, None) == capi.EINVAL
    for mode in (-1, 3):
        assert q(C.byref(good()), mode, C.byref(plan)) == capi.EINVAL
    for prec in (0, 1):                                        # not a bf16 storage problem
        assert [q(C.byref(good(prec)), m, C.byref(plan)) for m in (0, 1, 2)] == [capi.EINVAL] * 3
    assert q(C.byref(good(3)), 2, C.byref(plan)) == capi.EINVAL and q(C.byref(good(3)), 1, C.byref(plan)) == capi.OK   # fp32 result: no wgrad
    d = good()
    d.Cin = 20                                                 # 16-byte voxel-line pieces need Cin % 8 == 0
    assert q(C.byref(d), 0, C.byref(plan)) == capi.EINVAL
    d = good()
    d.Cout = 36                                                # ... and Cout % 8 == 0 where the Cout-channel tensor is a source
    assert q(C.byref(d), 0, C.byref(plan)) == capi.OK and q(C.byref(d), 1, C.byref(plan)) == capi.EINVAL
    d = good()
    d.tile_hint = 35                                           # names no conv_gather16_kernel instance: the launcher refuses it too
    assert q(C.byref(d), 0, C.byref(plan)) == capi.EINVAL
