"""CPU: what every case of wgrad_cases.CASES reaches in ssbev_conv_bwd_weight, asked of the library itself.

ssbev_conv_wgrad_plan_query answers from select_wgrad, plan_wgrad_reduce and the Lds instance choice -- the functions the launch
reads -- and makes no device call.  For every case: the answer equals the hand-written `expect` and, where the planner is
mirrored in wgrad_cases.py, the mirror; the fold plan equals the mirror of plan_wgrad_reduce; ssbev_conv_bwd_weight_workspace
equals what the plan implies; the size cap holds; the integers of the exact regime keep every sum exact; and the properties the
cases reach are, as a set, the ones wgrad_cases.REQUIRED lists: a shape that silently moves to another path fails here."""
import ctypes as C

import pytest

import wgrad_cases as T
from stereoscene_amd import capi, functional as F

IDS = [c.id for c in T.CASES]


@pytest.fixture(scope="module", autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def test_ids_are_unique_and_props_are_known():
    assert len(set(IDS)) == len(IDS)
    for c in T.CASES:
        for p in c.props.split():
            assert p in T.REQUIRED or p.startswith(T.EXTRA_OK_PREFIXES), (c.id, p)


@pytest.mark.parametrize("cid", IDS)
def test_plan_is_the_expected_one(cid):
    c = T.BY_ID[cid]
    plan = T.query(T.dims(c))
    assert {k: v for k, v in plan.items() if v or k == "kind"} == c.expect
    kind = T.KINDS[plan["kind"]]
    m = T.mirror(c, kind)
    if m is not None:
        assert {k: plan[k] for k in m} == m
    if kind != "ThinSide":
        fold = T.plan_wgrad_reduce(plan["nchunks"], plan["taps"], plan["Cq"], plan["Cp"])
        assert {k: plan[k] for k in fold} == fold
    else:
        assert (plan["two_stage"], plan["nsl"], plan["per"], plan["final"]) == (0, 0, 0, 0)
    if kind in ("ChannelsFirst", "Direct"):
        Cp, Cq = (c.Cin, c.Cout) if c.tr else (c.Cout, c.Cin)
        assert {k: plan[k] for k in ("MQ", "MP", "TH", "TW")} == T.wgrad_cfg(Cp, Cq, c.k[1], c.k[2])
    if kind == "Lds":
        assert plan["nchunks"] == plan["nseg"] * plan["nranges"] * plan["ksplit"]
        assert plan["ksplit"] == {0: 1, 1: 4, 2: 2, 3: 1}[plan["cfg"]]
        wino = plan["cfg"] == 1 and plan["RG"] % 2 == 0 and c.hint != 6
        assert plan["instance"] == (0 if not wino else (2 if plan["Wseg"] == 32 and c.hint != 5 else 1))
    if kind == "Dh":
        assert plan["taps"] == 48 and plan["gpc"] == capi.load().ssbev_conv_chunk_groups(C.byref(T.dims(c)), 2)


@pytest.mark.parametrize("cid", IDS)
def test_workspace_and_size_cap(cid):
    c = T.BY_ID[cid]
    d = T.dims(c)
    plan = T.query(d)
    ws = capi.load().ssbev_conv_bwd_weight_workspace(C.byref(d))
    assert ws == plan["workspace"] == T.implied_workspace(c, plan)
    assert T.largest_tensor(c, ws) <= (T.CAP_ONE if cid in T.BIG_CASES else T.CAP)
    assert len(T.BIG_CASES) <= 1


@pytest.mark.parametrize("cid", IDS)
def test_props_are_what_the_plan_reaches(cid):
    c = T.BY_ID[cid]
    assert set(c.props.split()) == T.reached(c, T.query(T.dims(c)))


def test_every_required_path_is_reached():
    got = set()
    for c in T.CASES:
        got |= T.reached(c, T.query(T.dims(c)))
    got = {p for p in got if not p.startswith(T.EXTRA_OK_PREFIXES) or p in T.REQUIRED}
    assert got == T.REQUIRED, (sorted(T.REQUIRED - got), sorted(got - T.REQUIRED))
    assert not (T.UNREACHABLE & got), "reachable after all: move it into REQUIRED"


@pytest.mark.parametrize("cid", IDS)
def test_exact_regime_stays_exact(cid):
    """max A x 16 < 2^24, A the float64 weight gradient of |x|, |gy| of the case's integer inputs: every partial sum in any order
    is an integer below 2^24 / 16, and the 4 fractional bits two nested F(2,3) stages can add still fit the fp32 significand."""
    c = T.BY_ID[cid]
    x, gy = T.exact_inputs(c)
    assert x.abs().max().item() <= c.lim and gy.abs().max().item() <= c.lim and x.abs().max().item() >= 1
    assert (x == x.round()).all() and (gy == gy.round()).all()
    A = T.reference(c, x.abs(), gy.abs())
    assert A.max().item() * 16 < 2 ** 24, A.max().item()
    plan = T.query(T.dims(c))
    xi, gi = T.indicator_inputs(c, plan)
    ind = xi if c.tr else gi
    marked = {tuple(int(v) for v in i) for i in (ind.abs().sum(1) > 0).nonzero()}
    assert marked == set(T.boundary_voxels(c, plan)) and 1 <= len(marked) <= 4


def test_padded_problems_of_the_wrappers_keep_their_kind():
    """Cases with a channel count that is no multiple of 4 reach the library padded when they come through autograd (the thin-side
    kind excepted): the padded problem must stay on the kind the case is there for."""
    for c in T.CASES:
        plain = c.Cin % 4 == 0 and c.Cout % 4 == 0
        assert plain or T.KINDS[c.expect["kind"]] == "ThinSide" or c.id in T.AUTOGRAD_PADDED, c.id
    for cid, (cin, cout, kind, two_stage) in T.AUTOGRAD_PADDED.items():
        c = T.BY_ID[cid]
        assert (cin, cout) == (c.Cin + (-c.Cin) % 4, c.Cout + (-c.Cout) % 4)
        plan = T.query(T.dims(c._replace(Cin=cin, Cout=cout)))
        assert (T.KINDS[plan["kind"]], plan["two_stage"]) == (kind, two_stage), (cid, plan)
        # ... and the wrapper's operand plan hands exactly these channel counts to ssbev_conv_bwd_weight
        saved = F.TILE_HINT
        F.TILE_HINT = c.hint
        try:
            p = F._conv_operands((c.B,) + tuple(c.grid) + (c.Cin,), T.wshape(c), (c.s, c.p, c.dl, bool(c.tr), c.op), False)
        finally:
            F.TILE_HINT = saved
        assert (p.wgrad_kind, p.wgrad.Cin, p.wgrad.Cout) == ("direct", cin, cout), (cid, p)


def test_bf16_storage_is_named_and_bad_arguments_are_refused():
    lib = capi.load()
    c = T.BY_ID["lds_wino"]
    plan = T.query(T.dims(c, precision=2))
    assert T.KINDS[plan["kind"]] == "Bf16Storage"
    assert plan["workspace"] == lib.ssbev_conv_bwd_weight_workspace(C.byref(T.dims(c, precision=2)))
    assert all(v == 0 for k, v in plan.items() if k not in ("kind", "workspace"))
    out = capi.ConvWgradPlan()
    assert lib.ssbev_conv_wgrad_plan_query(None, C.byref(out)) == capi.EINVAL
    assert lib.ssbev_conv_wgrad_plan_query(C.byref(T.dims(c)), None) == capi.EINVAL
    bad = T.dims(c)
    bad.kd = 0
    assert lib.ssbev_conv_wgrad_plan_query(C.byref(bad), C.byref(out)) == capi.EINVAL


def test_golden_tool_labels_come_from_the_query():
    """tools/make_golden_conv_dispatch.py::wgrad_kind names the query's kind with the labels of conv_dispatch.json."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location("make_golden_conv_dispatch", os.path.join(ROOT, "tools", "make_golden_conv_dispatch.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    assert len(tool.WGRAD_KINDS) == len(T.KINDS)
    for c in T.CASES:
        d = T.dims(c)
        assert tool.wgrad_kind(capi.load(), d) == tool.WGRAD_KINDS[T.query(d)["kind"]]
