"""ops.conv_plan -- the one place the op wrappers decide how a conv call runs -- against the test's own restatement of the
entry-point ladder (tests/conv_ref.planned) and against the direct host queries of the C ABI.  Needs no GPU.

Covered: every route of conv_ref.ROUTES (entry point and kernel name equal planned()); every geometry of
tools/route_table.geometries() under conv math 0 / 1 / 2, both settings of ops._USE_PACKED and ops._PLANES_ENV, the three
operations and both operand forms (weight form and bytes, BatchNorm-partial layout, stat tiles and workspace equal the query
that belongs to the chosen entry point; every rung above the chosen one does not apply); and the cache: flipping the conv math
or a switch between two calls on one descriptor gives what an empty cache gives."""
import ctypes
import importlib.util
import os

import pytest

from tests import conv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture()
def lib():
    from iswm_amd import _lib
    lib = _lib.load()
    before = lib.iswm_get_conv_math()
    yield lib
    lib.iswm_set_conv_math(before)


def _tool():
    spec = importlib.util.spec_from_file_location("route_table", os.path.join(ROOT, "tools", "route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def plan_for(d, op, planes):
    """what a wrapper does with an operand of this form: a Planes operand no planes kernel takes is joined and planned again
    (here on the same descriptor: the pitches of the lists are those of a dense tensor either way)"""
    from iswm_amd import ops
    p = ops.conv_plan(d, op, planes)
    if planes and not p.planes:
        assert p.entry is None and p.name is None
        p = ops.conv_plan(d, op, False)
    assert p.entry is not None and R.KIND[p.entry] == p.kind
    return p


@pytest.mark.parametrize("rid", [rt.id for rt in R.ROUTES])
def test_plan_equals_the_restated_ladder(rid, lib):
    rt = R.ROUTE[rid]
    cin, cout = rt.geom[3], rt.geom[4]
    want = R.planned(rt)
    with R.conv_math(rt):
        got = {}
        if "fwd" in rt.names:
            got["fwd"] = plan_for(R.desc(rt), "fwd", R.planes_operand(rt, cin))
        if "dgrad" in rt.names:
            got["dgrad"] = plan_for(R.desc(rt), "dgrad", R.planes_operand(rt, cout))
        if "wgrad" in rt.names:        # the planes kernel is asked about Cout padded to 8, the fp32 one about the conv itself
            from iswm_amd import ops
            p = ops.conv_plan(R.desc(rt, cout=(cout + 7) // 8 * 8), "wgrad", True) if R.planes_operand(rt, cin) else None
            got["wgrad"] = p if (p is not None and p.planes) else plan_for(R.desc(rt), "wgrad", False)
    assert {k: (p.entry, p.name) for k, p in got.items()} == want


def check_against_queries(lib, ops, d, op, planes, p):
    """the fields of plan p against the queries of its entry point, and the rungs above it against theirs"""
    ref, m = ctypes.byref(d), d.N * d.Ho * d.Wo
    ohwi_bytes = 4 * d.Cout * d.KH * d.KW * d.Cin
    planes_on = ops._PLANES_ENV and lib.iswm_get_conv_math() >= 1
    dirn = int(op == "dgrad")
    none = dict(wform=None, wbytes=0, tiles=0, tile_rows=0, rows_stored=False, stat_tiles=0, workspace=0)
    if op == "wgrad":
        ok = planes and planes_on and bool(lib.iswm_conv2d_wgrad_planes_ok(ref))
        if planes:
            want = dict(none, entry="iswm_conv2d_wgrad_planes", workspace=lib.iswm_conv2d_wgrad_planes_workspace(ref)) if ok \
                else dict(none, entry=None)
        else:
            want = dict(none, entry="iswm_conv2d_wgrad", workspace=lib.iswm_conv2d_wgrad_workspace(ref))
    elif planes:
        nb = lib.iswm_conv2d_pl2_weight_bytes(ref, dirn) if planes_on else 0
        if not nb:
            want = dict(none, entry=None)
        elif dirn:
            want = dict(none, entry="iswm_conv2d_dgrad_pl2", wform="pl2", wbytes=nb, stat_tiles=lib.iswm_conv2d_dgrad_pl2_stat_tiles(ref))
        else:
            tr = lib.iswm_conv2d_pl2_tile_rows(ref, 0)
            want = dict(none, entry="iswm_conv2d_fwd_pl2", wform="pl2", wbytes=nb, tile_rows=tr, tiles=(m + tr - 1) // tr)
    else:
        nb = lib.iswm_conv2d_packed_weight_bytes(ref, dirn) if ops._USE_PACKED else 0
        if nb and dirn:
            want = dict(none, entry="iswm_conv2d_dgrad_packed", wform="x6", wbytes=nb)
        elif nb:
            t, r = ctypes.c_int(-1), ctypes.c_int(-1)
            assert lib.iswm_conv2d_fwd_packed_stat_layout(ref, ctypes.byref(t), ctypes.byref(r)) == 0
            want = dict(none, entry="iswm_conv2d_fwd_packed", wform="x6", wbytes=nb, tiles=t.value, tile_rows=r.value, rows_stored=True)
        elif dirn:
            wt = bool(lib.iswm_conv2d_dgrad_wants_wt(ref))
            want = dict(none, entry="iswm_conv2d_dgrad_wt" if wt else "iswm_conv2d_dgrad", wform="wt" if wt else "ohwi", wbytes=ohwi_bytes)
        else:
            want = dict(none, entry="iswm_conv2d_fwd", wform="ohwi", wbytes=ohwi_bytes, tiles=lib.iswm_conv2d_stat_tiles(ref),
                        tile_rows=lib.iswm_conv2d_stat_tile_rows(ref))
    want["planes"] = bool(planes and want["entry"])
    want["kind"] = R.KIND[want["entry"]] if want["entry"] else 0
    want["name"] = R.kernel_name(lib, d, want["kind"]) if want["entry"] else None
    assert p._asdict() == want, (op, planes, p, want)


def test_plan_fields_equal_the_direct_queries(lib, monkeypatch):
    from iswm_amd import ops
    tool = _tool()
    n = 0
    for gid, g in tool.geometries().items():
        d = tool._desc(g)
        for math in (0, 1, 2):
            assert lib.iswm_set_conv_math(math) == 0
            for packed in (True, False):
                for env in (True, False):
                    monkeypatch.setattr(ops, "_USE_PACKED", packed)
                    monkeypatch.setattr(ops, "_PLANES_ENV", env)
                    for op in ("fwd", "dgrad", "wgrad"):
                        for planes in (False, True):
                            check_against_queries(lib, ops, d, op, planes, ops.conv_plan(d, op, planes))
                            n += 1
    assert n == len(tool.geometries()) * 3 * 2 * 2 * 3 * 2


def test_pitches_are_part_of_the_key(lib):
    """the planes weight gradient needs pitches that are multiples of 8 elements (iswm_conv2d_wgrad_planes_ok): the same
    geometry at another pitch gets another answer, whichever was asked first"""
    from iswm_amd import ops
    tool = _tool()
    g = (2, 17, 19, 64, 64, 1, 1, 0, 1)
    lib.iswm_set_conv_math(1)
    for order in ((64, 68), (68, 64)):
        ops._PLANS.clear()
        got = {ldx: ops.conv_plan(tool._desc(g + (ldx, 64)), "wgrad", True).entry for ldx in order}
        assert got == {64: "iswm_conv2d_wgrad_planes", 68: None}


def test_no_stale_plan_after_a_switch_or_the_conv_math_moves(lib, monkeypatch):
    from iswm_amd import ops
    d = _tool()._desc((2, 17, 19, 64, 64, 1, 1, 0, 1))
    settings = [(math, packed, env) for math in (0, 1, 2) for packed in (True, False) for env in (True, False)]

    def ask(math, packed, env):
        lib.iswm_set_conv_math(math)
        monkeypatch.setattr(ops, "_USE_PACKED", packed)
        monkeypatch.setattr(ops, "_PLANES_ENV", env)
        return [ops.conv_plan(d, op, planes) for op in ("fwd", "dgrad", "wgrad") for planes in (False, True)]

    cold = {}
    for s in settings:
        ops._PLANS.clear()
        cold[s] = ask(*s)
    ops._PLANS.clear()
    for s in settings + settings[::-1] + settings[::5]:          # every setting after every kind of predecessor, cache warm
        assert ask(*s) == cold[s], s
    # ... and the answers do move where the library's do: the planes kernels need a planes conv math and the switch,
    # the packed kernels theirs
    fwd_pl, fwd_f32 = 1, 0
    assert cold[(1, True, True)][fwd_pl].entry == "iswm_conv2d_fwd_pl2" and cold[(0, True, True)][fwd_pl].entry is None
    assert cold[(1, True, False)][fwd_pl].entry is None
    assert cold[(1, True, True)][fwd_f32].entry == "iswm_conv2d_fwd_packed"
    assert cold[(1, False, True)][fwd_f32].entry == "iswm_conv2d_fwd"
    assert cold[(1, True, True)][fwd_pl].name != cold[(2, True, True)][fwd_pl].name
