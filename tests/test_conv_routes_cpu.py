"""The route planner against the table recorded before it existed (needs no GPU).

tests/golden/conv_routes.json (one line per geometry: pack / unpack of tools/route_table.py) holds every pure host query of the
convolution C ABI -- kernel names, BatchNorm-partial layouts, packed-weight sizes, workspaces -- for conv math 0, 1 and 2 over
the geometries of tools/route_table.py, recorded from the
commit named in its "recorded_from" (the last one whose entry points, name function and layout queries each restated the tile
choice on their own).  The table regenerated from the current library must equal it entry by entry: no geometry changes its
kernel, its tile structure or its workspace.

One entry depends on the device, not on the planner: the stem's weight-gradient workspace (iswm_conv2d_wgrad_workspace of the
stem_* geometries under conv math 1) is one slab per workgroup, and the workgroup count is capped by the compute units of the
current device -- 256 where there is none.  The recording was made without a device, so these rows hold on a machine without
a GPU and on a 256-CU part (MI355X); on a part with another CU count they would differ without any planner change."""
import importlib.util
import json
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_routes.json")


def _tool():
    spec = importlib.util.spec_from_file_location("route_table", os.path.join(ROOT, "tools", "route_table.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def tables():
    from iswm_amd import _lib
    lib = _lib.load()
    before = lib.iswm_get_conv_math()
    tool = _tool()
    with open(GOLDEN) as f:
        packed = json.load(f)
    assert packed["recorded_from"] and packed["queries"] == tool.QUERIES
    golden = tool.unpack(packed)                             # one line per geometry in the file; here {query: value}
    now = json.loads(json.dumps(tool.table(lib)))            # tuples -> lists, as the file has them
    assert lib.iswm_get_conv_math() == before                # the conv math it found is back
    return golden, now


def test_geometry_list_is_the_recorded_one(tables):
    golden, now = tables
    assert now["geometries"] == golden["geometries"]
    assert list(now["routes"]) == list(golden["routes"]) and list(now["packing"]) == list(golden["packing"])


def test_every_route_query_equals_the_recording(tables):
    golden, now = tables
    diff = []
    for gid, per_math in golden["routes"].items():
        for math, want in per_math.items():
            got = now["routes"][gid][math]
            assert sorted(got) == sorted(want), (gid, math)      # the same queries
            diff += ["%s math %s %s: %r != %r" % (gid, math, q, got[q], v) for q, v in want.items() if got[q] != v]
    assert not diff, "\n".join(diff[:40])


def test_every_packing_query_equals_the_recording(tables):
    golden, now = tables
    diff = ["%s math %s kind %d: %r != %r" % (key, math, kind, now["packing"][key][math][kind], v)
            for key, per_math in golden["packing"].items() for math, kinds in per_math.items() for kind, v in enumerate(kinds)
            if now["packing"][key][math][kind] != v]
    assert not diff, "\n".join(diff[:40])


def test_table_covers_every_family():
    """the recording reaches each kernel family and both sides of the planners' thresholds (a table of one kernel would pass
    the equality above and show nothing)"""
    with open(GOLDEN) as f:
        routes = _tool().unpack(json.load(f))["routes"]
    names = set(v for per_math in routes.values() for q in per_math.values() for k, v in q.items() if k.startswith("kernel_name") and v)
    families = set(n.split("<")[0] for n in names)
    assert families == {"k_conv_fwd", "k_conv_dgrad", "k_conv_fwd_u", "k_conv_dgrad_u", "k_conv_x6", "k_conv_x6_patch", "k_conv_pl2",
                        "k_conv_pl2w", "k_stem_fwd", "k_stem_wgrad", "k_conv_wgrad", "k_wgrad_pl", "k_wgrad_plw", "k_wgrad_pls"}
    one = lambda gid, q: routes[gid]["1"][q]
    for a, b, q in [("x6_tiles383", "x6_tiles384", "kernel_name.3"), ("x6_dg_2k_le", "x6_dg_2k_gt", "kernel_name.4"),
                    ("x6_m131071", "x6_m131072", "kernel_name.0"), ("x6_k960", "x6_m131072", "kernel_name.0"),
                    ("cols64_fwd", "cols72_fwd", "kernel_name.5"), ("wide_c252", "wide_c256", "kernel_name.5"),
                    ("wide_k192", "wide_c256", "kernel_name.5"), ("wide_dg_k448", "wide_dg_k512", "kernel_name.6"),
                    ("wide_m20480", "wide_c256", "pl2_tile_rows.0"), ("wg_k128", "wg_k136", "kernel_name.7"),
                    ("wg_p20000", "wg_p20001", "kernel_name.7"), ("wg_pad3", "wg_pad4", "kernel_name.7"),
                    ("wg_rect_c320", "wg_rect_pad4", "kernel_name.7"), ("w1_k864", "w1_k1440", "kernel_name.2"),
                    ("patch_small", "x6_patch", "kernel_name.3"), ("stem_wo16", "stem_wo17", "kernel_name.0")]:
        assert one(a, q) != one(b, q), (a, b, q)
