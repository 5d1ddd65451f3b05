#!/usr/bin/env python
"""Every pure host query of the convolution C ABI over a fixed geometry list, as JSON.  Needs no GPU.

    python tools/route_table.py [--lib path/to/libiswm_hip.so] [--recorded-from COMMIT] [-o out.json]

For conv math 0, 1 and 2 and each geometry: iswm_conv2d_kernel_name kinds 0-7 (each where its entry point's own
preconditions hold), the BatchNorm-partial layouts (stat_tile_rows / stat_tiles, fwd_packed_stat_layout, pl2_tile_rows,
dgrad_pl2_stat_tiles), the packed-weight sizes, dgrad_wants_wt and the weight-gradient workspaces; and
iswm_packed_weight_bytes / iswm_pack_job_blocks kinds 0-3 over the (Cout, taps, Cin) triples of the list.

tests/golden/conv_routes.json is this table recorded from the commit BEFORE the route planner (csrc/conv_api.hip) existed;
tests/test_conv_routes_cpu.py regenerates it from the current library and compares entry by entry.  --lib points the run at
another build of the library (the recording run).

The MobileNetV2 rows (the mb_* routes of tests/conv_ref.py, the depthwise shapes dw9 .. dw12 and the mbv2_* geometries of
conv_ref.BENCH_MOBILENET) were added later and recorded from the planner itself (the file's "recorded_later" names the commit): they pin
what the planner answers today from here on and prove nothing by themselves -- what they select is checked against float64 in
tests/test_conv_kernels_gpu.py.  --keep FILE copies "recorded_from" and every row FILE already has from FILE (after checking
that the queried library still gives them) and records only the rows FILE lacks."""
import argparse
import collections
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# Edge shapes: one geometry on either side of each threshold of the planners.  (n, h, w, cin, cout, k, stride, pad, dil)
EDGES = collections.OrderedDict([
    # conv_pick_tile_x6: tiles64 = ceil(M / 128) * ceil(cols / 64) < 384 -> 64 x 64 tiles
    ("x6_tiles383", (1, 1, 49024, 64, 64, 1, 1, 0, 1)), ("x6_tiles384", (1, 1, 49025, 64, 64, 1, 1, 0, 1)),
    # ... write-dominated pointwise data gradient: 2 * K <= cols
    ("x6_dg_2k_le", (1, 1, 30000, 128, 64, 1, 1, 0, 1)), ("x6_dg_2k_gt", (1, 1, 30000, 128, 96, 1, 1, 0, 1)),
    # ... 128 x 128 tiles: forward, cols % 128 == 0, M >= 131072 and K >= 1024
    ("x6_m131071", (1, 1, 131071, 1024, 128, 1, 1, 0, 1)), ("x6_m131072", (1, 1, 131072, 1024, 128, 1, 1, 0, 1)),
    ("x6_k960", (1, 1, 131072, 960, 128, 1, 1, 0, 1)), ("x6_c192", (1, 1, 131072, 1024, 192, 1, 1, 0, 1)),
    # cols <= 64: the 64-column layouts of k_conv_pl2, pick_tile, use_narrow_tile
    ("cols64_fwd", (2, 17, 19, 64, 64, 1, 1, 0, 1)), ("cols72_fwd", (2, 17, 19, 64, 72, 1, 1, 0, 1)),
    ("cols72_dgrad", (2, 17, 19, 72, 64, 1, 1, 0, 1)), ("cols48", (1, 128, 129, 48, 48, 1, 1, 0, 1)),
    ("cols68_f32", (1, 128, 129, 48, 68, 1, 1, 0, 1)), ("cols192", (1, 128, 129, 64, 192, 1, 1, 0, 1)),
    ("cols196", (1, 128, 129, 64, 196, 1, 1, 0, 1)),
    # conv_pl2_plan: 256-column tiles from cols 256 and K 256 (data gradient: K 512) where two rounds of 128-column tiles become one
    ("wide_c252", (1, 1, 20640, 256, 252, 1, 1, 0, 1)), ("wide_c256", (1, 1, 20640, 256, 256, 1, 1, 0, 1)),
    ("wide_k192", (1, 1, 20640, 192, 256, 1, 1, 0, 1)), ("wide_dg_k448", (1, 1, 20640, 256, 448, 1, 1, 0, 1)),
    ("wide_dg_k512", (1, 1, 20640, 256, 512, 1, 1, 0, 1)), ("wide_dg_c252", (1, 1, 20640, 252, 512, 1, 1, 0, 1)),
    ("wide_m20480", (1, 1, 20480, 256, 256, 1, 1, 0, 1)), ("wide_s2_dgrad", (1, 2, 41280, 512, 512, 1, 2, 0, 1)),
    # planes weight gradient: 256-wide tiles (Ktot <= 128; pointwise and P > 20000; padding waste)
    ("wg_k128", (1, 13, 13, 128, 64, 1, 1, 0, 1)), ("wg_k136", (1, 13, 13, 136, 64, 1, 1, 0, 1)),
    ("wg_k320", (1, 13, 13, 320, 64, 1, 1, 0, 1)), ("wg_k384", (1, 13, 13, 384, 64, 1, 1, 0, 1)),
    ("wg_p20000", (1, 1, 20000, 256, 64, 1, 1, 0, 1)), ("wg_p20001", (1, 1, 20001, 256, 64, 1, 1, 0, 1)),
    # ... culling vote from pad 4; tap rectangles with Cin % 256 == 0 as well
    ("wg_pad3", (1, 19, 19, 128, 64, 3, 1, 3, 3)), ("wg_pad4", (1, 19, 19, 128, 64, 3, 1, 4, 4)),
    ("wg_rect_pad3", (1, 19, 19, 256, 64, 3, 1, 3, 3)), ("wg_rect_pad4", (1, 19, 19, 256, 64, 3, 1, 4, 4)),
    ("wg_rect_c320", (1, 19, 19, 320, 64, 3, 1, 4, 4)), ("wg_rect_s2", (1, 19, 19, 256, 64, 3, 2, 4, 4)),
    # ... one column block per XCD: (Cin >> 8) == 8 and taps of similar size
    ("wg_rect_c1792", (1, 33, 33, 1792, 64, 3, 1, 6, 6)), ("wg_rect_c2048", (1, 33, 33, 2048, 64, 3, 1, 6, 6)),
    ("wg_rect_c2304", (1, 33, 33, 2304, 64, 3, 1, 6, 6)), ("wg_rect_c2048_d18", (1, 33, 33, 2048, 64, 3, 1, 18, 18)),
    # round-1 weight gradient: 128 x 128 tiles need Cout % 128 == 0 and Ktot % 128 == 0 or >= 1024
    ("w1_k864", (1, 13, 13, 96, 128, 3, 1, 1, 1)), ("w1_k1440", (1, 13, 13, 160, 128, 3, 1, 1, 1)),
    ("w1_k1152_c64", (1, 13, 13, 128, 64, 3, 1, 1, 1)), ("w1_split", (4, 65, 65, 128, 128, 1, 1, 0, 1)),
    # halo patches: 80 % row utilisation; the stem's Wo > 16
    ("patch_small", (1, 5, 5, 64, 64, 3, 1, 1, 1)), ("patch_s2", (1, 21, 23, 64, 64, 3, 2, 1, 1)),
    ("stem_wo16", (1, 37, 31, 4, 64, 7, 2, 3, 1)), ("stem_wo17", (1, 37, 33, 4, 64, 7, 2, 3, 1)),
    ("stem_ld", (1, 38, 38, 4, 64, 7, 2, 3, 1, 4, 72)),
])


def geometries():
    """{id: (n, h, w, cin, cout, k, stride, pad, dil[, ldx, ldy])}: the routes of tests/conv_ref.py, the producer cases of
    tests/bn_partials_ref.py (forward extras, ASPP branches, depthwise shapes as dense descriptors), the production shapes,
    the edge list and MobileNetV2's bench geometries"""
    from tests import bn_partials_ref as B
    from tests import conv_ref as R
    from tests.test_production_shapes import PROD
    out = collections.OrderedDict()
    for rt in R.ROUTES + B.EXTRA + [b for cid in R.ASPP for b in R.aspp_routes(cid)]:
        out[rt.id] = tuple(rt.geom)
    for i, (n, h, w, c, cw, s, d, _) in enumerate(B.dw_cases()):
        out["dw%d" % i] = (n, h, w, c, c, 3, s, d, d)
    for c in PROD:
        out["prod_n%d_%dx%d_c%d-%d_k%d_s%d_d%d" % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[8])] = tuple(c)
    out.update(EDGES)
    # MobileNetV2 at the maps of the bench input.  Like the routes, the list lives with the tests (conv_ref.BENCH_MOBILENET), so
    # that this tool and a tests tree always agree on the geometry list -- also a tests tree from before that list existed
    out.update(getattr(R, "BENCH_MOBILENET", {}))
    return out


def _desc(g):
    from iswm_amd import _lib
    from tests.conv_ref import out_size
    n, h, w, cin, cout, k, stride, pad, dil = g[:9]
    ldx, ldy = (g[9], g[10]) if len(g) > 9 else (cin, cout)
    return _lib.ConvDesc(n, h, w, cin, out_size(h, k, stride, pad, dil), out_size(w, k, stride, pad, dil), cout, k, k, stride, pad,
                         dil, ldx, ldy)


def _name(lib, ref, kind):
    buf = ctypes.create_string_buffer(64)
    assert lib.iswm_conv2d_kernel_name(ref, kind, buf, 64) == 0
    return buf.value.decode()


# one row per (geometry, conv math): kernel names (an index into the file's "kernels" list; null where the entry point's own
# preconditions do not hold) and then the layout / size / workspace queries, in this order
QUERIES = ["kernel_name.%d" % k for k in range(8)] + [
    "stat_tile_rows", "stat_tiles", "fwd_packed_stat_layout", "packed_weight_bytes.0", "pl2_weight_bytes.0", "pl2_tile_rows.0",
    "packed_weight_bytes.1", "pl2_weight_bytes.1", "pl2_tile_rows.1", "dgrad_pl2_stat_tiles", "dgrad_wants_wt", "wgrad_workspace",
    "wgrad_planes_ok", "wgrad_planes_workspace"]


def queries(lib, g):
    """every query of one geometry under the library's current conv math: {name of QUERIES: value}"""
    d = _desc(g)
    ref = ctypes.byref(d)
    q = {}
    # the entry points' own preconditions (validate() holds for the whole list): gathered channels % 32 for the packed
    # kernels, % 64 and an 8-element pitch for the planes kernels, everything % 8 for the planes weight gradient
    ok = {0: True, 1: True, 2: True, 3: d.Cin % 32 == 0, 4: d.Cout % 32 == 0, 5: d.Cin % 64 == 0 and d.ldx % 8 == 0,
          6: d.Cout % 64 == 0 and d.ldy % 8 == 0,
          7: d.Cin % 8 == 0 and d.Cout % 8 == 0 and d.ldx % 8 == 0 and d.ldy % 8 == 0}
    for kind in range(8):
        q["kernel_name.%d" % kind] = _name(lib, ref, kind) if ok[kind] else None
    q["stat_tile_rows"] = lib.iswm_conv2d_stat_tile_rows(ref)
    q["stat_tiles"] = lib.iswm_conv2d_stat_tiles(ref)
    t, r = ctypes.c_int(-1), ctypes.c_int(-1)
    assert lib.iswm_conv2d_fwd_packed_stat_layout(ref, ctypes.byref(t), ctypes.byref(r)) == 0
    q["fwd_packed_stat_layout"] = [t.value, r.value]
    for kind in (0, 1):
        q["packed_weight_bytes.%d" % kind] = lib.iswm_conv2d_packed_weight_bytes(ref, kind)
        q["pl2_weight_bytes.%d" % kind] = lib.iswm_conv2d_pl2_weight_bytes(ref, kind)
        q["pl2_tile_rows.%d" % kind] = lib.iswm_conv2d_pl2_tile_rows(ref, kind)
    q["dgrad_pl2_stat_tiles"] = lib.iswm_conv2d_dgrad_pl2_stat_tiles(ref)
    q["dgrad_wants_wt"] = lib.iswm_conv2d_dgrad_wants_wt(ref)
    q["wgrad_workspace"] = lib.iswm_conv2d_wgrad_workspace(ref)
    q["wgrad_planes_ok"] = lib.iswm_conv2d_wgrad_planes_ok(ref)
    q["wgrad_planes_workspace"] = lib.iswm_conv2d_wgrad_planes_workspace(ref)
    return q


def table(lib):
    """{"geometries": {id: geom}, "routes": {id: {math: {query: value}}}, "packing": {"Cout,taps,Cin": {math: [[bytes, blocks] x 4]}}};
    leaves the library's conv math as it found it"""
    geoms = geometries()
    triples = sorted(set((g[4], g[5] * g[5], g[3]) for g in geoms.values()))
    routes = collections.OrderedDict((gid, collections.OrderedDict()) for gid in geoms)
    packing = collections.OrderedDict(("%d,%d,%d" % t, collections.OrderedDict()) for t in triples)
    old = lib.iswm_get_conv_math()
    try:
        for math in (0, 1, 2):
            assert lib.iswm_set_conv_math(math) == 0
            for gid, g in geoms.items():
                routes[gid][str(math)] = queries(lib, g)
            for t in triples:
                packing["%d,%d,%d" % t][str(math)] = [[lib.iswm_packed_weight_bytes(t[0], t[1], t[2], kind),
                                                       lib.iswm_pack_job_blocks(t[0], t[1], t[2], kind)] for kind in range(4)]
    finally:
        lib.iswm_set_conv_math(old)
    return collections.OrderedDict([("geometries", collections.OrderedDict((k, list(v)) for k, v in geoms.items())),
                                    ("routes", routes), ("packing", packing)])


# ---- the file form: one line per geometry, rows in QUERIES order, kernel names as indices into one sorted list ---------------------
def pack(tab, recorded_from=None, recorded_later=None, names=()):
    """names: a kernel list to keep (its indices stay; names it lacks are appended, sorted)"""
    found = set(q[k] for per in tab["routes"].values() for q in per.values() for k in QUERIES[:8] if q[k] is not None)
    names = list(names) + sorted(found - set(names))
    row = lambda q: [None if q[k] is None else names.index(q[k]) for k in QUERIES[:8]] + [q[k] for k in QUERIES[8:]]
    return collections.OrderedDict([
        ("recorded_from", recorded_from), ("recorded_later", recorded_later), ("queries", QUERIES), ("kernels", names),
        ("routes", collections.OrderedDict((gid, [tab["geometries"][gid]] + [row(per[m]) for m in "012"])
                                           for gid, per in tab["routes"].items())),
        ("packing", collections.OrderedDict((k, [per[m] for m in "012"]) for k, per in tab["packing"].items()))])


def unpack(packed):
    """the form table() returns, from the file form"""
    names = packed["kernels"]
    def q(row):
        return dict((k, v if i >= 8 or v is None else names[v]) for i, (k, v) in enumerate(zip(packed["queries"], row)))
    return collections.OrderedDict([
        ("geometries", collections.OrderedDict((gid, v[0]) for gid, v in packed["routes"].items())),
        ("routes", collections.OrderedDict((gid, dict((str(m), q(v[1 + m])) for m in range(3))) for gid, v in packed["routes"].items())),
        ("packing", collections.OrderedDict((k, dict((str(m), v[m]) for m in range(3))) for k, v in packed["packing"].items()))])


def dumps(packed):
    """JSON with one line per geometry / weight shape"""
    j = lambda v: json.dumps(v, separators=(",", ":"))
    out = ["{", '"recorded_from":%s,' % j(packed["recorded_from"])]
    if packed.get("recorded_later"):
        out.append('"recorded_later":%s,' % j(packed["recorded_later"]))
    out += ['"queries":%s,' % j(packed["queries"]), '"kernels":%s,' % j(packed["kernels"])]
    for key in ("routes", "packing"):
        out.append('"%s":{' % key)
        items = list(packed[key].items())
        out += ['%s:%s%s' % (j(k), j(v), "," if i + 1 < len(items) else "") for i, (k, v) in enumerate(items)]
        out.append("}," if key == "routes" else "}")
    return "\n".join(out + ["}"]) + "\n"


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", help="libiswm_hip.so to query instead of this tree's")
    ap.add_argument("--recorded-from", help="commit the queried library was built from (stored in the output)")
    ap.add_argument("--keep", help="an earlier recording: its rows and its recorded_from stay, only the rows it lacks are recorded")
    ap.add_argument("-o", "--output", help="file to write (default: stdout)")
    a = ap.parse_args()
    from iswm_amd import _lib
    if a.lib:
        _lib.LIB_PATH = os.path.abspath(a.lib)
    tab = table(_lib.load())
    if a.keep:
        with open(a.keep) as f:
            old = json.load(f)
        packed = pack(tab, old["recorded_from"], None, old["kernels"])
        for key in ("routes", "packing"):
            stale = [k for k, v in old[key].items() if json.loads(json.dumps(packed[key].get(k))) != v]
            assert not stale, "the queried library no longer gives the kept rows: %s" % stale[:8]
        later = dict(old.get("recorded_later") or {})
        new = [k for k in packed["routes"] if k not in old["routes"]]
        if new:
            later[a.recorded_from or "unknown"] = later.get(a.recorded_from or "unknown", []) + new
        packed["recorded_later"] = later or None
    else:
        packed = pack(tab, a.recorded_from)
    text = dumps(packed)
    if a.output:
        with open(a.output, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
