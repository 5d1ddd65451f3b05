"""tests/conv_ref.py on the CPU (no GPU, runs anywhere): the split emulation, the route table of
tests/test_conv_kernels_gpu.py, the condition that makes its bound meaningful, and the fp32 floors.

Route table: every GPU case names the kernel it has to reach; the library's own host-side queries (iswm_conv2d_kernel_name,
the packed-weight / planes predicates, the weight gradient's kernel kind and workspace) must select exactly that kernel.

Sensitivity condition: for every GPU case and every quantity, a product that lacks one of the five non-leading plane pairs,
or reads the mid plane where the lo plane belongs (either operand), must err by at least 3 x the bound (4 x floor) under the
case's own metric.  It is a condition on the INPUTS: a case that failed it would be reshaped (shorter K, or isolated).  The
stage-isolating kinds have zero operands outside one K stage, so there the mutant is confined to that stage by construction.
Exempt, with the reason: exact-integer operands (mid and lo planes are zero and the GPU test asserts equality -- the bound is 0)
and the one-plane bf16 mode (its kernels have no mid or lo plane to lose; the restatement runs on rounded operands).  The
exact-fp32 routes are held to the same condition: their bound must be as sharp as the bf16x6 routes'.

Floors: measured again here (one thread); each recorded figure must lie within [measured / 1.25, 2 x measured], and
profiles/conv_kernel_tests.txt must carry the recorded figures.  `pytest -s` prints them."""
import os
import re

import pytest
import torch

from tests import conv_ref as R
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOAT_CASES = [c for c in R.CASES if c[1] != "int"]
FLOAT_ASPP = [c for c in R.ASPP_CASES if c[1] != "int"]
SENSITIVITY = 3.0
MEASURED = {}


def put(k, v):
    MEASURED[k] = max(MEASURED.get(k, 0.0), v)


# ---- split3 / six_term -----------------------------------------------------------------------------------------------------
def test_split3_is_exact_and_bf16_representable():
    x = torch.randn(3, 11, 13, 72, generator=R.gen("split"))
    x[0, 0, 0, :8] = torch.tensor([0.0, 1e-30, -1e-30, -3e38, 1.0, -1.0, 65504.0, 3.0e38])   # tests/test_planes.py's special values
    x[0, 0, 1, :4] = torch.tensor([-0.0, 2.0 ** -100, 1.0 + 2.0 ** -23, -(2.0 - 2.0 ** -23)])
    hi, mid, lo = R.split3(x)
    assert torch.equal((hi + mid) + lo, x) and torch.equal(hi.double() + mid.double() + lo.double(), x.double())
    for p in (hi, mid, lo):
        assert not (p.view(torch.int32) & 0xFFFF).any() and torch.equal(p.bfloat16().float(), p)
    assert torch.equal(torch.signbit(hi[x != 0]), torch.signbit(x[x != 0]))
    assert bool((mid.abs() <= hi.abs() * 2.0 ** -7).all()) and bool((lo.abs() <= hi.abs() * 2.0 ** -15).all())


def test_six_term_product_and_what_each_missing_term_costs():
    """the GEMMs of the issue: six terms reproduce the fp32 product to ~1e-7 of the largest entry, any of ah.bl / al.bh / am.bm
    missing costs ~1e-5, ah.bm / am.bh or a misrouted plane ~3e-3 -- and the old 2e-5 bound saw none of the first three"""
    mm = lambda a, b: a.double() @ b.double()
    for m, k, n in [(500, 64, 64), (500, 576, 64), (300, 2048, 32)]:
        g = R.gen("gemm", k)
        x, w = torch.randn(m, k, generator=g), torch.randn(k, n, generator=g) * (2.0 / k) ** 0.5
        ref = mm(x, w)
        floor = rel_err(x @ w, ref)
        assert rel_err(R.six_term(mm, x, w), ref) <= 2e-7 and floor <= 1e-6
        errs = dict((name, rel_err(R.six_term(mm, x, w, keep), ref)) for name, keep in R.MUTANTS.items())
        print("gemm K %4d floor %.2e " % (k, floor) + " ".join("%s %.1e" % kv for kv in errs.items()))
        for name, e in errs.items():
            assert e >= SENSITIVITY * 4 * floor, (k, name, e, floor)
        assert sum(e < 2e-5 for e in errs.values()) == 3            # invisible to the older tests' bound
        # a term missing from ONE 64-wide K stage only: diluted by about sqrt(stages); isolating that stage restores it
        inside = lambda b: torch.cat([b[:64], torch.zeros_like(b[64:])])
        keep = R.MUTANTS["drop am.bm"]
        e_stage = rel_err(R.six_term(mm, x, w, keep, stage=inside), ref)
        e_iso = rel_err(R.six_term(mm, x, inside(w), keep), mm(x, inside(w)))
        assert e_stage <= errs["drop am.bm"] * 1.01 and e_iso >= 0.7e-5
        if k > 64:
            assert e_stage < 0.8 * errs["drop am.bm"]


# ---- route table -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", R.ROUTES, ids=[r.id for r in R.ROUTES])
def test_route_table(rt):
    plan = R.planned(rt)
    for op, name in rt.names.items():
        assert plan[op][1] == name, (rt.id, op, plan[op])
    if rt.mode in ("pl", "bf16pl"):                # a planes route takes the planes entry points wherever the network would
        cin, cout = rt.geom[3], rt.geom[4]
        if "fwd" in plan and R.planes_operand(rt, cin):
            assert plan["fwd"][0] == "iswm_conv2d_fwd_pl2"
        if "dgrad" in plan:
            assert (plan["dgrad"][0] == "iswm_conv2d_dgrad_pl2") == R.planes_operand(rt, cout)
        if "wgrad" in plan:                        # x travels as planes exactly when its channels are a multiple of 64
            assert (plan["wgrad"][0] == "iswm_conv2d_wgrad_planes") == R.planes_operand(rt, cin)
        if not rt.id.startswith("mb_"):            # every row from before the MobileNetV2 ones: planes x, the planes weight gradient
            assert cin % 64 == 0 and plan.get("wgrad", ("iswm_conv2d_wgrad_planes",))[0] == "iswm_conv2d_wgrad_planes"


def test_route_table_reaches_every_listed_kernel():
    names = set(v for rt in R.ROUTES for v in rt.names.values())
    want = ["k_conv_pl2<%d, 1, 3, %s>" % (r, d) for r in (8, 9, 10) for d in ("false", "true")]
    want += ["k_conv_pl2<%d, 2, 3, %s>" % (r, d) for r in (4, 5) for d in ("false", "true")]
    want += ["k_conv_pl2w<8, 3, false>", "k_conv_pl2w<8, 3, true>", "k_wgrad_pl<3>", "k_wgrad_plw<3>", "k_wgrad_pls<3>",
             "k_stem_fwd<6>", "k_stem_wgrad", "k_conv_x6<64, 64, false, true, 3>", "k_conv_x6<64, 64, true, true, 3>",
             "k_conv_x6_patch<false, 3>", "k_conv_x6_patch<true, 3>", "k_conv_wgrad<64, 64, 2, true, 3>", "k_conv_fwd_u<64, 64>",
             "k_conv_dgrad_u<64, 64>", "k_conv_fwd<64>", "k_conv_fwd<128>", "k_conv_dgrad<64>", "k_conv_dgrad<128>",
             "k_conv_x6<64, 64, false, true, 1>", "k_conv_pl2<8, 1, 1, false>", "k_wgrad_pls<1>",
             "k_conv_x6<128, 64, false, true, 3>", "k_conv_x6<128, 64, true, true, 3>", "k_conv_pl2w<9, 3, false>",
             "k_wgrad_pl<1>", "k_wgrad_plw<1>",
             # every instantiation of the round-1 kernels on csrc/conv_tile32.h that no row above names
             "k_conv_fwd_u<128, 64>", "k_conv_fwd_u<128, 128>", "k_conv_dgrad_u<128, 64>", "k_conv_dgrad_u<128, 128>",
             "k_conv_x6<64, 64, true, true, 1>", "k_conv_x6<128, 64, false, true, 1>", "k_conv_x6<128, 64, true, true, 1>",
             "k_conv_x6<64, 64, false, false, 3>", "k_conv_x6<64, 64, true, false, 3>", "k_conv_x6<128, 64, false, false, 3>",
             "k_conv_x6<128, 64, true, false, 3>", "k_conv_x6<128, 128, false, false, 3>"]
    assert not [n for n in want if n not in names]
    assert set(("k_conv_pl2w<8, 3, false>", "k_conv_pl2<8, 1, 3, false>")) <= set(
        v for rt in R.ROUTES if rt.id not in R.NO_DENSE for v in rt.names.values())       # a dense case reaches them too
    ws = dict((rid, R.wgrad_workspace(R.ROUTE[rid])) for rid in ("pl_narrow", "pl_wsplit", "pl_rect_split", "pl_rect", "pl_3x3"))
    assert ws["pl_narrow"] > 0 and ws["pl_wsplit"] > 0 and ws["pl_rect_split"] > 0      # multi-split: both reduction kernels run
    assert ws["pl_rect"] == 0 and ws["pl_3x3"] == 0
    s2, s3 = R.ROUTE["pl_s2"].geom, R.ROUTE["pl_s3"].geom
    assert (s2[6], s3[6]) == (2, 3)                                                       # the parity-ordered data gradient
    for cid in R.ASPP:
        n, h, w, cin, cout, rates = R.ASPP[cid]
        assert R.aspp_plan_bytes(cid, 0) > 0 and R.aspp_plan_bytes(cid, 1) > 0
    assert max(R.ASPP["aspp_small"][1:3]) < 18 and min(R.ASPP["aspp_large"][1:3]) > 18
    # the channel situations of MobileNetV2: (kernel, columns it writes, K chunks of 64, K) per operation of every row
    sit = set()
    for rt in R.ROUTES:
        cin, cout, k = rt.geom[3], rt.geom[4], rt.geom[5]
        for op, name in rt.names.items():
            cols, kk = {"fwd": (cout, cin), "dgrad": (cin, cout), "wgrad": (cout, 0)}[op]
            sit.add((name, cols, (kk + 63) // 64, k * k * kk))
    has = lambda name, pred: any(s[0] == name and pred(*s[1:]) for s in sit)
    for name in ("k_conv_pl2<4, 2, 3, false>", "k_conv_pl2<4, 2, 3, true>", "k_conv_x6<64, 64, false, true, 3>",
                 "k_conv_x6<64, 64, true, true, 3>", "k_conv_pl2<5, 2, 3, false>", "k_conv_pl2<5, 2, 3, true>"):
        assert has(name, lambda cols, ch, kk: cols < 64), name                 # fewer columns than a column block
    for name in ("k_conv_pl2<8, 1, 3, false>", "k_conv_pl2<8, 1, 3, true>"):
        assert has(name, lambda cols, ch, kk: ch >= 9 and ch % 2 == 1), name   # an odd chunk count >= 9 (9 and 15)
        assert has(name, lambda cols, ch, kk: cols in (96, 160)), name         # ragged columns below / above one block
    assert has("k_conv_pl2<9, 1, 3, false>", lambda cols, ch, kk: cols == 160 and ch == 9)
    assert has("k_conv_pl2<4, 2, 3, false>", lambda cols, ch, kk: ch == 3) and has("k_conv_pl2<8, 1, 3, false>", lambda cols, ch, kk: ch == 6)
    for name in ("k_conv_fwd<64>", "k_conv_dgrad<64>", "k_conv_fwd<128>"):       # general-K kernels below one 32-wide K step
        assert has(name, lambda cols, ch, kk: 0 < kk < 32), name
    assert has("k_conv_fwd<64>", lambda cols, ch, kk: kk in (36, 144)) and has("k_conv_dgrad<64>", lambda cols, ch, kk: kk == 144)
    for rows in (16, 24, 144):                                                 # output rows of k_conv_wgrad
        assert has("k_conv_wgrad<64, 64, 2, true, 3>", lambda cols, ch, kk: cols == rows), rows
    for cols_ in (24, 32, 96, 160):                                             # the accumulating data gradient of the residual blocks
        assert any(rt.geom[3] == cols_ and "dgrad" in rt.names for rt in R.ROUTES if rt.id.startswith("mb_")), cols_


def test_tiny_maps_take_the_walks_redivide_branch():
    """the pixel walk of the planes weight gradients advances KS pixels per step (32; 16 in k_wgrad_pls) with a carry when a step
    crosses at most one row boundary more than KS / Wo rows and one image (KS / Wo + 1 <= Ho), and divides again otherwise:
    every pl_tiny_* row has to be on the dividing side, over all of N x Ho x Wo or -- pl_tiny_rect -- over tap rectangles
    of which some carry and some divide, each of them over more than one stage (the first stage only divides)"""
    tiny = [rt for rt in R.ROUTES if rt.id.startswith("pl_tiny_")]
    assert sorted(rt.id for rt in tiny) == ["pl_tiny_3x3", "pl_tiny_d4", "pl_tiny_rect", "pl_tiny_s2"]
    for rt in tiny:
        n, h, w, cin, cout, k, stride, pad, dil = rt.geom
        ho, wo = R.out_size(h, k, stride, pad, dil), R.out_size(w, k, stride, pad, dil)
        ks = 16 if rt.names["wgrad"].startswith("k_wgrad_pls") else 32
        if rt.id != "pl_tiny_rect":
            assert ks // wo + 1 > ho, rt.id
            continue
        assert pad >= 4 and stride == 1 and cin % 256 == 0                  # rect mode (wgrad_rect_mode)
        assert R.wgrad_workspace(rt) == 0                                    # one split: a tile walks its whole rectangle
        walked = set()                 # the walk advances from the second stage on: a rectangle of more than KS pixels
        for t in range(k * k):
            dh, dw = (t // k) * dil - pad, (t % k) * dil - pad
            rh = max(0, min(ho, h - dh) - max(0, -dh))
            rw = max(0, min(wo, w - dw) - max(0, -dw))
            assert rh > 0 and rw > 0                                         # no empty tap: every rectangle is walked
            if n * rh * rw > ks:
                walked.add(ks // max(1, rw) + 1 <= rh)
        assert walked == {False, True}                                       # some rectangle carries, some divides again


def test_mobilenet_tile_thresholds():
    """each mb_*_m128 / _r9 / _r5 row sits at the SMALLEST map where the planner leaves the tile of the 286-row rows: one row
    fewer (a 1 x 1 x M map) still gets the small tile, the threshold itself the row's kernel.  A planner change that moves a
    threshold fails here instead of silently un-covering a tile."""
    at = {"mb_16_96_m128": ("fwd", 16385, "k_conv_fwd<64>"), "mb_96_24_m128": ("dgrad", 16385, "k_conv_dgrad<64>"),
          "mb_32_192_m128": ("fwd", 16257, "k_conv_x6<64, 64, false, true, 3>"),
          "mb_576_160_r9": ("fwd", 16385, "k_conv_pl2<8, 1, 3, false>"), "mb_192_32_r5": ("fwd", 32769, "k_conv_pl2<4, 2, 3, false>"),
          "mb_32_192_r5": ("dgrad", 32769, "k_conv_pl2<4, 2, 3, true>"),
          "mb_16_96_dg128": ("dgrad", 49025, "k_conv_x6<64, 64, true, true, 3>"),
          "mb_960_320_w9": ("fwd", 16385, "k_conv_pl2w<8, 3, false>")}
    assert set(at) == set(rt.id for rt in R.ROUTES if rt.id.startswith("mb_") and rt.sub)
    for rid, (op, m, small) in at.items():
        rt = R.ROUTE[rid]
        n, h, w = rt.geom[:3]
        assert m <= n * h * w < m + 1024, rid
        flat = lambda rows: rt._replace(geom=(1, 1, rows) + tuple(rt.geom[3:]))
        assert R.planned(flat(m))[op][1] == rt.names[op], rid
        below = R.planned(flat(m - 1))[op][1]
        assert below != rt.names[op] and below == small, (rid, below)


def test_every_route_has_every_operand_kind():
    for rt in R.ROUTES:
        ks = R.kinds(rt)
        assert ks[:4] == ["dense", "scaled", "int", "s0"] or (rt.id in R.NO_DENSE and ks[:2] == ["int", "s0"])
        if rt.id.startswith("stem"):                # 7 x 7 x 4: first and last tap forward, first and last pixel step backward
            assert ks[4:] == ["sL"]
            continue
        if rt.geom[5] == 3:
            assert all("t%d" % t in ks for t in range(1, 9))
        stages = rt.geom[5] ** 2 * max(rt.geom[3] if "fwd" in rt.names else 0, rt.geom[4] if "dgrad" in rt.names else 0) // 64
        if stages > 2:
            assert "s1" in ks and "sL" in ks


def test_isolating_operands_leave_one_stage():
    rt = R.ROUTE["pl_3x3"]
    for kind, tap, c0 in (("s0", 0, 0), ("s1", 0, 64), ("sL", 8, 64), ("t5", 5, 0)):
        o = R.operands(rt, kind)
        nz = o["w_f"].view(128, 9, 128).abs().sum(0) > 0
        assert nz[tap, c0:c0 + 64].all() and int(nz.sum()) == 64
        nz = o["w_d"].view(128, 9, 128).abs().sum(2) > 0
        assert nz[c0:c0 + 64, tap].all() and int(nz.sum()) == 64
        assert int((o["dy_w"].view(-1, 128).abs().sum(1) > 0).sum()) in (32, 135 - 128)
    o = R.operands(R.ROUTE["pl_wide"], "h1")
    nz = o["w_f"].view(512, 512).abs().sum(0) > 0
    assert nz[32:64].all() and int(nz.sum()) == 32
    o = R.operands(R.ROUTE["pl_3x3"], "int")
    for k in ("x", "dy", "w_f", "base"):
        hi, mid, lo = R.split3(o[k])
        assert torch.equal(hi, o[k]) and not mid.any() and not lo.any()


# ---- sensitivity + floors, case by case ------------------------------------------------------------------------------------
def _sensitivity(tag, key_of, ops, refs, factors, exempt, base=None):
    """base: what the accumulating data gradient adds into (on the compared channels) -- dx_acc is held to its own bound"""
    for q, (f, a, b) in ops.items():
        if exempt or float(refs[q].abs().max()) == 0.0:      # (a zeroed ASPP branch next to the isolated one: nothing to lose)
            continue
        terms = R.plane_terms(f, a, b)
        checks = [(q, lambda m: m)] + ([("dx_acc", lambda m: base + m)] if q == "dx" else [])
        for qq, form in checks:
            bound = R.bound(key_of(qq))
            worst = min((rel_err(form(R.combine(terms, keep).double()) * factors[q], refs[qq]), name) for name, keep in R.MUTANTS.items())
            print("sens %-30s %-22s weakest mutant %.2e (%s) = %.1f x bound" % (tag, key_of(qq), worst[0], worst[1], worst[0] / bound))
            assert worst[0] >= SENSITIVITY * bound, (tag, qq, worst, bound)


DONE = set()


def measure(rid, kind):
    """floors of one case into MEASURED (once), then its sensitivity condition"""
    if (rid, kind) in DONE:
        return
    if rid in R.ASPP:
        os_ = R.aspp_operands(rid, kind)
        ref = R.aspp_restate(rid, os_)
        for q, v in R.aspp_floor(rid, os_, ref).items():
            put("%s.%s" % (rid, q), v)
        rts, ops = R.aspp_routes(rid), R.aspp_bilinear_ops(rid, os_)
        br = lambda q: int(q[1]) if q[0] == "b" else 0
        factors = dict((q, R.factor(rts[br(q)], os_[br(q)], q.split(".")[-1])) for q in ops)
        _sensitivity("%s-%s" % (rid, kind), lambda q: "%s.%s" % (rid, q), ops, ref, factors, False, os_[0]["base"].double())
    else:
        rt = R.ROUTE[rid]
        o = R.operands(rt, kind)
        ref = R.restate(rt, o)
        for q, v in R.floor(rt, o, ref).items():
            put(R.check_name(rt, q), v)
        if kind == "dense" and rid in R.SLICE_ROUTES:
            bias = R.bias_of(rt)
            with R.one_thread():
                f32 = R.restate(rt, o, torch.float32, bias=bias)["y"]
            put(R.check_name(rt, "y_bias"), rel_err(f32, R.restate(rt, o, bias=bias)["y"]))
        factors = dict((q, R.factor(rt, o, q)) for q in ("y", "dx", "dw"))
        _sensitivity("%s-%s" % (rid, kind), lambda q: R.check_name(rt, q), R.bilinear_ops(rt, o), ref, factors, R.MATH[rt.mode] == 2,
                     o["base"][..., R.channels(rt)[1]].double())
    DONE.add((rid, kind))


@pytest.mark.parametrize("rid,kind", FLOAT_CASES + FLOAT_ASPP, ids=["%s-%s" % c for c in FLOAT_CASES + FLOAT_ASPP])
def test_case_floor_and_sensitivity(rid, kind):
    measure(rid, kind)


def test_floors_are_the_recorded_ones():
    """the case tests above have measured every floor when the whole file runs; alone, this test measures what is missing"""
    for rid, kind in FLOAT_CASES + FLOAT_ASPP:
        measure(rid, kind)
    for k, v in sorted(MEASURED.items()):
        print("floor %-26s measured %.3e  recorded %.3e" % (k, v, R.FLOOR.get(k, float("nan"))))
    assert set(MEASURED) == set(R.FLOOR), set(MEASURED) ^ set(R.FLOOR)
    for k, v in MEASURED.items():
        assert R.FLOOR[k] / 2 <= v <= 1.25 * R.FLOOR[k], "%s: measured %.3e, recorded %.3e" % (k, v, R.FLOOR[k])


def test_profile_carries_the_recorded_floors():
    text = open(os.path.join(ROOT, "profiles", "conv_kernel_tests.txt")).read()
    rows = dict((m.group(1), (float(m.group(2)), float(m.group(3)))) for m in
                re.finditer(r"^(\S+\.\S+)\s+(\d\.\de[-+]\d\d)\s+(\d\.\de[-+]\d\d)\s", text, re.M))
    for k, v in R.FLOOR.items():
        assert k in rows, k
        assert rows[k][0] == float("%.1e" % v) and abs(rows[k][1] - R.bound(k)) <= 0.06 * R.bound(k), (k, rows[k], v)
