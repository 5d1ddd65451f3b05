"""tests/dw3_ref.py on the CPU (no GPU, runs anywhere): which branch of csrc/dwconv3.hip every case of tests/test_dwconv3_gpu.py
reaches, the fp32 floors, and the faults those branches can have.

Branches: through the library's host queries (iswm_dwconv3x3_stat_tile_rows / _stat_tiles, iswm_dwconv3x3_bwd_workspace) and the
restated channel layout (dw3_ref.layout).  The 8-pixel statistic tile and the 2048-chunk cap are thresholds of the planner; each
big shape is held to its side of the threshold and a neighbouring shape to the other, so a planner change that moves one fails
here instead of silently un-covering a kernel.

Floors: measured again here (one thread); each recorded figure must lie within [measured / 1.25, 2 x measured], and
profiles/streaming_kernel_tests.txt must carry the recorded figures.

Emulated faults: each is applied to the float64 restatement of the case that reaches the branch and must miss an assertion of
the GPU file by >= 3 x its bound (an equality assertion: differ at all); one that is a no-op on a case says so.  The statistics
cut at the 4-pixel tile are shown in tests/test_bn_partials_cpu.py (measure_dw), on the tile sums themselves.  `pytest -s`
prints the table."""
import os
import re

import pytest
import torch

from tests import dw3_ref as D
from tests.conv_ref import one_thread
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSITIVITY = 3.0
MEASURED, DONE = {}, set()
BIG = D.BIG_FWD + D.BIG_BWD


# ---- branches ----------------------------------------------------------------------------------------------------------------
def test_forward_tile_thresholds():
    for case in D.CASES + D.BIG_FWD_NEIGHBOUR + D.BIG_BWD_NEIGHBOUR:                    # 4 pixels per thread
        q, rl = D.queries(case), D.layout(case[3])[1]
        assert q["tile_rows"] == 4 * rl and q["tiles"] == (q["pout"] + 4 * rl - 1) // (4 * rl), case
    want = [(12, 16, 3), (8, 32, 1)]                                                     # CQ, RL, channel blocks
    for case, near, lay in zip(D.BIG_FWD, D.BIG_FWD_NEIGHBOUR, want):
        q, (cq, rl, blocks, fallback) = D.queries(case), D.layout(case[3])
        assert (cq, rl, blocks) == lay and not fallback
        assert q["tile_rows"] == 8 * rl and q["tiles"] == (q["pout"] + 8 * rl - 1) // (8 * rl)
        assert 0 < q["pout"] % q["tile_rows"] < q["tile_rows"]                          # a short last tile
        assert q["pout"] // (rl * 8) * blocks >= 4096 > D.queries(near)["pout"] // (rl * 8) * blocks
        assert case[3:] == near[3:] and case[1] - near[1] <= 8 and case[2] - near[2] <= 10
        assert case[0] * case[1] * case[2] * case[3] * 4 < 140e6                         # (the GPU file's largest tensor)
    assert D.queries(D.BIG_FWD[1])["tiles"] > 2048                                       # the finalize's tail loop, from a real producer


def test_backward_chunk_cap():
    for case in D.CASES + D.BIG_BWD_NEIGHBOUR:
        q = D.queries(case)
        assert q["chunks"] == min(2048, max(1, (q["pout"] + 255) // 256)) and q["out_chunk"] <= 256, case
    assert max(D.queries(c)["chunks"] for c in D.CASES) == 25                            # what the small cases reach
    for case, near in zip(D.BIG_BWD, D.BIG_BWD_NEIGHBOUR):
        q = D.queries(case)
        assert q["chunks"] == 2048 and q["pout"] > 2048 * 256
        used = (q["pout"] + 256) // 257
        assert q["out_chunk"] == 257 and q["pout"] % 257 == 60 and used == 2046        # chunk 2045 ragged, chunks 2046 and 2047 EMPTY
        assert case[3:] == near[3:] and D.queries(near)["out_chunk"] == 256
    assert D.BIG_BWD[1][5] == 2 and D.queries(D.BIG_BWD[1])["in_chunk"] == 1026 and D.BIG_BWD[0][5] == 1


def test_layouts_and_small_geometry():
    lay = dict((c[3], D.layout(c[3])) for c in D.CASES + BIG)
    assert lay[32][:3] == (8, 32, 1) and lay[96][:3] == (12, 16, 2) and lay[144][:3] == (12, 16, 3) and lay[48][:3] == (12, 16, 1)
    assert lay[20] == (16, 16, 1, True) and lay[72] == (16, 16, 2, True) and lay[8] == (16, 16, 1, True)
    assert [D.CASES[i][3:5] for i in D.FALLBACK] == [(20, 20), (72, 70)]                 # 11 idle lanes; a block two quads wide, Cw < C
    small = [D.CASES[i] for i in D.SMALL_GEOMETRY]
    s2d2 = [c for c in small if c[5] == 2 and c[6] == 2 and c[1] > 1]
    assert sorted((c[1] % 2, c[2] % 2) for c in s2d2) == [(0, 0), (1, 1)]                # stride 2 with dilation 2: even and odd map
    assert any(c[2] == 1 and c[1] > 1 and c[5] == 1 for c in small) and any(c[2] == 1 and c[1] > 1 and c[5] == 2 for c in small)
    assert any(c[1] == 1 and c[2] == 1 and c[0] > 1 for c in small) and any(c[:3] == (1, 1, 1) for c in small)
    assert D.subset_channels(144, 144) == list(range(0, 4)) + list(range(44, 48)) + list(range(96, 100)) + list(range(140, 144))
    assert D.subset_channels(32, 32) == list(range(0, 4)) + list(range(28, 32)) and D.subset_channels(8, 8) == list(range(8))
    assert len(set(D.case_id(c) for c in D.CASES + BIG)) == len(D.CASES + BIG)


# ---- the data gradient as the kernel writes it (and with the parity test on the wrong index) ------------------------------------------
def dx_by_taps(case, r, parity="th"):
    """dx[n, ih, iw, c] = sum over taps with th = ih + dil - kh dil >= 0, th divisible by the stride and oh = th / stride < Ho
    (likewise in w) of dy[n, oh, ow, c] w[c, kh, kw], in float64.  parity "ih": the divisibility test applied to ih / iw"""
    n, h, w, c, cw, s, d, _ = case
    ho, wo = D.out_hw(case)
    dy, wt = r["dy"][..., :cw].double(), r["w"].double()
    dx = torch.zeros(n, h, w, cw, dtype=torch.float64)

    def axis(size, osize, k):
        i = torch.arange(size)
        t = i + d - k * d
        ok = (t >= 0) & ((t if parity == "th" else i) % s == 0) & (torch.div(t, s, rounding_mode="floor") < osize)
        return ok, torch.div(t, s, rounding_mode="floor").clamp(0, osize - 1)
    for kh in range(3):
        okh, oh = axis(h, ho, kh)
        for kw in range(3):
            okw, ow = axis(w, wo, kw)
            m = (okh[:, None] & okw[None, :])[None, :, :, None]
            dx += dy[:, oh][:, :, ow] * wt[:, 0, kh, kw] * m
    return dx


def test_restatement_is_the_tap_formula():
    for i in (1, 4, 10, 11, 13, 6):
        case = D.CASES[i]
        r = D.inputs(case)
        ref = D.restate(case, r)
        assert rel_err(dx_by_taps(case, r), ref["dx"][..., :case[4]]) < 1e-14


# ---- floors and faults, case by case ------------------------------------------------------------------------------------------------------
def put(k, v):
    MEASURED[k] = max(MEASURED.get(k, 0.0), v)


def row(fault, case, what, ratio):
    print("fault %-52s %-34s %-8s %s" % (fault, D.case_id(case), what, "no-op on this case" if ratio is None else "%.3g x bound" % ratio))
    assert ratio is None or ratio >= SENSITIVITY, (fault, D.case_id(case), what, ratio)


def measure(case):
    if case in DONE:
        return
    n, h, w, c, cw, s, d, _ = case
    big = case in BIG
    r = D.inputs(case)
    ch = D.subset_channels(c, cw) if big else None
    parts = D.big_parts(case) if big else ("y", "dx", "dx_acc", "dw")
    need = ("y",) if parts == ("y",) else ("y", "dx", "dw")
    ref = D.restate(case, r, ch, parts=need)
    with one_thread():
        f32 = D.restate(case, r, ch, torch.float32, parts=need)
    for q in parts:
        put(D.key(case, q), rel_err(f32[q], ref[q]))
    bound = lambda q: D.bound(case, q) if D.key(case, q) in D.FLOOR else float("nan")
    q = D.queries(case)
    if cw < c:
        # a channel >= Cw given a non-zero weight (its neighbour's): y, dx there must be EXACTLY zero
        bad = (r["x"][..., cw] * r["w"][cw - 1, 0, 1, 1]).abs().max()
        row("channel >= Cw given a non-zero weight", case, "y == 0", float("inf") if float(bad) > 0 else 0.0)
    if s == 2 and "dx" in parts and not big:
        mut = dx_by_taps(case, r, "ih")
        same = torch.equal(mut, dx_by_taps(case, r))
        row("stride-2 parity test on ih, not ih + dil - kh dil", case, "dx", None if same else rel_err(mut, ref["dx"][..., :cw]) / bound("dx"))
        assert same == (d % 2 == 0)                         # an even dilation leaves the parity of ih: the mutant is equivalent there
    if case in D.BIG_FWD:
        # the 4-pixel kernel on the 8-pixel layout: the second half of every tile's rows is never written
        tr = q["tile_rows"]
        y = ref["y"].reshape(-1, len(ch)).clone()
        rows_ = torch.arange(y.shape[0]) % tr >= tr // 2
        y[rows_] = 0
        row("4-pixel kernel on the 8-pixel layout (rows unwritten)", case, "y", rel_err(y, ref["y"].reshape(-1, len(ch))) / bound("y"))
    if case in D.BIG_BWD:
        oc, ic = q["out_chunk"], q["in_chunk"]
        assert oc == 257
        last = torch.zeros(q["pout"], dtype=torch.bool)
        last[oc - 1::oc] = True                              # the last output pixel of every full chunk
        rm = dict(r, dy=r["dy"] * last.view(1, r["ho"], r["wo"], 1))
        part = D.restate(case, rm, ch, parts=("dw",))["dw"]
        assert int(last.sum()) >= 2044
        row("a chunk drops its last output pixel (out_chunk 257)", case, "dw", rel_err(ref["dw"] - part, ref["dw"]) / bound("dw"))
        row("a chunk counts its last output pixel twice", case, "dw", rel_err(ref["dw"] + part, ref["dw"]) / bound("dw"))
        lin = torch.zeros(q["pin"], dtype=torch.bool)
        lin[ic - 1::ic] = True
        keep = (~lin).view(1, h, w, 1)
        row("a chunk drops its last input pixel (in_chunk %d)" % ic, case, "dx", rel_err(ref["dx"] * keep, ref["dx"]) / bound("dx"))
        base = r["dx0"][..., ch].double()
        row("... accumulating", case, "dx_acc", rel_err(torch.where(keep, ref["dx_acc"], base), ref["dx_acc"]) / bound("dx_acc"))
    DONE.add(case)


@pytest.mark.parametrize("case", D.CASES + BIG, ids=[D.case_id(c) for c in D.CASES + BIG])
def test_case_floor_and_faults(case):
    measure(case)


def test_every_fault_has_a_case_that_sees_it():
    cases = D.CASES + BIG
    assert sum(c[4] < c[3] for c in cases) >= 2                                           # a channel >= Cw
    assert sum(c[5] == 2 and c[6] % 2 == 1 for c in D.CASES) >= 3                         # the parity test (odd dilation)
    assert len(D.BIG_FWD) == 2 and len(D.BIG_BWD) == 2                                    # the tile cut, the chunk ends


def test_floors_are_the_recorded_ones():
    """the case tests above have measured every floor when the whole file runs; alone, this test measures what is missing"""
    for case in D.CASES + BIG:
        measure(case)
    for k, v in sorted(MEASURED.items()):
        print("floor %-44s measured %.3e  recorded %.3e" % (k, v, D.FLOOR.get(k, float("nan"))))
    assert set(MEASURED) == set(D.FLOOR), set(MEASURED) ^ set(D.FLOOR)
    for k, v in MEASURED.items():
        assert D.FLOOR[k] / 2 <= v <= 1.25 * D.FLOOR[k], "%s: measured %.3e, recorded %.3e" % (k, v, D.FLOOR[k])


def test_profile_carries_the_recorded_floors():
    text = open(os.path.join(ROOT, "profiles", "streaming_kernel_tests.txt")).read()
    rows = dict((m.group(1), (float(m.group(2)), float(m.group(3)))) for m in
                re.finditer(r"^(dw3\.\S+)\s+(\d\.\de[-+]\d\d)\s+(\d\.\de[-+]\d\d)\s", text, re.M))
    for k, v in D.FLOOR.items():
        assert k in rows, k
        b = 4.0 * v
        assert rows[k][0] == float("%.1e" % v) and abs(rows[k][1] - b) <= 0.06 * b, (k, rows[k], v)
