"""tests/bn_partials_ref.py on the CPU (no GPU, runs anywhere): the tile structure each case of tests/test_bn_partials_gpu.py
claims, the fp32 floors, and the condition that makes its bounds meaningful.

Tile structure: through the library's host queries (iswm_conv2d_stat_tiles / _stat_tile_rows, iswm_conv2d_fwd_packed_stat_layout,
iswm_conv2d_pl2_tile_rows, iswm_dwconv3x3_stat_tile_rows / _stat_tiles, iswm_conv2d_dgrad_pl2_stat_tiles): the one-row and the
tile_rows - 1 last tiles, the patch layout, the tile of a strided 1 x 1 data gradient that no tap reaches, the depthwise
kernel's 8-pixel tiles on the two production shapes only, and more than 2048 tiles only in the synthetic finalize cases and
in the larger of those two shapes.

Sensitivity condition: for every case, each plausible wrong epilogue (bn_partials_ref.fwd_mutants, the backward mutants
below) must miss at least one assertion of the GPU file by 3 x its bound (an equality assertion: differ at all).  It is a
condition on the INPUTS -- seeds, the offset kind's scale -- and on the metric; a mutant that is a no-op on a shape (no short
last tile, a single tile) is not formed for it, and bn_partials_ref.NEEDS_MEAN names the one mutant that only the offset kind
can see on the tile_rows - 1 shapes.

Floors: measured again here; each recorded figure must lie within [measured / 1.25, 2 x measured], and
profiles/bn_partials_tests.txt must carry the recorded figures.  `pytest -s` prints them."""
import os
import re

import pytest
import torch

from tests import bn_partials_ref as B
from tests import conv_ref as R
from tests.util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSITIVITY = 3.0
MEASURED = {}
DONE = set()


def put(k, v):
    MEASURED[k] = max(MEASURED.get(k, 0.0), v)


def caught(errs):
    """errs: [(error of the mutant, bound of that assertion or None for an equality assertion)] -> the best ratio"""
    best = 0.0
    for e, b in errs:
        if b is None or b == 0.0:
            best = max(best, float("inf") if e > 0 else 0.0)
        else:
            best = max(best, e / b)
    return best


# ---- tile structure ---------------------------------------------------------------------------------------------------------------
def test_forward_tile_structure():
    for rt in B.FWD_ROUTES:
        e, name, m, t, tr = B.fwd_layout(rt)
        assert name == rt.names["fwd"], (rt.id, name)
        assert t <= 2048, rt.id                      # more than 2048 tiles only in the synthetic finalize cases
        if rt.id in B.PATCH:
            assert tr == 0 and e == "iswm_conv2d_fwd_packed" and t >= 1
            continue
        assert tr > 0 and t == (m + tr - 1) // tr, rt.id
        if rt.id in B.ONE_ROW_LAST:
            assert m % tr == 1 and t > 1
        if rt.id in B.SHORT_LAST:
            assert m % tr == tr - 1 and t > 1
    assert sorted(tr for tr in set(B.fwd_layout(rt)[4] for rt in B.FWD_ROUTES)) == [0, 64, 96, 128, 144, 160]
    assert B.fwd_layout(B.ROUTE["pl_map1"])[2:] == (3, 1, 128)
    for rid in B.RAGGED:
        assert B.ROUTE[rid].geom[4] % 128 != 0 and B.fwd_layout(B.ROUTE[rid])[0] == "iswm_conv2d_fwd_pl2"
    assert set(B.IDENTITY) <= set(B.ROUTE) and not (set(B.IDENTITY) & set(B.PATCH))
    assert max(B.FIN_TILES) > 2048 and 2049 in B.FIN_TILES and 33 in B.FIN_TILES and 513 in B.FIN_TILES


def test_depthwise_tile_structure():
    from tests import dw3_ref as D
    lay = [B.dw_layout(i) for i in range(len(B.dw_cases()))]
    assert set(tr for _, _, tr in lay) == set((64, 128, 256))              # the <4> and the <8> pixel forms at 16 and 32 pixel lanes
    for i, (m, t, tr) in enumerate(lay):
        c = B.dw_cases()[i][3]
        assert t == (m + tr - 1) // tr and (t <= 2048 or i == B.DW_BIG[1])
        assert tr == D.layout(c)[1] * (8 if i in B.DW_BIG else 4)           # 8 pixels per thread on the two production shapes only
    for i in B.DW_BIG:
        m, t, tr = lay[i]
        assert 0 < m % tr < tr - 1                                          # a short last tile
    assert lay[B.DW_BIG[1]][1] > 2048 and 2 * lay[B.DW_BIG[1]][1] * 32 + 2 * B.PAD <= 1 << 19      # (fits the GPU file's sentinel buffer)
    assert all(D.layout(B.dw_cases()[i][3])[3] for i in B.DW_FALLBACK)      # idle quad lanes
    assert lay[B.DW_SINGLE_ROW][:2] == (9, 1)
    m, t, tr = lay[B.DW_SHORT]
    assert t == 2 and m % tr == tr - 1
    assert lay[B.DW_IDENTITY][1] > 1
    assert any(c[7] for c in B.dw_cases()) and any(c[4] < c[3] for c in B.dw_cases())       # the sliced one, the one with Cw < C


def test_backward_tile_structure():
    """a stride-2 1 x 1 data gradient reaches one pixel in four; in the kernel's parity-major row order the other classes fill
    whole tiles that no tap reaches.  pl_s2_1x1 is the route table's only strided 1 x 1; its 338 rows
    are 98 reached rows and then 240 that are not: tiles 1 and 2 of its three"""
    rt = R.ROUTE["pl_s2_1x1"]
    m, tiles, tr = B.dgrad_layout(rt)
    assert (m, tiles, tr) == (338, 3, 128)
    assert int(B.parity_rows(rt).sum()) == 2 * 7 * 7 and B.untouched_tiles(rt, tr) == [1, 2]
    for rid in B.BWD_ROUTES:
        rt = R.ROUTE[rid]
        m, tiles, tr = B.dgrad_layout(rt)
        wm = 2 if rt.geom[3] <= 64 else 1
        assert tiles == (m + tr - 1) // tr * wm and R.planned(rt)["dgrad"][0] == "iswm_conv2d_dgrad_pl2"
        if rid != "pl_s2_1x1":
            assert bool(B.parity_rows(rt).all())


# ---- forward: floors and sensitivity ------------------------------------------------------------------------------------------------
def _merge_level(tag, key, y, tile_rows, exact_counts=None):
    """floors of a merge-level check (patch layout, ASPP) on raster tiles of tile_rows, and its mutants"""
    n = B.counts(y.shape[0], tile_rows)
    mean, var = B.batch_stats(y)
    s32, q32 = B.tile_stats(y, tile_rows, torch.float32)
    m32, v32 = B.merge(s32, q32, n)
    put(key + ".mean", rel_err(m32, mean))
    put(key + ".var", rel_err(v32, var))
    return mean, var, n


def measure_fwd(rid, kind):
    if (rid, kind) in DONE:
        return
    rt = B.ROUTE[rid]
    o = B.operands(rt, kind)
    y = B.stored_y_cpu(rt, o)
    e, name, m, t, tr = B.fwd_layout(rt)
    tag = "%s-%s" % (rid, kind)
    if rid in B.PATCH:                              # the patch tiling is the kernel's: floor and mutants on raster tiles of <= 128
        mean, var, n = _merge_level(tag, rid, y, 128)
        s, m2 = B.tile_stats(y, 128)
        bm, bv = B.bound(rid + ".mean"), B.bound(rid + ".var")
        muts = dict((k, v) for k, v in B.fwd_mutants(y, 128).items() if k in
                    ("M2 about the batch mean", "planes swapped", "neighbouring channel", "last row dropped", "row past M included"))
        for name_, (ms, mq) in muts.items():
            if ms.shape != s.shape:
                continue
            mm, mv = B.merge(ms, mq, n)
            ratio = caught([(rel_err(mm, mean), bm), (rel_err(mv, var), bv)])
            print("sens %-24s %-26s %.1f x bound" % (tag, name_, ratio))
            assert ratio >= SENSITIVITY, (tag, name_, ratio)
        # (a count off by one needs no showing here: the GPU file asserts the published counts' sum EQUAL to M)
        DONE.add((rid, kind))
        return
    ref = B.tile_stats(y, tr)
    f32 = B.tile_stats(y, tr, torch.float32)
    if kind == "int":
        assert torch.equal(f32[0].double(), ref[0])   # partial sums stay below 2^24: the GPU file asserts equality
    else:
        put(rid + ".S", B.tile_err(f32[0], ref[0]))
    put(rid + ".M2", B.tile_err(f32[1], ref[1]))
    if rid in B.IDENTITY and kind == "offset":
        put(rid + ".identity", identity_residual(y, f32[0], f32[1], tr))
    bs, bq = (None if kind == "int" else B.bound(rid + ".S")), B.bound(rid + ".M2")
    for name_, (ms, mq) in B.fwd_mutants(y, tr).items():
        ratio = caught([(B.tile_err(ms, ref[0]), bs), (B.tile_err(mq, ref[1]), bq)])
        ex = B.exempt(name_, kind, rid in B.SHORT_LAST)
        print("sens %-24s %-26s %.1f x bound%s" % (tag, name_, ratio, " (exempt: NEEDS_MEAN)" if ex else ""))
        assert ratio >= SENSITIVITY or ex, (tag, name_, ratio)
    DONE.add((rid, kind))


def identity_residual(y, s_pub, m2_pub, tile_rows):
    """|var_true - var_pair - (cross + shift)| / max var_true for published partials (s_pub, m2_pub): what is left is the error of
    the published M2_t alone"""
    terms, _ = B.identity_terms(y, s_pub, tile_rows)
    _, var = B.batch_stats(y)
    _, var_pair = B.merge(s_pub, m2_pub, B.counts(y.shape[0], tile_rows))
    return float((var - var_pair - terms).abs().max() / var.abs().max())


@pytest.mark.parametrize("rid,kind", B.FWD_CASES, ids=["%s-%s" % c for c in B.FWD_CASES])
def test_forward_floor_and_sensitivity(rid, kind):
    measure_fwd(rid, kind)


def test_identity_sees_what_the_pair_merge_loses():
    """the pair-merge identity is not vacuous: on the offset kind of the 1 x 1 routes (no padded border: |mean| / sigma ~ 130) the
    cross and shift terms are 3 x the bound they are asserted within or more, so leaving them out fails the assertion.  On
    pl_3x3 (border) and the depthwise case (K = 9) they are not: bn_partials_ref.IDENTITY says so"""
    assert sum(B.ROUTE[rid].geom[5] == 1 for rid in B.IDENTITY) >= 3
    for rid in B.IDENTITY:
        rt = B.ROUTE[rid]
        y = B.stored_y_cpu(rt, B.operands(rt, "offset"))
        tr = B.fwd_layout(rt)[4]
        s32, q32 = B.tile_stats(y, tr, torch.float32)
        terms, _ = B.identity_terms(y, s32, tr)
        mean, var = B.batch_stats(y)
        ratio = float((mean.abs() / var.sqrt()).max())
        loss = float(terms.abs().max() / var.abs().max())
        print("identity %-10s max |mean|/sigma %.1f  pair-merge loss %.2e (2^-23 |mean|/sigma = %.2e)" % (rid, ratio, loss, ratio * 2.0 ** -23))
        if rt.geom[5] == 1:
            assert loss >= SENSITIVITY * B.bound(rid + ".identity"), (rid, loss)


def test_bias_in_the_sums_breaks_the_bit_identity():
    """the GPU file asserts the partials with and without a bias equal: a bias inside S_t is not"""
    for rid in B.BIAS_ROUTES:
        rt = R.ROUTE[rid]
        y = B.stored_y_cpu(rt, B.operands(rt, "dense"))
        tr = B.fwd_layout(rt)[4] or 128
        s = B.tile_stats(y, tr)[0]
        assert not torch.equal(B.fwd_mutants(y, tr, R.bias_of(rt))["bias in S_t"][0].float(), s.float())


def measure_aspp(cid, kind):
    if (cid, kind) in DONE:
        return
    for b, (rt, o) in enumerate(zip(R.aspp_routes(cid), B.aspp_operands(cid, kind))):
        y = B.stored_y_cpu(rt, o)
        mean, var, n = _merge_level("%s-%s" % (cid, kind), cid, y, B.ASPP_TILE_ROWS)
        bm, bv = B.bound(cid + ".mean"), B.bound(cid + ".var")
        s, m2 = B.tile_stats(y, B.ASPP_TILE_ROWS)
        for name_, (ms, mq) in B.fwd_mutants(y, B.ASPP_TILE_ROWS).items():
            if ms.shape != s.shape or name_ in ("tiles 0 and 1 swapped", "last count = tile_rows"):
                continue                                # equal counts: a swap does not change the merge; counts are the test's own
            mm, mv = B.merge(ms, mq, n)
            ratio = caught([(rel_err(mm, mean), bm), (rel_err(mv, var), bv)])
            print("sens %s-%s b%d %-26s %.1f x bound" % (cid, kind, b, name_, ratio))
            assert ratio >= SENSITIVITY, (cid, kind, b, name_, ratio)
    DONE.add((cid, kind))


@pytest.mark.parametrize("cid,kind", B.ASPP_CASES, ids=["%s-%s" % c for c in B.ASPP_CASES])
def test_aspp_floor_and_sensitivity(cid, kind):
    measure_aspp(cid, kind)


def measure_dw(i, kind):
    if ("dw", i, kind) in DONE:
        return
    x, wt = B.dw_inputs(i, kind)
    y = B.dw_stored_y_cpu(i, x, wt)
    m, t, tr = B.dw_layout(i)
    key = "dw3_%d" % i
    ref, f32 = B.tile_stats(y, tr), B.tile_stats(y, tr, torch.float32)
    if kind == "int":
        assert torch.equal(f32[0].double(), ref[0])
    else:
        put(key + ".S", B.tile_err(f32[0], ref[0]))
    put(key + ".M2", B.tile_err(f32[1], ref[1]))
    if i == B.DW_IDENTITY and kind == "offset":
        put(key + ".identity", identity_residual(y, f32[0], f32[1], tr))
    cw = B.dw_cases()[i][4]
    bs, bq = (None if kind == "int" else B.bound(key + ".S")), B.bound(key + ".M2")
    muts = B.fwd_mutants(y[:, :cw], tr)
    if i in B.DW_BIG:
        # the 4-pixel kernel launched on the 8-pixel layout: a tile's statistics cover its first tile_rows / 2 rows only (the
        # other rows of y are never written either, which the convolution tests see)
        v, n_t, valid = B._tiled(y[:, :cw].double(), tr)
        half = valid & (torch.arange(tr) < tr // 2).view(1, tr, 1)
        s_h = (v * half).sum(1)
        dev_h = (v - (s_h / half.sum(1).clamp_min(1))[:, None]) * half
        muts["statistics cut at the 4-pixel tile"] = (s_h, (dev_h * dev_h).sum(1))
    for name_, (ms, mq) in muts.items():                                # (channels past Cw are zero: asserted equal to zero)
        ratio = caught([(B.tile_err(ms, ref[0][:, :cw]), bs), (B.tile_err(mq, ref[1][:, :cw]), bq)])
        ex = B.exempt(name_, kind, i == B.DW_SHORT)
        print("sens dw3_%d-%s %-26s %.1f x bound%s" % (i, kind, name_, ratio, " (exempt: NEEDS_MEAN)" if ex else ""))
        assert ratio >= SENSITIVITY or ex, (i, kind, name_, ratio)
    DONE.add(("dw", i, kind))


DW = B.DW_CASE_KINDS


@pytest.mark.parametrize("i,kind", DW, ids=["dw3_%d-%s" % c for c in DW])
def test_depthwise_floor_and_sensitivity(i, kind):
    assert len(B.dw_cases()) == 13 and set(i for i, _ in DW) == set(range(13))
    measure_dw(i, kind)


# ---- finalize ---------------------------------------------------------------------------------------------------------------------------
def fin_params(c):
    g = R.gen("fin-params", c)
    return (torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g),
            torch.rand(c, generator=g) + 0.5)


def measure_fin():
    if "fin" in DONE:
        return
    for planes in (2, 3):
        for c, tiles, lay in B.FIN_CASES:
            if planes == 3 and lay == "counts":
                continue
            flat, n, tr = B.fin_partials(c, tiles, lay, planes)
            gamma, beta, rm, rv = fin_params(c)
            for mom in (0.1, 1.0):
                exp = B.fin_expected(flat, n, c, planes, gamma, beta, rm, rv, mom)
                f32 = B.fin_fp32(exp, gamma, rm, rv, mom)
                for k, v in f32.items():
                    put(B.fin_key(k, mom, c), rel_err(v, exp[k]))
            # a merge that mistakes the layout is far outside the bound: counts of the last tile, planes, tile slots
            if planes == 2 and tiles > 1:
                p = flat[:2 * tiles * c].view(2, tiles, c)
                _, var = B.merge(p[0], p[1], n)
                nbad = n.clone()
                nbad[-1] = n[0] if lay == "rows" else n[-1] + 1
                assert rel_err(B.merge(p[0], p[1], nbad)[1], var) >= SENSITIVITY * B.bound("fin.var")
                assert rel_err(B.merge(p[1], p[0], n)[1], var) >= SENSITIVITY * B.bound("fin.var")
                if tiles > 2:                         # tail tiles left out (the register-resident head only)
                    keep = min(tiles - 1, 2048)
                    assert rel_err(B.merge(p[0][:keep], p[1][:keep], n[:keep])[1], var) >= SENSITIVITY * B.bound("fin.var")
    DONE.add("fin")


def test_finalize_floors_and_sensitivity():
    measure_fin()


# ---- backward ---------------------------------------------------------------------------------------------------------------------------
def stored_dx_cpu(rid, code, acc, b):
    rt = R.ROUTE[rid]
    o = R.operands(rt, "dense")
    dx = R.conv_dgrad(rt, o["dy"], o["w_d"]).float()
    if acc:
        dx = o["base"] + dx
    return (dx * B.pattern(3, b) if code == 3 else dx), o


def measure_bwd(rid, code, acc):
    if (rid, code, acc) in DONE:
        return
    b = B.bwd_inputs(rid)
    dx, o = stored_dx_cpu(rid, code, acc, b)
    pat = B.pattern(code, b)
    ref = B.bwd_sums(dx, pat, b)
    f32 = B.bwd_sums(dx, pat, b, torch.float32)
    key = "bwd.%s" % rid
    put(key + ".sum_dz", rel_err(f32[0], ref[0]))
    put(key + ".sum_dzx", rel_err(f32[1], ref[1]))
    dz = dx * pat
    for training in (True, False):
        dy = B.bn_backward_ref(dz, b, training)[0]
        put(key + (".dy" if training else ".dy_eval"), rel_err(B.bn_backward_fp32(dz, b, training, f32), dy))
    bz, bx = B.bound(key + ".sum_dz"), B.bound(key + ".sum_dzx")
    muts = {}
    if code == 2:
        muts["pattern from y > 0"] = B.bwd_sums(dx, B.pattern(2, b, "y>0"), b)
    if code == 3:
        # the stored dx is already masked, so the sums cannot see the pattern: the GPU file asserts the stored tensor equal to
        # the unmasked gradient under the hi-plane pattern, element by element
        # -- where the full value is positive and its hi plane is not (2^-140), a pattern from the full value lets the gradient through
        full, hi = B.pattern(3, b, "full"), B.pattern(3, b)
        plain = stored_dx_cpu(rid, 0, acc, b)[0]
        assert int((full & ~hi).sum()) > 100 and not dx[full & ~hi].any() and int((plain[full & ~hi] != 0).sum()) > 100
    rt = R.ROUTE[rid]
    if acc and rid == "pl_s2_1x1":
        gone = dx * B.parity_rows(rt).unsqueeze(-1)
        muts["old gradient of untouched tiles left out"] = B.bwd_sums(gone, pat, b)
    muts["sums swapped"] = (ref[1], ref[0])
    muts["neighbouring channel"] = (ref[0].roll(1), ref[1].roll(1))
    for name_, (mz, mx) in muts.items():
        ratio = caught([(rel_err(mz, ref[0]), bz), (rel_err(mx, ref[1]), bx)])
        print("sens bwd %s code %d acc %d %-42s %.1f x bound" % (rid, code, acc, name_, ratio))
        assert ratio >= SENSITIVITY, (rid, code, acc, name_, ratio)
    DONE.add((rid, code, acc))


@pytest.mark.parametrize("rid,code,acc", B.BWD_CASES, ids=["%s-code%d-acc%d" % c for c in B.BWD_CASES])
def test_backward_floor_and_sensitivity(rid, code, acc):
    measure_bwd(rid, code, acc)


# ---- the recorded floors ------------------------------------------------------------------------------------------------------------------
def test_floors_are_the_recorded_ones():
    """the case tests above have measured every floor when the whole file runs; alone, this test measures what is missing"""
    for c in B.FWD_CASES:
        measure_fwd(*c)
    for c in B.ASPP_CASES:
        measure_aspp(*c)
    for c in DW:
        measure_dw(*c)
    measure_fin()
    for c in B.BWD_CASES:
        measure_bwd(*c)
    for k, v in sorted(MEASURED.items()):
        print("floor %-28s measured %.3e  recorded %.3e" % (k, v, B.FLOOR.get(k, float("nan"))))
    assert set(MEASURED) == set(B.FLOOR), set(MEASURED) ^ set(B.FLOOR)
    for k, v in MEASURED.items():
        assert B.FLOOR[k] / 2 <= v <= 1.25 * B.FLOOR[k], "%s: measured %.3e, recorded %.3e" % (k, v, B.FLOOR[k])


def test_profile_carries_the_recorded_floors():
    text = open(os.path.join(ROOT, "profiles", "bn_partials_tests.txt")).read()
    rows = dict((m.group(1), (float(m.group(2)), float(m.group(3)))) for m in
                re.finditer(r"^(\S+\.\S+)\s+(\d\.\de[-+]\d\d)\s+(\d\.\de[-+]\d\d)\s", text, re.M))
    for k, v in B.FLOOR.items():
        assert k in rows, k
        assert rows[k][0] == float("%.1e" % v) and abs(rows[k][1] - B.bound(k)) <= 0.06 * B.bound(k), (k, rows[k], v)
