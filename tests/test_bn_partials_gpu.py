"""The BatchNorm partials of every producer, iswm_bn_finalize / iswm_bn_finalize_res on their own, and the backward sums of
iswm_conv2d_dgrad_pl2_bn with their consumer, against the float64 restatements of tests/bn_partials_ref.py.

Every producer check reads back the tensor the kernel itself stored (y forward, dx backward) and restates the partials from
those fp32 values in float64: the convolution arithmetic drops out, what is left is the fp32 summation and centring of the
epilogue.  Rule: rel_err <= 4 x FLOOR[check] (tile sums: tile by tile, bn_partials_ref.tile_err), FLOOR = a plain sequential fp32
restatement on the CPU (tests/test_bn_partials_cpu.py re-measures it and shows that each plausible wrong epilogue -- a last
tile counted full, a row too few or too many, M2 about the batch mean, swapped planes / tiles / channels, a wrong ReLU
pattern, untouched tiles left out -- misses these assertions by 3 x the bound).  Exact-integer operands: S_t equal.  One-row
tiles: S_t the row bit for bit, M2_t zero.  Each test asserts the entry point and the kernel it reached, and every partials
buffer lies inside a sentinel buffer: exactly its documented size is written.  profiles/bn_partials_tests.txt has the figures.

The statistics leave the bias out (include/iswm_hip.h): with and without a bias the partials are the same bits."""
import ctypes

import pytest
import torch

from tests import bn_partials_ref as B
from tests import conv_ref as R
from tests.test_conv_kernels_gpu import dev, to_dev
from tests.util import rel_err

pytestmark = pytest.mark.gpu

FAILED = []
PART_ARG = {"iswm_conv2d_fwd_pl2": 6, "iswm_conv2d_fwd_packed": 5, "iswm_conv2d_fwd": 5, "iswm_dwconv3x3_fwd_stats": 5,
            "iswm_conv2d_dgrad_pl2_bn": 15}
BUF = 1 << 19                                      # (the 4169 tiles x 32 channels of the largest depthwise case: 266 816)


def note(tag, key, err, bound):
    """print the figure and note a miss; settle() asserts once a test has printed all of its figures"""
    print("bnp %-34s %-24s err %.3e  bound %.3e" % (tag, key, err, bound))
    if not err <= bound:
        FAILED.append("%s %s %.3e > %.3e" % (tag, key, err, bound))


def same(tag, what, ok):
    print("bnp %-34s %-24s %s" % (tag, what, "equal" if ok else "DIFFERS"))
    if not ok:
        FAILED.append("%s %s differs" % (tag, what))


def settle():
    missed = list(FAILED)
    del FAILED[:]
    assert not missed, missed


class Redirect(object):
    """records (entry point, device kernel name) of every producer call the wrappers make, and points the partials argument
    into a sentinel-filled buffer: [PAD sentinels][partials][sentinels]"""

    def __init__(self, monkeypatch, size, dtype=torch.float32):
        """size: elements the producer will write, from the host's tile queries -- checked against the buffer BEFORE any launch"""
        from iswm_amd import _lib, ops
        assert 0 < size and 2 * B.PAD + size <= BUF, "the partials of this case do not fit the sentinel buffer"
        self.size = size
        self.calls, lib, real = [], _lib.load(), ops.call
        self.buf = torch.full((BUF,), B.SENTINEL, dtype=dtype, device=dev())
        esz = self.buf.element_size()

        def spy(name, *a):
            if name in PART_ARG:
                a = list(a)
                assert a[PART_ARG[name]] is not None
                a[PART_ARG[name]] = ctypes.c_void_p(self.buf.data_ptr() + B.PAD * esz)
                self.calls.append((name, R.kernel_name(lib, a[0]._obj, R.KIND[name]) if name in R.KIND else None))
            return real(name, *a)

        monkeypatch.setattr(ops, "call", spy)

    def take(self):
        out, self.calls = self.calls, []
        return out

    def partials(self):
        """the `size` elements the kernel had to write, on the host; everything around them must still be the sentinel and none
        of them may be (every slot written)"""
        host, size = self.buf.cpu(), self.size
        inside = host[B.PAD:B.PAD + size]
        assert bool((host[:B.PAD] == B.SENTINEL).all()) and bool((host[B.PAD + size:] == B.SENTINEL).all()), "written outside the buffer"
        assert not bool((inside == B.SENTINEL).any()), "a slot of the partials was not written"
        self.buf.fill_(B.SENTINEL)
        return inside.clone()


def fwd_size(rt):
    e, name, m, tiles, tr = B.fwd_layout(rt)
    return 2 * tiles * rt.geom[4] + (tiles if tr == 0 else 0)


def forward(rt, o, spy, bias=None, ybuf=None):
    """ops.conv2d_fwd with want_stats as the network calls it -> (stored y [M, Cout] host, partials [2, T, Cout] host, trailing
    counts or None, tile_rows)"""
    from iswm_amd import ops
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    plan = R.planned(rt)
    e, name, m, tiles, tr = B.fwd_layout(rt)
    with R.conv_math(rt):
        xd = to_dev(rt, o["x"], cin)
        g = ops.ConvGeom(xd, cout, k, k, stride, pad, dil)
        out = None if ybuf is None else ybuf[..., 8:8 + cout]
        y, _, lay = ops.conv2d_fwd(xd, o["w_f"].to(dev()), g, bias=None if bias is None else bias.to(dev()), out=out, want_stats=True)
        assert spy.take() == [plan["fwd"]] and plan["fwd"] == (e, name) and name == rt.names["fwd"]
        assert tuple(lay) == (tiles, tr)
    assert spy.size == 2 * tiles * cout + (tiles if tr == 0 else 0)
    flat = spy.partials()
    return (y.cpu().reshape(-1, cout), flat[:2 * tiles * cout].view(2, tiles, cout),
            flat[2 * tiles * cout:] if tr == 0 else None, tr)


def check_tiles(tag, key, p, y, tr, exact, ch=None):
    """S_t, M2_t of every tile against float64 of those rows of the stored y"""
    ref = B.tile_stats(y, tr)
    if exact:
        same(tag, key + ".S", torch.equal(p[0].double(), ref[0]))
    ch = slice(None) if ch is None else ch
    if not exact:
        note(tag, key + ".S", B.tile_err(p[0][:, ch], ref[0][:, ch]), B.bound(key + ".S"))
    note(tag, key + ".M2", B.tile_err(p[1][:, ch], ref[1][:, ch]), B.bound(key + ".M2"))
    last = y.shape[0] - (p.shape[1] - 1) * tr
    if last == 1:                                   # a one-row tile: its sum is the row, its M2 nothing
        same(tag, key + " one-row tile", torch.equal(p[0][-1], y[-1]) and not p[1][-1].any())


def check_identity(tag, key, p, y, tr):
    """the pair-merge identity: the rounding of the published S_t is the whole of what the pair merge loses"""
    terms, _ = B.identity_terms(y, p[0], tr)
    mean, var = B.batch_stats(y)
    _, var_pair = B.merge(p[0], p[1], B.counts(y.shape[0], tr))
    res = float((var - var_pair - terms).abs().max() / var.abs().max())
    ratio = float((mean.abs() / var.sqrt()).max())
    loss = float((var - var_pair).abs().max() / var.abs().max())
    print("bnp %-34s pair-merge loss %.3e at max |mean|/sigma %.1f (2^-23 |mean|/sigma = %.2e)" % (tag, loss, ratio, ratio * 2.0 ** -23))
    note(tag, key + ".identity", res, B.bound(key + ".identity"))


# ---- forward partials ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rid,kind", B.FWD_CASES, ids=["%s-%s" % c for c in B.FWD_CASES])
def test_forward_partials_vs_stored_output(rid, kind, monkeypatch):
    rt = B.ROUTE[rid]
    tag = "%s-%s" % (rid, kind)
    y, p, cnt, tr = forward(rt, B.operands(rt, kind), Redirect(monkeypatch, fwd_size(rt)))
    m, cout = y.shape
    if tr == 0:                                     # image patches of varying size: the counts, then the merge
        same(tag, "counts integral in [1, 128]", bool((cnt == cnt.round()).all()) and float(cnt.min()) >= 1 and float(cnt.max()) <= 128)
        same(tag, "counts sum to M", float(cnt.double().sum()) == m)
        mean, var = B.batch_stats(y)
        pm, pv = B.merge(p[0], p[1], cnt)
        note(tag, rid + ".mean", rel_err(pm, mean), B.bound(rid + ".mean"))
        note(tag, rid + ".var", rel_err(pv, var), B.bound(rid + ".var"))
    else:
        check_tiles(tag, rid, p, y, tr, kind == "int")
        if rid in B.IDENTITY and kind == "offset":
            check_identity(tag, rid, p, y, tr)
    settle()


@pytest.mark.parametrize("rid", B.BIAS_ROUTES)
def test_forward_partials_leave_the_bias_out(rid, monkeypatch):
    """with and without a bias, y written into a channel slice of a sentinel-filled buffer: the partials are the same bits, y
    differs by the bias (one fp32 rounding of the sum), the sentinels of y and around the partials survive"""
    rt = R.ROUTE[rid]
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    ho, wo = R.out_size(h, k, stride, pad, dil), R.out_size(w, k, stride, pad, dil)
    o, bias, spy = B.operands(rt, "dense"), R.bias_of(rt), Redirect(monkeypatch, fwd_size(rt))
    got = []
    for b in (None, bias):
        ybuf = torch.full((n, ho, wo, cout + 72), 7.0, device=dev())
        y, p, cnt, tr = forward(rt, o, spy, bias=b, ybuf=ybuf)
        assert bool((ybuf[..., :8] == 7.0).all()) and bool((ybuf[..., 8 + cout:] == 7.0).all())
        got.append((y, p, cnt))
    (y0, p0, c0), (y1, p1, c1) = got
    assert torch.equal(p0, p1) and (c0 is None or torch.equal(c0, c1)), "the partials depend on the bias"
    diff = (y1.double() - y0.double() - bias.double()).abs().max()
    print("bnp %-34s y(bias) - y - bias: %.3e of max|y|" % (rid + "-bias", float(diff / y1.abs().max())))
    assert float(diff) <= 2.0 ** -23 * float(torch.maximum(y0.abs().max(), y1.abs().max()))
    assert float((y1 - y0).abs().max()) > 0.5


# ---- the fused ASPP (rows sorted by tap set: merge-level) -----------------------------------------------------------------------
@pytest.mark.parametrize("cid,kind", B.ASPP_CASES, ids=["%s-%s" % c for c in B.ASPP_CASES])
def test_aspp_partials_merge_to_the_stored_outputs(cid, kind, monkeypatch):
    from iswm_amd import ops
    n, h, w, cin, cout, rates = R.ASPP[cid]
    ksize, dil = [1, 3, 3, 3], [1] + list(rates)
    rts, os_ = R.aspp_routes(cid), B.aspp_operands(cid, kind)
    calls, real = [], ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a: (calls.append(name), real(name, *a))[1])
    with R.conv_math(rts[0]):
        xp = ops.split_planes(os_[0]["x"].to(dev()))
        ldp = ops.pgeom(xp)[4]
        wf = []
        for o, kk, dl in zip(os_, ksize, dil):
            d = ops.ConvDesc(n, h, w, cin, h, w, cout, kk, kk, 1, dl * (kk - 1) // 2, dl, ldp, cout)
            buf = torch.empty((ops._pl2_bytes(d, 0) // 4,), dtype=torch.float32, device=dev())
            ops.call("iswm_conv2d_pl2_pack_weights", ctypes.byref(d), 0, ops._p(o["w_f"].to(dev())), ops._p(buf), ops._stream())
            wf.append(buf)
        res = ops.aspp_fwd(xp, ksize, dil, cout, wf, True)
        assert res is not None and calls.count("iswm_aspp_fwd") == 1
        ys, parts, tiles = res
    m = n * h * w
    cnt = B.counts(m, B.ASPP_TILE_ROWS)
    assert tiles == cnt.numel()
    for b in range(4):
        y, p = ys[b].cpu().reshape(m, cout), parts[b].cpu()
        assert tuple(p.shape) == (2, tiles, cout)
        mean, var = B.batch_stats(y)
        pm, pv = B.merge(p[0], p[1], cnt)
        tag = "%s-%s b%d" % (cid, kind, b)
        note(tag, cid + ".mean", rel_err(pm, mean), B.bound(cid + ".mean"))
        note(tag, cid + ".var", rel_err(pv, var), B.bound(cid + ".var"))
    settle()


# ---- depthwise 3 x 3 ---------------------------------------------------------------------------------------------------------------------
DW = B.DW_CASE_KINDS


@pytest.mark.parametrize("i,kind", DW, ids=["dw3_%d-%s" % c for c in DW])
def test_depthwise_partials_vs_stored_output(i, kind, monkeypatch):
    from iswm_amd import ops
    n, h, w, c, cw, s, d, sliced = B.dw_cases()[i]
    x, wt = B.dw_inputs(i, kind)
    m, tiles, tr = B.dw_layout(i)
    spy = Redirect(monkeypatch, 2 * tiles * c)
    xd = x.to(dev())
    if sliced:
        buf = torch.full((n, h, w, c + 12), 7.0, device=dev())
        buf[..., 4:4 + c] = xd
        xd = buf[..., 4:4 + c]
    g = ops.ConvGeom(xd, c, 3, 3, s, d, d)
    ybuf = torch.full((n, g.ho, g.wo, c + 12), 7.0, device=dev())
    out = ybuf[..., 8:8 + c] if sliced else None
    y, _, lay = ops.dwconv3x3_fwd_stats(xd, wt.to(dev()), g, True, out=out)
    assert spy.take() == [("iswm_dwconv3x3_fwd_stats", None)] and tuple(lay) == (tiles, tr) and m == n * g.ho * g.wo
    if sliced:
        assert bool((ybuf[..., :8] == 7.0).all()) and bool((ybuf[..., 8 + c:] == 7.0).all())
    p = spy.partials().view(2, tiles, c)
    y = y.cpu().reshape(m, c)
    tag, key = "dw3_%d-%s" % (i, kind), "dw3_%d" % i
    assert not p[:, :, cw:].any() and not y[:, cw:].any()           # channels past Cw see zero weights
    check_tiles(tag, key, p, y, tr, kind == "int", slice(0, cw))
    if i == B.DW_IDENTITY and kind == "offset":
        check_identity(tag, key, p, y, tr)
    settle()


# ---- the finalize on synthetic partials ------------------------------------------------------------------------------------------------
def fin_params(c):
    g = R.gen("fin-params", c)
    return (torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.3, torch.randn(c, generator=g),
            torch.rand(c, generator=g) + 0.5)


def run_finalize(tag, flat, n, c, tr, planes, gamma, beta, rm, rv, mom):
    """one finalize call against the float64 merge of the same partials"""
    from iswm_amd import ops
    tiles = n.numel()
    d = lambda t: None if t is None else t.to(dev())
    fd = flat.to(dev())
    part = fd[:planes * tiles * c].view(planes, tiles, c)            # (the counts of the tile_rows = 0 layout follow in `fd`)
    rmd, rvd = (None, None) if rm is None else (rm.to(dev()), rv.to(dev()))
    coef = ops.bn_finalize(part, tiles, int(n.sum()), tr, d(gamma), d(beta), rmd, rvd, mom).cpu()
    exp = B.fin_expected(flat, n, c, planes, gamma, beta, rm, rv, mom)
    same(tag, "shift", torch.equal(coef[1], exp["shift"].float()))
    same(tag, "save_mean", torch.equal(coef[2], exp["mean"].float()))
    note(tag, "fin.invstd", rel_err(coef[3], exp["invstd"]), B.bound("fin.invstd"))
    note(tag, "fin.scale", rel_err(coef[0], exp["scale"]), B.bound("fin.scale"))
    if rm is not None:
        note(tag, B.fin_key("rmean", mom, c), rel_err(rmd, exp["rmean"]), B.bound(B.fin_key("rmean", mom, c)))
        note(tag, B.fin_key("rvar", mom, c), rel_err(rvd, exp["rvar"]), B.bound(B.fin_key("rvar", mom, c)))
        if mom == 1.0:                              # the running variance IS the unbiased batch variance: the biased one from it
            tot = float(n.sum())
            var = rvd.cpu().double() * ((tot - 1) / tot if tot > 1 else 1.0)
            note(tag, "fin.var", rel_err(var, exp["var"]), B.bound("fin.var"))
    return coef, exp


@pytest.mark.parametrize("c,tiles,lay", B.FIN_CASES, ids=["c%d_t%d_%s" % x for x in B.FIN_CASES])
def test_finalize_vs_float64_merge(c, tiles, lay):
    gamma, beta, rm, rv = fin_params(c)
    for planes in ((2,) if lay == "counts" else (2, 3)):
        flat, n, tr = B.fin_partials(c, tiles, lay, planes)
        for mom in (0.1, 1.0):
            run_finalize("fin%d c%d t%d %s m%g" % (planes, c, tiles, lay, mom), flat, n, c, tr, planes, gamma, beta, rm, rv, mom)
    settle()


@pytest.mark.parametrize("planes", [2, 3])
def test_finalize_edges(planes):
    c = 5
    gamma, beta, rm, rv = fin_params(c)
    # one row in all: the unbiased variance falls back to the biased one (0)
    flat, n, tr = B.fin_partials(c, 1, "rows", planes, count_one=True)
    if planes == 3:
        flat[2 * c:] = 0                            # (one row: no residual)
    coef, exp = run_finalize("fin%d count 1" % planes, flat, n, c, tr, planes, gamma, beta, rm, rv, 1.0)
    assert not exp["var"].any() and torch.equal(coef[3], torch.full((c,), float(exp["invstd"][0])).float())
    # a constant channel: var 0, invstd = 1 / sqrt(eps)
    flat, n, tr = B.fin_partials(c, 33, "rows", planes, zero_m2_channel=2)
    if planes == 3:
        flat[2 * 33 * c:].view(33, c)[:, 2] = 0
    coef, exp = run_finalize("fin%d constant channel" % planes, flat, n, c, tr, planes, gamma, beta, rm, rv, 0.1)
    assert float(exp["var"][2]) == 0.0 and float(coef[3][2]) == float(torch.tensor(1.0 / (float(torch.tensor(B.EPS)) ** 0.5)).float())
    # no gamma / beta / running buffers
    flat, n, tr = B.fin_partials(c, 33, "rows", planes)
    coef, exp = run_finalize("fin%d no parameters" % planes, flat, n, c, tr, planes, None, None, None, None, 0.1)
    assert not coef[1].any() and torch.equal(coef[0], coef[3])
    settle()


# ---- the backward sums of iswm_conv2d_dgrad_pl2_bn and their consumer ---------------------------------------------------------------------
def dgrad_bn(rt, o, b, code, acc, spy):
    """-> (stored dx on the device, BnStats whose partials are the redirected buffer's, partials on the host [2, T, Cin])"""
    from iswm_amd import ops
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    m, tiles, tr = B.dgrad_layout(rt)
    dyd = to_dev(rt, o["dy"], cout)
    g = ops.ConvGeom(torch.empty(n, h, w, cin, device="meta"), cout, k, k, stride, pad, dil)
    coef = [b[k_].to(dev()) for k_ in ("scale", "shift", "mean", "invstd")]
    st = ops.BnStats(b["y"].to(dev()), coef, code == 2, mask=ops.split_planes(b["saved"].to(dev())) if code == 3 else None)
    if code == 3:                                   # the device's hi plane is the restatement's
        assert torch.equal(st.mask.t[0].float().cpu(), B.hi_plane(b["saved"]))
    dx = o["base"].to(dev()) if acc else None
    dx = ops.conv2d_dgrad(dyd, o["w_d"].to(dev()), g, (n, h, w, cin), dx=dx, accumulate=acc, bn_stats=st)
    assert spy.take() == [("iswm_conv2d_dgrad_pl2_bn", rt.names["dgrad"])]
    assert st.tiles == tiles and st.masked == (code == 3)
    assert spy.size == 2 * tiles * cin
    p = spy.partials().view(2, tiles, cin)
    st.partials = p.to(dev())
    return dx, st, p


@pytest.mark.parametrize("rid,code,acc", B.BWD_CASES, ids=["%s-code%d-acc%d" % c for c in B.BWD_CASES])
def test_backward_sums_and_their_consumer(rid, code, acc, monkeypatch):
    from iswm_amd import ops
    rt = R.ROUTE[rid]
    cin = rt.geom[3]
    o, b = R.operands(rt, "dense"), B.bwd_inputs(rid)
    tag, key = "%s-code%d-acc%d" % (rid, code, acc), "bwd.%s" % rid
    spy = Redirect(monkeypatch, 2 * B.dgrad_layout(rt)[1] * cin, torch.float64)
    with R.conv_math(rt):
        dxd, st, p = dgrad_bn(rt, o, b, code, acc, spy)
        dx = dxd.cpu()
        pat = B.pattern(code, b)
        # the stored gradient: float64 for codes 0 and 2; code 3 = the code-0 gradient under the hi-plane pattern, bit for bit
        # (also in tiles no tap reaches: with accumulate they hold the old gradient, masked)
        if code == 3:
            plain = dgrad_bn(rt, o, b, 0, acc, spy)[0].cpu()
            same(tag, "dx == mask(plain dx)", torch.equal(dx, torch.where(pat, plain, torch.zeros_like(plain))))
            assert int((~pat).sum()) > 100
        else:
            q = "dx_acc" if acc else "dx"
            note(tag, R.check_name(rt, q), rel_err(dx, R.restate(rt, o)[q]), R.bound(R.check_name(rt, q)))
        # 1. the partials: summed over their tile axis, against float64 of the stored dx
        ref = B.bwd_sums(dx, pat, b)
        note(tag, key + ".sum_dz", rel_err(p[0].sum(0), ref[0]), B.bound(key + ".sum_dz"))
        note(tag, key + ".sum_dzx", rel_err(p[1].sum(0), ref[1]), B.bound(key + ".sum_dzx"))
        # 2. the consumer, and the reducing path on the same inputs
        dz = dx * pat
        relu = code == 2
        yd, gd = st.y, b["gamma"].to(dev())
        # the producer's saved activation, as the network hands it over (with mask_scale / mask_shift its pattern is recomputed
        # from y and the tensor is not read, but the entry point wants its pitch)
        act = torch.relu((b["y"] - b["mean"]) * b["scale"] + b["shift"]).to(dev()) if relu else None
        for training in (True, False):
            want = B.bn_backward_ref(dz, b, training)
            kdy = key + (".dy" if training else ".dy_eval")
            outs = {}
            for planes in (False, True):
                for fused in (True, False):
                    dg, db = torch.empty(cin, device=dev()), torch.empty(cin, device=dev())
                    dy, _ = ops.bn_backward(dxd, act, yd, st.coef, gd, relu, training, dg, db, dy_planes=planes,
                                            stats=st if fused else None)
                    dy = ops.as_f32(dy).cpu()
                    t2 = "%s %s %s %s" % (tag, "train" if training else "eval", "planes" if planes else "fp32", "stats" if fused else "reduce")
                    note(t2, key + ".sum_dzx", rel_err(dg, want[1]), B.bound(key + ".sum_dzx"))
                    note(t2, key + ".sum_dz", rel_err(db, want[2]), B.bound(key + ".sum_dz"))
                    note(t2, kdy, rel_err(dy, want[0]), B.bound(kdy))
                    outs[(planes, fused)] = dy
            same(tag, "dy planes == dy fp32", torch.equal(outs[(True, True)], outs[(False, True)]))
            eq = torch.equal(outs[(False, True)], outs[(False, False)])
            print("bnp %-34s dy from the taken sums %s dy from the reducing path (%s)" % (tag, "==" if eq else "!=", "train" if training else "eval"))
            if not training:                        # eval: dy = gamma invstd dz per element, no sum enters: the same bits
                same(tag, "eval dy stats == reduce", eq)
    settle()
