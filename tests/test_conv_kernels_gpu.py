"""Every convolution kernel route against the float64 restatement of tests/conv_ref.py, through the op wrappers over the C ABI:
forward, data gradient (plain and accumulating into a non-trivial base) and weight gradient, as the route has them.

Rule: rel_err = max|a - b| / max|b| against float64 must be <= 4 x FLOOR[check], FLOOR = torch's own fp32 CPU operator on the
same inputs (tests/test_conv_ref_cpu.py re-measures it and shows that this bound sees a single missing or misrouted plane
product in every case, also when only one K stage carries it).  Exact-integer operands must come out equal.  Nothing is
taken from the kernel under test; each test asserts the entry point the wrapper took and the kernel it launches, so a planner
change cannot move a case to another kernel unnoticed.  profiles/conv_kernel_tests.txt has the measured figures.

The BatchNorm partials of the epilogues are pinned tile by tile in tests/test_bn_partials_gpu.py."""
import ctypes

import pytest
import torch

from tests import conv_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


FAILED = []


def compare(tag, key, got, ref, exact):
    """print the figure and note a miss; settle() asserts once a test has printed all of its figures.  Equality for the
    exact-integer operands, else the bound of tests/conv_ref.py (4 x floor)"""
    if exact:
        ok = torch.equal(got.double(), ref.double())
        print("conv %-34s %-22s %s" % (tag, key, "equal" if ok else "DIFFERS (rel %.3e)" % rel_err(got, ref)))
    else:
        err = rel_err(got, ref)
        ok = err <= R.bound(key)
        print("conv %-34s %-22s err %.3e  bound %.3e" % (tag, key, err, R.bound(key)))
    if not ok:
        FAILED.append("%s %s" % (tag, key))


def settle():
    missed = list(FAILED)
    del FAILED[:]
    assert not missed, missed


class Spy(object):
    """records (entry point, device kernel name) of every convolution call the wrappers make"""

    def __init__(self, monkeypatch):
        from iswm_amd import _lib, ops
        self.calls, lib, real = [], _lib.load(), ops.call

        def spy(name, *a):
            if name in R.KIND:
                self.calls.append((name, R.kernel_name(lib, a[0]._obj, R.KIND[name])))
            elif name in ("iswm_aspp_fwd", "iswm_aspp_bwd"):
                self.calls.append((name, None))
            return real(name, *a)

        monkeypatch.setattr(ops, "call", spy)

    def take(self):
        out, self.calls = self.calls, []
        return out


def to_dev(rt, t, c, wider=0, at=0):
    """an activation on the device in the form the route gives it: planes where the network would (gathered channels % 64 == 0
    on a planes route), else fp32.  wider > 0: a channel slice [at, at + c) of a buffer of `wider` channels whose other
    channels hold a sentinel"""
    from iswm_amd import ops
    t = t.to(dev())
    if wider:
        buf = torch.full(tuple(t.shape[:3]) + (wider,), 1.0e4, device=dev())
        buf[..., at:at + c] = t
        t = buf
    if R.planes_operand(rt, c):
        p = ops.split_planes(t.contiguous())
        return p[..., at:at + c] if wider else p
    return t[..., at:at + c] if wider else t


def run_route(rt, o, spy, exact, tag, ref):
    from iswm_amd import ops
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    plan = R.planned(rt)
    with R.conv_math(rt):
        xd = to_dev(rt, o["x"], cin)
        g = ops.ConvGeom(xd, cout, k, k, stride, pad, dil)
        got = {}
        if "fwd" in rt.names:
            got["y"] = ops.conv2d_fwd(xd, o["w_f"].to(dev()), g)[0].cpu()
            assert spy.take() == [plan["fwd"]] and plan["fwd"][1] == rt.names["fwd"]
        if "dgrad" in rt.names:
            dyd, wd = to_dev(rt, o["dy"], cout), o["w_d"].to(dev())
            got["dx"] = ops.conv2d_dgrad(dyd, wd, g, (n, h, w, cin)).cpu()
            acc = o["base"].to(dev())
            ops.conv2d_dgrad(dyd, wd, g, (n, h, w, cin), dx=acc, accumulate=True)
            got["dx_acc"] = acc.cpu()
            assert spy.take() == [plan["dgrad"]] * 2 and plan["dgrad"][1] == rt.names["dgrad"]
        if "wgrad" in rt.names:
            dyw = to_dev(rt, o["dy_w"], cout)
            dw = ops.conv2d_wgrad(xd, dyw, g)
            got["dw"] = dw.cpu()
            assert spy.take() == [plan["wgrad"]] and plan["wgrad"][1] == rt.names["wgrad"]
            if ops.is_planes(dyw):                    # the fp32-dy form splits dy on the way in: the same bits
                assert torch.equal(ops.conv2d_wgrad(xd, o["dy_w"].to(dev()), g), dw)
            if rt.id.startswith("stem"):
                assert not got["dw"][..., 3].any()    # the padding channel of the image receives no gradient
    out = R.unscale(rt, o, got)
    for q in out:
        compare(tag, R.check_name(rt, q), out[q], ref[q], exact)
    settle()


@pytest.mark.parametrize("rid,kind", R.CASES, ids=["%s-%s" % c for c in R.CASES])
def test_conv_route_vs_float64(rid, kind, monkeypatch):
    rt = R.ROUTE[rid]
    o = R.operands(rt, kind)
    run_route(rt, o, Spy(monkeypatch), kind == "int", "%s-%s" % (rid, kind), R.restate(rt, o))


# ---- bias, channel slices of wider buffers, sentinels --------------------------------------------------------------------------
@pytest.mark.parametrize("rid", R.SLICE_ROUTES)
def test_conv_bias_and_channel_slices(rid, monkeypatch):
    """x, dy read from channel slices of wider buffers; y, dx written (and dx accumulated) into channel slices of wider buffers
    whose other channels must keep their sentinel; bias on the forward"""
    from iswm_amd import ops
    rt = R.ROUTE[rid]
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    o = R.operands(rt, "dense")
    bias = R.bias_of(rt)
    ref = R.restate(rt, o, bias=bias)
    spy, plan, tag = Spy(monkeypatch), R.planned(rt), rid + "-slices"
    with R.conv_math(rt):
        xd = to_dev(rt, o["x"], cin, wider=cin + 128, at=64)
        dyd = to_dev(rt, o["dy"], cout, wider=cout + 64, at=64)
        g = ops.ConvGeom(xd, cout, k, k, stride, pad, dil)
        ybuf = torch.full((n, g.ho, g.wo, cout + 72), 7.0, device=dev())
        ops.conv2d_fwd(xd, o["w_f"].to(dev()), g, bias=bias.to(dev()), out=ybuf[..., 8:8 + cout])
        assert [c[0] for c in spy.take()] == [plan["fwd"][0]]
        assert bool((ybuf[..., :8] == 7.0).all()) and bool((ybuf[..., 8 + cout:] == 7.0).all())
        dxbuf = torch.full((n, h, w, cin + 40), -3.0, device=dev())
        ops.conv2d_dgrad(dyd, o["w_d"].to(dev()), g, (n, h, w, cin), dx=dxbuf[..., 32:32 + cin])
        dx = dxbuf[..., 32:32 + cin].cpu()
        assert bool((dxbuf[..., :32] == -3.0).all()) and bool((dxbuf[..., 32 + cin:] == -3.0).all())
        dxbuf[..., 32:32 + cin] = o["base"].to(dev())
        ops.conv2d_dgrad(dyd, o["w_d"].to(dev()), g, (n, h, w, cin), dx=dxbuf[..., 32:32 + cin], accumulate=True)
        assert bool((dxbuf[..., :32] == -3.0).all()) and bool((dxbuf[..., 32 + cin:] == -3.0).all())
        assert [c[0] for c in spy.take()] == [plan["dgrad"][0]] * 2
        dw = ops.conv2d_wgrad(xd, dyd, g)
        assert [c[0] for c in spy.take()] == [plan["wgrad"][0]]
        got = dict(y_bias=ybuf[..., 8:8 + cout].cpu(), dx=dx, dx_acc=dxbuf[..., 32:32 + cin].cpu(), dw=dw.cpu())
    ref["y_bias"] = ref.pop("y")
    out = R.unscale(rt, o, got)
    for q in out:
        compare(tag, R.check_name(rt, q), out[q], ref[q], False)
    settle()


# ---- the data gradient that also serves the producer's BatchNorm backward ---------------------------------------------------------
@pytest.mark.parametrize("rid", ["pl_3x3", "pl_1x1", "pl_s2", "pl_narrow"])
@pytest.mark.parametrize("code", [0, 2, 3])
@pytest.mark.parametrize("accumulate", [False, True])
def test_conv_dgrad_bn_relu_codes(rid, code, accumulate, monkeypatch):
    """iswm_conv2d_dgrad_pl2_bn at each relu code.  Codes 0 and 2 store the plain gradient (the pattern only enters the
    BatchNorm partials: tests/test_bn_partials_gpu.py::test_backward_sums_and_their_consumer pins those); code 3 stores it
    masked by (hi plane of the producer's saved output > 0): the reference applies the same mask in float64 and masked elements must be exactly 0 -- on a saved output that
    holds exact zeros, negative zeros and tiny positive values (2^-100: its hi plane is still positive)"""
    from iswm_amd import ops
    rt = R.ROUTE[rid]
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    o = R.operands(rt, "dense")
    ref = R.restate(rt, o)
    gm = R.gen(rid, "bn")
    saved = torch.randn(n, h, w, cin, generator=gm)
    flat = saved.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = 2.0 ** -100
    keep = (saved > 0).double()
    spy = Spy(monkeypatch)
    with R.conv_math(rt):
        dyd = to_dev(rt, o["dy"], cout)
        g = ops.ConvGeom(torch.empty(n, h, w, cin, device="meta"), cout, k, k, stride, pad, dil)
        yprod = torch.randn(n, h, w, cin, generator=gm).to(dev())
        coef = [torch.rand(cin, generator=gm).add(0.5).to(dev()) for _ in range(4)]
        st = ops.BnStats(yprod, coef, code == 2, mask=ops.split_planes(saved.to(dev())) if code == 3 else None)
        dx = o["base"].to(dev()) if accumulate else None
        dx = ops.conv2d_dgrad(dyd, o["w_d"].to(dev()), g, (n, h, w, cin), dx=dx, accumulate=accumulate, bn_stats=st)
        assert spy.take() == [("iswm_conv2d_dgrad_pl2_bn", rt.names["dgrad"])]
        assert st.partials is not None and st.masked == (code == 3)
        got = dx.cpu()
    q = "dx_acc" if accumulate else "dx"
    want = ref[q] * keep if code == 3 else ref[q]
    if code == 3:
        masked = got[keep == 0]
        assert masked.numel() > 100 and not masked.any()
    compare("%s-bn%d" % (rid, code), R.check_name(rt, q), got, want, False)
    settle()


# ---- the fused ASPP pair --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,kind", R.ASPP_CASES, ids=["%s-%s" % c for c in R.ASPP_CASES])
def test_aspp_pair_vs_float64(cid, kind, monkeypatch):
    """iswm_aspp_fwd / iswm_aspp_bwd: the four branch outputs, the summed data gradient (plain and accumulating) and the four
    weight gradients the backward launch also computes"""
    from iswm_amd import ops
    n, h, w, cin, cout, rates = R.ASPP[cid]
    ksize, dil = [1, 3, 3, 3], [1] + list(rates)
    rts, os_ = R.aspp_routes(cid), R.aspp_operands(cid, kind)
    ref = R.aspp_restate(cid, os_)
    spy = Spy(monkeypatch)
    with R.conv_math(rts[0]):
        xp = ops.split_planes(os_[0]["x"].to(dev()))
        ldp = ops.pgeom(xp)[4]

        def pack(wt, kk, dl, kind_, ldx, ldy):
            d = ops.ConvDesc(n, h, w, cin, h, w, cout, kk, kk, 1, dl * (kk - 1) // 2, dl, ldx, ldy)
            buf = torch.empty((ops._pl2_bytes(d, kind_) // 4,), dtype=torch.float32, device=dev())
            ops.call("iswm_conv2d_pl2_pack_weights", ctypes.byref(d), kind_, ops._p(wt.to(dev())), ops._p(buf), ops._stream())
            return buf

        wf = [pack(o["w_f"], kk, dl, 0, ldp, cout) for o, kk, dl in zip(os_, ksize, dil)]
        wdg = [pack(o["w_d"], kk, dl, 1, cin, 4 * cout) for o, kk, dl in zip(os_, ksize, dil)]
        res = ops.aspp_fwd(xp, ksize, dil, cout, wf, False)
        assert res is not None and spy.take() == [("iswm_aspp_fwd", None)]
        got = dict(("b%d.y" % b, y.cpu()) for b, y in enumerate(res[0]))
        dyc = ops.split_planes(torch.cat([o["dy"] for o in os_], 3).to(dev()))
        dx = ops.aspp_dgrad(dyc, ksize, dil, cin, cout, wdg)
        assert dx is not None
        acc = os_[0]["base"].to(dev())
        ops.aspp_dgrad(dyc, ksize, dil, cin, cout, wdg, dx=acc, accumulate=True)
        dyw = ops.split_planes(torch.cat([o["dy_w"] for o in os_], 3).to(dev()))
        dws = [torch.empty(cout, kk, kk, cin, device=dev()) for kk in ksize]
        ops.aspp_dgrad(dyw, ksize, dil, cin, cout, wdg, dx=torch.zeros(n, h, w, cin, device=dev()), accumulate=True, x=xp, dws=dws)
        assert spy.take() == [("iswm_aspp_bwd", None)] * 3
        got.update(dx=dx.cpu(), dx_acc=acc.cpu())
        got.update(("b%d.dw" % b, t.cpu()) for b, t in enumerate(dws))
    for q, v in got.items():
        b = int(q[1]) if q[0] == "b" else 0
        f = R.factor(rts[b], os_[b], q.split(".")[-1])
        compare("%s-%s" % (cid, kind), "%s.%s" % (cid, q), v.double() * f, ref[q], kind == "int")
    settle()
