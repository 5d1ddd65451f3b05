"""The INT8 kernels (csrc/qconv.hip, csrc/quant.hip) at the edge shapes of tests/quant_cases.py, and the INT8 network
at the smallest maps a real model meets, against the numpy restatement tests/quant_ref.py: every comparison is
equality.  tests/test_quant_cpu.py asserts, without a GPU, that each case has the property it exists for."""
import functools

import numpy as np
import pytest
import torch

from tests import quant_cases as Q
from tests import quant_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def _t(v):
    return torch.from_numpy(np.ascontiguousarray(v)).to(dev())


def _ids(table):
    return [c.id for c in table]


def _packed_weights(c, o):
    cout_p = Q.ceil16(c.Cout)
    wp = np.zeros((cout_p, c.k, c.k, c.Cin), np.int8)
    wp[:c.Cout] = o["w"].transpose(0, 2, 3, 1)
    m, a = np.zeros(cout_p), np.zeros(cout_p)
    m[:c.Cout], a[:c.Cout] = o["mul"], o["add"]
    return _t(wp.reshape(cout_p, -1)), _t(m), _t(a)


@pytest.mark.parametrize("c", Q.QCONV, ids=_ids(Q.QCONV))
def test_qconv_edge_case(c):
    """k_qconv into a channel slice between sentinels; x_slice reads a channel slice; a residual has pitch pad4(cstore)"""
    from iswm_amd import ops
    o = Q.qconv_operands(c)
    want = Q.qconv_expected(c, o)
    t = Q.qconv_tiles(c)
    w, mul, add = _packed_weights(c, o)
    x = _t(o["xbuf"])[..., o["x0"]:o["x0"] + c.Cin]
    ld = Q.pad4(c.Cout) + 32
    shape = (c.N, t["Ho"], t["Wo"], ld)
    sentinel = 7.0 if c.f32 else 55
    buf = torch.full(shape, sentinel, dtype=torch.float32 if c.f32 else torch.int8, device=dev())
    res = None
    if c.residual:
        rbuf = np.full(shape[:3] + (Q.pad4(c.Cout),), 101, np.int8)
        rbuf[..., :c.Cout] = o["res"]
        res = _t(rbuf)[..., :c.Cout]
    ops.qconv_fwd(x, w, mul, add, c.k, c.stride, c.pad, c.dil, c.relu, o["lo"], 1.0 if c.f32 else o["inv_s"],
                  out=buf[..., 16:16 + c.Cout], res=res, s_res=o["s_res"], out_f32=c.f32, cstore=c.Cout)
    b = buf.cpu().numpy()
    got = b[..., 16:16 + c.Cout]
    assert np.array_equal(got, want), "%d of %d differ" % ((got != want).sum(), want.size)
    assert (b[..., :16] == sentinel).all() and (b[..., 16 + c.Cout:] == sentinel).all()


@pytest.mark.parametrize("cid", ["cstore_3_i8", "cstore_3_f32", "cstore_17_res"])
def test_qconv_default_output_with_a_ragged_cstore(cid):
    """qconv_fwd's own output for cstore % 4 != 0: a view of cstore channels on a pad4(cstore) pitch"""
    from iswm_amd import ops
    c = Q.QCONV_BY_ID[cid]
    o = Q.qconv_operands(c)
    w, mul, add = _packed_weights(c, o)
    res = None
    if c.residual:
        rbuf = np.zeros(o["res"].shape[:3] + (Q.pad4(c.Cout),), np.int8)
        rbuf[..., :c.Cout] = o["res"]
        res = _t(rbuf)[..., :c.Cout]
    y = ops.qconv_fwd(_t(o["xbuf"]), w, mul, add, c.k, c.stride, c.pad, c.dil, c.relu, o["lo"],
                      1.0 if c.f32 else o["inv_s"], res=res, s_res=o["s_res"], out_f32=c.f32, cstore=c.Cout)
    assert y.shape[3] == c.Cout and y.stride(2) == Q.pad4(c.Cout)
    assert np.array_equal(y.cpu().numpy(), Q.qconv_expected(c, o))


def test_one_pixel_views_keep_their_pitch():
    """ops.geom on a [1, 1, 1, C] channel slice reports the buffer's pitch, so a one-pixel convolution can store a
    ragged cstore (its default output has pitch 4) and a slice of a pitch the C ABI refuses is refused"""
    from iswm_amd import _lib, ops
    buf = torch.zeros((1, 1, 1, 96), dtype=torch.int8, device=dev())
    assert ops.i8geom(buf[..., 16:19]) == (1, 1, 1, 3, 96) and ops.i8geom(buf) == (1, 1, 1, 96, 96)
    assert ops.i8geom(buf.expand(1, 1, 1, 96)) == (1, 1, 1, 96, 96)
    c = Q.QConv("one_pixel_cstore3", 1, 1, 1, 64, 3, 1, 1, 0, 1, False, False, False, "")
    o = Q.qconv_operands(c)
    w, mul, add = _packed_weights(c, o)
    y = ops.qconv_fwd(_t(o["xbuf"]), w, mul, add, 1, 1, 0, 1, False, o["lo"], o["inv_s"], cstore=3)
    assert y.shape == (1, 1, 1, 3) and np.array_equal(y.cpu().numpy(), Q.qconv_expected(c, o))
    odd = torch.zeros((1, 1, 1, 72), dtype=torch.int8, device=dev())[..., :64]      # pitch 72: not a multiple of 16
    with pytest.raises(_lib.IswmError, match="ldx % 16 == 0"):
        ops.qconv_fwd(odd, w, mul, add, 1, 1, 0, 1, False, o["lo"], o["inv_s"], cstore=3)


@pytest.mark.parametrize("c", Q.ABSMAX, ids=_ids(Q.ABSMAX))
def test_absmax_edge_case(c):
    from iswm_amd import ops
    buf = Q.absmax_operands(c)
    want = R.absmax(buf[..., c.c0:c.c0 + c.C], None, c.amax0)
    t = _t(buf)
    src = (ops.split_planes(t) if c.planes else t)[..., c.c0:c.c0 + c.C]
    a = torch.full((1,), c.amax0, dtype=torch.float32, device=dev())
    ops.absmax(src, a)
    assert a.item() == want
    if c.c0 == 0:                                               # the same through the channel-count argument
        a.fill_(c.amax0)
        ops.absmax(ops.split_planes(t) if c.planes else t, a, c.C)
        assert a.item() == want


@pytest.mark.parametrize("c", Q.QUANTIZE, ids=_ids(Q.QUANTIZE))
def test_quantize_i8_edge_case(c):
    from iswm_amd import ops
    x = Q.quantize_operands(c)
    want = R.quantize(x, c.inv_s, c.lo)
    xp = np.full(x.shape[:3] + (Q.pad4(c.C),), 77.0, np.float32)      # past C inside the last group: never quantized
    xp[..., :c.C] = x
    if c.id == "near_ties_planes":
        src = ops.Planes(Q.planes_by_rounding(xp).to(dev()))
    else:
        src = ops.split_planes(_t(xp)) if c.planes else _t(xp)
    q = ops.quantize_i8(src[..., :c.C], c.inv_s, c.lo, ldy=c.ldy).cpu().numpy()
    assert q.shape == x.shape[:3] + (c.ldy,)
    assert np.array_equal(q[..., :c.C], want) and not q[..., c.C:].any()


@pytest.mark.parametrize("c", Q.QGAP, ids=_ids(Q.QGAP))
def test_qgap_edge_case(c):
    from iswm_amd import ops
    buf = Q.qgap_operands(c)
    want = R.qgap(buf[..., :c.C], c.s_in)
    y = ops.qgap(_t(buf)[..., :c.C], c.s_in, 1.0 / c.s_in, ldy=c.ldy).cpu().numpy()
    assert y.shape == (c.N, 1, 1, c.ldy)
    assert np.array_equal(y[..., :c.C], want) and not y[..., c.C:].any()


@pytest.mark.parametrize("c", Q.QBCAST, ids=_ids(Q.QBCAST))
def test_qbcast_edge_case(c):
    from iswm_amd import ops
    rng = Q.rng_of("qbcast_" + c.id)
    v = rng.integers(-128, 128, (c.N, 1, 1, c.ldv)).astype(np.int8)
    v[0, 0, 0, 0] = -128
    buf = torch.full((c.N, c.H, c.W, c.C + 24), 9, dtype=torch.int8, device=dev())
    ops.qbcast(_t(v)[..., :c.C], buf[..., 8:8 + c.C])
    b = buf.cpu().numpy()
    assert np.array_equal(b[..., 8:8 + c.C], np.broadcast_to(v[..., :c.C], (c.N, c.H, c.W, c.C)))
    assert (b[..., :8] == 9).all() and (b[..., 8 + c.C:] == 9).all()


@pytest.mark.parametrize("c", Q.QBILINEAR, ids=_ids(Q.QBILINEAR))
def test_qbilinear_edge_case(c):
    """source and destination are both channel slices of wider buffers"""
    from iswm_amd import ops
    x = Q.qbilinear_operands(c)
    want = R.qbilinear(x, c.s_in, c.Ho, c.Wo, c.inv_s)
    c0, tail = Q.QBIL_PITCH
    src = np.full((c.N, c.Hi, c.Wi, c0 + c.C + tail), 99, np.int8)
    src[..., c0:c0 + c.C] = x
    dst = torch.full((c.N, c.Ho, c.Wo, c0 + c.C + tail), 3, dtype=torch.int8, device=dev())
    ops.qbilinear(_t(src)[..., c0:c0 + c.C], c.s_in, c.inv_s, dst[..., c0:c0 + c.C])
    d = dst.cpu().numpy()
    assert np.array_equal(d[..., c0:c0 + c.C], want)
    if c.id == "identity":
        assert np.array_equal(d[..., c0:c0 + c.C], x)               # against the input itself
    assert (d[..., :c0] == 3).all() and (d[..., c0 + c.C:] == 3).all()


@functools.lru_cache(maxsize=None)
def _r50(os_):
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=os_, pretrained_backbone=False)
    m.load_state_dict(synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, os_)), strict=True)
    return m.to(dev()).eval()


@pytest.mark.parametrize("os_,n,h,w", Q.NETWORK)
def test_network_at_the_smallest_maps(os_, n, h, w):
    """deeplabv3plus_resnet50 on 33 x 33 and 33 x 49 inputs: at output stride 16 the layer4 map is 3 x 3 (3 x 4), so
    M = 9 N (12 N) is below one row block of a wave at N = 1, the rate 12 and 18 branches are centre-only, and the
    pooled branch runs at M = N.  body(stem(x)) equals the restatement bit for bit, a batch equals its batch-1 calls."""
    from iswm_amd import quant
    from oracle.synth import synth_images
    m = _r50(os_)
    amax = quant.calibrate(m, [synth_images(n, h, w, seed=s).to(dev()) for s in (1, 2)])
    qm = quant.quantize_model(m, amax)
    x = synth_images(n, h, w, seed=7).to(dev())
    with torch.no_grad():
        q = qm.stem(x)
        yl = qm.body(q)
        assert torch.equal(qm.forward_lowres(x), yl)
        one = torch.cat([qm.forward_lowres(x[i:i + 1]) for i in range(n)])
    assert q.shape == (n, (h + 3) // 4, (w + 3) // 4, 64)
    assert torch.equal(one, yl)
    want = R.forward_body(qm.state_int8(), q.cpu().numpy())
    got = yl.cpu().numpy()
    assert got.shape == want.shape[:3] + (4,)
    assert np.array_equal(got[..., :2], want), np.abs(got[..., :2] - want).max()
