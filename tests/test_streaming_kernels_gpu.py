"""The streaming (non-MFMA) kernels every step goes through -- csrc/loss.hip, resize.hip, dwconv.hip, optim.hip, misc.hip
(dropout, copies), pool.hip and the plain passes of bn.hip -- each against the float64 restatement of its operation in
tests/streaming_ref.py, at the smallest shapes that reach every path of the kernel: both class-axis paths of the loss and the
boundary between them, its finalize lane loop and block cap, downscales / unequal ratios / single pixels through the bilinear
gather window, every filter shape of the general depthwise kernels, the optimizers' scalar tails, the Philox stream bit for bit,
ragged channel blocks and pitched operands of the pooling kernels, and BatchNorm inputs whose mean is thousands of standard
deviations from zero.

The second BatchNorm table ("bn2", ordinary statistics: the large-mean floors are too wide to see a lost plane) adds the forms
every training step of the default configuration runs: both sides of the reduce pass's `M <= 8192` switch, a thread that walks
two fp32 runs of 8 rows (the second ragged), the 1024-tile cap of iswm_colstat_tiles with k_bn_bwd_finalize<double, 4> at 259 and
1024 tiles (also on ready partials, iswm_bn_backward_stats_pl), a ragged second column block in the 4-channel kernels and in
k_bn_apply8, k_bn_apply8's pair loop and tail row at 0 - 4 rows per thread, the 4-channel kernel with plane loads and stores where
the dispatch of iswm_bn_apply_pl refuses the 8-channel one, and every activation x residual x format combination of the dispatch
macros (ReLU + residual reads the pattern from the saved output: fp32, or the hi plane).  The same passes, split / join, and
max-pool, global pool, broadcast and bilinear resize into Planes also run in the one-plane mode of conv math "bf16": a one-plane
store must be torch's round-to-nearest-even bfloat16 of the fp32-format result bit for bit, a one-plane read is exact (the
restatement is fed the rounded tensor, the bounds stay).  Which path each case reaches is asserted on the CPU from the restated
plan (tests/test_streaming_ref_cpu.py), never from a kernel's name or code.

The bound rule.  Every float comparison is rel_err = max|a - b| / max|b| against the float64 restatement and must be within
4 x FLOOR[check].  FLOOR[check] (tests/streaming_ref.py, measured again by tests/test_streaming_ref_cpu.py) is the error of
torch's own fp32 implementation of the same operation against the same restatement on the same inputs, the largest over the
check's cases.  The factor 4 is for a different summation order and FMA contraction between two fp32 implementations of the same
arithmetic; a wrong tap, weight, index or scale moves the error to 1e-2 or more.  Where that floor is 0 -- identity resize, data
movement, masks, the gradient of ignored pixels, channels past the weight's -- the assertion is equality.  No bound here was
chosen from what the kernels give.  profiles/streaming_kernel_tests.txt lists floor, bound and the error measured on an MI355X
for every check, and says where 4 x floor is looser than the bound the kernel's older test uses (large-mean BatchNorm: an fp32
mean costs half an ulp of the mean divided by the standard deviation).

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import streaming_ref as R
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def emit(line):
    print(line)
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write(line + "\n")


def check(key, actual, expected, what="", worst=None):
    """rel_err(actual, float64 restatement) <= 4 x FLOOR[key].  `worst` (a dict): the caller loops over many combinations of one
    check and reports only the largest figure per key (report_worst); every figure is still asserted here"""
    floor = R.FLOOR[key]
    bound = 4 * floor
    a = actual.detach().cpu() if torch.is_tensor(actual) else actual
    err = rel_err(a.reshape(expected.shape) if torch.is_tensor(a) else a, expected)
    line = "%-20s floor %.1e  bound %.1e  measured %.2e  %s" % (key, floor, bound, err, what)
    if worst is None:
        emit(line)
    elif err >= worst.get(key, (-1.0, ""))[0]:
        worst[key] = (err, line)
    assert err <= bound, line


def report_worst(worst, what):
    for key in sorted(worst):
        emit(worst[key][1] + "  (largest of " + what + ")")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


def sliced(t, off, extra=12, fill=7.0):
    """t [..., C] on the GPU as channels [off, off + C) of a buffer `extra` channels wider, filled with `fill` elsewhere"""
    t = t.to(dev())
    buf = torch.full(tuple(t.shape[:-1]) + (t.shape[-1] + extra,), fill, device=dev())
    buf[..., off:off + t.shape[-1]] = t
    return buf[..., off:off + t.shape[-1]]


def untouched(view, off, fill=7.0):
    base, c = view._base, view.shape[-1]
    return bool((base[..., :off] == fill).all()) and bool((base[..., off + c:] == fill).all())


# ======================================================================================================================
# loss
# ======================================================================================================================
def run_loss(logits, labels, wt, alpha, gamma, mode, up, upstream_tensor):
    from iswm_amd import ops
    d = dev()
    loss, sums, grad = ops.loss_fwd(logits.to(d), labels.to(d), None if wt is None else wt.to(d), R.IGNORE, alpha, gamma, mode)
    sums = sums.clone()
    upstream = torch.tensor([up], dtype=torch.float32, device=d) if upstream_tensor else None
    ops.loss_bwd_scale(grad, sums, upstream, mode, labels.numel())
    return loss, sums, grad


@pytest.mark.parametrize("case", R.LOSS_CASES, ids=R.LOSS_IDS)
def test_loss_value_sums_gradient(case):
    c, kind, mode, alpha, gamma, weighted, up, shape = case
    logits, labels, weight = R.loss_inputs(c, kind, R.LOSS_SHAPES[shape])
    wt = weight if weighted else None
    v, s, g = R.loss_ref(logits, labels, wt, R.IGNORE, alpha, gamma, mode)
    loss, sums, grad = run_loss(logits, labels, wt, alpha, gamma, mode, up, up != 1.0 or kind == "i64")
    check("loss.value.m%d" % mode, loss, v)
    check("loss.sums", sums, s)
    check("loss.grad.m%d" % mode, grad, g * R.f32(up))
    invalid = ~R.loss_valid(labels, c)
    assert int(invalid.sum()) >= 4
    at_invalid = grad.cpu().permute(0, 2, 3, 1)[invalid]
    assert torch.equal(at_invalid, torch.zeros_like(at_invalid)), "gradient of an ignored / out-of-range label is not exactly 0"


def test_loss_block_cap_second_trip():
    """2 x 2049 x 2049 pixels > 8192 blocks x 256 threads x 4: every thread goes round the grid-stride loop twice"""
    from iswm_amd import _lib
    logits, labels, weight = R.loss_inputs(2, "u8", R.LOSS_CAP_SHAPE)
    npix = labels.numel()
    assert _lib.load().iswm_loss_blocks(npix) == 8192 and npix > 8192 * 1024
    v, s, g = R.loss_ref(logits, labels, weight, R.IGNORE, 1.0, 0.0, 0)
    loss, sums, grad = run_loss(logits, labels, weight, 1.0, 0.0, 0, 1.0, False)
    check("loss.cap.value", loss, v)
    pick = torch.arange(0, npix // 2, 4099)                                   # a strided sample of the pixels, last block included
    pick = torch.cat([pick, torch.tensor([npix // 2 - 1])])
    sample = lambda t: t.reshape(2, 2, -1)[:, :, pick.to(t.device)]
    check("loss.cap.grad", sample(grad), sample(g))
    invalid = (~R.loss_valid(labels, 2)).to(dev())
    assert not bool(grad.permute(0, 2, 3, 1)[invalid].any())


@pytest.mark.parametrize("c", [3, 9], ids=["registers", "streamed"])
@pytest.mark.parametrize("mode", [1, 2])
def test_loss_all_confident_gradient_is_finite(c, mode):
    """logit gap 40 on the labelled class, gamma 0.5: 1 - pt == 0 in fp32, and powf(0, gamma - 1) is inf.  The true gradient is
    below 1e-20, far under anything fp32 resolves next to logits of 40: the kernel must give a finite value within 1e-12 of it
    (an absolute bound from that reasoning, outside the 4 x floor rule: the floor of a quantity that is 0 in fp32 is 0, and the
    restatement's 1e-26 is not 0)."""
    labels = torch.randint(0, c, (2, 7, 9), generator=R.gen(c))
    logits = torch.zeros(2, c, 7, 9).scatter_(1, labels[:, None], 40.0)
    v, _, g = R.loss_ref(logits, labels, None, R.IGNORE, 1.0, 0.5, mode)
    loss, _, grad = run_loss(logits, labels, None, 1.0, 0.5, mode, 1.0, False)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(loss).all())
    assert float((grad.cpu().double() - g).abs().max()) <= 1e-12 and abs(float(loss) - float(v)) <= 1e-12


# ======================================================================================================================
# bilinear resize
# ======================================================================================================================
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=R.RESIZE_IDS)
def test_bilinear_fwd_bwd(case):
    from iswm_amd import ops
    shape, c = case
    (hi, wi), (ho, wo) = shape
    x, dy = R.resize_inputs(shape, c)
    y = ops.bilinear_fwd(x.to(dev()), ho, wo)
    dx = ops.bilinear_bwd(dy.to(dev()), hi, wi)
    assert tuple(y.shape) == (R.RESIZE_N, ho, wo, c) and tuple(dx.shape) == (R.RESIZE_N, hi, wi, c)
    if (hi, wi) == (ho, wo):                                  # identity: every weight is exactly 1 or 0
        assert same_bits(y, x) and same_bits(dx, dy)
    check("bilinear.fwd", y, R.bilinear_fwd_ref(x, ho, wo))
    check("bilinear.bwd", dx, R.bilinear_bwd_ref(dy, hi, wi))


def test_bilinear_pitched_and_planes_operands():
    from iswm_amd import ops
    shape, c = R.RESIZE_SHAPES[3], 48                                        # (13, 40) -> (65, 7)
    (hi, wi), (ho, wo) = shape
    x, dy = R.resize_inputs(shape, c)
    dense = ops.bilinear_fwd(x.to(dev()), ho, wo)
    out = sliced(torch.zeros(R.RESIZE_N, ho, wo, c), 8, extra=16)
    ops.bilinear_fwd(sliced(x, 4), ho, wo, out=out)                          # pitched input, into a channel slice
    assert same_bits(out, dense) and untouched(out, 8)
    check("bilinear.fwd", out, R.bilinear_fwd_ref(x, ho, wo), "sliced")
    buf = ops.new_planes(R.RESIZE_N, ho, wo, c + 48, dev(), zero=True)       # into a Planes slice
    ops.bilinear_fwd(x.to(dev()), ho, wo, out=buf[..., 32:32 + c])
    full = buf.f32()
    assert same_bits(full[..., 32:32 + c], dense) and not full[..., :32].any() and not full[..., 32 + c:].any()
    dx = ops.bilinear_bwd(sliced(dy, 8), hi, wi)                             # from a pitched dy
    assert same_bits(dx, ops.bilinear_bwd(dy.to(dev()), hi, wi))
    check("bilinear.bwd", dx, R.bilinear_bwd_ref(dy, hi, wi), "pitched dy")


@pytest.mark.parametrize("shape", R.RESIZE_SHAPES, ids=["%dx%d_to_%dx%d" % (s[0] + s[1]) for s in R.RESIZE_SHAPES])
@pytest.mark.parametrize("c,cp", R.RESIZE_NCHW)
def test_bilinear_nchw_variants(c, cp, shape):
    """NHWC low-res (first C of cp channels; the rest hold garbage) -> NCHW, and its backward (channels >= C of dx: zero)"""
    from iswm_amd import ops
    (hi, wi), (ho, wo) = shape
    x, dy = R.resize_inputs(shape, c)
    xh = torch.full((R.RESIZE_N, hi, wi, cp), 9.0)
    xh[..., :c] = x
    xh = sliced(xh, 0, extra=8) if (c, cp) == (5, 8) else xh.to(dev())       # one family reads a pitched low-res tensor
    y = ops.bilinear_to_nchw_fwd(xh, c, ho, wo)
    assert tuple(y.shape) == (R.RESIZE_N, c, ho, wo)
    if (hi, wi) == (ho, wo):
        assert same_bits(y.permute(0, 2, 3, 1), x)
    check("bilinear_nchw.fwd", y.permute(0, 2, 3, 1), R.bilinear_fwd_ref(x, ho, wo))
    dx = ops.bilinear_to_nchw_bwd(dy.permute(0, 3, 1, 2).contiguous().to(dev()), hi, wi, cp)
    assert tuple(dx.shape) == (R.RESIZE_N, hi, wi, cp)
    check("bilinear_nchw.bwd", dx[..., :c], R.bilinear_bwd_ref(dy, hi, wi))
    if cp > c:
        assert not dx[..., c:].any()


# ======================================================================================================================
# depthwise convolution (the general kernels)
# ======================================================================================================================
_dw = functools.lru_cache(maxsize=None)(R.dw_case)


@pytest.mark.parametrize("case", R.DW_CASES, ids=R.DW_IDS)
def test_depthwise_fwd_dgrad_wgrad(case):
    from iswm_amd import ops
    n, h, w, c, cw, kh, kw, s, p, d, has_bias, sl = case
    r = _dw(case)
    view = (lambda t, off: sliced(t, off)) if sl else (lambda t, off: t.to(dev()).contiguous())
    x, dy, wt = view(r["x"], 4), view(r["dy"], 8), r["w"].to(dev())
    bias = r["bias"].to(dev()) if has_bias else None
    g = ops.ConvGeom(x, c, kh, kw, s, p, d)
    assert (g.ho, g.wo) == (r["ho"], r["wo"])
    y = ops.dwconv2d_fwd(x, wt, g, bias, view(torch.full((n, g.ho, g.wo, c), 3.0), 0))
    check("dw.y", y, r["y"])
    dx = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), view(torch.full((n, h, w, c), 3.0), 8))
    check("dw.dx", dx, r["dx"])
    acc = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), view(r["dx0"], 4), True)            # accumulates onto a non-zero dx
    check("dw.dx_acc", acc, r["dx"] + r["dx0"].double())
    dw = ops.dwconv2d_wgrad(x, dy, g, cw)
    assert tuple(dw.shape) == (cw, 1, kh, kw)
    check("dw.dw", dw, r["dw"])
    if cw < c:                                                                            # channels past the weight's: exactly zero
        assert not y[..., cw:].any() and not dx[..., cw:].any()
        assert torch.equal(acc[..., cw:].cpu(), r["dx0"][..., cw:])
    if sl:
        assert untouched(y, 0) and untouched(dx, 8) and untouched(acc, 4)


# ======================================================================================================================
# optimizers
# ======================================================================================================================
@pytest.mark.parametrize("n", R.OPT_N)
@pytest.mark.parametrize("cfg", R.SGD_CONFIGS, ids=lambda c: "mu%g_nesterov%d_wd%g" % (c[0], c[1], c[2]))
def test_sgd_step(cfg, n):
    from iswm_amd import ops
    mu, nesterov, wd = cfg
    p0, grads = R.opt_inputs(n)
    d = dev()
    p, buf, lr = p0.to(d), torch.zeros(n, device=d), torch.tensor([R.SGD_LR], dtype=torch.float32, device=d)
    assert p.data_ptr() % 16 == 0 and buf.data_ptr() % 16 == 0
    for g in grads:
        ops.sgd_step(p, g.to(d), buf, lr, mu, wd, nesterov)
    p_ref, buf_ref = R.sgd_ref(p0, grads, mu, nesterov, wd)
    check("sgd.p", p, p_ref)
    check("sgd.buf", buf, buf_ref)


@pytest.mark.parametrize("n", R.OPT_N)
@pytest.mark.parametrize("cfg", R.ADAM_CONFIGS, ids=lambda c: "%s_wd%g" % ("decoupled" if c[0] else "l2", c[1]))
def test_adam_step(cfg, n):
    from iswm_amd import ops
    decoupled, wd = cfg
    p0, grads = R.opt_inputs(n)
    d = dev()
    p, m, v = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    for t, g in enumerate(grads, 1):
        hyper = torch.tensor(R.adam_hyper(t), dtype=torch.float32, device=d)
        ops.adam_step(p, g.to(d), m, v, hyper, R.ADAM_BETAS[0], R.ADAM_BETAS[1], R.ADAM_EPS, wd, decoupled)
    p_ref, m_ref, v_ref = R.adam_ref(p0, grads, decoupled, wd)
    check("adam.p", p, p_ref)
    check("adam.m", m, m_ref)
    check("adam.v", v, v_ref)


# ======================================================================================================================
# dropout
# ======================================================================================================================
@pytest.mark.parametrize("p", R.DROPOUT_P)
@pytest.mark.parametrize("seed,offset", R.DROPOUT_STREAMS, ids=["s1234_o1", "high_words", "s7_o5"])
def test_dropout_is_the_philox_stream_bit_for_bit(seed, offset, p):
    from iswm_amd import ops
    for n in R.DROPOUT_N:
        g = R.gen(n)
        x, dy = torch.randn(n, generator=g), torch.randn(n, generator=g)
        y, mask = ops.dropout_fwd(x.to(dev()), p, seed, offset)
        keep = R.dropout_mask_ref(n, p, seed, offset)
        assert mask.dtype == torch.uint8 and np.array_equal(mask.cpu().numpy(), keep), (n, "mask differs from Philox4x32-10")
        scale = R.dropout_scale(p)
        y_ref = np.where(keep != 0, x.numpy() * scale, np.float32(0)).astype(np.float32)
        assert np.array_equal(y.cpu().numpy().view(np.uint32), y_ref.view(np.uint32)), (n, "y != x * (1 / (1 - p)) in fp32")
        if p == 0:
            assert keep.all() and same_bits(y, x)
        dx = ops.dropout_bwd(dy.to(dev()), mask, p)
        dx_ref = np.where(keep != 0, dy.numpy() * scale, np.float32(0)).astype(np.float32)
        assert np.array_equal(dx.cpu().numpy().view(np.uint32), dx_ref.view(np.uint32)), n


# ======================================================================================================================
# pooling / broadcast
# ======================================================================================================================
@pytest.mark.parametrize("case", R.POOL_CASES, ids=R.POOL_IDS)
def test_gap_fwd_and_bcast_bwd(case):
    from iswm_amd import ops
    n, hw, c = case
    x = R.pool_inputs(n, hw, c)
    p = ops.gap_fwd(x.to(dev()))
    dv = ops.bcast_bwd(x.to(dev()))
    assert tuple(p.shape) == (n, 1, 1, c) and tuple(dv.shape) == (n, 1, 1, c)
    check("gap.fwd", p, x.double().mean((1, 2), keepdim=True))
    check("bcast.bwd", dv, x.double().sum((1, 2), keepdim=True))


def test_gap_fwd_and_bcast_bwd_pitched_and_planes():
    from iswm_amd import ops
    x = R.pool_inputs(3, (33, 33), 304)
    xd = x.to(dev())
    p, dv = ops.gap_fwd(xd), ops.bcast_bwd(xd)
    xs = sliced(x, 8)
    assert same_bits(ops.gap_fwd(xs), p) and same_bits(ops.bcast_bwd(xs), dv)
    assert same_bits(ops.gap_fwd(ops.split_planes(xd)), p)
    wide = ops.new_planes(3, 33, 33, 320, dev(), zero=True)
    ops.split_planes(xd, out=wide[..., 16:320])
    assert same_bits(ops.gap_fwd(wide[..., 16:320]), p)


@pytest.mark.parametrize("c", R.POOL_C)
@pytest.mark.parametrize("hw", [(1, 7), (33, 33)], ids=["hw7", "hw1089"])
def test_bcast_fwd_and_gap_bwd_into_a_channel_slice(hw, c):
    from iswm_amd import ops
    n = 3
    x = R.pool_inputs(n, hw, c)
    nhw = hw[0] * hw[1]
    v = x[:, :1, :1].contiguous()
    out = sliced(torch.zeros(n, hw[0], hw[1], c), 8)
    ops.bcast_fwd(v.to(dev()), out)
    assert same_bits(out, v.expand(n, hw[0], hw[1], c)) and untouched(out, 8)
    dx = sliced(torch.full((n, hw[0], hw[1], c), 3.0), 4)
    ops.gap_bwd(v.to(dev()), dx, False)
    check("gap.bwd", dx, (v.double() / nhw).expand(n, hw[0], hw[1], c))
    acc = sliced(x, 4)
    ops.gap_bwd(v.to(dev()), acc, True)
    check("gap.bwd_acc", acc, x.double() + v.double() / nhw)
    assert untouched(dx, 4) and untouched(acc, 4)


@pytest.mark.parametrize("h,w,c", R.MAXPOOL_CASES)
def test_maxpool_single_row_column_and_ragged_channels(h, w, c):
    import torch.nn.functional as F
    from iswm_amd import ops
    x = torch.relu(torch.randn(2, c, h, w, generator=R.gen(h * w)))          # post-ReLU: many exact ties at 0
    x64 = x.double().requires_grad_(True)
    y_ref = F.max_pool2d(x64, 3, 2, 1)
    dy = torch.randn(y_ref.shape, generator=R.gen(c))
    y_ref.backward(dy.double())
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev())
    y, idx = ops.maxpool_fwd(xh)
    assert torch.equal(y.cpu().permute(0, 3, 1, 2).double(), y_ref.detach())
    dx = ops.maxpool_bwd(dy.permute(0, 2, 3, 1).contiguous().to(dev()), idx, tuple(xh.shape))
    check("maxpool.dx", dx.permute(0, 3, 1, 2), x64.grad)


# ======================================================================================================================
# layout changes, copies, argmax: bit-exact
# ======================================================================================================================
@pytest.mark.parametrize("c", [1, 5, 21])
def test_nchw_nhwc_layout_changes(c):
    from iswm_amd import ops
    x = torch.randn(2, c, 7, 9, generator=R.gen(c))
    cp = (c + 3) // 4 * 4
    xh = ops.nchw_to_nhwc(x.to(dev()))
    assert tuple(xh.shape) == (2, 7, 9, cp) and same_bits(xh[..., :c], x.permute(0, 2, 3, 1)) and not xh[..., c:].any()
    wide = ops.nchw_to_nhwc(x.to(dev()), cp + 8)
    assert same_bits(wide[..., :c], x.permute(0, 2, 3, 1)) and not wide[..., c:].any()
    src = sliced(x.permute(0, 2, 3, 1).contiguous(), 4)                      # back from a pitched slice
    assert same_bits(ops.nhwc_to_nchw(src), x)
    assert same_bits(ops.nhwc_to_nchw(src, max(c - 1, 1)), x[:, :max(c - 1, 1)])


def test_copy_channels_two_column_blocks_both_pitched():
    from iswm_amd import ops
    x = torch.randn(2, 5, 3, 1280, generator=R.gen(1280))
    src, dst = sliced(x, 8, extra=16), sliced(torch.zeros(2, 5, 3, 1280), 12, extra=24)
    ops.copy_channels(src, dst)
    assert same_bits(dst, x) and untouched(dst, 12)


@pytest.mark.parametrize("n", [3, 4, 4099])
def test_add_inplace_with_tail(n):
    from iswm_amd import ops
    g = R.gen(n)
    a, b = torch.randn(n, generator=g), torch.randn(n, generator=g)
    out = ops.add_inplace(a.to(dev()), b.to(dev()))
    assert same_bits(out, a + b)


@pytest.mark.parametrize("c", [1, 21])
def test_argmax_ties_and_minus_infinity(c):
    from iswm_amd import ops
    lg = torch.randn(2, c, 13, 11, generator=R.gen(c))
    if c > 1:
        lg[:, 3] = lg[:, 1]                                   # exact ties: the lowest index wins
        lg[:, 5] = float("-inf")                              # a -inf channel never wins ...
        lg[0, :, 0, :4] = float("-inf")                       # ... unless every channel is -inf: index 0
        lg[1, 0, 2, :] = float("-inf")                        # -inf in channel 0, the running maximum's start
    out = ops.argmax_nchw(lg.to(dev()))
    assert out.dtype == torch.int64 and torch.equal(out.cpu(), lg.max(1)[1])
    if c > 1:
        assert not bool((out == 5).any()) and not bool((out == 3).any())


# ======================================================================================================================
# BatchNorm, plain passes, at means far from zero
# ======================================================================================================================
def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().to(dev())


def nchw(t):
    return t.detach().cpu().permute(0, 3, 1, 2)


def pattern_differs_only_at_ties(mask, fwd, relu, key):
    """the kernel's activation pattern may differ from the float64 one only where the pre-activation is within the output bound
    of 0 (or of 6)"""
    z = fwd["z"]
    edge = torch.minimum(z.abs(), (z - 6).abs()) if (relu == 6 and relu is not True) else z.abs()
    diff = mask != R.bn_act_mask(fwd["out"], relu)
    return (not bool(diff.any())) or float(edge[diff].max()) <= 4 * R.FLOOR[key] * float(fwd["out"].abs().max())


def bn_statistics(x, gamma, beta):
    """colstat + bn_finalize at momentum 1 (the running buffers become the batch statistics) -> (coef, mean, unbiased variance)"""
    from iswm_amd import ops
    n, c, h, w = x.shape
    d = dev()
    partials, tiles, tile_rows = ops.colstat(nhwc(x))
    rm, rv = torch.zeros(c, device=d), torch.ones(c, device=d)
    coef = ops.bn_finalize(partials, tiles, n * h * w, tile_rows, gamma.to(d), beta.to(d), rm, rv, 1.0, R.BN_EPS)
    return coef, rm, rv


@pytest.mark.parametrize("shape", R.BN_SHAPES, ids=lambda s: "c%d" % s[1])
@pytest.mark.parametrize("stats", R.BN_STATS, ids=lambda s: "mean%g_std%g" % s)
def test_batchnorm_large_mean_batch_statistics(stats, shape):
    """colstat + bn_finalize where |mean| is 2000 - 3000 standard deviations.  A one-pass sum of squares is off by 0.6 - 3 here
    (test_streaming_ref_cpu.test_naive_variance_misses_the_bound_by_100x); the centred tile statistics are not.

    SCOPE: this pins the column-pass producer (ops.colstat = iswm_colstat_res, which serves depthwise filters other than 3 x 3
    and biased convolutions in front of a BatchNorm).  Its third plane R_t makes bn_finalize's merge exact.  Before it the
    variance was 1.3e-5 .. 3.3e-5 off here (bound 3e-7): the fp32 tile sum S_t puts the tile mean off by ulp(S_t) / n_t, and the
    merge M2 = sum M2_t + n_t (S_t / n_t - mean)^2 loses the cross term, ~2^-23 |mean| / sigma of the variance.  The OTHER producers
    of tile statistics -- the convolution epilogues and dwconv3.hip, which feed almost every BatchNorm of the models -- still
    publish the pair {S_t, M2_t} and still carry that error at such means.  tests/test_bn_partials_gpu.py pins them: every tile
    of every producer against float64 of the stored output at 4 x the fp32 floor, also at |mean| / sigma in the tens to
    hundreds, and the loss of their pair merge as an identity (the rounding of S_t is ALL of it).
    test_colstat_residual_plane_leaves_the_pair_alone shows the pair alone at this input."""
    x, gamma, beta, _, _ = R.bn_inputs(stats, shape, False)
    f = R.bn_fwd_ref(x, gamma, beta, None, False)
    coef, rm, rv = bn_statistics(x, gamma, beta)
    tag = ".mean%g" % stats[0]
    check("bn.mean" + tag, rm, f["mean"], "running")
    check("bn.mean" + tag, coef[2], f["mean"], "saved")
    check("bn.var" + tag, rv, f["var_unbiased"])


def test_colstat_residual_plane_leaves_the_pair_alone():
    """iswm_colstat_res (what ops.colstat runs) adds the plane R_t = sum (x - mu_t); {S_t, M2_t} keep the bits of iswm_colstat,
    R_t is that sum (|R_t| <= n_t ulp(mean): the rounding of the fp32 centre), and iswm_bn_finalize on the pair alone still gives
    what it gave (the convolution epilogues' and dwconv3's layout has no third plane, so at |mean| = 2000 sigma their variance
    keeps the ~3e-5 error the third plane removes: printed here, not asserted.  The mean of the pair is held to 1e-5, the bound
    of test_hip_kernels.test_batchnorm_train_fwd_bwd for that entry point -- outside the 4 x floor rule on purpose: this line
    only shows that the pair-only entry point is unchanged, its accuracy is that older test's business)"""
    import ctypes
    from iswm_amd import ops
    x, gamma, beta, _, _ = R.bn_inputs(R.BN_STATS[0], R.BN_SHAPES[1], False)
    xh = nhwc(x)
    m, c = xh.shape[0] * xh.shape[1] * xh.shape[2], xh.shape[3]
    p3, tiles, tile_rows = ops.colstat(xh)
    assert tuple(p3.shape) == (3, tiles, c)
    p2 = torch.empty((2, tiles, c), device=dev())
    ops.call("iswm_colstat", ctypes.c_void_p(xh.data_ptr()), m, c, c, ctypes.c_void_p(p2.data_ptr()), ops._stream())
    assert same_bits(p3[:2], p2)
    rows = xh.reshape(m, c).cpu()
    for t in (0, tiles - 1):
        tile = rows[t * tile_rows:(t + 1) * tile_rows]
        mu = p2[0, t].cpu() / np.float32(tile.shape[0])                          # the fp32 centre, as the kernel forms it
        dev64 = tile.double() - mu.double()                                      # each difference is exact in fp32
        slack = tile.shape[0] * 2.0 ** -24 * dev64.abs().sum(0)                  # worst case of an fp32 sum of n_t terms
        assert bool(((p3[2, t].cpu().double() - dev64.sum(0)).abs() <= slack).all())
    f = R.bn_fwd_ref(x, gamma, beta, None, False)
    coef2 = ops.bn_finalize(p2, tiles, m, tile_rows, None, None, None, None, 0.1)
    print("pair alone: variance rel err %.2e" % rel_err(1.0 / coef2[3].double().cpu() ** 2 - R.BN_EPS, f["var"]))
    assert rel_err(coef2[2], f["mean"]) <= 1e-5


@pytest.mark.parametrize("case", R.BN_CASES, ids=R.BN_IDS)
def test_batchnorm_train_large_mean(case):
    """bn_apply and bn_backward on the kernels' own statistics where |mean| is 2000 - 3000 standard deviations:
    (y - mean) * scale + beta survives this.

    The statistics come from ops.colstat (see the scope note of test_batchnorm_large_mean_batch_statistics); with the pair-only
    merge dy, which is proportional to 1 / sqrt(var), was 8.7e-6 .. 1.5e-5 off and missed its bound in 5 of these 12 cases."""
    from iswm_amd import ops
    stats, shape, (relu, res) = case
    n, c, h, w = shape
    tag = ".mean%g" % stats[0]
    x, gamma, beta, resid, dout = R.bn_inputs(stats, shape, res)
    f = R.bn_fwd_ref(x, gamma, beta, resid, relu)
    d = dev()
    yh, gd = nhwc(x), gamma.to(d)
    coef, _, _ = bn_statistics(x, gamma, beta)
    o = ops.bn_apply(yh, coef, relu, nhwc(resid) if res else None)
    check("bn.out" + tag, nchw(o), f["out"])
    mask = R.bn_act_mask(nchw(o), relu)
    assert pattern_differs_only_at_ties(mask, f, relu, "bn.out" + tag)
    dy_ref, dg_ref, db_ref, dres_ref = R.bn_bwd_ref(f, gamma, dout, mask, True)
    dg, db = torch.empty(c, device=d), torch.empty(c, device=d)
    dy, dres = ops.bn_backward(nhwc(dout), o, yh, coef, gd, relu, True, dg, db, want_dres=res)
    check("bn.dgamma" + tag, dg, dg_ref)
    check("bn.dbeta" + tag, db, db_ref)
    if res:
        assert torch.equal(nchw(dres).double(), dres_ref)
    check("bn.dy" + tag, nchw(dy), dy_ref)


def test_batchnorm_eval_backward():
    """training=False at ordinary statistics: dy = gamma invstd dz on the running statistics, no batch terms"""
    from iswm_amd import ops
    x, gamma, beta, _, dout = R.bn_inputs((0.5, 2.0), R.BN_SHAPES[1], False)
    c = 64
    mean, var = torch.randn(c, generator=R.gen(3)) * 0.1 + 0.5, torch.rand(c, generator=R.gen(4)) + 3.5
    f = R.bn_fwd_ref(x, gamma, beta, None, True, mean, var)
    d = dev()
    gd = gamma.to(d)
    coef = ops.bn_eval_coeffs(gd, beta.to(d), mean.to(d), var.to(d), R.BN_EPS)
    yh = nhwc(x)
    o = ops.bn_apply(yh, coef, True)
    check("bn_eval.out", nchw(o), f["out"])
    mask = nchw(o) > 0
    assert pattern_differs_only_at_ties(mask, f, True, "bn_eval.out")
    dy_ref, dg_ref, db_ref, _ = R.bn_bwd_ref(f, gamma, dout, mask, False)
    dg, db = torch.empty(c, device=d), torch.empty(c, device=d)
    dy, _ = ops.bn_backward(nhwc(dout), o, yh, coef, gd, True, False, dg, db)
    check("bn_eval.dy", nchw(dy), dy_ref)
    check("bn_eval.dgamma", dg, dg_ref)
    check("bn_eval.dbeta", db, db_ref)


# ======================================================================================================================
# BatchNorm, second table (streaming_ref "bn2"): the row / column structure of the passes, the planes forms, one-plane mode
# ======================================================================================================================
@pytest.fixture
def conv_math(request):
    """conv math 1 (bf16x6: activations held as three exact bf16 planes) or 2 ("bf16": one plane, rounded to nearest even)"""
    from iswm_amd import _lib
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    lib.iswm_set_conv_math(request.param)
    yield request.param
    lib.iswm_set_conv_math(old)


BOTH_MATHS = pytest.mark.parametrize("conv_math", [1, 2], ids=["planes3", "plane1"], indirect=True)


def relu_code(relu):
    return 6 if (relu == 6 and relu is not True) else int(bool(relu))


def fp32_buf(shape):
    return torch.full(tuple(shape), R.SENTINEL, device=dev())


def planes_view(shape, width=None, off=0):
    """(view, buffer): a Planes view of channels [off, off + C) of a buffer `width` channels wide that holds SENTINEL in every
    plane"""
    from iswm_amd import ops
    n, h, w, c = shape
    buf = ops.new_planes(n, h, w, width or c, dev())
    buf.t.fill_(R.SENTINEL)
    return (buf if (width or c) == c else buf[..., off:off + c]), buf


def rest_untouched(buf, off, c):
    """the channels of the buffer outside [off, off + c) keep the sentinel in every plane"""
    return bool((buf.t[..., :off] == R.SENTINEL).all()) and bool((buf.t[..., off + c:] == R.SENTINEL).all())


def as_planes(t, width=None, off=0):
    from iswm_amd import ops
    view, _ = planes_view(tuple(t.shape), width, off)
    return ops.split_planes(t, out=view)


def bf16_bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def one_plane_is_rne(p, fp32_form):
    """the single plane holds torch's round-to-nearest-even bfloat16 of the fp32-format result, bit for bit"""
    return p.t.shape[0] == 1 and torch.equal(bf16_bits(p.t[0]), bf16_bits(fp32_form.detach().cpu().to(torch.bfloat16)))


def stored_equal(p, fp32_form):
    """a Planes result of data movement: three planes join to the fp32 form's bits, one plane is its rounding"""
    return same_bits(p.f32(), fp32_form) if p.t.shape[0] == 3 else one_plane_is_rne(p, fp32_form)


class Bn2:
    """the inputs of one bn2 case on both sides: NCHW on the CPU for the restatement, NHWC on the GPU for the kernels.  With
    (mean, invstd) the statistics are given (eval-mode coefficients), without they are the batch's, from colstat + bn_finalize"""

    def __init__(self, x, gamma, beta, resid, dout, mean=None, invstd=None):
        self.x, self.gamma, self.beta, self.resid, self.dout, self.mean, self.invstd = x, gamma, beta, resid, dout, mean, invstd
        self.var = None if mean is None else R.given_var(invstd)
        self.yh, self.rh, self.dh, self.gd = nhwc(x), nhwc(resid), nhwc(dout), gamma.to(dev())
        self.shape = tuple(self.yh.shape)
        self._coef, self._fwd = None, {}

    def coef(self):
        if self._coef is None:
            self._coef = (bn_statistics(self.x, self.gamma, self.beta)[0] if self.mean is None else
                          R.bn_coef(self.gamma, self.beta, self.mean, self.invstd).to(dev()))
        return self._coef

    def fwd(self, relu, res):
        """the float64 forward; res: None, "exact", or "bf16" (the residual as one plane holds it: a one-plane READ is exact, so
        the restatement is fed the rounded tensor).  Kept only for the small cases."""
        k = (relu_code(relu), res)
        if k in self._fwd:
            return self._fwd[k]
        resid = None if res is None else (R.bf16_rne(self.resid) if res == "bf16" else self.resid)
        f = R.bn_fwd_ref(self.x, self.gamma, self.beta, resid, relu, self.mean, self.var)
        if self.x.numel() < (1 << 20):
            self._fwd[k] = f
        return f


# the seeded CPU inputs are built once; a Bn2 (its GPU tensors, its float64 results) lives for one test only
_bn2_batch_inputs = functools.lru_cache(maxsize=None)(R.bn2_batch_inputs)
_bn2_given_inputs = functools.lru_cache(maxsize=None)(R.bn2_given_inputs)


def bn2_batch_case(cid):
    return Bn2(*_bn2_batch_inputs(cid))


def bn2_given_case(shape, identity=0):
    return Bn2(*_bn2_given_inputs(shape, identity))


def bn2_forward(case, tag, relu, res=None, out="f32", what="", worst=None):
    """bn_apply into an fp32 tensor and, with out = ("planes", [buffer channels, offset]), into a Planes tensor or channel slice;
    res: None, "f32" or ("planes", [buffer channels, offset]).  The fp32 form goes to float64; three planes go to float64 as
    well, one plane must be the rounding of the fp32 form.  Returns (float64 forward, fp32 output, Planes output or None)"""
    from iswm_amd import ops
    one = ops.nplanes() == 1
    rop, kind = None, None
    if res == "f32":
        rop, kind = case.rh, "exact"
    elif res is not None:
        rop, kind = as_planes(case.rh, *res[1:]), ("bf16" if one else "exact")
    f = case.fwd(relu, kind)
    key, c = "bn2.out." + tag, case.shape[3]
    o32 = ops.bn_apply(case.yh, case.coef(), relu, rop, out=fp32_buf(case.shape))
    check(key, nchw(o32), f["out"], what + " fp32 out", worst)
    op = None
    if out != "f32":
        op, buf = planes_view(case.shape, *out[1:])
        ops.bn_apply(case.yh, case.coef(), relu, rop, out=op)
        assert rest_untouched(buf, out[2] if len(out) > 2 else 0, c), what
        if one:
            assert one_plane_is_rne(op, o32), what
        else:
            check(key, nchw(op.f32()), f["out"], what + " planes out", worst)
    return f, o32, op


def bn2_backward(case, tag, f, relu, saved, training, want_dres, dy_planes, what="", worst=None, stats=None):
    """bn_backward on the saved output `saved` (fp32 or Planes), dy as fp32 and, with dy_planes, as Planes too.  The pattern is the
    kernel's own: that of the saved output as handed over (one plane: of the STORED, rounded value), which may differ from the
    float64 one only at ties -- except for a one-plane saved output, whose rounding moves the pattern by design and whose bits
    bn2_forward has tied to the fp32 form"""
    from iswm_amd import ops
    one = ops.nplanes() == 1
    c = case.shape[3]
    recomputed = relu_code(relu) == 1 and not want_dres
    if recomputed:
        # the contract of ops.bn_backward: want_dres says whether the stage had a residual.  ReLU without it never reads the saved
        # output: the pattern is recomputed from y as (y - mean) * scale + beta > 0 -- for a stage that did add a residual that is
        # the pattern of the forward WITHOUT it, and that is what is held here (the models ask for dres whenever they add one)
        src, ftie = ops.bn_apply(case.yh, case.coef(), True, out=fp32_buf(case.shape)), case.fwd(True, None)
    else:
        src, ftie = (saved.f32() if ops.is_planes(saved) else saved), f
    mask = R.bn_act_mask(nchw(src), relu)
    if recomputed or not (one and ops.is_planes(saved)):
        assert pattern_differs_only_at_ties(mask, ftie, relu, "bn2.out." + tag), what
    dy_ref, dg_ref, db_ref, dres_ref = R.bn_bwd_ref(f, case.gamma, case.dout, mask, training)
    kdy = "bn2.%s.%s" % ("dy" if training else "dy_eval", tag)

    def run(dy_buf):
        dg, db = fp32_buf((c,)), fp32_buf((c,))
        dy, dres = ops.bn_backward(case.dh, saved if relu else None, case.yh, case.coef(), case.gd, relu, training, dg, db,
                                   want_dres=want_dres, dy=dy_buf, stats=stats)
        if want_dres:
            assert torch.equal(nchw(dres).double(), dres_ref), what + ": dres is not dout under the pattern"
        return dy, dg, db

    dy, dg, db = run(fp32_buf(case.shape))
    check("bn2.dgamma." + tag, dg, dg_ref, what, worst)
    check("bn2.dbeta." + tag, db, db_ref, what, worst)
    check(kdy, nchw(dy), dy_ref, what + " fp32 dy", worst)
    if dy_planes:
        view, _ = planes_view(case.shape)
        dyp, dgp, dbp = run(view)
        assert same_bits(dgp, dg) and same_bits(dbp, db), what
        if one:
            assert one_plane_is_rne(dyp, dy), what
        else:
            check(kdy, nchw(dyp.f32()), dy_ref, what + " planes dy", worst)


BN2_BATCH_RUNS = [(cid, 1) for cid in R.BN2_BATCH] + [("cols2_pl", 2)]


@pytest.mark.parametrize("cid,conv_math", BN2_BATCH_RUNS, ids=["%s_math%d" % r for r in BN2_BATCH_RUNS], indirect=["conv_math"])
def test_bn2_rows_and_columns(cid, conv_math):
    """bn_apply and bn_backward on the kernels' own batch statistics at the row and channel counts where the passes change shape
    (what each case reaches: BN2_CLAIMS of tests/test_streaming_ref_cpu.py, asserted there from the restated plan): both sides of
    the reduce pass's `M <= 8192` (above it with the recomputed ReLU pattern and with no activation + residual: the reduce and
    apply kernels' RELU == 0 forms), a thread with two fp32 runs of 8 rows (the second ragged), the 1024-tile cap with the finalize
    at 259 and 1024 tiles, a ragged second column block in the 4-channel kernels and in k_bn_apply8"""
    (n, h, w), c, (relu, res), planes = R.BN2_BATCH[cid]
    case = bn2_batch_case(cid)
    fmt = ("planes",) if planes else "f32"
    f, o32, op = bn2_forward(case, cid, relu, res=fmt if res else None, out=fmt, what=cid)
    for saved in (o32, op)[:2 if planes else 1]:
        bn2_backward(case, cid, f, relu, saved, True, res, planes, "%s saved %s" % (cid, "planes" if saved is op else "fp32"))


@pytest.mark.parametrize("conv_math", [1], ids=["planes3"], indirect=True)
@pytest.mark.parametrize("cid", ["runs", "tilecap"])
def test_bn2_backward_on_ready_partials(cid, conv_math):
    """ops.bn_backward(stats=...) -- iswm_bn_backward_stats_pl: finalize + apply on partials [2][tiles][C] that a producer wrote --
    with the partials the reduce pass of iswm_bn_backward_pl leaves in its workspace for the same inputs, tiles ==
    iswm_colstat_tiles(M): k_bn_bwd_finalize<double, 4> at 259 and at 1024 tiles on ready partials"""
    import ctypes
    from iswm_amd import _lib, ops
    lib = _lib.load()
    (n, h, w), c, (relu, res), planes = R.BN2_BATCH[cid]
    case = bn2_batch_case(cid)
    f, o32, _ = bn2_forward(case, cid, relu, res="f32", what=cid)
    m, tiles = n * h * w, lib.iswm_colstat_tiles(n * h * w)
    need = lib.iswm_bn_bwd_workspace(m, c)
    assert need == (2 * tiles * c + 2 * c) * 8
    ws = torch.zeros(need // 8, dtype=torch.float64, device=dev())
    coef, p = case.coef(), ops._p
    dg, db, dy, dres = fp32_buf((c,)), fp32_buf((c,)), fp32_buf(case.shape), fp32_buf(case.shape)
    ops.call("iswm_bn_backward_pl", p(case.dh), c, p(o32), c, 0, p(case.yh), c, m, c, p(coef[2]), p(coef[3]), p(case.gd), None, None,
             relu_code(relu), 1, p(dg), p(db), p(dy), c, 0, p(dres), c, p(ws), need, ops._stream())
    st = ops.BnStats(case.yh, coef, relu)
    st.partials, st.tiles = ws[:2 * tiles * c].clone(), tiles
    bn2_backward(case, cid, f, relu, o32, True, True, planes, cid + " ready partials", stats=st)


BN2_WALK_RUNS = [(wid, 1) for wid in R.BN2_WALK] + [("walk33", 2)]


@pytest.mark.parametrize("wid,conv_math", BN2_WALK_RUNS, ids=["%s_math%d" % r for r in BN2_WALK_RUNS], indirect=["conv_math"])
def test_bn2_apply8_pair_walk(wid, conv_math):
    """k_bn_apply8 at 64 channels (32 row lanes) with 7, 33 and 100 rows: threads with no row or the tail row only, with the tail
    row only or one pair, with a pair and the tail row or two pairs; ReLU, a Planes residual through ld8x, given statistics, the
    backward in training and in eval form on the fp32 and on the Planes saved output"""
    case = bn2_given_case((1, R.BN2_WALK_C, 1, R.BN2_WALK[wid]))
    f, o32, op = bn2_forward(case, wid, True, res=("planes",), out=("planes",), what=wid)
    for training in (True, False):
        for saved in (o32, op):
            bn2_backward(case, wid, f, True, saved, training, True, True,
                         "%s training %d saved %s" % (wid, training, "planes" if saved is op else "fp32"))


@BOTH_MATHS
@pytest.mark.parametrize("fid", list(R.BN2_FALLBACK))
def test_bn2_four_channel_kernel_on_planes(fid, conv_math):
    """bn_apply with a Planes output where the dispatch of iswm_bn_apply_pl must take the 4-channel kernel (8-byte plane loads and
    stores): C % 8 == 4, an output slice that is not 16-byte aligned, a pitch of 76, a residual of pitch 76 or misaligned -- and
    "off8", the aligned slice of the same buffer, which takes the 8-channel kernel.  The expected form of each case is in
    streaming_ref.BN2_FALLBACK and is asserted from the restated condition on the CPU (test_bn2_fallback_forms)"""
    c, (ow, oo), (rw, ro), form = R.BN2_FALLBACK[fid]
    n, h, w = R.BN2_FALLBACK_ROWS
    case = bn2_given_case((n, c, h, w))
    what = "%s (%d-channel kernel)" % (fid, form)
    tag = R.fallback_tag(fid)
    f, o32, op = bn2_forward(case, tag, True, res=("planes", rw, ro), out=("planes", ow, oo), what=what)
    for training in (True, False):
        bn2_backward(case, tag, f, True, op, training, True, True, "%s training %d" % (what, training))


BN2_GRID_RES = {"none": None, "f32": "f32", "planes": ("planes",), "slice": ("planes", 96, 16)}


@BOTH_MATHS
@pytest.mark.parametrize("res", list(BN2_GRID_RES))
@pytest.mark.parametrize("relu", R.BN2_RELUS, ids=["none", "relu", "relu6"])
def test_bn2_activation_residual_format_grid(relu, res, conv_math):
    """every combination the dispatch macros of bn.hip instantiate, at 3 x 9 x 11 x 72: activation x residual (none, fp32, Planes,
    a Planes slice of a 96-channel buffer) x output (fp32, Planes, a Planes slice of a 128-channel buffer); the backward with the
    saved output as fp32 and as Planes (the pattern through ld4x_hi), dy as fp32 and as Planes, with and without dres, in training
    and in eval form.  Channels 0..7 are the identity and carry streaming_ref.BF16_EDGE: bf16 ties of both parities, values in the
    bf16 ulp below 6 and just above 0.

    Convention of the one-plane mode (conv math "bf16"): a stored activation IS its rounding to nearest even, and the ReLU6 pattern
    is that of the stored value -- an output of 5.99 is stored as 6.0 and passes no gradient.  The restatement takes its pattern
    from the joined output, so both agree; the three-plane mode reads the pattern from the hi plane, whose truncation decides
    0 < x < 6 as the fp32 value does."""
    from iswm_amd import ops
    case = bn2_given_case(R.BN2_GRID_SHAPE, 8)
    worst, tag = {}, R.grid_tag(relu, BN2_GRID_RES[res])
    for out in (("planes",), ("planes", 128, 40)):
        what = "relu %d res %s out %s" % (relu_code(relu), res, "slice" if len(out) > 1 else "planes")
        f, o32, op = bn2_forward(case, tag, relu, BN2_GRID_RES[res], out, what, worst)
    if relu_code(relu) == 6:
        rounded_up = (op.f32() == 6) & (o32 < 6)
        assert bool(rounded_up.any()) == (conv_math == 2)              # the case the convention is about is in the data
    for saved in (o32, op):
        for training in (True, False):
            for want_dres in (False, True):
                bn2_backward(case, tag, f, relu, saved, training, want_dres, True, "%s saved %s training %d dres %d" % (
                    what, "planes" if saved is op else "fp32", training, want_dres), worst)
    report_worst(worst, "relu %d res %s math %d" % (relu_code(relu), res, conv_math))


@BOTH_MATHS
def test_split_join_ties_and_second_grid_trip(conv_math):
    """split_planes then f32(): the identity under bf16x6, torch's .to(bfloat16).float() under conv math "bf16" -- on bf16 ties of
    both parities and on the 33 124 x 256 tensor of `tilecap`, whose 2.1 M float4 groups take the grid-stride loop of both kernels
    (2048 blocks x 256 threads) round more than once"""
    from iswm_amd import ops
    edge = torch.tensor(R.BF16_EDGE + [-v for v in R.BF16_EDGE] + [65504.0, -3e38, 1.0, -1.0]).view(1, 1, 5, 8)
    big = bn2_batch_case("tilecap").yh
    assert big.numel() // 4 > 2048 * 256
    for x in (edge.to(dev()), big):
        p = ops.split_planes(x)
        assert p.t.shape[0] == (3 if conv_math == 1 else 1)
        if conv_math == 1:                  # the identity of tests/test_planes.py: equal as values (the join of -0.0 is +0.0)
            assert torch.equal(p.f32().cpu(), x.cpu())
        else:
            want = x.cpu().to(torch.bfloat16).float()
            assert same_bits(p.f32(), want)
            assert one_plane_is_rne(p, x)
            assert not torch.equal(want, R.bf16_trunc(x.cpu()))        # truncation would differ


# ======================================================================================================================
# pooling, broadcast and resize into Planes, in both plane counts
# ======================================================================================================================
@BOTH_MATHS
@pytest.mark.parametrize("h,w,c", R.MAXPOOL_CASES)
def test_maxpool_into_planes(h, w, c, conv_math):
    """maxpool_fwd(planes=True): values and indices equal to the fp32 form's and to ATen's (tap kh * 3 + kw -> ATen's flat input
    index); the stored planes are the fp32 values (three planes) or their rounding (one plane)"""
    import torch.nn.functional as F
    from iswm_amd import ops
    x = torch.relu(torch.randn(2, c, h, w, generator=R.gen(h * w)))
    x.view(-1)[:len(R.BF16_EDGE)] = torch.tensor(R.BF16_EDGE)
    y_ref, i_ref = F.max_pool2d(x.double(), 3, 2, 1, return_indices=True)
    xh = x.permute(0, 2, 3, 1).contiguous().to(dev())
    y_f, i_f = ops.maxpool_fwd(xh)
    y_p, i_p = ops.maxpool_fwd(xh, planes=True)
    assert torch.equal(nchw(y_f).double(), y_ref) and torch.equal(i_f, i_p) and stored_equal(y_p, y_f)
    ho, wo = y_ref.shape[2:]
    tap = nchw(i_f).long()
    flat = (torch.arange(ho)[:, None] * 2 - 1 + tap // 3) * w + (torch.arange(wo)[None, :] * 2 - 1 + tap % 3)
    assert torch.equal(flat, i_ref)


@BOTH_MATHS
@pytest.mark.parametrize("c", [48, 304])
@pytest.mark.parametrize("hw", [(1, 7), (33, 33)], ids=["hw7", "hw1089"])
def test_gap_fwd_from_planes(hw, c, conv_math):
    """gap_fwd through ld4x from a Planes tensor and from a pitched Planes slice: the four-rows-in-flight loop and its tail.  One
    plane: the read is exact, so the restatement is the mean of the rounded tensor"""
    from iswm_amd import ops
    x = R.pool_inputs(3, hw, c)
    held = x if conv_math == 1 else R.bf16_rne(x)
    want = held.double().mean((1, 2), keepdim=True)
    xd = x.to(dev())
    check("gap.fwd", ops.gap_fwd(ops.split_planes(xd)), want, "planes")
    check("gap.fwd", ops.gap_fwd(as_planes(xd, c + 16, 8)), want, "planes slice, pitch %d" % (c + 16))


@BOTH_MATHS
@pytest.mark.parametrize("hw", [(1, 1), (1, 7), (33, 33)], ids=["hw1", "hw7", "hw1089"])
def test_bcast_fwd_into_a_planes_slice(hw, conv_math):
    from iswm_amd import ops
    n, c = 3, 48
    v = R.pool_inputs(n, (1, 1), c)
    v.view(-1)[:len(R.BF16_EDGE)] = torch.tensor(R.BF16_EDGE)
    view, buf = planes_view((n, hw[0], hw[1], c), c + 24, 8)
    ops.bcast_fwd(v.to(dev()), view)
    assert stored_equal(view, v.expand(n, hw[0], hw[1], c).contiguous()) and rest_untouched(buf, 8, c)


@BOTH_MATHS
@pytest.mark.parametrize("shape", R.RESIZE_SMALLEST + [R.RESIZE_SHAPES[1]], ids=lambda s: "%dx%d_to_%dx%d" % (s[0] + s[1]))
def test_bilinear_fwd_into_a_planes_slice(shape, conv_math):
    from iswm_amd import ops
    c = 48
    (hi, wi), (ho, wo) = shape
    x, _ = R.resize_inputs(shape, c)
    ref = R.bilinear_fwd_ref(x, ho, wo)
    dense = ops.bilinear_fwd(x.to(dev()), ho, wo)
    check("bilinear.fwd", dense, ref, "fp32 form")
    view, buf = planes_view((R.RESIZE_N, ho, wo, c), c + 48, 32)
    ops.bilinear_fwd(x.to(dev()), ho, wo, out=view)
    assert rest_untouched(buf, 32, c)
    if conv_math == 2:
        assert one_plane_is_rne(view, dense)
    else:
        check("bilinear.fwd", view.f32(), ref, "planes slice")
