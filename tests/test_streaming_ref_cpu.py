"""tests/streaming_ref.py against independent authorities, on the CPU (no GPU, runs anywhere) -- so that the GPU tests of
tests/test_streaming_kernels_gpu.py do not check a kernel against its author's second opinion -- and the fp32 floors.

Authorities: F.cross_entropy and autograd through the float64 focal expression; F.interpolate and its autograd; torch.optim;
the Random123 known-answer vectors of Philox4x32-10; F.batch_norm and its autograd.  (The depthwise restatement IS
F.conv2d(groups) in float64; it is tied to a direct tap loop here.)

Floors: for every float comparison of the GPU tests, torch's own fp32 implementation of the operation is compared with the
float64 restatement on the same inputs (single-threaded, so the figures do not depend on the machine's core count); the
largest figure over a check's cases must lie in [FLOOR / 2, 1.25 FLOOR] of the recorded streaming_ref.FLOOR entry, so the
table can neither rot nor be inflated.  `pytest -s` prints the measured figures.

For the second BatchNorm table (streaming_ref "bn2") this file also asserts, from plan_rows and the dispatch thresholds of bn.hip
restated in Python and the library's own tile count and workspace size, which path every case reaches (rows and fp32 runs per
thread, column blocks, groups in the last block, 4- or 8-channel apply kernel), and shows on the restatement alone that the
faults those cases are there for -- a row, a run, a column block, a tile slot, a plane or a pattern lost -- miss the GPU
assertions by at least 3 x the bound."""
import contextlib
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import streaming_ref as R
from tests.util import rel_err


@contextlib.contextmanager
def one_thread():
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        yield
    finally:
        torch.set_num_threads(old)


def check_floors(measured):
    for k, v in sorted(measured.items()):
        print("floor %-28s measured %.3e  recorded %.3e" % (k, v, R.FLOOR.get(k, float("nan"))))
    for k, v in measured.items():
        assert k in R.FLOOR, "no recorded floor for %s (measured %.3e)" % (k, v)
        assert R.FLOOR[k] / 2 <= v <= 1.25 * R.FLOOR[k], "%s: measured %.3e, recorded %.3e" % (k, v, R.FLOOR[k])


def put(d, k, v):
    d[k] = max(d.get(k, 0.0), v)


# ---- loss ------------------------------------------------------------------------------------------------------------
def focal_autograd(logits64, labels, weight, alpha, gamma, mode):
    """the reference's FocalLoss expression in float64 with autograd: ce = F.cross_entropy(reduction='none'), pt = exp(-ce)"""
    z = logits64.clone().requires_grad_(True)
    ce = F.cross_entropy(z, labels.long(), weight=None if weight is None else weight.double(), ignore_index=R.IGNORE,
                         reduction="none")
    f = alpha * (1 - torch.exp(-ce)) ** gamma * ce
    v = f.mean() if mode == 1 else f.sum()
    v.backward()
    return v.detach(), z.grad


@pytest.mark.parametrize("c,kind,weighted", [(2, "u8", True), (5, "i64", False), (21, "i64", True), (9, "u8", False)])
def test_loss_mode0_is_cross_entropy(c, kind, weighted):
    logits, labels, weight = R.loss_inputs(c, kind, (3, 13, 11))
    wt = weight if weighted else None
    value, sums, grad = R.loss_ref(logits, labels, wt, R.IGNORE, 1.0, 0.0, 0)
    z = logits.double().requires_grad_(True)
    lab = labels.long().clone()
    lab[~R.loss_valid(labels, c)] = R.IGNORE                # F.cross_entropy rejects out-of-range labels: the kernel ignores them
    ref = F.cross_entropy(z, lab, weight=None if wt is None else wt.double(), ignore_index=R.IGNORE)
    ref.backward()
    assert rel_err(value, ref) < 1e-13 and rel_err(grad, z.grad) < 1e-13
    invalid = ~R.loss_valid(labels, c)
    assert int(invalid.sum()) >= 5 and float(grad.permute(0, 2, 3, 1)[invalid].abs().max()) == 0.0
    assert abs(float(sums[1]) - float((wt.double()[lab[~invalid]] if weighted else (~invalid).double()).sum())) < 1e-9


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("alpha,gamma", [(1.0, 0.0), (0.25, 2.0), (1.0, 0.5)])
@pytest.mark.parametrize("c,weighted", [(3, True), (9, False)])
def test_loss_focal_is_autograd_of_the_focal_expression(mode, alpha, gamma, c, weighted):
    """in-range labels and moderate logits: at ce == 0 autograd through pow has no finite derivative for gamma < 1"""
    g = R.gen(c + mode)
    logits = torch.randn(2, c, 7, 9, generator=g) * 3
    labels = torch.randint(0, c, (2, 7, 9), generator=g)
    labels[0, 0, :4] = R.IGNORE
    weight = (torch.rand(c, generator=g) + 0.5) if weighted else None
    value, _, grad = R.loss_ref(logits, labels, weight, R.IGNORE, alpha, gamma, mode)
    v_ref, g_ref = focal_autograd(logits.double(), labels, weight, alpha, gamma, mode)
    assert rel_err(value, v_ref) < 1e-12 and rel_err(grad, g_ref) < 1e-11


def test_loss_confident_pixels_have_a_finite_gradient():
    logits = torch.zeros(1, 3, 2, 2)
    logits[:, 1] = 40.0
    labels = torch.ones(1, 2, 2, dtype=torch.int64)
    value, _, grad = R.loss_ref(logits, labels, None, R.IGNORE, 1.0, 0.5, 1)
    assert bool(torch.isfinite(grad).all()) and bool(torch.isfinite(value)) and float(grad.abs().max()) < 1e-20


def loss_fp32(logits, labels, weight, alpha, gamma, mode):
    """torch's own fp32 evaluation: F.cross_entropy + autograd for mode 0; for the focal modes the closed form of loss_ref in fp32
    on torch's fp32 log_softmax (autograd through pow gives nan at the ce == 0 pixels that logits of magnitude 30 produce)"""
    c = logits.shape[1]
    if mode == 0:
        z = logits.clone().requires_grad_(True)
        lab = labels.long().clone()
        lab[~R.loss_valid(labels, c)] = R.IGNORE
        v = F.cross_entropy(z, lab, weight=weight, ignore_index=R.IGNORE)
        v.backward()
        wsum = (weight[lab[lab != R.IGNORE]] if weight is not None else (lab != R.IGNORE).float()).sum()
        return v.detach(), torch.stack([v.detach() * wsum, wsum]), z.grad
    return R.loss_ref(logits, labels, weight, R.IGNORE, alpha, gamma, mode, dtype=torch.float32,
                      log_softmax=lambda t: F.log_softmax(t, 1))


def test_floors_loss():
    m = {}
    with one_thread():
        for c, kind, mode, alpha, gamma, weighted, up, shape in R.LOSS_CASES:
            logits, labels, weight = R.loss_inputs(c, kind, R.LOSS_SHAPES[shape])
            wt = weight if weighted else None
            v, s, g = R.loss_ref(logits, labels, wt, R.IGNORE, alpha, gamma, mode)
            v32, s32, g32 = loss_fp32(logits, labels, wt, alpha, gamma, mode)
            put(m, "loss.value.m%d" % mode, rel_err(v32, v))
            put(m, "loss.sums", rel_err(s32, s))
            put(m, "loss.grad.m%d" % mode, rel_err(g32 * np.float32(up), g * R.f32(up)))
        logits, labels, weight = R.loss_inputs(2, "u8", R.LOSS_CAP_SHAPE)
        v, s, g = R.loss_ref(logits, labels, weight, R.IGNORE, 1.0, 0.0, 0)
        v32, s32, g32 = loss_fp32(logits, labels, weight, 1.0, 0.0, 0)
        put(m, "loss.cap.value", rel_err(v32, v))
        put(m, "loss.cap.grad", rel_err(g32, g))
    check_floors(m)


# ---- bilinear --------------------------------------------------------------------------------------------------------
def interp_fp32(x, dy, ho, wo):
    xr = x.permute(0, 3, 1, 2).contiguous().requires_grad_(True)
    y = F.interpolate(xr, size=(ho, wo), mode="bilinear", align_corners=False)
    y.backward(dy.permute(0, 3, 1, 2).contiguous())
    return y.detach().permute(0, 2, 3, 1), xr.grad.permute(0, 2, 3, 1)


def test_bilinear_is_interpolate_and_floors():
    """at every GPU case: the float32-index restatement against F.interpolate(fp32) and its autograd"""
    m = {}
    with one_thread():
        for shape, c in R.RESIZE_CASES:
            (hi, wi), (ho, wo) = shape
            x, dy = R.resize_inputs(shape, c)
            y32, dx32 = interp_fp32(x, dy, ho, wo)
            ef, eb = rel_err(y32, R.bilinear_fwd_ref(x, ho, wo)), rel_err(dx32, R.bilinear_bwd_ref(dy, hi, wi))
            assert ef < 1e-6 and eb < 1e-6, (shape, c, ef, eb)          # a wrong index or weight gives 1e-2 or more
            put(m, "bilinear.fwd", ef)
            put(m, "bilinear.bwd", eb)
        for c, cp in R.RESIZE_NCHW:
            for shape in R.RESIZE_SHAPES:
                (hi, wi), (ho, wo) = shape
                x, dy = R.resize_inputs(shape, c)
                y32, dx32 = interp_fp32(x, dy, ho, wo)
                put(m, "bilinear_nchw.fwd", rel_err(y32, R.bilinear_fwd_ref(x, ho, wo)))
                put(m, "bilinear_nchw.bwd", rel_err(dx32, R.bilinear_bwd_ref(dy, hi, wi)))
    check_floors(m)


def test_bilinear_identity_and_float64_indices():
    x, dy = R.resize_inputs(((7, 5), (7, 5)), 4)
    assert torch.equal(R.bilinear_fwd_ref(x, 7, 5), x.double()) and torch.equal(R.bilinear_bwd_ref(dy, 7, 5), dy.double())
    # the reason for float32 indices: torch's float64 interpolate is 7e-6 away from its float32 one at 129 -> 37
    x, _ = R.resize_inputs(((129, 129), (37, 53)), 4)
    y64 = F.interpolate(x.double().permute(0, 3, 1, 2), size=(37, 53), mode="bilinear", align_corners=False).permute(0, 2, 3, 1)
    assert rel_err(R.bilinear_fwd_ref(x, 37, 53), y64) > 1e-6


def test_bilinear_gather_window_without_its_slack_is_never_short():
    """The backward gathers, per input index i, over outputs [floor(a) - 1, ceil(b) + 1] with a = (i - 0.5) / scale - 0.5,
    b = (i + 1.5) / scale - 0.5 (resize.hip: out_range).  An output o can reference i only if scale (o + 0.5) - 0.5 lies in
    (i - 1, i + 1), i.e. o in the open interval (a, b), so [floor(a), ceil(b)] already holds every candidate: the one index of
    slack only guards the fp32 rounding of a and b.  This emulates that fp32 arithmetic (contracted to a fused multiply-add and
    not) for every pair of sizes up to 48 -> 96 and the sizes of the GPU cases and finds no input whose referencing outputs leave
    the un-slacked window -- which is why dropping the slack changes no result and no test can catch it (the mutation table of
    profiles/streaming_kernel_tests.txt).  The slack stays in the kernel: it costs two candidates of weight 0 per axis and covers
    the sizes no emulation has visited."""
    f = np.float32
    sizes = {(i, o) for i in range(1, 49) for o in range(1, 97)} | {(h, k) for (hi, wi), (ho, wo) in R.RESIZE_SHAPES
                                                                   for h, k in ((hi, ho), (wi, wo))}
    for inn, out in sorted(sizes):
        i0, i1, l0, l1 = R.bilinear_index(inn, out)
        inv = f(1) / (f(inn) / f(out))
        i = np.arange(inn)
        refs = ((i0[None] == i[:, None]) & (l0[None] != 0)) | ((i1[None] == i[:, None]) & (l1[None] != 0))      # [in, out]
        o = np.arange(out)
        first = np.where(refs, o[None], out).min(1)
        last = np.where(refs, o[None], -1).max(1)
        lo_f, hi_f = i.astype(f) - f(0.5), i.astype(f) + f(1.5)
        for a, b in (((lo_f.astype(np.float64) * inv - 0.5).astype(f), (hi_f.astype(np.float64) * inv - 0.5).astype(f)),
                     ((lo_f * inv).astype(f) - f(0.5), (hi_f * inv).astype(f) - f(0.5))):
            lo, hi = np.maximum(np.floor(a), 0), np.minimum(np.ceil(b), out - 1)
            used = last >= 0
            assert (first[used] >= lo[used]).all() and (last[used] <= hi[used]).all(), (inn, out)


# ---- depthwise -------------------------------------------------------------------------------------------------------
def test_depthwise_restatement_is_the_tap_sum():
    """y[n, oh, ow, c] = b[c] + sum_kh,kw x[n, oh s - p + kh d, ow s - p + kw d, c] w[c, kh, kw], written as a loop"""
    for case in (R.DW_CASES[1], R.DW_CASES[5], R.DW_CASES[8]):
        n, h, w, c, cw, kh, kw, s, p, d, _, _ = case
        r = R.dw_case(case)
        xp = F.pad(r["x"].double(), (0, 0, p, p, p, p))
        y = torch.zeros(n, r["ho"], r["wo"], c, dtype=torch.float64)
        for a in range(kh):
            for b in range(kw):
                win = xp[:, a * d:a * d + (r["ho"] - 1) * s + 1:s, b * d:b * d + (r["wo"] - 1) * s + 1:s, :cw]
                y[..., :cw] += win * r["w"].double()[:, 0, a, b]
        if r["bias"] is not None:
            y[..., :cw] += r["bias"].double()
        assert rel_err(r["y"], y) < 1e-14


def test_floors_depthwise():
    m = {}
    with one_thread():
        for case in R.DW_CASES:
            n, h, w, c, cw, kh, kw, s, p, d, _, _ = case
            r = R.dw_case(case)
            r32 = R.dw_ref(r["x"], r["w"], r["bias"], r["dy"], cw, s, p, d, torch.float32)
            put(m, "dw.y", rel_err(r32["y"], r["y"]))
            put(m, "dw.dx", rel_err(r32["dx"], r["dx"]))
            put(m, "dw.dx_acc", rel_err(r32["dx"] + r["dx0"], r["dx"] + r["dx0"].double()))
            put(m, "dw.dw", rel_err(r32["dw"], r["dw"]))
    check_floors(m)


# ---- optimizers ------------------------------------------------------------------------------------------------------
def test_optimizer_restatement_and_floors():
    """sgd_ref / adam_ref ARE torch.optim on float64 parameters; pinned here: one hand-computed nesterov step, the buffer
    convention at momentum 0, and the bias corrections the kernel is handed"""
    p0, grads = R.opt_inputs(7)
    p, buf = R.sgd_ref(p0, grads[:1], 0.9, True, 1e-4)
    d = grads[0].double() + R.f32(1e-4) * p0.double()
    assert rel_err(buf, d) < 1e-15 and rel_err(p, p0.double() - R.SGD_LR * (d + R.f32(0.9) * d)) < 1e-15
    p, buf = R.sgd_ref(p0, grads[:1], 0.0, False, 1e-2)
    assert rel_err(p, p0.double() - R.SGD_LR * buf) < 1e-15
    p, m1, v1 = R.adam_ref(p0, grads[:1], True, 1e-2)
    h = R.adam_hyper(1)
    g = grads[0].double()
    mm, vv = (1 - R.ADAM_BETAS[0]) * g, (1 - R.ADAM_BETAS[1]) * g * g
    want = p0.double() * (1 - R.ADAM_LR * R.f32(1e-2)) - R.ADAM_LR / h[1] * mm / (vv.sqrt() / h[2] ** 0.5 + R.ADAM_EPS)
    assert rel_err(m1, mm) < 1e-15 and rel_err(v1, vv) < 1e-15 and rel_err(p, want) < 1e-14
    m = {}
    with one_thread():
        for n in R.OPT_N:
            p0, grads = R.opt_inputs(n)
            for mu, nest, wd in R.SGD_CONFIGS:
                a, b = R.sgd_ref(p0, grads, mu, nest, wd), R.sgd_ref(p0, grads, mu, nest, wd, torch.float32)
                put(m, "sgd.p", rel_err(b[0], a[0]))
                put(m, "sgd.buf", rel_err(b[1], a[1]))
            for dec, wd in R.ADAM_CONFIGS:
                a, b = R.adam_ref(p0, grads, dec, wd), R.adam_ref(p0, grads, dec, wd, torch.float32)
                for k, name in enumerate(("adam.p", "adam.m", "adam.v")):
                    put(m, name, rel_err(b[k], a[k]))
    check_floors(m)


# ---- Philox ----------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """the three Random123 known-answer vectors of philox4x32-10"""
    kat = [
        ([0, 0, 0, 0], [0, 0], [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]),
        ([0xffffffff] * 4, [0xffffffff] * 2, [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]),
        ([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0], [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]),
    ]
    ctr = np.array([k[0] for k in kat], dtype=np.uint64)
    key = np.array([k[1] for k in kat], dtype=np.uint64)
    out = R.philox4x32_10(ctr, key)
    assert out.dtype == np.uint32 and out.tolist() == [k[2] for k in kat]


def test_dropout_mask_layout():
    """element 4 i + k takes word k of counter (i, 0, offset lo, offset hi) under key (seed lo, seed hi)"""
    seed, offset, n, p = 2 ** 32 + 7, 2 ** 32 + 5, 23, 0.5
    mask = R.dropout_mask_ref(n, p, seed, offset)
    for e in (0, 5, 22):
        word = int(R.philox4x32_10(np.array([[e // 4, 0, 5, 1]]), np.array([[7, 1]]))[0, e % 4])
        assert int(mask[e]) == int(np.float32(word >> 8) * np.float32(2.0 ** -24) >= np.float32(p))
    assert not np.array_equal(mask, R.dropout_mask_ref(n, p, 7, 5))           # the high words matter
    assert R.dropout_mask_ref(4096, 0.0, 1234, 1).all()
    assert abs(float(R.dropout_mask_ref(65539, 0.1, 1234, 1).mean()) - 0.9) < 5e-3


# ---- pooling ---------------------------------------------------------------------------------------------------------
def test_floors_pooling():
    m = {}
    with one_thread():
        for n, hw, c in R.POOL_CASES:
            x = R.pool_inputs(n, hw, c)
            nhw = hw[0] * hw[1]
            put(m, "gap.fwd", rel_err(F.adaptive_avg_pool2d(x.permute(0, 3, 1, 2), 1)[:, :, 0, 0], x.double().mean((1, 2))))
            put(m, "bcast.bwd", rel_err(x.sum((1, 2)), x.double().sum((1, 2))))
            v = x[:, 0, 0]
            put(m, "gap.bwd", rel_err(v / nhw, v.double() / nhw))
            put(m, "gap.bwd_acc", rel_err(x + (v / nhw)[:, None, None], x.double() + (v.double() / nhw)[:, None, None]))
        for h, w, c in R.MAXPOOL_CASES:
            x = torch.relu(torch.randn(2, c, h, w, generator=R.gen(h * w)))
            x32, x64 = x.clone().requires_grad_(True), x.double().requires_grad_(True)
            y32, y64 = F.max_pool2d(x32, 3, 2, 1), F.max_pool2d(x64, 3, 2, 1)
            dy = torch.randn(y32.shape, generator=R.gen(c))
            y32.backward(dy)
            y64.backward(dy.double())
            put(m, "maxpool.dx", rel_err(x32.grad, x64.grad))
    check_floors(m)


# ---- BatchNorm -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def bn_torch_fp32(stats, shape, act):
    """torch's fp32 F.batch_norm (+ residual, activation) with autograd, momentum 1: the running buffers become the batch mean
    and the unbiased batch variance"""
    relu, res = act
    x, gamma, beta, resid, dout = R.bn_inputs(stats, shape, res)
    c = shape[1]
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rr = resid.clone().requires_grad_(True) if res else None
    rm, rv = torch.zeros(c), torch.ones(c)
    z = F.batch_norm(xr, rm, rv, gr, br, True, 1.0, R.BN_EPS)
    out = R.bn_act(z + rr if res else z, relu)
    out.backward(dout)
    return dict(mean=rm, var_unbiased=rv, out=out.detach(), dy=xr.grad, dgamma=gr.grad, dbeta=br.grad,
                dres=rr.grad if res else None)


@pytest.mark.parametrize("relu,res", [(False, False), (True, False), (6, True)])
def test_batchnorm_restatement_is_batch_norm_and_its_autograd(relu, res):
    x, gamma, beta, resid, dout = R.bn_inputs((0.5, 2.0), (2, 8, 9, 7), res)
    xr, gr, br = (t.double().requires_grad_(True) for t in (x, gamma, beta))
    rr = resid.double().requires_grad_(True) if res else None
    rm, rv = torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64)
    z = F.batch_norm(xr, rm, rv, gr, br, True, 1.0, R.BN_EPS)
    out = R.bn_act(z + rr if res else z, relu)
    out.backward(dout.double())
    f = R.bn_fwd_ref(x, gamma, beta, resid, relu)
    dy, dg, db, dres = R.bn_bwd_ref(f, gamma, dout, R.bn_act_mask(f["out"], relu), True)
    assert rel_err(f["mean"], rm) < 1e-14 and rel_err(f["var_unbiased"], rv) < 1e-13 and rel_err(f["out"], out) < 1e-13
    assert rel_err(dy, xr.grad) < 1e-11 and rel_err(dg, gr.grad) < 1e-12 and rel_err(db, br.grad) < 1e-13
    if res:
        assert torch.equal(dres, rr.grad)
    # eval form on given statistics
    xe, ge = x.double().requires_grad_(True), gamma.double().requires_grad_(True)
    mean, var = torch.randn(8, generator=R.gen(3)).double(), torch.rand(8, generator=R.gen(4)).double() + 0.5
    oe = R.bn_act(F.batch_norm(xe, mean, var, ge, beta.double(), False, 0.1, R.BN_EPS), relu)
    oe.backward(dout.double())
    fe = R.bn_fwd_ref(x, gamma, beta, None, relu, mean, var)
    dye, dge, _, _ = R.bn_bwd_ref(fe, gamma, dout, R.bn_act_mask(fe["out"], relu), False)
    assert rel_err(fe["out"], oe) < 1e-13 and rel_err(dye, xe.grad) < 1e-12 and rel_err(dge, ge.grad) < 1e-12


def bn_floor_case(stats, shape, act):
    """torch-fp32 against the restatement, the backward on torch-fp32's OWN activation pattern"""
    relu, res = act
    x, gamma, beta, resid, dout = R.bn_inputs(stats, shape, res)
    t = bn_torch_fp32(stats, shape, act)
    f = R.bn_fwd_ref(x, gamma, beta, resid, relu)
    dy, dg, db, _ = R.bn_bwd_ref(f, gamma, dout, R.bn_act_mask(t["out"], relu), True)
    return dict(mean=rel_err(t["mean"], f["mean"]), var=rel_err(t["var_unbiased"], f["var_unbiased"]),
                out=rel_err(t["out"], f["out"]), dy=rel_err(t["dy"], dy), dgamma=rel_err(t["dgamma"], dg),
                dbeta=rel_err(t["dbeta"], db))


def test_floors_batchnorm():
    m = {}
    with one_thread():
        for stats, shape, act in R.BN_CASES:
            for k, v in bn_floor_case(stats, shape, act).items():
                put(m, "bn.%s.mean%g" % (k, stats[0]), v)
        x, gamma, beta, _, dout = R.bn_inputs((0.5, 2.0), R.BN_SHAPES[1], False)          # eval-mode backward, ordinary statistics
        mean, var = torch.randn(64, generator=R.gen(3)) * 0.1 + 0.5, torch.rand(64, generator=R.gen(4)) + 3.5
        xe, ge, be = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
        oe = F.relu(F.batch_norm(xe, mean, var, ge, be, False, 0.1, R.BN_EPS))
        oe.backward(dout)
        fe = R.bn_fwd_ref(x, gamma, beta, None, True, mean, var)
        dy, dg, db, _ = R.bn_bwd_ref(fe, gamma, dout, oe > 0, False)
        m.update({"bn_eval.out": rel_err(oe, fe["out"]), "bn_eval.dy": rel_err(xe.grad, dy),
                  "bn_eval.dgamma": rel_err(ge.grad, dg), "bn_eval.dbeta": rel_err(be.grad, db)})
    check_floors(m)


@pytest.mark.parametrize("stats", R.BN_STATS, ids=lambda s: "mean%g_std%g" % s)
def test_naive_variance_misses_the_bound_by_100x(stats):
    """discrimination: a one-pass fp32 E[x^2] - E[x]^2 must be at least 100 x outside the variance bound (4 x floor) at every
    large-mean input -- otherwise the GPU variance check could not tell centred tile statistics from uncentred ones"""
    for shape in R.BN_SHAPES:
        x = R.bn_inputs(stats, shape, False)[0]
        err = rel_err(R.naive_var_fp32(x), x.double().var((0, 2, 3), unbiased=False))
        bound = 4 * R.FLOOR["bn.var.mean%g" % stats[0]]
        print("naive fp32 variance rel err %.3e, bound %.3e" % (err, bound))
        assert err >= 100 * bound


# ---- BatchNorm, second table (bn2): path claims, floors, mutants ---------------------------------------------------------
# what each case of streaming_ref.BN2_BATCH / BN2_WALK reaches, asserted below from the restated plan_rows and thresholds.
#   reduce: (double throughout, tiles, RL, column blocks, groups in the last block, rows per thread, runs of 8 per thread, finalize CPB)
#   apply:  (channels per thread of bn_apply, column blocks, groups in the last block, rows per thread)
BN2_CLAIMS = {
    "rows8192": dict(reduce=(True, 256, 64, 1, 4, [0, 1], [0, 1], 4), apply=(4, 1, 4, [4])),
    "rows8193": dict(reduce=(False, 257, 64, 1, 4, [0, 1], [0, 1], 4), apply=(4, 1, 4, [3, 4])),
    "rows8193_plain": dict(reduce=(False, 257, 64, 1, 4, [0, 1], [0, 1], 4), apply=(4, 1, 4, [3, 4])),
    "runs": dict(reduce=(False, 259, 2, 1, 128, [15, 16], [2], 4), apply=(8, 1, 64, [3, 4])),
    "tilecap": dict(reduce=(False, 1024, 4, 1, 64, [8, 9], [1, 2], 4), apply=(4, 1, 64, [3, 4])),
    "cols2": dict(reduce=(True, 2, 1, 2, 2, [18, 19], [3], 16), apply=(4, 2, 2, [3, 4])),
    "cols2_pl": dict(reduce=(True, 2, 1, 3, 2, [18, 19], [3], 16), apply=(8, 2, 1, [3, 4])),
    "walk7": dict(reduce=(True, 1, 16, 1, 16, [0, 1], [0, 1], 16), apply=(8, 1, 8, [0, 1])),
    "walk33": dict(reduce=(True, 2, 16, 1, 16, [1, 2], [1], 16), apply=(8, 1, 8, [1, 2])),
    "walk100": dict(reduce=(True, 4, 16, 1, 16, [1, 2], [1], 16), apply=(8, 1, 8, [3, 4])),
}


def bn2_shape(cid):
    """(rows, channels, planes) of a batch or walk case"""
    if cid in R.BN2_BATCH:
        (n, h, w), c, _, planes = R.BN2_BATCH[cid]
        return n * h * w, c, planes
    return R.BN2_WALK[cid], R.BN2_WALK_C, True


@pytest.mark.parametrize("cid", list(BN2_CLAIMS))
def test_bn2_cases_reach_the_paths_they_claim(cid):
    """plan_rows, `dbl = M <= 8192`, the finalize's `tiles > 32` and the 1024-tile cap restated in streaming_ref; the tile count and
    the workspace size are the library's own"""
    from iswm_amd import _lib
    lib = _lib.load()
    m, c, planes = bn2_shape(cid)
    s = R.reduce_structure(m, c)
    assert s["tiles"] == lib.iswm_colstat_tiles(m)
    assert lib.iswm_bn_bwd_workspace(m, c) == (2 * s["tiles"] * c + 2 * c) * 8           # double [2][tiles][C] + [2][C]
    p = s["plan"]
    got = (s["dbl"], s["tiles"], p["RL"], p["colblocks"], p["last_groups"], s["rows"], s["runs"], s["finalize"])
    assert got == BN2_CLAIMS[cid]["reduce"], got
    dense = (3 if planes else 0, c, 0, m * c)
    form = R.bn_apply_form(c, c, dense, dense)
    p = R.plan_rows(m, c // 2 if form == 8 else c)
    got = (form, p["colblocks"], p["last_groups"], R.walk_lengths(m, p))
    assert got == BN2_CLAIMS[cid]["apply"], got
    if cid == "tilecap":
        assert -(-m // 32) == 1036 and m * c // 4 > 2048 * 256                           # uncapped tiles; a second grid-stride trip
    if cid == "runs":                                                                    # the second run is ragged for SOME threads
        assert {len(R.walk(m, s["plan"], b, l)) % R.BN_RUN for b in range(s["tiles"]) for l in range(2)} == {7, 0}
    if form == 8:                                       # k_bn_apply8: rows // 2 pair iterations, rows % 2 tail rows
        pairs_tail = {(r // 2, r % 2) for r in got[3]}
        want = {"runs": {(1, 1), (2, 0)}, "cols2_pl": {(1, 1), (2, 0)}, "walk7": {(0, 0), (0, 1)}, "walk33": {(0, 1), (1, 0)},
                "walk100": {(1, 1), (2, 0)}}[cid]
        assert pairs_tail == want, pairs_tail


def test_bn2_fallback_forms():
    """the dispatch of iswm_bn_apply_pl restated (streaming_ref.bn_apply_form), in both plane counts"""
    n, h, w = R.BN2_FALLBACK_ROWS
    m = n * h * w
    for fid, (c, (ow, oo), (rw, ro), want) in R.BN2_FALLBACK.items():
        for planes in (3, 1):
            assert R.bn_apply_form(c, c, (planes, ow, oo, m * ow), (planes, rw, ro, m * rw)) == want, (fid, planes)
    assert R.bn_apply_form(64, 64, (0, 64, 0, 0)) == 4                                   # an fp32 output: always the 4-channel kernel
    assert R.bn_apply_form(64, 64, (3, 64, 0, m * 64), (0, 64, 0, 0)) == 8               # an fp32 residual does not matter


def test_bf16_restatements():
    x = torch.cat([torch.randn(4096, generator=R.gen(5)) * 3, torch.tensor(R.BF16_EDGE)])
    hi, mid, lo = R.split3(x)
    assert torch.equal(hi + mid + lo, x) and torch.equal((hi.double() + mid.double() + lo.double()).float(), x)
    for p in (hi, mid, lo):
        assert torch.equal(p.to(torch.bfloat16).float(), p)
    e = dict(zip(R.BF16_EDGE, R.bf16_rne(torch.tensor(R.BF16_EDGE)).tolist()))
    assert e[1.00390625] == 1.0 and e[1.01171875] == 1.015625 and e[5.953125] == 5.9375 and e[5.984375] == 6.0 and e[5.99] == 6.0
    assert float(R.bf16_trunc(torch.tensor([5.99]))) == 5.96875


def torch_bn_fp32(x, gamma, beta, resid, dout, relu, mean=None, var=None, eps=R.BN_EPS):
    """torch's fp32 F.batch_norm (+ residual, activation) and autograd; batch statistics, or the given ones in eval mode"""
    xr, gr, br = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    rr = resid.clone().requires_grad_(True) if resid is not None else None
    z = F.batch_norm(xr, mean, var, gr, br, mean is None, 0.1, eps)
    out = R.bn_act(z + rr if rr is not None else z, relu)
    out.backward(dout)
    return dict(out=out.detach(), dy=xr.grad, dgamma=gr.grad, dbeta=br.grad)


def bn2_floor_batch(cid, round_resid=False):
    from tests.bn_partials_ref import bwd_sums
    (n, h, w), c, (relu, res), _ = R.BN2_BATCH[cid]
    x, gamma, beta, resid, dout = R.bn2_batch_inputs(cid)
    resid = (R.bf16_rne(resid) if round_resid else resid) if res else None
    t = torch_bn_fp32(x, gamma, beta, resid, dout, relu)
    f = R.bn_fwd_ref(x, gamma, beta, resid, relu)
    mask = R.bn_act_mask(t["out"], relu)
    dy, dg, db, _ = R.bn_bwd_ref(f, gamma, dout, mask, True)
    if n * h * w > R.BN_DBL_ROWS:                      # the kernel adds fp32 runs: the sequential-fp32 restatement is the floor
        nhwc = lambda v: v.permute(0, 2, 3, 1).contiguous()
        b = dict(y=nhwc(x), mean=f["mean"].float(), invstd=(1.0 / torch.sqrt(f["var"] + R.BN_EPS)).float())
        s0, s1 = bwd_sums(nhwc(dout), nhwc(mask).float(), b, torch.float32)
        t["dbeta"], t["dgamma"] = s0, s1
    figs = {k: rel_err(t[k], v) for k, v in (("out", f["out"]), ("dy", dy), ("dgamma", dg), ("dbeta", db))}
    return figs, dict(f=f, dy=dy, dgamma=dg, dbeta=db, mask=mask, dout=dout, gamma=gamma, resid=resid, relu=relu)


def bn2_floor_given(inputs, relu, res):
    """res: None, "exact" or "bf16" (the residual as a one-plane tensor holds it)"""
    x, gamma, beta, resid, dout, mean, invstd = inputs
    resid = None if res is None else (R.bf16_rne(resid) if res == "bf16" else resid)
    var = R.given_var(invstd)
    t = torch_bn_fp32(x, gamma, beta, resid, dout, relu, mean, var.float())
    f = R.bn_fwd_ref(x, gamma, beta, resid, relu, mean, var)
    mask = R.bn_act_mask(t["out"], relu)
    dy_eval, dg, db, _ = R.bn_bwd_ref(f, gamma, dout, mask, False)
    dy = R.bn_bwd_ref(f, gamma, dout, mask, True)[0]
    dy32 = R.bn_dy_train_fp32(x, mean, invstd, gamma, dout * mask, dg, db)
    figs = dict(out=rel_err(t["out"], f["out"]), dy_eval=rel_err(t["dy"], dy_eval), dy=rel_err(dy32, dy),
                dgamma=rel_err(t["dgamma"], dg), dbeta=rel_err(t["dbeta"], db))
    return figs, dict(f=f, dy=dy, dy_eval=dy_eval, dgamma=dg, dbeta=db, mask=mask, dout=dout, gamma=gamma, resid=resid, relu=relu)


def bn2_walk_inputs(wid):
    return R.bn2_given_inputs((1, R.BN2_WALK_C, 1, R.BN2_WALK[wid]))


def bn2_fallback_inputs(fid):
    n, h, w = R.BN2_FALLBACK_ROWS
    return R.bn2_given_inputs((n, R.BN2_FALLBACK[fid][0], h, w))


@functools.lru_cache(maxsize=None)
def bn2_measured():
    """({floor key: figure}, {check tag: the float64 results the mutants are applied to})"""
    m, refs = {}, {}
    with one_thread():
        for cid in R.BN2_BATCH:
            for rounded in ((False, True) if cid == "cols2_pl" else (False,)):
                figs, ref = bn2_floor_batch(cid, rounded)
                for k, v in figs.items():
                    put(m, "bn2.%s.%s" % (k, cid), v)
                refs[cid + ("/bf16res" if rounded else "")] = ref
        for wid in R.BN2_WALK:
            for res in (("exact", "bf16") if wid == "walk33" else ("exact",)):
                figs, ref = bn2_floor_given(bn2_walk_inputs(wid), True, res)
                for k, v in figs.items():
                    put(m, "bn2.%s.%s" % (k, wid), v)
                refs["%s/%s" % (wid, res)] = ref
        for fid in R.BN2_FALLBACK:
            for res in ("exact", "bf16"):
                figs, ref = bn2_floor_given(bn2_fallback_inputs(fid), True, res)
                for k, v in figs.items():
                    put(m, "bn2.%s.%s" % (k, R.fallback_tag(fid)), v)
                refs["%s/%s/%s" % (R.fallback_tag(fid), fid, res)] = ref
        grid = R.bn2_given_inputs(R.BN2_GRID_SHAPE, 8)
        for relu in R.BN2_RELUS:
            for res in (None, "exact", "bf16"):
                figs, ref = bn2_floor_given(grid, relu, res)
                for k, v in figs.items():
                    put(m, "bn2.%s.%s" % (k, R.grid_tag(relu, res)), v)
                refs["%s/%s" % (R.grid_tag(relu, res), res)] = ref
    return m, refs


def test_floors_bn2():
    check_floors(bn2_measured()[0])


def bn2_key(tag, quantity):
    return "bn2.%s.%s" % (quantity, tag.split("/")[0])


def test_bn2_store_mutants():
    """every float check of a bn2 store (out, dy, dgamma, dbeta) against the faults a store can have, on the restatement alone; each
    must miss its assertion by >= 3 x the bound (12 x floor):
      - an element left at the buffer's initial value (a dropped last row, the tail row of a pair walk, an unprocessed second
        column block): every buffer starts at SENTINEL in every plane, so the joined value is SENTINEL or 3 x SENTINEL;
      - the lo or the mid plane of a stored output or of dy dropped;
      - a one-plane store by truncation: the check is bit equality with round-to-nearest-even, so one differing element is a miss"""
    _, refs = bn2_measured()
    for tag, r in refs.items():
        for q in ("out", "dy", "dy_eval", "dgamma", "dbeta"):
            ref = r["f"]["out"] if q == "out" else r.get(q)
            if ref is None:
                continue
            need = 12 * R.FLOOR[bn2_key(tag, q)]
            scale = float(ref.abs().max())
            for s in (R.SENTINEL, 3 * R.SENTINEL):
                assert float((ref - s).abs().min()) / scale >= need, (tag, q, s)
            if q in ("out", "dy", "dy_eval"):
                hi, mid, lo = R.split3(ref.float())
                assert float(lo.abs().max()) / scale >= need and float(mid.abs().max()) / scale >= need, (tag, q)
                assert not torch.equal(R.bf16_trunc(ref.float()), R.bf16_rne(ref.float())), (tag, q)


def test_bn2_residual_plane_mutants():
    """the lo or the mid plane of a three-plane residual not read: out moves by that plane wherever the activation passes"""
    _, refs = bn2_measured()
    seen = 0
    for tag, r in refs.items():
        if r["resid"] is None or "bf16" in tag:
            continue
        f = r["f"]
        need = 12 * R.FLOOR[bn2_key(tag, "out")]
        for plane in R.split3(r["resid"])[1:]:
            err = rel_err(R.bn_act(f["z"] - plane.double(), r["relu"]), f["out"])
            assert err >= need, (tag, err, need)
        seen += 1
    assert seen >= 10


def bn2_sum_errors(r, tag, drop):
    """(dgamma, dbeta, dy) errors over their bounds when the NHWC rows x channels of `drop` (a bool [M, C] mask) are missing from
    the sums of the backward"""
    f = r["f"]
    dz = (r["dout"].double() * r["mask"].double())
    c = dz.shape[1]
    keep = (~drop).t().double()                                      # [C, M]; M runs over (n, h, w) as the NHWC rows do
    dzr, xh = dz.permute(1, 0, 2, 3).reshape(c, -1), f["xhat"].permute(1, 0, 2, 3).reshape(c, -1)
    db, dg = (dzr * keep).sum(1), (dzr * xh * keep).sum(1)
    m = dzr.shape[1]
    k = (r["gamma"].double() / torch.sqrt(f["var"] + R.BN_EPS))[None, :, None, None]
    dy = k * (dz - db[None, :, None, None] / m - f["xhat"] * dg[None, :, None, None] / m)
    return (rel_err(dg, r["dgamma"]) / (4 * R.FLOOR[bn2_key(tag, "dgamma")]), rel_err(db, r["dbeta"]) / (4 * R.FLOOR[bn2_key(tag, "dbeta")]),
            rel_err(dy, r["dy"]) / (4 * R.FLOOR[bn2_key(tag, "dy")]))


BN2_SUM_MUTANT_TAGS = list(R.BN2_BATCH) + ["%s/exact" % w for w in R.BN2_WALK] + [
    "%s/%s/exact" % (R.fallback_tag(f), f) for f in ("c12", "off4")] + [
    "%s/%s" % (R.grid_tag(relu, res), res) for relu in R.BN2_RELUS for res in (None, "exact")]


@pytest.mark.parametrize("tag", BN2_SUM_MUTANT_TAGS)
def test_bn2_sum_mutants(tag):
    """faults of the reduce pass, on the restatement alone, for every case whose dgamma / dbeta / dy is checked (the batch cases,
    the walks, both fallback channel counts, the grid per activation with and without a residual); dgamma, dbeta AND dy must each
    miss by >= 3 x their bound:
      - the last row of one thread's walk is not added;
      - one whole run of 8 rows of one thread is missing (where a thread has a run);
      - tilecap: the partial of one block goes to another block's slot.  A block is blockIdx.x of a strided walk (gridDim.x ==
        tiles == 1024, rows b * RL + lane + k * 1024 * RL), and the finalize sums slots 0 .. tiles - 1: if block 1023 writes slot
        1022, the finalize reads block 1023's sums once, never block 1022's, and slot 1023 keeps the workspace's zeros -- all rows
        of block 1022 are missing;
      - the second column block is not reduced: its sums stay at SENTINEL (test_bn2_store_mutants)"""
    _, refs = bn2_measured()
    r = refs[tag]
    m, c = r["dout"].numel() // r["dout"].shape[1], r["dout"].shape[1]
    s = R.reduce_structure(m, c)
    block, lane, group = s["tiles"] // 2, s["plan"]["RL"] - 1, s["plan"]["C4"] - 1
    rows = R.walk(m, s["plan"], block, lane)
    if not rows:
        block, lane = 0, 0
        rows = R.walk(m, s["plan"], block, lane)
    muts = {"last_row": rows[-1:]}
    if len(rows) >= R.BN_RUN:
        muts["run"] = rows[:R.BN_RUN]
    for name, rr in muts.items():
        drop = torch.zeros(m, c, dtype=torch.bool)
        drop[rr, 4 * group:4 * group + 4] = True
        errs = bn2_sum_errors(r, tag, drop)
        print(tag, name, "miss / bound: dgamma %.1f dbeta %.1f dy %.1f" % errs)
        assert min(errs) >= 3, (tag, name, errs)
    if tag == "tilecap":
        lost = sorted(q for lane in range(s["plan"]["RL"]) for q in R.walk(m, s["plan"], s["tiles"] - 2, lane))
        assert len(lost) == 32 and lost[-1] - lost[0] > 28000                       # 4 lanes x 8 strided rows, no block of 32 rows
        drop = torch.zeros(m, c, dtype=torch.bool)
        drop[lost] = True
        errs = bn2_sum_errors(r, tag, drop)
        print(tag, "block 1023 into slot 1022: miss / bound: dgamma %.1f dbeta %.1f dy %.1f" % errs)
        assert min(errs) >= 3, errs


def test_planes_pool_resize_mutants():
    """the float checks of the pooling / resize passes on Planes (gap.fwd read through ld4x, bilinear.fwd stored through st4x) with
    the lo or the mid plane lost, on the restatement alone, at every shape of the GPU tests: >= 3 x the bound"""
    for c in (48, 304):
        for hw in ((1, 7), (33, 33)):
            x = R.pool_inputs(3, hw, c)
            want = x.double().mean((1, 2))
            for name, plane in zip(("mid", "lo"), R.split3(x)[1:]):
                err = rel_err((x.double() - plane.double()).mean((1, 2)), want)
                print("gap.fwd hw %d c %d without %s: %.2e (bound %.1e)" % (hw[0] * hw[1], c, name, err, 4 * R.FLOOR["gap.fwd"]))
                assert err >= 12 * R.FLOOR["gap.fwd"], (hw, c, name, err)
    for shape in R.RESIZE_SMALLEST + [R.RESIZE_SHAPES[1]]:
        x, _ = R.resize_inputs(shape, 48)
        ref = R.bilinear_fwd_ref(x, *shape[1])
        for name, plane in zip(("mid", "lo"), R.split3(ref.float())[1:]):
            err = rel_err(ref - plane.double(), ref)
            print("bilinear.fwd %s without %s: %.2e" % (shape, name, err))
            assert err >= 12 * R.FLOOR["bilinear.fwd"], (shape, name, err)
        assert not torch.equal(R.bf16_trunc(ref.float()), R.bf16_rne(ref.float()))          # one plane: truncation is not the rounding


@pytest.mark.parametrize("res", [None, "exact"])
def test_bn2_pattern_mutants(res):
    """the ReLU6 pattern read from the wrong value, on the grid's planted values in the bf16 ulp below 6.  Three planes: the
    pattern is that of the hi plane (truncation: the same as the fp32 value's); a read of the value rounded to nearest sees 6.0
    there.  One plane: the pattern is that of the STORED value, which is the rounded one; a truncating read sees 5.96875.  dres is
    held to equality, dy to its bound"""
    _, refs = bn2_measured()
    r = refs["%s/%s" % (R.grid_tag(6, res), res)]
    f = r["f"]
    out32 = f["out"].float()
    right3, wrong3 = R.bn_act_mask(R.bf16_trunc(out32), 6), R.bn_act_mask(R.bf16_rne(out32), 6)
    assert torch.equal(right3, R.bn_act_mask(out32, 6))
    right1, wrong1 = wrong3, right3
    for right, wrong in ((right3, wrong3), (right1, wrong1)):
        diff = (right != wrong) & (r["dout"] != 0)
        assert int(diff.sum()) >= 8
        for training, q in ((True, "dy"), (False, "dy_eval")):
            a = R.bn_bwd_ref(f, r["gamma"], r["dout"], wrong, training)[0]
            b = R.bn_bwd_ref(f, r["gamma"], r["dout"], right, training)[0]
            assert rel_err(a, b) >= 12 * R.FLOOR["bn2.%s.%s" % (q, R.grid_tag(6, res))]
