"""float64 restatements of the streaming (non-MFMA) kernels -- csrc/loss.hip, resize.hip, dwconv.hip, optim.hip, pool.hip, misc.hip
and the plain passes of bn.hip -- with the seeded inputs and the case lists that tests/test_streaming_ref_cpu.py (no GPU: ties
every restatement to an independent authority and measures the fp32 floors) and tests/test_streaming_kernels_gpu.py (the
kernels themselves) share.

Nothing here calls the product: numpy and torch float64 on the CPU only.  Each function writes the operation's mathematical
definition out again (the formulas of the kernels' header comments), not the kernels' code.

FLOOR holds, per check, the error of torch's OWN fp32 implementation of the same operation against these restatements on the
same inputs (largest over the check's cases, single-threaded CPU, rounded up to two digits); the GPU tests bound every float
comparison by 4 x FLOOR (rule and reasons: docstring of tests/test_streaming_kernels_gpu.py).  test_streaming_ref_cpu.py
measures every floor again and fails if a recorded figure is above 1.25 x or below half of what it measures.
One exception to "torch's own": the focal modes (loss.value / loss.grad .m1, .m2).  Autograd through pow gives nan at the
ce == 0 pixels that logits of magnitude 30 produce, so their floor is loss_ref's closed form evaluated in fp32 on torch's fp32
log_softmax -- an fp32 evaluation of the same formula, not an independent kernel.  Mode 0 is F.cross_entropy with autograd.
Two more, both in the second BatchNorm table (bn2.*).  (1) bn2.dgamma / bn2.dbeta where the reduce pass adds fp32 runs (more than
8192 rows: rows8193, rows8193_plain, runs, tilecap): ATen accumulates these sums in double, which is no fp32 floor for such a kernel, so the floor
is tests/bn_partials_ref.bwd_sums(dtype=float32) on the same inputs -- products in fp32, runs of at most RUN rows added in fp32,
the runs in double.  (2) bn2.dy.* of the cases whose statistics are GIVEN (walk*, fallback, grid): the training-mode dy on
statistics that are not the batch's is the derivative of nothing autograd can be handed, so the floor is bn_dy_train_fp32, the
closed form in fp32; their out, eval-mode dy_eval, dgamma and dbeta are F.batch_norm(training=False) with autograd.
"""
import numpy as np
import torch
import torch.nn.functional as F


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f32(v):
    """the value a C float argument carries, as a Python float"""
    return float(np.float32(v))


# ======================================================================================================================
# loss: weighted cross-entropy (mode 0), focal mean over ALL pixels (mode 1), focal sum (mode 2)
# ======================================================================================================================
LOSS_SHAPES = {"tiny": (1, 5, 5), "small": (3, 13, 11), "lanes": (2, 193, 193)}
# (C, label dtype, mode, alpha, gamma, class weights, upstream scalar, shape)
LOSS_CASES = [
    (3, "i64", 0, 1.0, 0.0, False, 1.0, "tiny"),
    (3, "u8", 1, 0.25, 2.0, True, 0.37, "tiny"),
    (3, "i64", 2, 1.0, 0.5, True, 1.0, "tiny"),
    (2, "u8", 0, 1.0, 0.0, True, 1.0, "small"),
    (2, "i64", 1, 0.25, 2.0, False, 0.37, "small"),
    (2, "u8", 2, 1.0, 0.5, False, 1.0, "small"),
    (8, "i64", 0, 1.0, 0.0, True, 0.37, "small"),
    (8, "u8", 1, 1.0, 0.5, False, 1.0, "small"),
    (8, "i64", 2, 0.25, 2.0, True, 1.0, "small"),
    (8, "u8", 2, 1.0, 0.0, False, 1.0, "small"),
    (9, "u8", 0, 1.0, 0.0, False, 1.0, "small"),
    (9, "i64", 1, 0.25, 2.0, True, 1.0, "small"),
    (9, "u8", 2, 1.0, 0.5, True, 0.37, "small"),
    (21, "i64", 0, 1.0, 0.0, True, 1.0, "small"),
    (21, "u8", 1, 1.0, 0.5, True, 0.37, "small"),
    (21, "i64", 2, 0.25, 2.0, False, 1.0, "small"),
    (2, "u8", 0, 1.0, 0.0, True, 0.37, "lanes"),
    (3, "i64", 1, 0.25, 2.0, True, 1.0, "lanes"),
    (9, "i64", 2, 1.0, 0.5, False, 1.0, "lanes"),
    (21, "u8", 0, 1.0, 0.0, False, 0.37, "lanes"),
]
LOSS_IDS = ["c%d_%s_m%d_a%g_g%g_%s_up%g_%s" % (c[0], c[1], c[2], c[3], c[4], "w" if c[5] else "now", c[6], c[7]) for c in LOSS_CASES]
LOSS_CAP_SHAPE = (2, 2049, 2049)          # 8 396 802 pixels > 8192 blocks x 1024: a second trip through the grid-stride loop
IGNORE = 255


def loss_inputs(c, label_kind, shape, seed=0, scale=30.0):
    """(logits fp32 [B,C,H,W] = randn * scale, labels, class weights fp32 [C]): ~5 % of the labels are IGNORE; int64 labels also
    carry a few -1 and C + 1, uint8 labels a few values in [C, 254] (all of which the kernel treats as ignored)"""
    b, h, w = shape
    g = gen(1000 + 7 * c + seed)
    logits = torch.randn(b, c, h, w, generator=g) * scale
    labels = torch.randint(0, c, (b, h, w), generator=g)
    r = torch.rand(b, h, w, generator=g)
    labels[r < 0.05] = IGNORE
    flat = labels.view(-1)
    n = flat.numel()
    if label_kind == "i64":
        flat[1 % n] = -1
        flat[(n // 3) % n] = -1
        flat[(n // 2) % n] = c + 1
        flat[n - 1] = c + 1
    else:
        flat[1 % n] = c
        flat[(n // 3) % n] = 254
        flat[(n // 2) % n] = min(c + 17, 254)
        labels = labels.to(torch.uint8)
    weight = torch.rand(c, generator=g) * 2 + 0.5
    return logits, labels, weight


def loss_ref(logits, labels, weight, ignore_index, alpha, gamma, mode, dtype=torch.float64, log_softmax=None):
    """(value, sums = [sum of the per-pixel terms, sum of the weights of the valid pixels], dL/dlogits) of
         mode 0   sum_i w[y_i] nll_i / sum_i w[y_i]                         over the valid pixels
         mode 1   mean over ALL pixels of f_i,  f = alpha (1 - pt)^gamma ce,  ce = w[y] nll (0 if invalid),  pt = exp(-ce)
         mode 2   sum_i f_i
    a label is valid iff label != ignore_index and 0 <= label < C; an invalid pixel adds no loss, no weight and has an exactly
    zero gradient.  `dtype` / `log_softmax` exist for the fp32 floor of the focal modes, where autograd through pow has no
    finite derivative at ce == 0: the same closed form evaluated in fp32 on torch's own fp32 log_softmax."""
    b, c, h, w = logits.shape
    z = logits.to(dtype).permute(0, 2, 3, 1).reshape(-1, c)
    y = labels.reshape(-1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    logp = (log_softmax or (lambda t: t - torch.logsumexp(t, 1, keepdim=True)))(z)
    nll = -logp.gather(1, yc[:, None])[:, 0]
    wy = weight.to(dtype)[yc] if weight is not None else torch.ones_like(nll)
    zero = torch.zeros_like(nll)
    if mode == 0:
        f, coef = wy * nll, wy
    else:
        ce = wy * nll
        if gamma == 0:
            f, coef = alpha * ce, alpha * wy
        else:
            pt = torch.exp(-ce)
            om = -torch.expm1(-ce)                                   # 1 - pt without the cancellation
            ok = (ce > 0) & (om > 0)
            oms = torch.where(ok, om, torch.ones_like(om))
            f = alpha * om ** gamma * ce
            coef = torch.where(ok, alpha * (oms ** gamma + gamma * oms ** (gamma - 1) * pt * ce), zero) * wy
    f, coef, wy = torch.where(valid, f, zero), torch.where(valid, coef, zero), torch.where(valid, wy, zero)
    s1, s2 = f.sum(), wy.sum()
    npix = z.shape[0]
    value = s1 / s2 if mode == 0 else (s1 / npix if mode == 1 else s1)
    norm = 1.0 / s2 if mode == 0 else (1.0 / npix if mode == 1 else 1.0)
    onehot = F.one_hot(yc, c).to(dtype)
    grad = coef[:, None] * (torch.exp(logp) - onehot) * norm
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return value, torch.stack([s1, s2]), grad.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous()


def loss_valid(labels, c, ignore_index=IGNORE):
    y = labels.long()
    return (y != ignore_index) & (y >= 0) & (y < c)


# ======================================================================================================================
# bilinear resize, align_corners=False
# ======================================================================================================================
# (Hi, Wi) -> (Ho, Wo)
RESIZE_SHAPES = [
    ((17, 23), (33, 129)),      # unequal upscale ratios
    ((33, 29), (17, 11)),       # downscale
    ((129, 129), (37, 53)),     # non-integer downscale
    ((13, 40), (65, 7)),        # up on one axis, down on the other
    ((7, 5), (7, 5)),           # identity
    ((1, 1), (9, 13)),          # single input pixel
    ((5, 3), (1, 1)),           # single output pixel
    ((2, 2), (3, 3)),           # small upscale
]
RESIZE_SMALLEST = [RESIZE_SHAPES[7], RESIZE_SHAPES[6]]
RESIZE_CASES = [(s, c) for s in RESIZE_SHAPES for c in (4, 48)] + [(s, 1280) for s in RESIZE_SMALLEST]
RESIZE_IDS = ["%dx%d_to_%dx%d_c%d" % (s[0] + s[1] + (c,)) for s, c in RESIZE_CASES]
RESIZE_NCHW = [(2, 4), (5, 8), (21, 24), (2, 8)]         # (C, cp)
RESIZE_N = 2


def resize_inputs(shape, c, n=RESIZE_N):
    (hi, wi), (ho, wo) = shape
    g = gen(hi * 1000 + wo + c)
    return torch.randn(n, hi, wi, c, generator=g) + 0.3, torch.randn(n, ho, wo, c, generator=g)


def bilinear_index(in_size, out_size):
    """(i0, i1, l0, l1) per output index, the index arithmetic in FLOAT32 as ATen's area_pixel_compute_source_index has it:
    scale = float32(in) / float32(out); src = scale * (dst + 0.5) - 0.5, clamped at 0; i0 = int(src); i1 = i0 + (i0 < in - 1);
    l1 = src - i0; l0 = 1 - l1.  (float64 indices differ from every fp32 implementation by ~7e-6 at 129 -> 37.)
    scale * (dst + 0.5) - 0.5 is ONE fused multiply-add, rounded once: both compilers contract it (ATen's CPU kernels measure
    1e-7 from this form and 1.5e-6 from the twice-rounded one at 17 -> 33).  The float64 product of a float32 scale and
    dst + 0.5 is exact, so rounding the float64 expression to float32 is that fused result."""
    scale = np.float32(in_size) / np.float32(out_size)
    dst = np.arange(out_size, dtype=np.float64)
    src = (np.float64(scale) * (dst + 0.5) - 0.5).astype(np.float32)
    src = np.maximum(src, np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    l0 = (np.float32(1) - l1).astype(np.float32)
    return i0, i1, l0, l1


def bilinear_matrix(in_size, out_size):
    """[out, in] float64 interpolation matrix of one axis"""
    i0, i1, l0, l1 = bilinear_index(in_size, out_size)
    m = np.zeros((out_size, in_size))
    o = np.arange(out_size)
    np.add.at(m, (o, i0), l0.astype(np.float64))
    np.add.at(m, (o, i1), l1.astype(np.float64))
    return torch.from_numpy(m)


def bilinear_fwd_ref(x, ho, wo):
    """x [N, Hi, Wi, C] -> float64 [N, Ho, Wo, C]"""
    _, hi, wi, _ = x.shape
    return torch.einsum("ah,nhwc,bw->nabc", bilinear_matrix(hi, ho), x.double(), bilinear_matrix(wi, wo))


def bilinear_bwd_ref(dy, hi, wi):
    """the transpose: dy [N, Ho, Wo, C] -> float64 [N, Hi, Wi, C]"""
    _, ho, wo, _ = dy.shape
    return torch.einsum("ah,nabc,bw->nhwc", bilinear_matrix(hi, ho), dy.double(), bilinear_matrix(wi, wo))


# ======================================================================================================================
# depthwise convolution
# ======================================================================================================================
# (N, H, W, C, Cw, KH, KW, stride, pad, dil, bias, sliced)
DW_CASES = [
    (2, 13, 17, 24, 24, 5, 5, 1, 2, 1, True, False),       # 5x5, with bias
    (2, 14, 18, 72, 70, 3, 3, 2, 2, 2, False, False),      # stride 2 with dilation 2; Cw < C; second channel block in wgrad
    (1, 9, 9, 8, 8, 3, 3, 1, 0, 1, False, False),          # pad 0
    (2, 7, 9, 16, 16, 1, 1, 2, 0, 1, False, False),        # 1x1, stride 2
    (2, 11, 13, 48, 48, 7, 7, 3, 3, 1, False, False),      # 7x7, stride 3
    (2, 10, 12, 16, 16, 3, 1, 1, 0, 1, False, False),      # KH != KW
    (3, 41, 37, 32, 32, 3, 3, 1, 1, 1, False, False),      # 4 551 output pixels: two chunks, the last ragged
    (2, 14, 18, 72, 70, 3, 3, 2, 2, 2, True, True),        # x, y, dy, dx slices of wider buffers; bias with Cw < C
    (2, 9, 8, 12, 12, 2, 3, 2, 1, 1, False, True),         # even filter height, KH != KW, sliced
]
DW_IDS = ["n%d_%dx%d_c%d_cw%d_k%dx%d_s%d_p%d_d%d%s%s" % (c[:10] + ("_bias" if c[10] else "", "_sliced" if c[11] else ""))
          for c in DW_CASES]


def dw_out_size(h, k, s, p, d):
    return (h + 2 * p - d * (k - 1) - 1) // s + 1


def dw_case(case):
    """seeded NHWC inputs and the float64 results of F.conv2d(groups=Cw) (channels >= Cw: exactly zero)"""
    n, h, w, c, cw, kh, kw, s, p, d, has_bias, _ = case
    g = gen(sum(case[:10]))
    x = torch.randn(n, h, w, c, generator=g) + 0.7
    wt = torch.randn(cw, 1, kh, kw, generator=g) * 0.5 + 0.1
    bias = torch.randn(cw, generator=g) if has_bias else None
    ho, wo = dw_out_size(h, kh, s, p, d), dw_out_size(w, kw, s, p, d)
    dy = torch.randn(n, ho, wo, c, generator=g) + 0.2
    dx0 = torch.randn(n, h, w, c, generator=g)
    r = dw_ref(x, wt, bias, dy, cw, s, p, d, torch.float64)
    r.update(x=x, w=wt, bias=bias, dy=dy, dx0=dx0, ho=ho, wo=wo)
    return r


def dw_ref(x, wt, bias, dy, cw, s, p, d, dtype):
    c = x.shape[3]
    xr = x[..., :cw].permute(0, 3, 1, 2).to(dtype).requires_grad_(True)
    wr = wt.to(dtype).requires_grad_(True)
    y = F.conv2d(xr, wr, None if bias is None else bias.to(dtype), s, p, d, cw)
    y.backward(dy[..., :cw].permute(0, 3, 1, 2).to(dtype))
    pad = lambda t: F.pad(t.detach().permute(0, 2, 3, 1), (0, c - cw))
    return dict(y=pad(y), dx=pad(xr.grad), dw=wr.grad.detach())


# ======================================================================================================================
# optimizers
# ======================================================================================================================
OPT_N = [1, 3, 4, 7, 1023, 4098]
OPT_STEPS = 3
SGD_CONFIGS = [(0.9, True, 1e-4), (0.9, False, 0.0), (0.0, False, 1e-2)]       # (momentum, nesterov, weight decay)
ADAM_CONFIGS = [(False, 0.0), (False, 1e-2), (True, 0.0), (True, 1e-2)]        # (decoupled, weight decay)
SGD_LR, ADAM_LR, ADAM_BETAS, ADAM_EPS = f32(0.05), f32(1e-2), (f32(0.9), f32(0.999)), f32(1e-8)


def opt_inputs(n):
    g = gen(n)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * 0.5 for _ in range(OPT_STEPS)]


def sgd_ref(p0, grads, mu, nesterov, wd, dtype=torch.float64):
    """torch.optim.SGD on `dtype` CPU parameters -> (p, momentum buffer); hyper-parameters are the float32 values the kernel gets.
    With momentum 0 torch keeps no buffer: the kernel's is then g + wd * p of the last step."""
    mu, wd = f32(mu), f32(wd)
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.SGD([p], lr=SGD_LR, momentum=mu, weight_decay=wd, nesterov=nesterov)
    buf = None
    for g in grads:
        p.grad = g.to(dtype).clone()
        if mu == 0:
            buf = (p.grad + wd * p.detach()).clone()
        opt.step()
    if mu != 0:
        buf = opt.state[p]["momentum_buffer"]
    return p.detach().clone(), buf.detach().clone()


def adam_ref(p0, grads, decoupled, wd, dtype=torch.float64):
    """torch.optim.Adam (L2 decay) / AdamW (decoupled decay) -> (p, exp_avg, exp_avg_sq)"""
    p = torch.nn.Parameter(p0.to(dtype).clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=f32(wd))
    for g in grads:
        p.grad = g.to(dtype).clone()
        opt.step()
    st = opt.state[p]
    return p.detach().clone(), st["exp_avg"].detach().clone(), st["exp_avg_sq"].detach().clone()


def adam_hyper(t):
    """what FusedAdam hands the kernel at step t (1-based): [lr, 1 - b1^t, 1 - b2^t, 0]"""
    return [ADAM_LR, 1.0 - ADAM_BETAS[0] ** t, 1.0 - ADAM_BETAS[1] ** t, 0.0]


# ======================================================================================================================
# dropout: Philox4x32-10 (Salmon et al., SC'11; the Random123 definition)
# ======================================================================================================================
DROPOUT_N = [1, 5, 4096, 65539]
DROPOUT_P = [0.0, 0.1, 0.5]
DROPOUT_STREAMS = [(1234, 1), (2 ** 32 + 7, 2 ** 32 + 5), (7, 5)]              # the last two differ in the high words only


def philox4x32_10(ctr, key):
    """ctr [n, 4], key [n, 2] (uint32 values) -> [n, 4] uint32; ten rounds, key bumped by the Weyl constants between rounds"""
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    mask, sh = np.uint64(0xFFFFFFFF), np.uint64(32)
    c = [np.asarray(ctr, dtype=np.uint64)[:, k].copy() for k in range(4)]
    k0, k1 = (np.asarray(key, dtype=np.uint64)[:, k].copy() for k in range(2))
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                                  # 32 x 32 -> 64 bit products: no overflow in uint64
        c = [(p1 >> sh) ^ c[1] ^ k0, p1 & mask, (p0 >> sh) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + w0) & mask, (k1 + w1) & mask
    return np.stack(c, 1).astype(np.uint32)


def dropout_mask_ref(n, p, seed, offset):
    """keep mask (uint8 [n]) of the kernel's stream: counter = (i lo, i hi, offset lo, offset hi) for element group i, key =
    (seed lo, seed hi), element 4 i + k takes word k, u = float32(word >> 8) * 2^-24, keep iff u >= float32(p)"""
    n4 = (n + 3) // 4
    i = np.arange(n4, dtype=np.uint64)
    lo = lambda v: v & np.uint64(0xFFFFFFFF)
    hi = lambda v: v >> np.uint64(32)
    off, sd = np.full(n4, offset, dtype=np.uint64), np.full(n4, seed, dtype=np.uint64)
    words = philox4x32_10(np.stack([lo(i), hi(i), lo(off), hi(off)], 1), np.stack([lo(sd), hi(sd)], 1))
    u = (words >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return (u >= np.float32(p)).astype(np.uint8).reshape(-1)[:n]


def dropout_scale(p):
    return np.float32(1) / (np.float32(1) - np.float32(p))


# ======================================================================================================================
# pooling / broadcast
# ======================================================================================================================
POOL_C = [4, 48, 304]
POOL_HW = [(1, 1), (1, 7), (33, 33)]                   # HW = 1, 7, 1089
POOL_N = [1, 3]
POOL_CASES = [(n, hw, c) for c in POOL_C for hw in POOL_HW for n in POOL_N]
POOL_IDS = ["n%d_hw%d_c%d" % (n, hw[0] * hw[1], c) for n, hw, c in POOL_CASES]
MAXPOOL_CASES = [(1, 9, 4), (9, 1, 4), (7, 6, 304)]


def pool_inputs(n, hw, c):
    return torch.randn(n, hw[0], hw[1], c, generator=gen(n * 100000 + hw[0] * hw[1] * 100 + c)) + 0.5


# ======================================================================================================================
# BatchNorm (training statistics; + residual; + ReLU / ReLU6)
# ======================================================================================================================
BN_STATS = [(100.0, 0.05), (1000.0, 0.5), (30.0, 0.01)]          # (mean, std): |mean| >> std
BN_SHAPES = [(2, 8, 17, 19), (2, 64, 17, 19)]                    # NCHW
# (relu, residual); the second is the last BatchNorm of a ResNet bottleneck (the one ReLU case whose backward reads the pattern
# from the saved output); the last two are MobileNetV2's: ReLU6 after the expand / depthwise BatchNorm, and the projection
# BatchNorm plus the block's identity with no activation
BN_ACTS = [(True, False), (True, True), (6, True), (6, False), (False, True)]
BN_CASES = [(st, sh, act) for st in BN_STATS for sh in BN_SHAPES for act in BN_ACTS]
BN_IDS = ["mean%g_std%g_c%d_relu%d_res%d" % (st[0], st[1], sh[1], int(act[0]), int(act[1])) for st, sh, act in BN_CASES]
BN_EPS = 1e-5


def bn_inputs(stats, shape, res):
    """x NCHW = randn * std + mean (the channel means spread by a few std), gamma, beta, residual, upstream"""
    n, c, h, w = shape
    mean, std = stats
    g = gen(int(mean) + c)
    x = torch.randn(n, c, h, w, generator=g) * std + mean + torch.randn(1, c, 1, 1, generator=g) * 3 * std
    gamma, beta = torch.randn(c, generator=g) * 0.3 + 1, torch.randn(c, generator=g) * 0.1
    resid = torch.randn(n, c, h, w, generator=g) if res else None
    dout = torch.randn(n, c, h, w, generator=g)
    return x, gamma, beta, resid, dout


def bn_act(z, relu):
    return F.relu6(z) if (relu == 6 and relu is not True) else (F.relu(z) if relu else z)


def bn_act_mask(out, relu):
    """where the activation passes the gradient, from its OUTPUT: ReLU out > 0, ReLU6 0 < out < 6"""
    if relu == 6 and relu is not True:
        return (out > 0) & (out < 6)
    return out > 0 if relu else torch.ones_like(out, dtype=torch.bool)


def bn_fwd_ref(x, gamma, beta, resid, relu, mean=None, var=None, eps=BN_EPS):
    """float64 (batch mean, biased variance, unbiased variance, pre-activation z, output) of a BatchNorm over NCHW x; with
    `mean` / `var` given the eval form on those statistics"""
    x = x.double()
    if mean is None:
        mean, var = x.mean((0, 2, 3)), x.var((0, 2, 3), unbiased=False)
    mean, var = mean.double(), var.double()
    m = x.numel() // x.shape[1]
    xhat = (x - mean[None, :, None, None]) / torch.sqrt(var + eps)[None, :, None, None]
    z = xhat * gamma.double()[None, :, None, None] + beta.double()[None, :, None, None]
    if resid is not None:
        z = z + resid.double()
    return dict(mean=mean, var=var, var_unbiased=var * m / max(m - 1, 1), xhat=xhat, z=z, out=bn_act(z, relu))


def bn_bwd_ref(fwd, gamma, dout, mask, training, eps=BN_EPS):
    """closed-form float64 backward with the activation's pass pattern GIVEN (`mask`, bool): (dy, dgamma, dbeta, dres).
         dz = dout * mask; dbeta = sum dz; dgamma = sum dz xhat;
         training: dy = gamma invstd (dz - mean(dz) - xhat mean(dz xhat));   eval: dy = gamma invstd dz
    The pattern is an input because two fp32 evaluations may decide an output within rounding of 0 (or 6) differently; the
    tests bound where the patterns may differ."""
    dz = dout.double() * mask.double()
    xhat = fwd["xhat"]
    dbeta, dgamma = dz.sum((0, 2, 3)), (dz * xhat).sum((0, 2, 3))
    m = dz.numel() // dz.shape[1]
    k = (gamma.double() / torch.sqrt(fwd["var"] + eps))[None, :, None, None]
    if training:
        dy = k * (dz - dbeta[None, :, None, None] / m - xhat * dgamma[None, :, None, None] / m)
    else:
        dy = k * dz
    return dy, dgamma, dbeta, dz


def naive_var_fp32(x):
    """the one-pass fp32 variance E[x^2] - E[x]^2 per channel -- what the kernels must NOT be (discrimination check only)"""
    x = x.float()
    return ((x * x).mean((0, 2, 3)) - x.mean((0, 2, 3)) ** 2).double()


# ======================================================================================================================
# BatchNorm, second table ("bn2"): the row / column structure of the passes, the planes forms and the one-plane mode, all at
# ordinary statistics (mean about 0.5, std about 2) -- the large-mean floors above are 2.7e-5 .. 9.9e-5, too wide to see a lost plane
# ======================================================================================================================
BN2_STATS = (0.5, 2.0)
SENTINEL = 7.0                  # every output buffer of a bn2 check holds this (in every plane) before the kernel runs
BN_DBL_ROWS = 8192              # bn.hip, bn_backward_impl: the reduce pass works in double throughout for M <= 8192 ...
BN_RUN = 8                      # ... and above adds fp32 runs of 8 of a thread's rows, each flushed into double
COLSTAT_TILE_CAP = 1024         # iswm_colstat_tiles: min(1024, ceil(M / 32))
BN_FINALIZE16_TILES = 32        # k_bn_bwd_finalize<double, 16> up to 32 tiles, <double, 4> above


def plan_rows(m, c, fixed=0):
    """rowmap.h plan_rows(M, C, fixed_rowblocks), restated; last_groups = float4 groups of the last column block"""
    c4 = c // 4
    cq = min(c4, 256)
    rl = 256 // cq
    colblocks = -(-c4 // cq)
    rowblocks = fixed if fixed > 0 else max(1, min(-(-m // (4 * rl)), max(1, 8192 // colblocks)))
    return dict(C4=c4, CQ=cq, RL=rl, colblocks=colblocks, rowblocks=rowblocks, last_groups=c4 - (colblocks - 1) * cq)


def colstat_tiles(m):
    return max(1, min(COLSTAT_TILE_CAP, -(-m // 32)))


def walk(m, plan, block, lane):
    """the rows of thread (blockIdx.x = block, row lane = lane): from block * RL + lane in steps of rowblocks * RL"""
    return list(range(block * plan["RL"] + lane, m, plan["rowblocks"] * plan["RL"]))


def walk_lengths(m, plan):
    """the set of row counts over all threads of one column block"""
    step = plan["rowblocks"] * plan["RL"]
    return sorted({max(0, -(-(m - s) // step)) for s in range(step)})


def reduce_structure(m, c):
    """what bn_backward's first pass does at [M, C]: (double throughout?, tiles, plan, row counts per thread, runs of 8 per thread)"""
    tiles = colstat_tiles(m)
    plan = plan_rows(m, c, tiles)
    rows = walk_lengths(m, plan)
    return dict(dbl=m <= BN_DBL_ROWS, tiles=tiles, plan=plan, rows=rows, runs=sorted({-(-r // BN_RUN) for r in rows}),
                finalize=16 if tiles <= BN_FINALIZE16_TILES else 4)


def bn_apply_form(c, ldy, out, res=None):
    """channels per thread of iswm_bn_apply_pl, the dispatch condition of bn.hip restated.  out / res = (planes 0 | 1 | 3, row pitch,
    channel offset of the slice in a 16-byte aligned buffer, plane stride): 8 (k_bn_apply8) needs a planes output, C, every pitch
    and every three-plane stride a multiple of 8, and 16-byte aligned slices; everything else runs the 4-channel k_bn_apply"""
    def wide(op):
        planes, ld, off, ps = op
        return ld % 8 == 0 and (off * (2 if planes else 4)) % 16 == 0 and (planes != 3 or ps % 8 == 0)
    ok = out[0] != 0 and c % 8 == 0 and ldy % 8 == 0 and wide(out) and (res is None or wide(res))
    return 8 if ok else 4


# statistics from the batch (colstat + bn_finalize).  id -> ((N, H, W), C, (relu, residual), planes); planes: bn_apply writes
# Planes, the backward reads the saved output from them and writes dy as Planes.  What each reaches: BN2_CLAIMS below.
BN2_BATCH = {
    "rows8192": ((1, 64, 128), 16, (True, False), False),
    "rows8193": ((1, 3, 2731), 16, (True, False), False),
    "rows8193_plain": ((1, 3, 2731), 16, (False, True), False),      # no activation + residual (MobileNetV2's projection BatchNorm)
    "runs": ((1, 91, 91), 512, (True, True), True),
    "tilecap": ((1, 182, 182), 256, (6, True), False),
    "cols2": ((1, 1, 37), 1032, (6, False), False),
    "cols2_pl": ((1, 1, 37), 2056, (True, True), True),
}
# given statistics (M = 7 cannot be a training batch): 64 channels, planes out, ReLU + Planes residual; id -> rows
BN2_WALK = {"walk7": 7, "walk33": 33, "walk100": 100}
BN2_WALK_C = 64
# the 4-channel kernel with plane loads and stores next to the 8-channel one, at M = 35 rows, given statistics.
# id -> (C, (out buffer channels, offset), (residual buffer channels, offset), expected channels per thread)
BN2_FALLBACK_ROWS = (1, 5, 7)
BN2_FALLBACK = {
    "c12": (12, (12, 0), (12, 0), 4),                # C % 8 == 4
    "off4": (64, (72, 4), (64, 0), 4),               # output slice 8 bytes past a 16-byte boundary
    "off8": (64, (72, 8), (64, 0), 8),               # the same buffer, aligned slice: the 8-channel kernel
    "ldo76": (64, (76, 8), (64, 0), 4),              # output pitch 76 (and a plane stride of 35 x 76) is no multiple of 8
    "res76": (64, (64, 0), (76, 8), 4),              # residual pitch 76
    "res_off4": (64, (64, 0), (72, 4), 4),           # residual slice misaligned
}


def fallback_tag(fid):
    """the floor keys of a fallback case: one set per channel count -- the five C = 64 geometries run the same inputs"""
    return "fallback_c%d" % BN2_FALLBACK[fid][0]


def grid_tag(relu, res):
    """the floor keys of a grid combination: one set per activation and per residual present / absent"""
    return "grid_relu%d_res%d" % (6 if (relu == 6 and relu is not True) else int(bool(relu)), int(res is not None))


BN2_GRID_SHAPE = (3, 72, 9, 11)                      # NCHW; channels 0..7 are the identity (scale 1, mean 0, beta 0)
BN2_RELUS = [False, True, 6]
# values a bf16 store or a pattern read can get wrong: ties in both parities of the kept bit (1 + 2^-8 rounds down to 1, 1 + 2^-7 + 2^-8
# up to 1.015625; 5.953125 down to 5.9375, 5.984375 up to 6), values in the bf16 ulp below 6 (which round UP to 6.0 but truncate
# to 5.96875), values just above 0, and the clamps' own edges
BF16_EDGE = [1.00390625, 1.01171875, -1.00390625, -1.01171875, 5.953125, 5.984375, 5.99, 5.9999995, 5.97, 5.96875, 6.0, 6.5,
             1e-30, 2.0 ** -126, 1e-3, 0.0, 3.00390625, 3.01171875]


def bf16_trunc(t):
    """the hi plane: fp32 with the low 16 bits cleared"""
    return (t.contiguous().view(torch.int32) & -65536).view(torch.float32)


def bf16_rne(t):
    """the one plane of conv math "bf16": round to nearest even (torch's own conversion), back in fp32"""
    return t.to(torch.bfloat16).float()


def split3(t):
    """(hi, mid, lo) of planes.h: hi + mid + lo == t exactly"""
    hi = bf16_trunc(t)
    r1 = t - hi
    mid = bf16_trunc(r1)
    return hi, mid, bf16_trunc(r1 - mid)


def bn2_batch_inputs(cid):
    (n, h, w), c, (relu, res), planes = BN2_BATCH[cid]
    return bn_inputs(BN2_STATS, (n, c, h, w), True)


def given_stats(c, identity=0):
    """(mean, invstd) fp32 [C] of an eval-mode BatchNorm (the restatement's variance is given_var(invstd)); the first `identity`
    channels are mean 0, invstd 1"""
    g = gen(900 + c)
    mean, var = torch.randn(c, generator=g) * 0.1 + 0.5, torch.rand(c, generator=g) + 3.5
    invstd = 1.0 / torch.sqrt(var)
    mean[:identity], invstd[:identity] = 0.0, 1.0
    return mean, invstd


def given_var(invstd):
    """the float64 variance whose 1 / sqrt(var + eps) is the fp32 invstd the kernels are handed"""
    return 1.0 / invstd.double() ** 2 - BN_EPS


def bn_coef(gamma, beta, mean, invstd):
    """coef [4, C] = (scale, beta, mean, invstd) as iswm_bn_eval_coeffs forms it: scale = fp32(gamma * invstd)"""
    return torch.stack([gamma * invstd, beta, mean, invstd])


def bn2_given_inputs(shape, identity=0):
    """NCHW inputs + given statistics; with `identity` > 0 (the grid) those channels have gamma 1, beta 0, residual 0, x spread
    over [-1, 7] and BF16_EDGE planted, so their output IS act(x) exactly"""
    n, c, h, w = shape
    x, gamma, beta, resid, dout = bn_inputs(BN2_STATS, shape, True)
    mean, invstd = given_stats(c, identity)
    if identity:
        gamma[:identity], beta[:identity] = 1.0, 0.0
        resid[:, :identity] = 0.0
        x[:, :identity] = torch.rand(n, identity, h, w, generator=gen(77)) * 8 - 1
        edge = torch.tensor(BF16_EDGE)
        for k in range(identity):
            flat = x[:, k].reshape(-1)
            flat[k:k + 3 * edge.numel():3] = edge.roll(k)
            x[:, k] = flat.view(n, h, w)
    return x, gamma, beta, resid, dout, mean, invstd


def bn_dy_train_fp32(x, mean, invstd, gamma, dz, dgamma64, dbeta64):
    """the training-mode dy of bn_bwd_ref evaluated in fp32 on GIVEN statistics and fp32-rounded sums: the floor where the
    statistics are not the batch's, so that autograd has no such function"""
    m = x.numel() // x.shape[1]
    b = lambda t: t.float()[None, :, None, None]
    xhat = (x - b(mean)) * b(invstd)
    return b(gamma) * b(invstd) * (dz - b(dbeta64 / m) - xhat * b(dgamma64 / m))


# ======================================================================================================================
# fp32 floors (see the module docstring); measured by tests/test_streaming_ref_cpu.py
# ======================================================================================================================
FLOOR = {
    "adam.m": 1.0e-7,
    "adam.p": 1.8e-7,
    "adam.v": 1.3e-7,
    "bcast.bwd": 1.6e-7,
    "bilinear.bwd": 5.0e-7,
    "bilinear.fwd": 1.1e-7,
    "bilinear_nchw.bwd": 7.8e-7,
    "bilinear_nchw.fwd": 1.2e-7,
    "bn.dbeta.mean100": 2.3e-7,
    "bn.dbeta.mean1000": 2.4e-7,
    "bn.dbeta.mean30": 1.6e-7,
    "bn.dgamma.mean100": 5.5e-5,
    "bn.dgamma.mean1000": 5.5e-5,
    "bn.dgamma.mean30": 9.9e-5,
    "bn.dy.mean100": 3.6e-6,
    "bn.dy.mean1000": 2.4e-6,
    "bn.dy.mean30": 6.2e-6,
    "bn.mean.mean100": 3.8e-8,
    "bn.mean.mean1000": 3.0e-8,
    "bn.mean.mean30": 3.2e-8,
    "bn.out.mean100": 2.7e-5,
    "bn.out.mean1000": 2.6e-5,
    "bn.out.mean30": 6.7e-5,
    "bn.var.mean100": 7.4e-8,
    "bn.var.mean1000": 7.3e-8,
    "bn.var.mean30": 9.0e-8,
    "bn2.dbeta.cols2": 1.2e-7,
    "bn2.dbeta.cols2_pl": 6.8e-8,
    "bn2.dbeta.fallback_c12": 1.8e-7,
    "bn2.dbeta.fallback_c64": 1.5e-7,
    "bn2.dbeta.grid_relu0_res0": 9.7e-8,
    "bn2.dbeta.grid_relu0_res1": 9.7e-8,
    "bn2.dbeta.grid_relu1_res0": 1.1e-7,
    "bn2.dbeta.grid_relu1_res1": 8.6e-8,
    "bn2.dbeta.grid_relu6_res0": 8.7e-8,
    "bn2.dbeta.grid_relu6_res1": 7.0e-8,
    "bn2.dbeta.rows8192": 3.0e-7,
    "bn2.dbeta.rows8193": 3.2e-8,
    "bn2.dbeta.rows8193_plain": 4.0e-8,
    "bn2.dbeta.runs": 5.7e-8,
    "bn2.dbeta.tilecap": 5.9e-8,
    "bn2.dbeta.walk100": 1.2e-7,
    "bn2.dbeta.walk33": 6.6e-8,
    "bn2.dbeta.walk7": 6.4e-8,
    "bn2.dgamma.cols2": 1.7e-7,
    "bn2.dgamma.cols2_pl": 2.4e-7,
    "bn2.dgamma.fallback_c12": 9.4e-8,
    "bn2.dgamma.fallback_c64": 3.4e-8,
    "bn2.dgamma.grid_relu0_res0": 8.3e-8,
    "bn2.dgamma.grid_relu0_res1": 8.3e-8,
    "bn2.dgamma.grid_relu1_res0": 7.8e-8,
    "bn2.dgamma.grid_relu1_res1": 7.8e-8,
    "bn2.dgamma.grid_relu6_res0": 5.9e-8,
    "bn2.dgamma.grid_relu6_res1": 5.4e-8,
    "bn2.dgamma.rows8192": 4.5e-7,
    "bn2.dgamma.rows8193": 1.8e-7,
    "bn2.dgamma.rows8193_plain": 2.0e-7,
    "bn2.dgamma.runs": 2.2e-7,
    "bn2.dgamma.tilecap": 1.1e-7,
    "bn2.dgamma.walk100": 1.1e-7,
    "bn2.dgamma.walk33": 9.5e-8,
    "bn2.dgamma.walk7": 3.7e-8,
    "bn2.dy.cols2": 1.2e-7,
    "bn2.dy.cols2_pl": 9.3e-8,
    "bn2.dy.fallback_c12": 7.8e-8,
    "bn2.dy.fallback_c64": 1.2e-7,
    "bn2.dy.grid_relu0_res0": 8.6e-8,
    "bn2.dy.grid_relu0_res1": 8.6e-8,
    "bn2.dy.grid_relu1_res0": 8.6e-8,
    "bn2.dy.grid_relu1_res1": 8.6e-8,
    "bn2.dy.grid_relu6_res0": 1.1e-7,
    "bn2.dy.grid_relu6_res1": 8.1e-8,
    "bn2.dy.rows8192": 1.1e-7,
    "bn2.dy.rows8193": 1.4e-7,
    "bn2.dy.rows8193_plain": 1.6e-7,
    "bn2.dy.runs": 1.5e-7,
    "bn2.dy.tilecap": 1.5e-7,
    "bn2.dy.walk100": 7.6e-8,
    "bn2.dy.walk33": 1.1e-7,
    "bn2.dy.walk7": 1.4e-7,
    "bn2.dy_eval.fallback_c12": 5.6e-8,
    "bn2.dy_eval.fallback_c64": 5.5e-8,
    "bn2.dy_eval.grid_relu0_res0": 6.1e-8,
    "bn2.dy_eval.grid_relu0_res1": 6.1e-8,
    "bn2.dy_eval.grid_relu1_res0": 6.1e-8,
    "bn2.dy_eval.grid_relu1_res1": 6.1e-8,
    "bn2.dy_eval.grid_relu6_res0": 6.1e-8,
    "bn2.dy_eval.grid_relu6_res1": 6.1e-8,
    "bn2.dy_eval.walk100": 6.8e-8,
    "bn2.dy_eval.walk33": 6.2e-8,
    "bn2.dy_eval.walk7": 4.4e-8,
    "bn2.out.cols2": 1.3e-7,
    "bn2.out.cols2_pl": 1.5e-7,
    "bn2.out.fallback_c12": 5.5e-8,
    "bn2.out.fallback_c64": 1.0e-7,
    "bn2.out.grid_relu0_res0": 5.3e-8,
    "bn2.out.grid_relu0_res1": 7.2e-8,
    "bn2.out.grid_relu1_res0": 6.2e-8,
    "bn2.out.grid_relu1_res1": 9.9e-8,
    "bn2.out.grid_relu6_res0": 7.9e-8,
    "bn2.out.grid_relu6_res1": 1.2e-7,
    "bn2.out.rows8192": 7.5e-8,
    "bn2.out.rows8193": 9.7e-8,
    "bn2.out.rows8193_plain": 1.3e-7,
    "bn2.out.runs": 1.1e-7,
    "bn2.out.tilecap": 2.3e-7,
    "bn2.out.walk100": 5.7e-8,
    "bn2.out.walk33": 7.1e-8,
    "bn2.out.walk7": 9.0e-8,
    "bn_eval.dbeta": 1.5e-7,
    "bn_eval.dgamma": 7.0e-8,
    "bn_eval.dy": 7.8e-8,
    "bn_eval.out": 6.2e-8,
    "dw.dw": 2.8e-6,
    "dw.dx": 1.5e-7,
    "dw.dx_acc": 1.4e-7,
    "dw.y": 2.8e-7,
    "gap.bwd": 5.3e-8,
    "gap.bwd_acc": 5.7e-8,
    "gap.fwd": 2.0e-7,
    "loss.cap.grad": 2.0e-7,
    "loss.cap.value": 8.6e-8,
    "loss.grad.m0": 3.4e-7,
    "loss.grad.m1": 2.6e-7,
    "loss.grad.m2": 2.6e-7,
    "loss.sums": 9.3e-8,
    "loss.value.m0": 1.2e-7,
    "loss.value.m1": 1.1e-7,
    "loss.value.m2": 7.3e-8,
    "maxpool.dx": 7.2e-8,
    "sgd.buf": 1.1e-7,
    "sgd.p": 1.1e-7,
}
