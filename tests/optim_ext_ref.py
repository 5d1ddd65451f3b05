"""float64 restatements of what csrc/optim.hip adds to the fused step -- the gradient norm, the clip factor, the clipped SGD /
Adam / AdamW step and the EMA recurrence -- with the seeded inputs and case lists that tests/test_optim_ext_cpu.py (no GPU: the
fp32 floors, the host logic) and tests/test_optim_ext_gpu.py (the kernels and the optimizer classes) share.  The method is that of
tests/streaming_ref.py, whose optimizer configurations and hyper-parameter constants are imported, not copied.

Nothing here calls the product.  The clipped step IS torch.nn.utils.clip_grad_norm_ followed by torch.optim.SGD / Adam / AdamW
on float64 parameters, with the fp32 hyper-parameter values the kernel receives; the EMA is the recurrence
ema_t = ema_{t-1} + w_t (p_t - ema_{t-1}), w_t = float32(1 - d_t), d_t = min(decay, (1 + t) / (10 + t)) (or decay, without
warm-up), written out here and not taken from iswm_amd.optim.

FLOOR holds, per check, the error of torch's OWN fp32 clip + step (and of the same recurrence in fp32 on torch's fp32 weights)
against these restatements on the same inputs, the largest over the check's cases, rounded up to two digits; the GPU tests bound
every float comparison by 4 x FLOOR (rule: docstring of tests/test_streaming_kernels_gpu.py) and tests/test_optim_ext_cpu.py
measures every floor again: a recorded figure above 1.25 x or below half of the measured one fails.
The "big_*" floors (clip and EMA together at 2 097 157 elements) are two to four orders above the small-size ones, and that is
torch's own: its fp32 norm of two million elements is good to ~3e-5, which every clipped quantity inherits, and among two
million Adam elements some have g + wd * p within rounding of zero, where m / sqrt(v) is decided by that rounding and a
whole lr-sized update hangs on it (3e-3 of max |p|).  What holds the kernels' indexing at that size to the bit is the
comparison with the plain kernels in test_second_trip_with_clip_and_ema; a lost or doubled element is an error of order 1.
"""
import numpy as np
import torch

from tests.streaming_ref import ADAM_BETAS, ADAM_CONFIGS, ADAM_EPS, ADAM_LR, SGD_CONFIGS, SGD_LR, f32, gen

# raw kernels: one element, a tail only, one float4, float4 + tail, just under / at / over one workgroup's float4s, and the first
# size at which the 2048-workgroup cap of the grid sends the float4 loop round a second time (with a 1-element tail)
KERNEL_N = [1, 3, 4, 5, 255, 1023, 1025, 2048 * 256 * 4 + 5]
# steps: the raw-kernel sizes below the grid cap (plus 7, a float4 with a 3-element tail), every configuration; the SGD kernels
# walk float4s (1025: a second workgroup), the Adam kernels elements (1025: five workgroups)
STEP_N = [1, 3, 4, 5, 7, 255, 1023, 1025]
# ... and the second trip of the grid-stride loop under the 2048-workgroup cap, with clip AND EMA together, for these
STEP_BIG = KERNEL_N[-1]
BIG_CASES = [("sgd", 0), ("adam", 1), ("adam", 3)]       # (family, index into SGD_CONFIGS / ADAM_CONFIGS): nesterov, L2 Adam, AdamW
BIG_IDS = ["sgd_nesterov", "adam_l2", "adamw"]
STEPS = 3
EMA_DECAY = 0.5                  # the warm-up (1 + t) / (10 + t) reaches it at t = 8
EMA_STEPS_WARM, EMA_STEPS_PLAIN = 12, 3


def step_inputs(n, steps=STEPS):
    g = gen(4000 + n)
    return torch.randn(n, generator=g), [torch.randn(n, generator=g) * 0.5 for _ in range(steps)]


def norm64(*ranges):
    """the L2 norm over all the ranges, float64"""
    return float(np.sqrt(sum(float(np.sum(np.asarray(r, dtype=np.float64) ** 2)) for r in ranges)))


def coef64(norm, max_norm):
    return min(1.0, max_norm / (norm + 1e-6))


def clipping_max_norm(grads):
    """half the first step's norm (so the series clips), as the float32 the kernel is handed"""
    return f32(0.5 * norm64(grads[0].numpy()))


def decay_at(decay, t, warmup):
    return min(decay, (1.0 + t) / (10.0 + t)) if warmup else decay


def ema_weight(decay, t, warmup):
    """slot 3 of the hyper block at EMA update t (1-based): float32(1 - d_t)"""
    return f32(1.0 - decay_at(decay, t, warmup))


def _run(opt, p, grads, dtype, max_norm, ema, before_step=None):
    """steps `opt` over `grads`; -> (norms before clipping, ema or None).  ema = (decay, warmup) or None"""
    norms = []
    avg = p.detach().clone() if ema is not None else None
    for t, g in enumerate(grads, 1):
        p.grad = g.to(dtype).clone()
        if max_norm is not None:
            norms.append(float(torch.nn.utils.clip_grad_norm_([p], max_norm)))
        if before_step is not None:
            before_step(p)
        opt.step()
        if ema is not None:
            avg += ema_weight(ema[0], t, ema[1]) * (p.detach() - avg)
    return norms, avg


def sgd_ext_ref(p0, grads, cfg, max_norm=None, ema=None, dtype=torch.float64):
    """-> dict(p, buf, norms, ema); the buffer convention at momentum 0 is streaming_ref.sgd_ref's (g + wd * p of the last step)"""
    mu, nesterov, wd = f32(cfg[0]), cfg[1], f32(cfg[2])
    p = torch.nn.Parameter(p0.to(dtype).clone())
    opt = torch.optim.SGD([p], lr=SGD_LR, momentum=mu, weight_decay=wd, nesterov=nesterov)
    last = {}

    def keep(q):
        last["buf"] = (q.grad + wd * q.detach()).clone()
    norms, avg = _run(opt, p, grads, dtype, max_norm, ema, keep if mu == 0 else None)
    buf = last["buf"] if mu == 0 else opt.state[p]["momentum_buffer"]
    return dict(p=p.detach().clone(), buf=buf.detach().clone(), norms=norms, ema=avg)


def adam_ext_ref(p0, grads, cfg, max_norm=None, ema=None, dtype=torch.float64):
    decoupled, wd = cfg
    p = torch.nn.Parameter(p0.to(dtype).clone())
    cls = torch.optim.AdamW if decoupled else torch.optim.Adam
    opt = cls([p], lr=ADAM_LR, betas=ADAM_BETAS, eps=ADAM_EPS, weight_decay=f32(wd))
    norms, avg = _run(opt, p, grads, dtype, max_norm, ema)
    st = opt.state[p]
    return dict(p=p.detach().clone(), m=st["exp_avg"].detach().clone(), v=st["exp_avg_sq"].detach().clone(), norms=norms,
                ema=avg)


def adam_hyper(t, w=0.0):
    """the hyper block of step t (1-based): [lr, 1 - b1^t, 1 - b2^t, 1 - d_t]"""
    return [ADAM_LR, 1.0 - ADAM_BETAS[0] ** t, 1.0 - ADAM_BETAS[1] ** t, w]


def big_case(family, index, dtype=torch.float64):
    """(cfg, p0, grads, max_norm, restatement) of a BIG_CASES entry: three steps at STEP_BIG with clipping (half the first norm)
    and EMA (EMA_DECAY, warm-up) together"""
    cfg = (SGD_CONFIGS if family == "sgd" else ADAM_CONFIGS)[index]
    p0, grads = step_inputs(STEP_BIG)
    mx = clipping_max_norm(grads)
    ref = (sgd_ext_ref if family == "sgd" else adam_ext_ref)(p0, grads, cfg, mx, (EMA_DECAY, True), dtype)
    return cfg, p0, grads, mx, ref


SGD_IDS = ["mu%g_nesterov%d_wd%g" % (c[0], c[1], c[2]) for c in SGD_CONFIGS]
ADAM_IDS = ["%s_wd%g" % ("decoupled" if c[0] else "l2", c[1]) for c in ADAM_CONFIGS]
EMA_SERIES = [(EMA_STEPS_WARM, True), (EMA_STEPS_PLAIN, False)]          # (steps, warm-up)

# fp32 floors (see the module docstring); measured by tests/test_optim_ext_cpu.py
FLOOR = {
    "big_adam.ema": 3.0e-3,
    "big_adam.m": 1.5e-4,
    "big_adam.p": 3.1e-3,
    "big_adam.v": 5.6e-5,
    "big_sgd.buf": 2.9e-5,
    "big_sgd.ema": 1.5e-6,
    "big_sgd.p": 1.8e-6,
    "clip_adam.m": 2.3e-7,
    "clip_adam.p": 1.7e-7,
    "clip_adam.v": 2.7e-7,
    "clip_sgd.buf": 2.5e-7,
    "clip_sgd.p": 1.0e-7,
    "ema_adam.ema": 4.3e-7,
    "ema_sgd.ema": 2.5e-7,
}
