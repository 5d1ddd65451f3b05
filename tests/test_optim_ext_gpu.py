"""Gradient-norm clipping and EMA weights inside the fused optimizer step, on the GPU: the norm / finalize / extended-step / swap
kernels of csrc/optim.hip against the float64 restatements of tests/optim_ext_ref.py, and the optimizer classes, train and predict
on top of them.

Bounds.  A float comparison with a restatement is rel_err <= 4 x FLOOR[check] (tests/optim_ext_ref.py; the rule and its reasons
are in the docstring of tests/test_streaming_kernels_gpu.py).  The norm is held to ONE fp32 ulp of float32(float64 norm): double
accumulation of fewer than 2^26 terms errs by less than 2^-27 relative, under half an fp32 ulp, and the single rounding to fp32
gives the ulp; the double sum itself is held to that 2^-27.  The clip factor is an fp32 add and an IEEE fp32 divide of the
returned norm, both correctly rounded, so it is compared for equality with numpy's.  Everything that must be "the same" --
coef == 1 against the plain kernels, an EMA run against a run without, the restored weights, resume, a frozen parameter, the
gradient arena -- is compared bit for bit."""
import glob
import io
import os

import numpy as np
import pytest
import torch

from tests import optim_ext_ref as X
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same_bits(a, b):
    return tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


def check(key, actual, expected, what=""):
    floor = X.FLOOR[key]
    err = rel_err(actual.detach().cpu().reshape(expected.shape), expected)
    line = "%-14s floor %.1e  bound %.1e  measured %.2e  %s" % (key, floor, 4 * floor, err, what)
    print(line)
    assert err <= 4 * floor, line


# ---- the norm and the clip factor ------------------------------------------------------------------------------------
def run_norm(ranges, max_norm, state=None):
    """-> (sum of squares float64, norm float32, coef float32) of the kernels over `ranges` (device tensors)"""
    from iswm_amd import ops
    slots, clip = state if state is not None else ops.new_clip_state(dev())
    for k, r in enumerate(ranges):
        ops.grad_sqnorm(r, slots, accumulate=k > 0)
    ops.clip_finalize(slots, max_norm, clip)
    host = clip.cpu().numpy()
    return float(ops.clip_sumsq(clip).cpu()), host[ops.CLIP_NORM], host[ops.CLIP_COEF]


def check_norm(ranges_host, max_norm, state=None, what=""):
    ranges = [r.to(dev()) for r in ranges_host]
    sumsq, norm, coef = run_norm(ranges, max_norm, state)
    ref = X.norm64(*[r.numpy() for r in ranges_host])
    ref32 = np.float32(ref)
    ulp = float(np.spacing(ref32)) if ref > 0 else 0.0
    print("norm %-28s kernel %.9e  float64 %.9e  ulps %.2f" % (what, norm, ref, abs(float(norm) - float(ref32)) / ulp if ulp else 0))
    assert np.isfinite(norm) and abs(float(norm) - float(ref32)) <= ulp, (what, norm, ref)
    assert abs(sumsq - ref * ref) <= 2.0 ** -27 * ref * ref + 2.0 ** -52 * ref * ref, (what, sumsq, ref * ref)
    want = np.float32(max_norm) / (norm + np.float32(1e-6))
    want = want if want < 1 else np.float32(1)
    assert coef == want and coef.dtype == np.float32, (what, coef, want)
    return sumsq, norm, coef


@pytest.mark.parametrize("n", X.KERNEL_N)
def test_norm_value(n):
    g = torch.randn(n, generator=X.gen(n)) * 3
    _, norm, coef = check_norm([g], X.f32(0.5 * X.norm64(g.numpy())), what="n=%d" % n)
    assert 0.49 < coef < 0.51
    _, _, coef = check_norm([g], 1e9, what="n=%d far bound" % n)
    assert coef == 1
    sumsq, norm, coef = check_norm([torch.zeros(n)], 1.0, what="n=%d zeros" % n)
    assert sumsq == 0 and norm == 0 and coef == 1
    # squares that overflow fp32 (1e40): finite and right in double
    check_norm([torch.full((n,), 1e20)], 1.0, what="n=%d of 1e20" % n)


def test_norm_over_several_ranges_and_stale_slots():
    from iswm_amd import ops
    big = X.KERNEL_N[-1]
    parts = [torch.randn(n, generator=X.gen(50 + n)) for n in (1023, 5, big, 1025)]
    state = ops.new_clip_state(dev())
    check_norm(parts[:2] + parts[3:], 0.5, state, "small, smaller, larger grid")
    check_norm(parts, 0.5, state, "the full grid in the middle")
    check_norm(parts[2:], 0.5, state, "full grid first")
    check_norm(parts[1:2], 0.5, state, "one workgroup after a full grid")       # the other 2047 slots must be zero again


def test_norm_is_deterministic():
    from iswm_amd import ops
    for n in (1025, X.KERNEL_N[-1]):
        g = (torch.randn(n, generator=X.gen(7)) * 3).to(dev())
        h = torch.randn(1023, generator=X.gen(8)).to(dev())
        runs = [run_norm([g, h], 0.25, st) for st in (None, None, ops.new_clip_state(dev()))]
        for r in runs[1:]:
            assert np.float64(r[0]).tobytes() == np.float64(runs[0][0]).tobytes()
            assert r[1].tobytes() == runs[0][1].tobytes() and r[2].tobytes() == runs[0][2].tobytes()


def test_nonfinite_norm_propagates():
    g = torch.randn(1025, generator=X.gen(1))
    g[77] = float("nan")
    _, norm, coef = run_norm([g.to(dev())], 1.0)
    assert np.isnan(norm) and np.isnan(coef)
    g[77] = float("inf")
    _, norm, coef = run_norm([g.to(dev())], 1.0)
    assert np.isinf(norm) and coef == 0


# ---- the clipped step, raw kernels -----------------------------------------------------------------------------------
def clip_block(g, max_norm, state):
    from iswm_amd import ops
    ops.grad_sqnorm(g, state[0])
    ops.clip_finalize(state[0], max_norm, state[1])
    return state[1]


@pytest.mark.parametrize("n", X.STEP_N)
@pytest.mark.parametrize("cfg", X.SGD_CONFIGS, ids=X.SGD_IDS)
def test_clipped_sgd_step(cfg, n):
    from iswm_amd import ops
    mu, nesterov, wd = cfg
    p0, grads = X.step_inputs(n)
    d = dev()
    lr = torch.tensor([X.SGD_LR, 0, 0, 0], dtype=torch.float32, device=d)
    state = ops.new_clip_state(d)
    # a bound of half the first norm: clips
    mx = X.clipping_max_norm(grads)
    p, buf = p0.to(d), torch.zeros(n, device=d)
    coefs = []
    for g in grads:
        gd = g.to(d)
        clip = clip_block(gd, mx, state)
        ops.sgd_step_ex(p, gd, buf, lr, mu, wd, nesterov, clip=clip)
        coefs.append(float(clip[ops.CLIP_COEF]))
        assert same_bits(gd, g), "the gradient arena must stay unclipped"
    ref = X.sgd_ext_ref(p0, grads, cfg, mx)
    assert coefs[0] < 1 and abs(coefs[0] - X.coef64(ref["norms"][0], mx)) < 1e-6
    check("clip_sgd.p", p, ref["p"])
    check("clip_sgd.buf", buf, ref["buf"])
    # a bound far above the norm: coef == 1 and the plain kernel's bits
    p, buf, q, qbuf = p0.to(d), torch.zeros(n, device=d), p0.to(d), torch.zeros(n, device=d)
    for g in grads:
        gd = g.to(d)
        clip = clip_block(gd, 1e9, state)
        ops.sgd_step_ex(p, gd, buf, lr, mu, wd, nesterov, clip=clip)
        ops.sgd_step(q, gd, qbuf, lr, mu, wd, nesterov)
        assert float(clip[ops.CLIP_COEF]) == 1.0
    assert same_bits(p, q) and same_bits(buf, qbuf)
    # neither operand: the plain kernel's bits too
    r, rbuf = p0.to(d), torch.zeros(n, device=d)
    for g in grads:
        ops.sgd_step_ex(r, g.to(d), rbuf, lr, mu, wd, nesterov)
    assert same_bits(r, q) and same_bits(rbuf, qbuf)


@pytest.mark.parametrize("n", X.STEP_N)
@pytest.mark.parametrize("cfg", X.ADAM_CONFIGS, ids=X.ADAM_IDS)
def test_clipped_adam_step(cfg, n):
    from iswm_amd import ops
    decoupled, wd = cfg
    p0, grads = X.step_inputs(n)
    d = dev()
    state = ops.new_clip_state(d)
    hypers = [torch.tensor(X.adam_hyper(t), dtype=torch.float32, device=d) for t in range(1, len(grads) + 1)]
    args = (X.ADAM_BETAS[0], X.ADAM_BETAS[1], X.ADAM_EPS, wd, decoupled)
    mx = X.clipping_max_norm(grads)
    p, m, v = p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)
    coefs = []
    for g, hyper in zip(grads, hypers):
        gd = g.to(d)
        clip = clip_block(gd, mx, state)
        ops.adam_step_ex(p, gd, m, v, hyper, *args, clip=clip)
        coefs.append(float(clip[ops.CLIP_COEF]))
        assert same_bits(gd, g), "the gradient arena must stay unclipped"
    ref = X.adam_ext_ref(p0, grads, cfg, mx)
    assert coefs[0] < 1 and abs(coefs[0] - X.coef64(ref["norms"][0], mx)) < 1e-6
    check("clip_adam.p", p, ref["p"])
    check("clip_adam.m", m, ref["m"])
    check("clip_adam.v", v, ref["v"])
    a, b, c = ([p0.to(d), torch.zeros(n, device=d), torch.zeros(n, device=d)] for _ in range(3))
    for g, hyper in zip(grads, hypers):
        gd = g.to(d)
        clip = clip_block(gd, 1e9, state)
        ops.adam_step_ex(a[0], gd, a[1], a[2], hyper, *args, clip=clip)
        ops.adam_step(b[0], gd, b[1], b[2], hyper, *args)
        ops.adam_step_ex(c[0], gd, c[1], c[2], hyper, *args)
        assert float(clip[ops.CLIP_COEF]) == 1.0
    for k in range(3):
        assert same_bits(a[k], b[k]) and same_bits(c[k], b[k]), k


# ---- the second trip of the grid-stride loop: clip and EMA together at 2048 * 256 * 4 + 5 ------------------------------------
@pytest.mark.parametrize("family,index", X.BIG_CASES, ids=X.BIG_IDS)
def test_second_trip_with_clip_and_ema(family, index):
    """the extended kernels where stream_grid's 2048-workgroup cap sends a thread round its loop again (SGD: the float4 loop's
    second trip is one float4, then a 1-element tail; Adam: four trips over elements): a clipped series with EMA against float64,
    then coef == 1 with EMA, EMA alone, and no operand, each against the plain kernel bit for bit"""
    from iswm_amd import ops
    cfg, p0, grads, mx, ref = X.big_case(family, index)
    n, d = X.STEP_BIG, dev()
    assert n // 4 > 2048 * 256 and n % 4 == 1 and p0.numel() == n
    sgd = family == "sgd"
    nstate = 1 if sgd else 2
    gds = [g.to(d) for g in grads]

    def hyper(t, w):
        h = [X.SGD_LR, 0.0, 0.0, w] if sgd else X.adam_hyper(t, w)
        return torch.tensor(h, dtype=torch.float32, device=d)

    def run(max_norm, with_ema, plain=False):
        """-> ([p, state...], ema or None, coefs) after the three steps"""
        bufs = [p0.to(d)] + [torch.zeros(n, device=d) for _ in range(nstate)]
        ema = p0.to(d) if with_ema else None
        state, coefs = ops.new_clip_state(d), []
        for t, gd in enumerate(gds, 1):
            clip = clip_block(gd, max_norm, state) if max_norm is not None else None
            h = hyper(t, X.ema_weight(X.EMA_DECAY, t, True))
            if sgd:
                args = (cfg[0], cfg[2], cfg[1])
                if plain:
                    ops.sgd_step(bufs[0], gd, bufs[1], h, *args)
                else:
                    ops.sgd_step_ex(bufs[0], gd, bufs[1], h, *args, clip=clip, ema=ema)
            else:
                args = (X.ADAM_BETAS[0], X.ADAM_BETAS[1], X.ADAM_EPS, cfg[1], cfg[0])
                if plain:
                    ops.adam_step(bufs[0], gd, bufs[1], bufs[2], h, *args)
                else:
                    ops.adam_step_ex(bufs[0], gd, bufs[1], bufs[2], h, *args, clip=clip, ema=ema)
            if clip is not None:
                coefs.append(float(clip[ops.CLIP_COEF]))
        return bufs, ema, coefs
    # clip and EMA together against the restatement
    bufs, ema, coefs = run(mx, True)
    assert coefs[0] < 1 and abs(coefs[0] - X.coef64(ref["norms"][0], mx)) < 1e-6
    for key, t in zip(("p", "buf") if sgd else ("p", "m", "v"), bufs):
        check("big_%s.%s" % (family, key), t, ref[key])
    check("big_%s.ema" % family, ema, ref["ema"])
    for gd, g in zip(gds, grads):
        assert same_bits(gd, g), "the gradient arena must stay unclipped"
    # the same steps bit for bit: plain kernel == no operand == coef 1 == EMA alone == coef 1 with EMA; one EMA for both
    plain = run(None, False, plain=True)[0]
    one_ema, ema1, coefs = run(1e9, True)
    assert coefs == [1.0] * len(gds)
    only_ema, ema2, _ = run(None, True)
    for other in (run(None, False)[0], run(1e9, False)[0], one_ema, only_ema):
        for a, b in zip(other, plain):
            assert same_bits(a, b)
    assert same_bits(ema1, ema2) and not same_bits(ema1, plain[0])


# ---- EMA, through the optimizer classes ------------------------------------------------------------------------------
def make_opt(family, params, cfg):
    from iswm_amd import optim
    if family == "sgd":
        return optim.FusedSGD(params, lr=X.SGD_LR, momentum=cfg[0], nesterov=cfg[1], weight_decay=cfg[2])
    cls = optim.FusedAdamW if cfg[0] else optim.FusedAdam
    return cls(params, lr=X.ADAM_LR, betas=X.ADAM_BETAS, eps=X.ADAM_EPS, weight_decay=cfg[1])


def opt_state(opt):
    return [opt._buf] if hasattr(opt, "_buf") else [opt._m, opt._v]


FAMILY_CASES = [("sgd", c) for c in X.SGD_CONFIGS] + [("adam", c) for c in X.ADAM_CONFIGS]
FAMILY_IDS = ["sgd_" + i for i in X.SGD_IDS] + ["adam_" + i for i in X.ADAM_IDS]


@pytest.mark.parametrize("family,cfg", FAMILY_CASES, ids=FAMILY_IDS)
def test_ema_follows_the_restatement(family, cfg):
    d = dev()
    for n in X.STEP_N:
        for steps, warm in X.EMA_SERIES:
            p0, grads = X.step_inputs(n, steps)
            p, q = torch.nn.Parameter(p0.to(d)), torch.nn.Parameter(p0.to(d))
            opt, plain = make_opt(family, [p], cfg), make_opt(family, [q], cfg)
            opt.enable_ema(X.EMA_DECAY, warmup=warm)
            for g in grads:
                p.grad, q.grad = g.to(d), g.to(d)
                opt.step()
                plain.step()
            ref = (X.sgd_ext_ref if family == "sgd" else X.adam_ext_ref)(p0, grads, cfg, ema=(X.EMA_DECAY, warm))
            check("ema_%s.ema" % family, opt._ema[:n], ref["ema"], "n=%d steps=%d warmup=%d" % (n, steps, warm))
            assert opt._ema_updates == steps
            # the step itself is the plain one, bit for bit
            assert same_bits(opt.arena.data, plain.arena.data)
            for a, b in zip(opt_state(opt), opt_state(plain)):
                assert same_bits(a, b)
            sd = opt.ema_state_dict(torch.nn.ParameterList([p]))
            assert sd["num_updates"] == steps and same_bits(sd["params"]["0"], opt._ema[:n])


# ---- segments: a frozen parameter in the middle ----------------------------------------------------------------------
@pytest.mark.parametrize("family,cfg", [("sgd", X.SGD_CONFIGS[0]), ("adam", X.ADAM_CONFIGS[1])], ids=["sgd", "adam"])
def test_frozen_parameter_is_untouched_and_outside_the_norm(family, cfg):
    d = dev()
    n = X.STEP_N[-1]
    p0, grads = X.step_inputs(n)                   # the two live parameters are this case cut in two: 7 + (n - 7) elements
    mid0 = torch.randn(6, generator=X.gen(9))
    cuts = [slice(0, 7), None, slice(7, n)]
    ps = [torch.nn.Parameter(p0[cuts[0]].clone().to(d)), torch.nn.Parameter(mid0.to(d)), torch.nn.Parameter(p0[cuts[2]].clone().to(d))]
    opt = make_opt(family, ps, cfg)
    mx = X.clipping_max_norm(grads)
    opt.set_grad_clip(mx)
    opt.enable_ema(0.9)
    a = opt.arena
    lo, hi = a.offsets[1], a.offsets[2]
    assert (lo, hi) == (8, 16)
    for flat, val in zip(opt_state(opt) + [opt._ema], (7.0, 5.0, 3.0)):        # sentinels in the frozen range
        flat[lo:hi] = val
    before = [t.clone() for t in opt_state(opt) + [opt._ema, a.data]]
    norms = []
    for g in grads:
        opt.zero_grad()
        a.grad[lo:hi] = 100.0                      # a stale gradient in the frozen range must not reach the norm
        ps[0].grad, ps[2].grad = g[cuts[0]].to(d), g[cuts[2]].to(d)
        assert opt._segments() == [(0, lo), (hi, a.numel)]
        opt.step()
        norms.append(float(opt.last_grad_norm))
    for t, b in zip(opt_state(opt) + [opt._ema, a.data], before):
        assert same_bits(t[lo:hi], b[lo:hi])
    assert same_bits(ps[1], mid0)
    ref = (X.sgd_ext_ref if family == "sgd" else X.adam_ext_ref)(p0, grads, cfg, mx)
    for got, want in zip(norms, ref["norms"]):
        w32 = np.float32(want)
        assert abs(got - float(w32)) <= float(np.spacing(w32)), (got, want)
    got = torch.cat([ps[0].detach().reshape(-1), ps[2].detach().reshape(-1)])
    check("clip_%s.p" % family, got, ref["p"])


# ---- swap --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", X.KERNEL_N)
def test_swap_kernel(n):
    from iswm_amd import ops
    g = X.gen(n)
    a0, b0 = torch.randn(n + 3, generator=g), torch.randn(n + 3, generator=g)
    a, b = a0.to(dev()), b0.to(dev())
    ops.swap_f32(a[:n], b[:n])
    assert same_bits(a[:n], b0[:n]) and same_bits(b[:n], a0[:n])
    assert same_bits(a[n:], a0[n:]) and same_bits(b[n:], b0[n:])               # nothing past the range


def test_ema_weights_swaps_in_the_average_and_restores():
    """the smallest model of the GPU suite (tests/test_mobilenet_gpu.py: deeplabv3plus_mobilenet, output stride 16, 2 x 97 x 81).
    Its output inside ema_weights() must be, bit for bit, that of a fresh model loaded from ema_model_state -- after an eval
    forward on the live weights has filled every packed-weight cache, so a swap that does not announce itself shows"""
    from iswm_amd import optim
    from iswm_amd.network import _hip, modeling
    from iswm_amd.utils.loss import CrossEntropyLoss
    from tests import mobilenet_ref as R
    from tests.test_mobilenet_gpu import H, N, W
    d = dev()

    def build(sd):
        m = modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16)
        m.load_state_dict(sd, strict=True)
        for mod in m.modules():
            if isinstance(mod, _hip.Dropout):
                mod.p = 0.0
        return m.to(d)
    x, lab = R.synth_images(N, H, W, 5).to(d), R.synth_labels(N, H, W, 5).to(d)
    model = build(R.synth_state("deeplabv3plus", 2, 16)).train()
    opt = optim.FusedSGD(model.parameters(), lr=1e-3, momentum=0.9, nesterov=True, weight_decay=1e-4)
    opt.enable_ema(0.5)
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]), ignore_index=255)
    for _ in range(2):
        opt.zero_grad()
        crit(model(x), lab).backward()
        opt.step()
    model.eval()
    with torch.no_grad():
        live_out = model(x).clone()
    live = opt.arena.data.clone()
    ckpt = {"model_state": {k: v.detach().clone() for k, v in model.state_dict().items()}, "ema_state": opt.ema_state_dict(model)}
    assert list(ckpt["ema_state"]["params"]) == [k for k, _ in model.named_parameters()]
    with opt.ema_weights():
        with torch.no_grad():
            ema_out = model(x).clone()
        assert same_bits(opt._ema, live)                      # the two buffers changed places
        inside = opt.ema_state_dict(model)
        from iswm_amd import ops
        real, launched = ops.call, []
        ops.call = lambda name, *a: (launched.append(name), real(name, *a))[1]
        try:
            opt.set_grad_clip(1.0)
            with pytest.raises(RuntimeError):
                opt.step()
        finally:
            ops.call = real
            opt.set_grad_clip(None)
        assert launched == [], "a refused step must launch nothing"
    assert same_bits(opt.arena.data, live)
    for k, v in ckpt["ema_state"]["params"].items():
        assert same_bits(inside["params"][k], v)
    with torch.no_grad():
        assert same_bits(model(x), live_out)                  # back on the live weights, caches included
    fresh = build(optim.ema_model_state(ckpt)).eval()
    with torch.no_grad():
        fresh_out = fresh(x)
    assert same_bits(ema_out, fresh_out)
    assert not same_bits(ema_out, live_out)


# ---- resume ----------------------------------------------------------------------------------------------------------
class Bag(torch.nn.Module):
    def __init__(self, tensors):
        super().__init__()
        self.w = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])


@pytest.mark.parametrize("family,cfg", [("sgd", X.SGD_CONFIGS[0]), ("adam", X.ADAM_CONFIGS[3])], ids=["sgd", "adamw"])
def test_resume_equals_the_uninterrupted_run(family, cfg):
    d = dev()
    g = X.gen(21)
    shapes = [(5, 3), (1025,), (2, 3, 3, 3)]
    init = [torch.randn(s, generator=g) for s in shapes]
    grads = [[torch.randn(s, generator=g) for s in shapes] for _ in range(4)]

    def make(tensors):
        bag = Bag(tensors).to(d)
        opt = make_opt(family, bag.parameters(), cfg)
        opt.set_grad_clip(0.7)
        return bag, opt

    def steps(bag, opt, which):
        for gs in which:
            opt.zero_grad()
            for p, gg in zip(bag.parameters(), gs):
                p.grad = gg.to(d)
            opt.step()
    whole, wopt = make(init)
    wopt.enable_ema(0.9)
    steps(whole, wopt, grads)
    first, fopt = make(init)
    fopt.enable_ema(0.9)
    steps(first, fopt, grads[:2])
    f = io.BytesIO()
    torch.save({"model_state": first.state_dict(), "optimizer_state": fopt.state_dict(), "ema_state": fopt.ema_state_dict(first)}, f)
    f.seek(0)
    ck = torch.load(f, map_location="cpu", weights_only=True)
    second, sopt = make([torch.zeros(s) for s in shapes])
    second.load_state_dict(ck["model_state"])
    sopt.load_state_dict(ck["optimizer_state"])
    sopt.load_ema_state_dict(second, ck["ema_state"])
    assert sopt._ema_updates == 2
    steps(second, sopt, grads[2:])
    assert same_bits(sopt.arena.data, wopt.arena.data) and same_bits(sopt._ema, wopt._ema)
    for a, b in zip(opt_state(sopt), opt_state(wopt)):
        assert same_bits(a, b)
    assert sopt._ema_updates == 4 and same_bits(sopt.last_grad_norm, wopt.last_grad_norm)
    assert not same_bits(sopt._ema, sopt.arena.data)


# ---- train / predict -------------------------------------------------------------------------------------------------
def test_train_entry_with_clipping_and_ema(tmp_path, capsys):
    from iswm_amd import optim, predict, train
    from iswm_amd.network import modeling
    ck = str(tmp_path / "ck")
    base = ["--model", "deeplabv3plus_mobilenet", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
            "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "2", "--val_interval", "2",
            "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0", "--clip_grad_norm", "1.0",
            "--ema_decay", "0.9"]
    train.main(base + ["--total_itrs", "4"])
    out = capsys.readouterr().out
    assert "Itrs 4/4" in out and "Validation @2" in out and "grad norm=" in out
    files = glob.glob(os.path.join(ck, "best_*.pth"))
    assert len(files) == 1
    ckpt = torch.load(files[0], map_location="cpu", weights_only=True)
    ema = ckpt["ema_state"]
    model = modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16)
    names = [k for k, _ in model.named_parameters()]
    assert list(ema["params"]) == names and ema["decay"] == 0.9 and ema["warmup"] is True
    assert ema["num_updates"] == ckpt["cur_itrs"]
    assert len(ckpt["model_state"]) == 362 and "param_groups" in ckpt["optimizer_state"]
    differ = [k for k in names if not torch.equal(ckpt["model_state"][k], ema["params"][k])]
    assert len(differ) > len(names) // 2, "model_state must be the live weights, not the average"
    loaded = predict.load_model(model, files[0], use_ema=True)
    sd = loaded.state_dict()
    for k in names:
        assert same_bits(sd[k], ema["params"][k]), k
    for k in sd:
        if k not in ema["params"]:
            assert torch.equal(sd[k], ckpt["model_state"][k]), k          # BatchNorm buffers: the live statistics
    capsys.readouterr()

    # --test_only --use_ema scores the EMA weights: two copies of the checkpoint with the SAME live weights whose EMA classifier
    # bias is pushed to all-foreground / all-background give different scores, and the first equals a plain --test_only run on
    # a checkpoint whose model_state is ema_model_state of it
    def scored(path, *flags):
        train.main(base + ["--test_only", "--ckpt", path] + list(flags))
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, lines
        return lines[0]
    bias = [k for k in names if tuple(ema["params"][k].shape) == (2,)][-1]
    paths = {}
    for tag, shift in (("fg", [-100.0, 100.0]), ("bg", [100.0, -100.0])):
        ck2 = dict(ckpt, ema_state=dict(ema, params=dict(ema["params"])))
        ck2["ema_state"]["params"][bias] = ema["params"][bias] + torch.tensor(shift)
        paths[tag] = str(tmp_path / ("ema_%s.pth" % tag))
        torch.save(ck2, paths[tag])
    torch.save(dict(ckpt, model_state=optim.ema_model_state(torch.load(paths["fg"], map_location="cpu", weights_only=True))),
               str(tmp_path / "overlaid.pth"))
    s_fg, s_bg = scored(paths["fg"], "--use_ema"), scored(paths["bg"], "--use_ema")
    assert s_fg != s_bg
    assert scored(str(tmp_path / "overlaid.pth")) == s_fg
    train.main(base + ["--total_itrs", str(ckpt["cur_itrs"] + 2), "--ckpt", files[0], "--continue_training"])
    out = capsys.readouterr().out
    assert "Model restored" in out and "Itrs %d/%d" % (ckpt["cur_itrs"] + 2, ckpt["cur_itrs"] + 2) in out
