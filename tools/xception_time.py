"""Timing of the Xception path on the GPU (not a test).

    python tools/xception_time.py [--batch 16] [--size 513] [--reps 20] [--out profiles/xception_time.txt]
                                  [--no-kernels] [--no-model] [--no-torch]

1. Kernel arms, on every distinct depthwise unit (C, map, dilation, padding, ReLU on load) of deeplabv3plus_xception (os 16) at
   the given input: what stands between the residual stream / the previous BatchNorm and the pointwise conv's planes operand,
   forward, and the data + weight gradient, backward, as
       composed = [ReLU pass] + iswm_dwconv2d_fwd + iswm_split_planes   | iswm_dwconv2d_dgrad + iswm_dwconv2d_wgrad [+ mask pass]
       new      = iswm_dwconv3x3_pre_fwd (planes out, pad columns zeroed) | iswm_dwconv3x3_pre_bwd
   (the ReLU and mask passes are torch's elementwise kernels: the library has none, which is the point; the composed arm does
   not zero the pad columns of a 768-wide operand, the new one does).  One process, alternating, device events, warm-up,
   operands rotating through a ring larger than the 256 MiB Infinity Cache.  The composed arm runs TWICE per round: the
   difference of its two timings is the run-to-run spread the comparison is read against.
2. Model: training images/s of deeplabv3plus_xception (forward, weighted CE, backward, SGD-nesterov) next to the same step of
   the stock-torch restatement (tests/xception_ref.py, fp32, PyTorch-ROCm ops) on the same GPU in the same call.
3. The step's device time by kernel group, from device events around every library call of one step.
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402
from mobilenet_time import RING_BYTES, log  # noqa: E402


def units(model, size):
    """[(C, map, dilation, padding, relu on load, pointwise input pitch)] of the 34 depthwise units, in execution order"""
    from iswm_amd.network.backbone import xception as X
    h = (size - 3) // 2 + 1 - 2                  # conv1 (3x3 stride 2 pad 0), conv2 (3x3 pad 0)
    out = []

    def sep(s, relu):
        nonlocal h
        dw = s.conv1
        out.append((dw.in_channels, h, dw.dilation[0], dw.padding[0], relu, s.pointwise.cin_p))
        h = h + 2 * dw.padding[0] - 2 * dw.dilation[0]
    for name, m in model.backbone.named_children():
        if isinstance(m, X.Block):
            us, first_relu, pool = m._units()
            for k, u in enumerate(us):
                sep(u[0], k == 0 and first_relu is not None)
            if pool is not None:
                h = (h - 1) // 2 + 1
        elif isinstance(m, X.SeparableConv2d):
            sep(m, False)
    return out


def time_kernels(f, model, batch, size, reps, warmup=3):
    from iswm_amd import ops
    dev = torch.device("cuda:0")
    geoms = units(model, size)
    uniq = []
    for g in geoms:
        if g not in uniq:
            uniq.append(g)
    log(f, "# depthwise units: batch %d, input %dx%d, os 16; %d units, %d distinct; %d timed repetitions each, %d warm-up" %
        (batch, size, size, len(geoms), len(uniq), reps, warmup))
    log(f, "%-30s %3s | %8s %8s %8s %6s %6s %6s | %8s %8s %8s %6s %6s %6s" %
        ("unit (C HxW dil pad relu pitch)", "n", "fwd A us", "fwd A' us", "new us", "A/new", "spread", "TB/s",
         "bwd A us", "bwd A' us", "new us", "A/new", "spread", "TB/s"))
    slower, tot = [], dict(fo=0.0, fn=0.0, bo=0.0, bn=0.0)
    for (c, h, d, p, relu, cp) in uniq:
        ho = h + 2 * p - 2 * d
        ex, ey = batch * h * h * c, batch * ho * ho * c
        per = 4 * ex * 3 + 4 * ey * 2 + 6 * batch * ho * ho * cp * 2
        ring = max(2, -(-RING_BYTES // per))
        xs = [torch.randn(batch, h, h, c, device=dev) + 0.1 for _ in range(ring)]
        xr = [torch.relu(t) for t in xs]             # the rectified copy the composed path stores forward and reads backward
        dys = [torch.randn(batch, ho, ho, c, device=dev) for _ in range(ring)]
        ys = [torch.empty(batch, ho, ho, c, device=dev) for _ in range(ring)]
        dxs = [torch.empty(batch, h, h, c, device=dev) for _ in range(ring)]
        po = [ops.new_planes(batch, ho, ho, cp, dev) for _ in range(ring)]
        pn = [ops.new_planes(batch, ho, ho, cp, dev) for _ in range(ring)]
        w = torch.randn(c, 1, 3, 3, device=dev) * 0.3
        g = ops.ConvGeom(xs[0], c, 3, 3, 1, p, d)
        dw = torch.empty(c, 1, 3, 3, device=dev)
        view = (lambda t: t[..., 0:c]) if cp > c else (lambda t: t)

        def fwd_old(i):
            x = torch.clamp(xs[i], min=0, out=xr[i]) if relu else xs[i]
            ops.split_planes(ops.dwconv2d_fwd(x, w, g, None, ys[i]), out=view(po[i]))

        def fwd_new(i):
            ops.dwconv3x3_pre_fwd(xs[i], w, g, relu, out=view(pn[i]))

        def bwd_old(i):
            ops.dwconv2d_dgrad(dys[i], w, g, tuple(xs[i].shape), dxs[i])
            ops.dwconv2d_wgrad(xr[i] if relu else xs[i], dys[i], g, c, dw)
            if relu:
                dxs[i].mul_(xs[i] > 0)

        def bwd_new(i):
            ops.dwconv3x3_pre_bwd(xs[i], dys[i], w, g, c, relu, dx=dxs[i], dw=dw)
        arms = [fwd_old, fwd_new, fwd_old, bwd_old, bwd_new, bwd_old]
        evs = [[] for _ in arms]
        for r in range(warmup + reps):
            for k, arm in enumerate(arms):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                arm((r * len(arms) + k) % ring)
                b.record()
                if r >= warmup:
                    evs[k].append((a, b))
        torch.cuda.synchronize()
        us = [1e3 * sum(a.elapsed_time(b) for a, b in e) / len(e) for e in evs]
        n = geoms.count((c, h, d, p, relu, cp))
        fb = 4 * ex + 6 * batch * ho * ho * cp
        bb = 4 * (ey + 2 * ex)
        fo, bo = min(us[0], us[2]), min(us[3], us[5])
        fs, bs = abs(us[0] - us[2]) / fo, abs(us[3] - us[5]) / bo
        log(f, "%-30s %3d | %8.1f %8.1f %8.1f %6.2f %5.1f%% %6.2f | %8.1f %8.1f %8.1f %6.2f %5.1f%% %6.2f" %
            ("%d %dx%d d%d p%d %s %d" % (c, h, h, d, p, "relu" if relu else "lin", cp), n, us[0], us[2], us[1], fo / us[1], 100 * fs,
             fb / us[1] * 1e-6, us[3], us[5], us[4], bo / us[4], 100 * bs, bb / us[4] * 1e-6))
        if us[1] > fo * (1 + fs):
            slower.append(("forward", c, h, d, p, relu))
        if us[4] > bo * (1 + bs):
            slower.append(("backward", c, h, d, p, relu))
        tot["fo"] += n * fo
        tot["fn"] += n * us[1]
        tot["bo"] += n * bo
        tot["bn"] += n * us[4]
        del xs, xr, dys, ys, dxs, po, pn
        torch.cuda.empty_cache()
    log(f, "all %d units: forward composed %.2f ms new %.2f ms; backward composed %.2f ms new %.2f ms" %
        (len(geoms), tot["fo"] * 1e-3, tot["fn"] * 1e-3, tot["bo"] * 1e-3, tot["bn"] * 1e-3))
    log(f, "(composed = the faster of its two runs; backward composed reads the rectified copy the composed forward would have "
           "stored, and is not charged for storing it)")
    log(f, "new path not slower than composed (beyond the composed arm's own spread) on every row: %s" %
        ("yes" if not slower else "NO: %s" % (slower,)))
    return slower


def _group(name, in_head):
    if in_head:
        return "head"
    if name.startswith("iswm_dwconv3x3_pre"):
        return "depthwise (pre-activation)"
    if name.startswith("iswm_bn_") or name.startswith("iswm_colstat"):
        return "BatchNorm passes"
    if name.startswith("iswm_maxpool"):
        return "max-pool"
    if name.startswith("iswm_conv2d") or name.startswith("iswm_pack_weights") or name in ("iswm_pad_weights", "iswm_unpad_weights",
                                                                                         "iswm_transpose_weights"):
        return "pointwise / skip / stem conv"
    return "other (layout, loss, resize, optimizer)"


def time_model(f, batch, size, steps, torch_arm):
    from iswm_amd import ops
    from iswm_amd.network import modeling
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss
    from tests import xception_ref as R
    dev = torch.device("cuda:0")
    sd = R.synth_state("deeplabv3plus", 2, 16)
    x = R.synth_images(batch, size, size, 0).to(dev)
    lab = R.synth_labels(batch, size, size, 0).to(dev)
    wgt = torch.tensor([1.0, 3.0])
    hyper = dict(lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)
    m = modeling.deeplabv3plus_xception(num_classes=2, output_stride=16)
    m.load_state_dict(sd)
    m = m.to(dev).train()
    opt = FusedSGD(m.parameters(), **hyper)
    crit = CrossEntropyLoss(weight=wgt, ignore_index=255)

    def step():
        opt.zero_grad()
        loss = crit(m(x), lab)
        loss.backward()
        opt.step()
        return loss

    def timed(fn, n):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n
    dt = timed(step, steps)
    log(f, "# model: deeplabv3plus_xception os16, batch %d, %dx%d, forward + weighted CE + backward + SGD-nesterov, %d timed "
           "steps after 3 warm-up" % (batch, size, size, steps))
    log(f, "HIP path          : %8.2f ms/step  %8.1f images/s" % (dt * 1e3, batch / dt))
    real, recs, state = ops.call, [], {"head": False}

    def call(name, *a):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(name, *a)
        e1.record()
        recs.append((_group(name, state["head"]), name, e0, e1))
        return r
    head = m.classifier
    hf, hb = head.fwd, head.bwd

    def scoped(fn):
        def run(*a, **k):
            state["head"] = True
            try:
                return fn(*a, **k)
            finally:
                state["head"] = False
        return run
    head.fwd, head.bwd = scoped(hf), scoped(hb)
    ops.call = call
    try:
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        step()
        t1.record()
        torch.cuda.synchronize()
    finally:
        ops.call = real
        del head.fwd, head.bwd
    groups, names = {}, {}
    for gname, name, e0, e1 in recs:
        ms = e0.elapsed_time(e1)
        groups[gname] = groups.get(gname, 0.0) + ms
        names[(gname, name)] = names.get((gname, name), 0.0) + ms
    total = sum(groups.values())
    log(f, "device time of one step by kernel group (%d library calls, %.2f ms inside calls, %.2f ms event-to-event):" %
        (len(recs), total, t0.elapsed_time(t1)))
    for gname, ms in sorted(groups.items(), key=lambda kv: -kv[1]):
        log(f, "  %-42s %8.2f ms  %5.1f %%" % (gname, ms, 100 * ms / total))
    log(f, "largest entry points:")
    for (gname, name), ms in sorted(names.items(), key=lambda kv: -kv[1])[:12]:
        log(f, "  %-28s %-34s %8.2f ms" % (gname, name, ms))
    if torch_arm:
        ref = R.build("deeplabv3plus", 2, 16, sd, dtype=torch.float32).to(dev).train()
        ropt = torch.optim.SGD(ref.parameters(), **hyper)
        wd = wgt.to(dev)

        def rstep():
            ropt.zero_grad()
            loss = R.weighted_ce(ref(x), lab, wd)
            loss.backward()
            ropt.step()
        t0 = time.perf_counter()
        rstep()
        torch.cuda.synchronize()
        log(f, "stock torch first step (kernel search) %.1f s" % (time.perf_counter() - t0))
        rdt = timed(rstep, steps)
        log(f, "stock torch %-6s: %8.2f ms/step  %8.1f images/s   (HIP path / torch = %.2fx)" %
            (torch.__version__.split("+")[0], rdt * 1e3, batch / rdt, rdt / dt))
    else:
        log(f, "stock torch       : not measured")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", type=str, default=None)
    ap.add_argument("--no-kernels", action="store_true")
    ap.add_argument("--no-model", action="store_true")
    ap.add_argument("--no-torch", action="store_true")
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("xception_time.py measures on the GPU; there is nothing to measure without one")
    f = open(o.out, "a" if (o.no_kernels and os.path.exists(o.out or "")) else "w") if o.out else None
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    slower = []
    if not o.no_kernels:
        from iswm_amd.network import modeling
        slower = time_kernels(f, modeling.deeplabv3plus_xception(num_classes=2, output_stride=16), o.batch, o.size, o.reps)
    if not o.no_model:
        time_model(f, o.batch, o.size, o.steps, not o.no_torch)
    if f is not None:
        f.close()
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
