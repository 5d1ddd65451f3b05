"""Timing of the MobileNetV2 path on the GPU (not a test).

    python tools/mobilenet_time.py [--batch 16] [--size 513] [--reps 20] [--out profiles/mobilenet_time.txt]
                                   [--no-kernels] [--no-model] [--no-torch]

1. Kernel arms, on the 17 depthwise geometries of deeplabv3plus_mobilenet (os 16) at the given input: the depthwise ->
   BatchNorm-statistics forward and the data + weight gradient backward, as
       old = iswm_dwconv2d_fwd + iswm_colstat            | iswm_dwconv2d_dgrad + iswm_dwconv2d_wgrad   (csrc/dwconv.hip)
       new = iswm_dwconv3x3_fwd_stats                    | iswm_dwconv3x3_bwd                          (csrc/dwconv3.hip)
   in one process, alternating, timed with device events after a warm-up.  Operands rotate through a ring of buffers larger
   than the 256 MiB Infinity Cache, so no arm is served a tensor the previous repetition left on the die.  Achieved bytes/s
   are against the operand-once count: x + y forward; dy + x + dx backward.
2. Model: training images/s of deeplabv3plus_mobilenet (forward, weighted CE, backward, SGD-nesterov) next to the same step
   of the stock-torch restatement (tests/mobilenet_ref.py, fp32, PyTorch-ROCm ops) on the same GPU in the same call.
3. The step's device time by kernel group (depthwise, backbone 1x1 / stem convolutions, BatchNorm passes, head, other),
   from device events around every library call of one step (the events slow the host down, not the kernels).
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20


def log(f, *a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    if f is not None:
        f.write(s + "\n")
        f.flush()


def depthwise_geometries(model, size):
    """[(C, H_in, stride, dilation)] of the 17 depthwise layers, in execution order"""
    from iswm_amd.network.backbone.mobilenetv2 import InvertedResidual
    h = (size - 1) // 2 + 1                    # features[0]: 3x3 stride 2 pad 1
    out = []
    for m in model.backbone.modules():
        if isinstance(m, InvertedResidual):
            dw = [c for c in m.conv if getattr(c, "groups", 1) > 1][0]
            out.append((dw.in_channels, h, dw.stride[0], dw.dilation[0]))
            h = (h - 1) // dw.stride[0] + 1
    return out


def time_kernels(f, model, batch, size, reps, warmup=3):
    from iswm_amd import ops
    dev = torch.device("cuda:0")
    geoms = depthwise_geometries(model, size)
    uniq = []
    for g in geoms:
        if g not in uniq:
            uniq.append(g)
    log(f, "# depthwise arms: batch %d, input %dx%d, os 16; %d layers, %d distinct geometries; %d timed repetitions each, "
           "%d warm-up" % (batch, size, size, len(geoms), len(uniq), reps, warmup))
    log(f, "%-26s %5s | %9s %9s %6s %7s | %9s %9s %6s %7s" % ("geometry (C HxW stride dil)", "count", "fwd old us", "fwd new us",
                                                               "ratio", "new TB/s", "bwd old us", "bwd new us", "ratio", "new TB/s"))
    slower = []
    tot = dict(fo=0.0, fn=0.0, bo=0.0, bn=0.0)
    for (c, h, s, d) in uniq:
        ho = (h - 1) // s + 1
        bytes_x, bytes_y = batch * h * h * c * 4, batch * ho * ho * c * 4
        ring = max(2, -(-RING_BYTES // (2 * bytes_x + 2 * bytes_y)))
        xs = [torch.randn(batch, h, h, c, device=dev) + 0.5 for _ in range(ring)]
        dys = [torch.randn(batch, ho, ho, c, device=dev) for _ in range(ring)]
        ys = [torch.empty(batch, ho, ho, c, device=dev) for _ in range(ring)]
        dxs = [torch.empty(batch, h, h, c, device=dev) for _ in range(ring)]
        w = torch.randn(c, 1, 3, 3, device=dev) * 0.3
        g = ops.ConvGeom(xs[0], c, 3, 3, s, d, d)
        dw = torch.empty(c, 1, 3, 3, device=dev)

        def fwd_old(i):
            ops.colstat(ops.dwconv2d_fwd(xs[i], w, g, None, ys[i]))

        def fwd_new(i):
            ops.dwconv3x3_fwd_stats(xs[i], w, g, True, out=ys[i])

        def bwd_old(i):
            ops.dwconv2d_dgrad(dys[i], w, g, tuple(xs[i].shape), dxs[i])
            ops.dwconv2d_wgrad(xs[i], dys[i], g, c, dw)

        def bwd_new(i):
            ops.dwconv3x3_bwd(xs[i], dys[i], w, g, c, dx=dxs[i], dw=dw)
        arms = [fwd_old, fwd_new, bwd_old, bwd_new]
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
        n = geoms.count((c, h, s, d))
        fb, bb = bytes_x + bytes_y, bytes_y + 2 * bytes_x
        log(f, "%-26s %5d | %9.1f %9.1f %6.2f %7.2f | %9.1f %9.1f %6.2f %7.2f" %
            ("%d %dx%d s%d d%d" % (c, h, h, s, d), n, us[0], us[1], us[0] / us[1], fb / us[1] * 1e-6, us[2], us[3], us[2] / us[3],
             bb / us[3] * 1e-6))
        if us[1] >= us[0]:
            slower.append(("forward", c, h, s, d))
        if us[3] >= us[2]:
            slower.append(("backward", c, h, s, d))
        tot["fo"] += n * us[0]
        tot["fn"] += n * us[1]
        tot["bo"] += n * us[2]
        tot["bn"] += n * us[3]
        del xs, dys, ys, dxs
        torch.cuda.empty_cache()
    log(f, "all 17 layers: forward old %.2f ms new %.2f ms; backward old %.2f ms new %.2f ms" %
        (tot["fo"] * 1e-3, tot["fn"] * 1e-3, tot["bo"] * 1e-3, tot["bn"] * 1e-3))
    log(f, "new path faster on every geometry, forward and backward: %s" % ("yes" if not slower else "NO: %s" % (slower,)))
    return slower


def _group(name, in_head):
    if in_head:
        return "head"
    if name.startswith("iswm_dwconv3x3"):
        return "depthwise"
    if name.startswith("iswm_bn_") or name.startswith("iswm_colstat"):
        return "BatchNorm passes"
    if name.startswith("iswm_conv2d") or name.startswith("iswm_pack_weights") or name in ("iswm_pad_weights", "iswm_unpad_weights",
                                                                                         "iswm_transpose_weights"):
        return "backbone 1x1 / stem conv"
    return "other (layout, loss, resize, optimizer)"


def time_model(f, batch, size, steps, torch_arm):
    from iswm_amd import ops
    from iswm_amd.network import modeling
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss
    from tests import mobilenet_ref as R
    dev = torch.device("cuda:0")
    sd = R.synth_state("deeplabv3plus", 2, 16)
    x = R.synth_images(batch, size, size, 0).to(dev)
    lab = R.synth_labels(batch, size, size, 0).to(dev)
    wgt = torch.tensor([1.0, 3.0])
    hyper = dict(lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True)

    m = modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16)
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
    log(f, "# model: deeplabv3plus_mobilenet os16, batch %d, %dx%d, forward + weighted CE + backward + SGD-nesterov, %d timed "
           "steps after 3 warm-up" % (batch, size, size, steps))
    log(f, "HIP path          : %8.2f ms/step  %8.1f images/s" % (dt * 1e3, batch / dt))

    # device time by kernel group: events around every library call of one step
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
        t0 = torch.cuda.Event(enable_timing=True)
        t1 = torch.cuda.Event(enable_timing=True)
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
        raise SystemExit("mobilenet_time.py measures on the GPU; there is nothing to measure without one")
    f = open(o.out, "w") if o.out else None
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    slower = []
    if not o.no_kernels:
        from iswm_amd.network import modeling
        slower = time_kernels(f, modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16), o.batch, o.size, o.reps)
    if not o.no_model:
        time_model(f, o.batch, o.size, o.steps, not o.no_torch)
    if f is not None:
        f.close()
    return 1 if slower else 0


if __name__ == "__main__":
    sys.exit(main())
