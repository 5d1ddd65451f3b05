"""Timing of the distillation criterion on the GPU (not a test), next to its sibling, the overlap criterion of the same build:

    O = overlap:  iswm_overlap_loss_fwd (+ coeffs), then iswm_overlap_loss_bwd     fwd 4C + 1 B/pixel, bwd 4C + 1 read + 4C written
    D = distill:  iswm_distill_loss_fwd (+ coeffs), then iswm_distill_loss_bwd     fwd 2 * 4C + 1,      bwd 2 * 4C + 1 read + 4C written

    python tools/distill_loss_time.py [--batch 16] [--size 513] [--reps 20] [--out FILE]      device events around each pass
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/distill_loss_time.py --kernels-only   kernel times, a run of its own
    python tools/distill_loss_time.py --step [--teacher deeplabv3plus_resnet101]               images/s of a training step

at [batch, 2, size, size] logits with uint8 labels, the method of tools/overlap_loss_time.py: both arms in one process,
alternating, after 3 warm-up repetitions; the operands rotate through a ring of buffers larger than the 256 MiB Infinity Cache, so
no pass reads a tensor the previous repetition left on the die.  A matrix product is enqueued in front of every timed pass, so the
host runs ahead and the pass's launches execute back to back between the two events: the kernels' own time, launch gaps included.
--step runs the MobileNetV2 student's training step (batch x 3 x size x size, SGD, weighted CE) alone and then with a frozen
teacher and the distillation criterion, in one process on one GPU, and prints images/s of both."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20
TAU = 2.0


def log(f, *a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    if f is not None:
        f.write(s + "\n")
        f.flush()


def passes(o, dev):
    """[(name, bytes per pixel, callable(i))]: the four passes on operand set i of the ring, and the ring's length"""
    from iswm_amd import ops
    npix = o.batch * o.size * o.size
    per_set = npix * (2 * 2 * 4 + 1 + 2 * 4)                   # two logit tensors, labels, the gradient a backward pass allocates
    ring = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn(o.batch, 2, o.size, o.size, device=dev, generator=g) for _ in range(ring)]
    ts = [torch.randn(o.batch, 2, o.size, o.size, device=dev, generator=g) for _ in range(ring)]
    ys = []
    for _ in range(ring):
        y = (torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.1).to(torch.uint8)
        y[torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.05] = 255
        ys.append(y)
    w = torch.tensor([1.0, 3.0], device=dev)
    up = torch.ones(1, device=dev)
    _, ocoef = ops.overlap_loss_coeffs(ops.overlap_loss_fwd(zs[0], ys[0], w, 255), 2, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, "foreground")
    _, dcoef = ops.distill_loss_coeffs(ops.distill_loss_fwd(zs[0], ts[0], ys[0], w, 255, TAU), 1.0, 1.0, TAU)
    c = 2
    return [("O overlap fwd", 4 * c + 1, lambda i: ops.overlap_loss_fwd(zs[i], ys[i], w, 255)),
            ("D distill fwd", 8 * c + 1, lambda i: ops.distill_loss_fwd(zs[i], ts[i], ys[i], w, 255, TAU)),
            ("O overlap bwd", 8 * c + 1, lambda i: ops.overlap_loss_bwd(zs[i], ys[i], w, 255, ocoef, up)),
            ("D distill bwd", 12 * c + 1, lambda i: ops.distill_loss_bwd(zs[i], ts[i], ys[i], w, 255, TAU, dcoef, up))], ring, npix


def time_passes(o, f, dev):
    arms, ring, npix = passes(o, dev)
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# logits [%d, 2, %d, %d] fp32 (student and teacher), uint8 labels (%d pixels), T = %g; ring of %d operand sets; "
           "%d warm-up + %d timed repetitions per pass, passes alternating" % (o.batch, o.size, o.size, npix, TAU, ring, o.warmup, o.reps))
    busy = torch.randn(4096, 4096, device=dev)
    evs = [[] for _ in arms]
    for r in range(o.warmup + o.reps):
        for k, (_, _, fn) in enumerate(arms):
            i = (r * len(arms) + k) % ring
            if not o.kernels_only:
                torch.mm(busy, busy)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn(i)
            b.record()
            if r >= o.warmup:
                evs[k].append((a, b))
        torch.cuda.synchronize()
    if o.kernels_only:
        log(f, "ran %d repetitions of each pass (kernel times: the trace of this run)" % (o.warmup + o.reps))
        return
    rate = {}
    for (name, nbytes, _), e in zip(arms, evs):
        ms = torch.tensor([a.elapsed_time(b) for a, b in e], dtype=torch.float64)
        rate[name] = nbytes * npix / float(ms.median()) * 1e-9
        log(f, "%-14s mean %.4f ms  median %.4f  min %.4f  max %.4f  std %.4f   %2d B/pixel -> %.2f TB/s at the median, %.2f at "
               "the min" % (name, ms.mean(), ms.median(), ms.min(), ms.max(), ms.std(), nbytes, rate[name],
                            nbytes * npix / float(ms.min()) * 1e-9))
    for kind in ("fwd", "bwd"):
        log(f, "%s: distill / overlap bandwidth = %.2f (the expectation to report against: within 20 %% of the sibling, >= 0.80)" %
            (kind, rate["D distill " + kind] / rate["O overlap " + kind]))


def time_steps(o, f, dev):
    from iswm_amd import network
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss, DistillationLoss
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# training step of deeplabv3plus_mobilenet, [%d, 3, %d, %d], SGD, weighted CE; alone and with a frozen %s teacher "
           "(random weights, eval mode, no_grad) and DistillationLoss(T = %g); %d warm-up + %d timed steps each" %
        (o.batch, o.size, o.size, o.teacher, TAU, o.warmup, o.steps))
    torch.manual_seed(0)
    x = torch.randn(o.batch, 3, o.size, o.size, device=dev)
    y = (torch.rand(o.batch, o.size, o.size, device=dev) < 0.1).to(torch.uint8)
    w = torch.tensor([1.0, 3.0])
    teacher = network.modeling.__dict__[o.teacher](num_classes=2, output_stride=16, pretrained_backbone=False)
    teacher.to(dev).eval().requires_grad_(False)
    for name, distill in (("student alone", False), ("student + teacher", True)):
        model = network.modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16, pretrained_backbone=False).to(dev).train()
        opt = FusedSGD(model.parameters(), momentum=0.9, weight_decay=1e-4, nesterov=True)
        crit = (DistillationLoss(temperature=TAU, weight=w) if distill else CrossEntropyLoss(weight=w)).to(dev)
        t0 = None
        for step in range(o.warmup + o.steps):
            if step == o.warmup:
                torch.cuda.synchronize()
                t0 = time.time()
            if distill:
                with torch.no_grad():
                    t_logits = teacher(x)
                loss = crit(model(x), y, t_logits)
            else:
                loss = crit(model(x), y)
            opt.zero_grad()
            loss.backward()
            opt.step()
        torch.cuda.synchronize()
        dt = time.time() - t0
        log(f, "%-18s %.1f images/s (%.1f ms per step of %d images), last loss %.4f" %
            (name, o.batch * o.steps / dt, 1e3 * dt / o.steps, o.batch, float(loss.detach())))
        del model, opt, crit


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--teacher", type=str, default="deeplabv3plus_resnet101")
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("distill_loss_time.py measures on the GPU; there is nothing to measure without one")
    if o.out and os.path.dirname(o.out):
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
    f = open(o.out, "w") if o.out else None
    dev = torch.device("cuda:0")
    (time_steps if o.step else time_passes)(o, f, dev)
    if f is not None:
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
