"""Timing of the distance map and of the boundary criterion on the GPU (not a test), next to its sibling, the overlap criterion
of the same build:

    M = map:       iswm_signed_edt (k_edt_columns, k_edt_rows)                      1 B read + 4 B written per pixel, 12 B of workspace traffic
    O = overlap:   iswm_overlap_loss_fwd (+ coeffs), then iswm_overlap_loss_bwd     fwd 4C + 1 B/pixel,     bwd 4C + 1 read + 4C written
    B = boundary:  iswm_boundary_loss_fwd (+ coeffs), then iswm_boundary_loss_bwd   fwd 4C + 1 + 4 |K|,     bwd 4C + 1 + 4 |K| read + 4C written

    python tools/boundary_loss_time.py [--batch 16] [--size 513] [--reps 20] [--out FILE]      device events around each pass
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/boundary_loss_time.py --kernels-only   kernel times, a run of its own
    python tools/boundary_loss_time.py --step [--models deeplabv3plus_mobilenet,deeplabv3plus_resnet101]   images/s of a training step

at [batch, 2, size, size] logits with uint8 labels and the foreground plane (|K| = 1), the method of tools/distill_loss_time.py:
all arms in one process, alternating, after 3 warm-up repetitions; the operands rotate through a ring of buffers larger than the
256 MiB Infinity Cache, so no pass reads a tensor the previous repetition left on the die.  A matrix product is enqueued in front
of every timed pass, so the host runs ahead and the pass's launches execute back to back between the two events: the kernels' own
time, launch gaps included.  The map's time depends on the labels (the row pass searches outward until it has passed the nearest
pixel of the other set), so it is timed on three label sets: a thin wavy band per image (the wave masks this trainer sees), the
same with 5 % ignored pixels sprinkled in, and no foreground at all (every pixel searches its whole row and finds nothing: the
longest search there is).  --step runs a model's training step (batch x 3 x size x size, SGD, weighted CE) alone and then with
BoundaryLoss, in one process on one GPU, and prints images/s of both."""
import argparse
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20
CLIP = 20.0


def log(f, *a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    if f is not None:
        f.write(s + "\n")
        f.flush()


def band_labels(batch, size, dev, seed, ignored=0.0):
    """uint8 [batch, size, size]: per image a wavy band 6 to 20 pixels thick at its own height, phase and slope"""
    g = torch.Generator(device=dev).manual_seed(seed)
    r = torch.rand(batch, 5, device=dev, generator=g)
    yy = torch.arange(size, device=dev).view(1, size, 1).float()
    xx = torch.arange(size, device=dev).view(1, 1, size).float()
    p = lambda k: r[:, k].view(batch, 1, 1)
    mid = size * (0.2 + 0.6 * p(0)) + size * 0.08 * torch.sin(xx * (2 * math.pi / size) * (1 + 2 * p(1)) + 6.28 * p(2)) + \
        (xx - size / 2) * (p(3) - 0.5) * 0.4
    y = ((yy - mid).abs() <= 3 + 7 * p(4)).to(torch.uint8)
    if ignored > 0:
        y[torch.rand(batch, size, size, device=dev, generator=g) < ignored] = 255
    return y


def passes(o, dev):
    """[(name, bytes per pixel, callable(i))]: the passes on operand set i of the ring, and the ring's length"""
    from iswm_amd import ops
    npix = o.batch * o.size * o.size
    per_set = npix * (2 * 4 + 1 + 4 + 2 * 4 + 4)               # logits, labels, the map, the gradient and the map a pass allocates
    ring = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn(o.batch, 2, o.size, o.size, device=dev, generator=g) for _ in range(ring)]
    ys = [band_labels(o.batch, o.size, dev, 10 + i, ignored=0.05) for i in range(ring)]
    clean = [band_labels(o.batch, o.size, dev, 10 + i) for i in range(ring)]
    empty = [torch.zeros_like(y) for y in ys[:2]]
    ms = [ops.signed_edt(y, 2) for y in ys]
    w = torch.tensor([1.0, 3.0], device=dev)
    up = torch.ones(1, device=dev)
    _, ocoef = ops.overlap_loss_coeffs(ops.overlap_loss_fwd(zs[0], ys[0], w, 255), 2, 1.0, 1.0, 0.5, 0.5, 1.0, 1.0, "foreground")
    _, bcoef = ops.boundary_loss_coeffs(ops.boundary_loss_fwd(zs[0], ys[0], ms[0], w, 255, "foreground", CLIP), 1, 1.0, 1.0)
    c = 2
    info = "largest |phi| of the band labels %.0f pixels, mean %.1f" % (float(ms[0].abs().max()) ** 0.5,
                                                                      float(ms[0].abs().float().sqrt().mean()))
    return [("M map band", 5, lambda i: ops.signed_edt(clean[i], 2)),
            ("M map band+ign", 5, lambda i: ops.signed_edt(ys[i], 2)),
            ("M map empty", 5, lambda i: ops.signed_edt(empty[i % 2], 2)),
            ("O overlap fwd", 4 * c + 1, lambda i: ops.overlap_loss_fwd(zs[i], ys[i], w, 255)),
            ("B boundary fwd", 4 * c + 1 + 4, lambda i: ops.boundary_loss_fwd(zs[i], ys[i], ms[i], w, 255, "foreground", CLIP)),
            ("O overlap bwd", 8 * c + 1, lambda i: ops.overlap_loss_bwd(zs[i], ys[i], w, 255, ocoef, up)),
            ("B boundary bwd", 8 * c + 1 + 4, lambda i: ops.boundary_loss_bwd(zs[i], ys[i], ms[i], w, 255, bcoef, up, "foreground",
                                                                              CLIP))], ring, npix, info


def time_passes(o, f, dev):
    arms, ring, npix, info = passes(o, dev)
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# logits [%d, 2, %d, %d] fp32, uint8 labels (%d pixels), foreground plane, clip %g; %s; ring of %d operand sets; "
           "%d warm-up + %d timed repetitions per pass, passes alternating" % (o.batch, o.size, o.size, npix, CLIP, info, ring,
                                                                             o.warmup, o.reps))
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
        log(f, "%-15s mean %.4f ms  median %.4f  min %.4f  max %.4f  std %.4f   %2d B/pixel -> %.2f TB/s at the median, %.2f at "
               "the min" % (name, ms.mean(), ms.median(), ms.min(), ms.max(), ms.std(), nbytes, rate[name],
                            nbytes * npix / float(ms.min()) * 1e-9))
    for kind in ("fwd", "bwd"):
        log(f, "%s: boundary / overlap bandwidth = %.2f (the expectation to report against: within 20 %% of the sibling, >= 0.80)" %
            (kind, rate["B boundary " + kind] / rate["O overlap " + kind]))
    log(f, "map: the estimate to report against is 0.1-0.3 ms for both launches together (the B/pixel of the M rows counts the "
           "labels read and the map written only; the 16-bit column distances go through a 4 B/pixel workspace three times)")


def time_steps(o, f, dev):
    from iswm_amd import network
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import BoundaryLoss, CrossEntropyLoss
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# training step, [%d, 3, %d, %d], SGD, weighted CE; alone and with BoundaryLoss(boundary_weight 0.01, clip %g) on band "
           "labels with 5 %% ignored; %d warm-up + %d timed steps each" % (o.batch, o.size, o.size, CLIP, o.warmup, o.steps))
    torch.manual_seed(0)
    x = torch.randn(o.batch, 3, o.size, o.size, device=dev)
    y = band_labels(o.batch, o.size, dev, 7, ignored=0.05)
    w = torch.tensor([1.0, 3.0])
    for model_name in o.models.split(","):
        rates = []
        for name, boundary in (("CE alone", False), ("CE + boundary", True)):
            model = network.modeling.__dict__[model_name](num_classes=2, output_stride=16, pretrained_backbone=False).to(dev).train()
            opt = FusedSGD(model.parameters(), momentum=0.9, weight_decay=1e-4, nesterov=True)
            crit = (BoundaryLoss(boundary_weight=0.01, clip=CLIP, weight=w) if boundary else CrossEntropyLoss(weight=w)).to(dev)
            t0 = None
            for step in range(o.warmup + o.steps):
                if step == o.warmup:
                    torch.cuda.synchronize()
                    t0 = time.time()
                loss = crit(model(x), y)
                opt.zero_grad()
                loss.backward()
                opt.step()
            torch.cuda.synchronize()
            dt = time.time() - t0
            rates.append(o.batch * o.steps / dt)
            log(f, "%-26s %-14s %.1f images/s (%.2f ms per step of %d images), last loss %.4f" %
                (model_name, name, rates[-1], 1e3 * dt / o.steps, o.batch, float(loss.detach())))
            del model, opt, crit
        log(f, "%-26s with / without the term: %.3f of the step rate" % (model_name, rates[1] / rates[0]))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--models", type=str, default="deeplabv3plus_mobilenet,deeplabv3plus_resnet101")
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("boundary_loss_time.py measures on the GPU; there is nothing to measure without one")
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
