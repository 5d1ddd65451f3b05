"""Timing of the fused optimizer step with gradient clipping and EMA weights on the GPU (not a test).

    python tools/optim_time.py [--model deeplabv3plus_resnet101] [--reps 20] [--inner 10] [--out profiles/optim_time.txt]

On flat arenas of the model's size (every parameter padded to 4 elements, as optim.ParamArena lays them out) it times, per
optimizer family (SGD-nesterov, AdamW), five arms through iswm_amd.ops:

    plain      iswm_sgd_step / iswm_adam_step                                   20 / 28 B per parameter
    clip       iswm_grad_sqnorm + iswm_clip_finalize + the extended step        +4 B read by the norm pass; the step itself unchanged
    ema        the extended step with an EMA buffer                             +8 B (read and write ema)
    both       norm pass + extended step with both operands                     +4 +8 B
    norm       iswm_grad_sqnorm + iswm_clip_finalize alone                      4 B per parameter

The method of tools/overlap_loss_time.py: all arms in one process, alternating, device events, warm-up repetitions first, and a
"device" mode in which a matrix product is enqueued before the events so the host runs ahead and the launches execute back to
back.  One timed window is --inner (10) back-to-back repetitions of the arm between one pair of events, 0.7 - 5 ms of device
work, and every figure printed is the window divided by --inner: a single 0.07 ms call is too short a window to trust.  One
step streams 0.9 - 1.4 GB, several times the 256 MiB Infinity Cache, so nothing it reads was left on the die by the previous
one; the norm arm alone reads 237 MB, which would fit, so its repetitions alternate between two gradient arenas.  Each arm's bytes over its time is printed as TB/s and as a fraction of the 8 TB/s HBM peak, next to the 6.29
TB/s a float4 copy reaches (MI355X_MICROARCH.md)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def log(f, *a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    if f is not None:
        f.write(s + "\n")
        f.flush()


def arena_numel(model_name):
    from iswm_amd.network import modeling
    m = getattr(modeling, model_name)(num_classes=2, output_stride=16, pretrained_backbone=False)
    return sum((p.numel() + 3) // 4 * 4 for p in m.parameters())


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", type=str, default="deeplabv3plus_resnet101")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=10, help="back-to-back repetitions of an arm inside one timed window")
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("optim_time.py measures on the GPU; there is nothing to measure without one")
    from iswm_amd import ops
    if o.out and os.path.dirname(o.out):
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
    f = open(o.out, "w") if o.out else None
    dev = torch.device("cuda:0")
    n = arena_numel(o.model)
    g = torch.Generator(device=dev).manual_seed(0)
    p = torch.randn(n, device=dev, generator=g) * 0.05
    grad = torch.randn(n, device=dev, generator=g) * 1e-3
    s1, s2, ema = torch.zeros_like(p), torch.zeros_like(p), p.clone()
    slots, clip = ops.new_clip_state(dev)
    hyper = torch.tensor([1e-4, 0.1, 0.001, 0.001], dtype=torch.float32, device=dev)
    max_norm = 1.0                                             # the norm of `grad` is ~7: every clipped step really scales g

    grad2, turn = grad.clone(), [0]

    def norm():
        ops.grad_sqnorm(grad, slots)
        ops.clip_finalize(slots, max_norm, clip)

    def norm_alone():                                          # two arenas in turn: one alone would stay in the Infinity Cache
        turn[0] ^= 1
        ops.grad_sqnorm(grad2 if turn[0] else grad, slots)
        ops.clip_finalize(slots, max_norm, clip)

    def sgd(c, e):
        if c is None and e is None:
            ops.sgd_step(p, grad, s1, hyper, 0.9, 1e-4, True)
        else:
            ops.sgd_step_ex(p, grad, s1, hyper, 0.9, 1e-4, True, c, e)

    def adam(c, e):
        if c is None and e is None:
            ops.adam_step(p, grad, s1, s2, hyper, 0.9, 0.999, 1e-8, 1e-2, True)
        else:
            ops.adam_step_ex(p, grad, s1, s2, hyper, 0.9, 0.999, 1e-8, 1e-2, True, c, e)

    def arms_of(step, base):
        return [("plain", lambda: step(None, None), base),
                ("clip", lambda: (norm(), step(clip, None)), base + 4),
                ("ema", lambda: step(None, ema), base + 8),
                ("both", lambda: (norm(), step(clip, ema)), base + 12),
                ("norm", norm_alone, 4)]
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# arenas of %s: %d elements (%.1f MB each); %d warm-up + %d timed windows per arm, arms alternating; a window is %d "
           "back-to-back repetitions, all times are per repetition" % (o.model, n, n * 4e-6, o.warmup, o.reps, o.inner))
    busy = torch.randn(4096, 4096, device=dev)
    for family, step, base in (("sgd", sgd, 20), ("adamw", adam, 28)):
        arms = arms_of(step, base)
        for mode in ("call", "device"):
            evs = [[] for _ in arms]
            for r in range(o.warmup + o.reps):
                for k, (_, fn, _) in enumerate(arms):
                    if mode == "device":
                        torch.mm(busy, busy)
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    for _ in range(o.inner):
                        fn()
                    b.record()
                    if r >= o.warmup:
                        evs[k].append((a, b))
                torch.cuda.synchronize()
            log(f, "## %s, %s time" % (family, mode))
            means = {}
            for (name, _, nbytes), e in zip(arms, evs):
                ms = torch.tensor([a.elapsed_time(b) / o.inner for a, b in e], dtype=torch.float64)
                means[name] = float(ms.mean())
                rate = nbytes * n / float(ms.mean()) * 1e3
                log(f, "%-6s mean %.4f ms  median %.4f  min %.4f  max %.4f  std %.4f   %2d B/param -> %.2f TB/s at the mean = %.2f "
                       "of the 8 TB/s peak, %.2f of the 6.29 TB/s copy rate" %
                    (name, ms.mean(), ms.median(), ms.min(), ms.max(), ms.std(), nbytes, rate * 1e-12, rate / HBM_PEAK,
                     rate / HBM_COPY))
            log(f, "over plain: clip %+.4f ms (norm alone %.4f), ema %+.4f ms, both %+.4f ms; expected from bytes at plain's rate: "
                   "clip %+.4f, ema %+.4f, both %+.4f" %
                (means["clip"] - means["plain"], means["norm"], means["ema"] - means["plain"], means["both"] - means["plain"],
                 means["plain"] * 4 / base, means["plain"] * 8 / base, means["plain"] * 12 / base))
    if f is not None:
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
