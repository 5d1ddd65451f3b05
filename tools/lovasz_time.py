"""Timing of the criterion on the GPU (not a test): forward plus backward of

    A = CrossEntropyLoss(weight)                                  iswm_loss_fwd + finalize, then iswm_loss_bwd_scale       33 B/pixel
    B = LovaszSoftmaxLoss(ce_weight=1, lovasz_weight=1, weight)   keys, count, 4 x (digit count + scan + scatter), weights,
                                                                  loss, then bwd                                          130 B/pixel

    python tools/lovasz_time.py [--batch 16] [--size 513] [--reps 20] [--out profiles/lovasz_time.txt]

at [batch, 2, size, size] logits with uint8 labels, the method of tools/ohem_time.py: both arms in one process, alternating, timed
with device events after 3 warm-up repetitions; logits and labels rotate through a ring of buffers larger than the 256 MiB
Infinity Cache, so no arm reads a tensor the previous repetition left on the die.  Bytes per pixel at C = 2 (one foreground
class), uint8 labels, by the source: A reads 8 + 1 and writes 8 (forward), then reads and writes 8 (scale) = 33; B reads 8 + 1 and
writes 4 (keys), reads 4 (count), per digit reads 4 (digit count) and reads and writes 4 + 4 (scatter; the first reads no index:
4 x 20 - 4 = 76), reads 4 (g count), reads 4 + 4 and writes 4 (apply), then reads 8 + 1 + 4 and writes 8 (backward) = 130.  The
tile tables are 1/16 of a byte per pixel and digit.  The yardstick is arm A in the same run; arm A's run-to-run spread is printed
next to the difference.  --trace_reps N instead runs arm B N times and nothing else, for a kernel trace collected in a run of
its own."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20
BYTES_A, BYTES_B = 33, 130


def log(f, *a):
    s = " ".join(str(v) for v in a)
    print(s, flush=True)
    if f is not None:
        f.write(s + "\n")
        f.flush()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace_reps", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("lovasz_time.py measures on the GPU; there is nothing to measure without one")
    from iswm_amd.utils.loss import CrossEntropyLoss, LovaszSoftmaxLoss
    if o.out and os.path.dirname(o.out):
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
    f = open(o.out, "w") if o.out else None
    dev = torch.device("cuda:0")
    npix = o.batch * o.size * o.size
    per_set = npix * (2 * 4 + 1 + 2 * 4)                        # logits, labels and the gradient
    ring = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn(o.batch, 2, o.size, o.size, device=dev, generator=g).requires_grad_(True) for _ in range(ring)]
    ys = []
    for _ in range(ring):
        y = (torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.05).to(torch.uint8)
        y[torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.05] = 255
        ys.append(y)
    w = torch.tensor([1.0, 3.0])
    lov = LovaszSoftmaxLoss(ce_weight=1.0, lovasz_weight=1.0, weight=w).to(dev)
    if o.trace_reps:
        for r in range(o.trace_reps):
            zs[r % ring].grad = None
            lov(zs[r % ring], ys[r % ring]).backward()
        torch.cuda.synchronize()
        return 0
    arms = [("A CrossEntropyLoss", CrossEntropyLoss(weight=w).to(dev)), ("B LovaszSoftmaxLoss", lov)]
    nbytes = [BYTES_A, BYTES_B]
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# criterion forward + backward, logits [%d, 2, %d, %d] fp32, uint8 labels (%d pixels, 5 %% foreground); B: ce_weight 1, "
           "lovasz_weight 1, foreground; ring of %d operand sets (%d MiB); %d warm-up + %d timed repetitions per arm, arms alternating"
        % (o.batch, o.size, o.size, npix, ring, ring * per_set >> 20, o.warmup, o.reps))
    lov(zs[0], ys[0])
    log(f, "# present (image, class) pairs of these inputs: %d; B moves %d B/pixel, A %d: expected B / A from bytes %.2f" %
        (int(lov.last_present), BYTES_B, BYTES_A, BYTES_B / BYTES_A))
    busy = torch.randn(4096, 4096, device=dev)
    # "call": the events sit right around the criterion's calls, so the time includes whatever the host makes the device wait.
    # "device": a matrix product is enqueued first, the host runs ahead while the device works on it, and the criterion's
    # launches then execute back to back between the two events -- the kernels' own time, launch gaps included, host excluded.
    for mode in ("call", "device"):
        evs = [[] for _ in arms]
        for r in range(o.warmup + o.reps):
            for k, (_, crit) in enumerate(arms):
                i = (r * len(arms) + k) % ring
                zs[i].grad = None
                if mode == "device":
                    torch.mm(busy, busy)
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                crit(zs[i], ys[i]).backward()
                b.record()
                if r >= o.warmup:
                    evs[k].append((a, b))
            torch.cuda.synchronize()
        stats = []
        log(f, "## %s time" % mode)
        for (name, _), e, nb in zip(arms, evs, nbytes):
            ms = torch.tensor([a.elapsed_time(b) for a, b in e], dtype=torch.float64)
            stats.append(ms)
            log(f, "%-24s mean %.4f ms  median %.4f  min %.4f  max %.4f  std %.4f   %.1f B/pixel -> %.2f TB/s at the mean, "
                   "%.2f at the min" % (name, ms.mean(), ms.median(), ms.min(), ms.max(), ms.std(), nb,
                                        nb * npix / float(ms.mean()) * 1e-9, nb * npix / float(ms.min()) * 1e-9))
        a, b = stats
        log(f, "B / A = %.2f (means), %.2f (medians); expected from bytes %.2f; B - A = %+.4f ms; arm A's own spread: std %.4f ms, "
               "range %.4f ms" % (float(b.mean() / a.mean()), float(b.median() / a.median()), nbytes[1] / nbytes[0],
                                  float(b.mean() - a.mean()), a.std(), a.max() - a.min()))
    if f is not None:
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
