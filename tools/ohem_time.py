"""Timing of the criterion on the GPU (not a test): forward plus backward of

    A = CrossEntropyLoss(weight)                                  iswm_loss_fwd + finalize, then iswm_loss_bwd_scale      33 B/pixel
    B = OhemCrossEntropyLoss(thresh, min_kept, weight)            keys, 3 x (hist + scan), sums, loss, then bwd     43 B/pixel + 8 per kept pixel

    python tools/ohem_time.py [--batch 16] [--size 513] [--thresh 0.7] [--min_kept 100000] [--reps 20] [--out profiles/ohem_time.txt]

at [batch, 2, size, size] logits with uint8 labels, the method of tools/overlap_loss_time.py: both arms in one process, alternating,
timed with device events after 3 warm-up repetitions; logits and labels rotate through a ring of buffers larger than the 256 MiB
Infinity Cache, so no arm reads a tensor the previous repetition left on the die.  Bytes per pixel at C = 2, uint8 labels, by the
source: A reads 8 + 1 and writes 8 (forward), then reads and writes 8 (scale) = 33; B reads 8 + 1 and writes 4 (keys), reads 4 three
times (one histogram per digit), reads 4 + 1 (sums), then reads 4 + 1, reads 8 only where the pixel is kept, and writes 8
(backward) = 43 + 8 x the kept fraction.  The yardstick is arm A in the same run; arm A's run-to-run spread is printed next to the
difference.  --trace_reps N instead runs arm B N times and nothing else, for a kernel trace collected in a run of its own."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20
BYTES_A, BYTES_B, BYTES_B_KEPT = 33, 43, 8


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
    ap.add_argument("--thresh", type=float, default=0.7)
    ap.add_argument("--min_kept", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--trace_reps", type=int, default=0)
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("ohem_time.py measures on the GPU; there is nothing to measure without one")
    from iswm_amd.utils.loss import CrossEntropyLoss, OhemCrossEntropyLoss
    if o.out and os.path.dirname(o.out):
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
    f = open(o.out, "w") if o.out else None
    dev = torch.device("cuda:0")
    npix = o.batch * o.size * o.size
    per_set = npix * (2 * 4 + 1 + 2 * 4 + 4)                   # logits, labels, the gradient and the keys the arm allocates
    ring = max(2, -(-RING_BYTES // per_set))
    g = torch.Generator(device=dev).manual_seed(0)
    zs = [torch.randn(o.batch, 2, o.size, o.size, device=dev, generator=g).requires_grad_(True) for _ in range(ring)]
    ys = []
    for _ in range(ring):
        y = (torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.1).to(torch.uint8)
        y[torch.rand(o.batch, o.size, o.size, device=dev, generator=g) < 0.05] = 255
        ys.append(y)
    w = torch.tensor([1.0, 3.0])
    ohem = OhemCrossEntropyLoss(thresh=o.thresh, min_kept=o.min_kept, weight=w).to(dev)
    if o.trace_reps:
        for r in range(o.trace_reps):
            zs[r % ring].grad = None
            ohem(zs[r % ring], ys[r % ring]).backward()
        torch.cuda.synchronize()
        return 0
    arms = [("A CrossEntropyLoss", CrossEntropyLoss(weight=w).to(dev)), ("B OhemCrossEntropyLoss", ohem)]
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# criterion forward + backward, logits [%d, 2, %d, %d] fp32, uint8 labels (%d pixels); B: thresh %g, min_kept %d; ring "
           "of %d operand sets (%d MiB); %d warm-up + %d timed repetitions per arm, arms alternating" %
        (o.batch, o.size, o.size, npix, o.thresh, o.min_kept, ring, ring * per_set >> 20, o.warmup, o.reps))
    ohem(zs[0], ys[0])
    frac = float(ohem.last_kept) / npix
    nbytes = [BYTES_A, BYTES_B + BYTES_B_KEPT * frac]
    log(f, "# kept fraction of these inputs: %.4f -> B moves %.1f B/pixel, A %d: expected B / A from bytes %.2f" %
        (frac, nbytes[1], BYTES_A, nbytes[1] / BYTES_A))
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
