"""Timing of the boundary validation metrics on the GPU (not a test), next to the route the code base offered before them:

    N = new call:   iswm_boundary_metrics (k_bm_contours, k_bm_columns, k_bm_rows, k_bm_finalize)   one call, both directions
    E = four maps:  iswm_signed_edt of the predicted masks, of the label masks and of their two contour images as labels: the
                    full-plane maps a host would sample at the other contour's pixels (the contour images are made outside the
                    timed region, and the sampling and the reductions are not timed either: the route's floor)

    python tools/boundary_metrics_time.py [--batch 16] [--size 513] [--reps 20] [--out FILE]      device events around each arm
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/boundary_metrics_time.py --kernels-only   kernel times, a run of its own
    python tools/boundary_metrics_time.py --trainer                      wall time of a --test_only validation, switch off and on

at uint8 [batch, size, size], two classes, the foreground plane: the band labels of tools/boundary_loss_time.py and a prediction
shifted by 3 pixels, and a batch whose labels are background only (no label contour: every predicted contour pixel searches its
whole row and finds nothing).  The method of tools/boundary_loss_time.py: all arms in one process, alternating, after 3 warm-up
repetitions; the operands rotate through a ring of buffers larger than the 256 MiB Infinity Cache; a matrix product is enqueued
in front of every timed arm, so the host runs ahead and the arm's launches execute back to back between the two events."""
import argparse
import importlib.util
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

RING_BYTES = 640 << 20


def _sibling():
    spec = importlib.util.spec_from_file_location("boundary_loss_time", os.path.join(ROOT, "tools", "boundary_loss_time.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def shifted(y, dy, dx):
    """the masks moved down by dy and right by dx, background coming in at the edge"""
    out = torch.zeros_like(y)
    h, w = y.shape[-2:]
    out[..., dy:, dx:] = y[..., :h - dy, :w - dx]
    return out


def arms(o, dev):
    from iswm_amd import ops
    sibling = _sibling()
    band, log = sibling.band_labels, sibling.log
    npix = o.batch * o.size * o.size
    per_set = npix * (2 + 2 + 4 * 8)                            # labels, predictions, two contour images, the maps and workspaces
    ring = max(2, -(-RING_BYTES // per_set))
    ys = [band(o.batch, o.size, dev, 10 + i) for i in range(ring)]
    ps = [shifted(y, 3, 0) if i % 2 else shifted(y, 0, 3) for i, y in enumerate(ys)]
    zeros = [torch.zeros_like(y) for y in ys[:2]]
    contour = lambda m: (ops.signed_edt(m, 2) == -1)[:, 0].to(torch.uint8)
    cy, cp = [contour(y) for y in ys], [contour(p) for p in ps]

    def four(p, y, sp, sy):
        return ops.signed_edt(p, 2), ops.signed_edt(y, 2), ops.signed_edt(sp, 2), ops.signed_edt(sy, 2)
    stats, dsum = ops.boundary_metrics(ps[0], ys[0], 2)
    n = stats[..., 0].double()
    info = "contour pixels per image: predicted %.0f, labelled %.0f of %d (%.2f %%); largest distance %.1f pixels" % (
        float(n[:, 0, 0].mean()), float(n[:, 0, 1].mean()), o.size * o.size, 100.0 * float(n.mean()) / (o.size * o.size),
        float(stats[..., 2].max()) ** 0.5)
    return [("N new, band", lambda i: ops.boundary_metrics(ps[i], ys[i], 2)),
            ("E four maps, band", lambda i: four(ps[i], ys[i], cp[i], cy[i])),
            ("N new, no label", lambda i: ops.boundary_metrics(ps[i], zeros[i % 2], 2)),
            ("E four maps, no label", lambda i: four(ps[i], zeros[i % 2], cp[i], zeros[i % 2]))], ring, npix, info, log


def time_arms(o, f, dev):
    table, ring, npix, info, log = arms(o, dev)
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    log(f, "# uint8 predictions and labels [%d, %d, %d] (%d pixels), 2 classes, the foreground plane, tolerance 2, percent 95; %s; "
           "ring of %d operand sets; %d warm-up + %d timed repetitions per arm, arms alternating" %
        (o.batch, o.size, o.size, npix, info, ring, o.warmup, o.reps))
    busy = torch.randn(4096, 4096, device=dev)
    evs = [[] for _ in table]
    for r in range(o.warmup + o.reps):
        for k, (_, fn) in enumerate(table):
            i = (r * len(table) + k) % ring
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
        log(f, "ran %d repetitions of each arm (kernel times: the trace of this run)" % (o.warmup + o.reps))
        return
    med = {}
    for (name, _), e in zip(table, evs):
        ms = torch.tensor([a.elapsed_time(b) for a, b in e], dtype=torch.float64)
        med[name] = float(ms.median())
        log(f, "%-22s mean %.4f ms  median %.4f  min %.4f  max %.4f  std %.4f" % (name, ms.mean(), ms.median(), ms.min(), ms.max(),
                                                                                 ms.std()))
    for kind in ("band", "no label"):
        log(f, "%s: new call / four maps = %.2f at the median" % (kind, med["N new, " + kind] / med["E four maps, " + kind]))


def time_trainer(o, f, dev):
    """wall time of train.main(--test_only) on the synthetic validation set, the switch off and on, each after one warm-up run"""
    import contextlib
    import io
    from iswm_amd import train
    log = _sibling().log
    base = ["--model", o.model, "--crop_size", str(o.size), "--val_batch_size", str(o.batch), "--num_workers", "0", "--test_only"]
    log(f, "# %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    for name, flags in (("switch off", []), ("switch on", ["--val_boundary_metrics"])):
        times = []
        for _ in range(1 + o.runs):
            torch.cuda.synchronize()
            t0 = time.time()
            with contextlib.redirect_stdout(io.StringIO()) as out:
                train.main(base + flags)
            torch.cuda.synchronize()
            times.append(time.time() - t0)
        score = [l for l in out.getvalue().splitlines() if l.startswith("{")][-1]
        log(f, "%-10s %s --test_only, %d x %d tiles in batches of %d: %.3f s (the %d runs after the first: %s)" %
            (name, o.model, o.size, o.size, o.batch, sorted(times[1:])[len(times[1:]) // 2], o.runs,
             " ".join("%.3f" % t for t in times[1:])))
        log(f, "           %s" % score)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=513)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--trainer", action="store_true")
    ap.add_argument("--model", type=str, default="deeplabv3plus_mobilenet")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("boundary_metrics_time.py measures on the GPU; there is nothing to measure without one")
    if o.out and os.path.dirname(o.out):
        os.makedirs(os.path.dirname(o.out), exist_ok=True)
    f = open(o.out, "w") if o.out else None
    dev = torch.device("cuda:0")
    (time_trainer if o.trainer else time_arms)(o, f, dev)
    if f is not None:
        f.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
