"""Timing of the CRF refinement on the GPU (not a test): ops.crf_refine at R = 5, D = 2, T = 5 (the defaults) next to ops.predict_maps
and ops.prob_maps at the same size, for scale.

    python tools/crf_time.py [--sizes 513,1024] [--reps 30] [--out FILE]

Device events around each arm, all arms in one process and alternating, after 3 warm-up repetitions; the operands rotate through a
ring of buffers; a matrix product is enqueued in front of every timed arm, so the host runs ahead and the arm's launches execute
back to back between the two events.  Reported: microseconds per frame and per iteration (median and range over the repetitions) and
the implied neighbour evaluations per second, H W ((2R+1)^2 - 1) per iteration (the count inside the image is a little lower: the
border pixels' windows are cut)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

R, D, T = 5, 2, 5


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="513,1024")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--ring", type=int, default=8)
    ap.add_argument("--out", default=None)
    o = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise RuntimeError("tools/crf_time.py needs a GPU")
    from iswm_amd import ops
    dev = torch.device("cuda")
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    filler = torch.randn((2048, 2048), device=dev)
    for size in (int(s) for s in o.sizes.split(",")):
        g = torch.Generator(device="cpu").manual_seed(size)
        hl = (size + 3) // 4
        ring = []
        for _ in range(o.ring):
            yl = (torch.randn((1, hl, hl, 4), generator=g) * 3.0).to(dev)
            low = torch.randint(0, 256, (1, 3, size // 8 + 2, size // 8 + 2), generator=g).float()
            img = torch.nn.functional.interpolate(low, size=(size, size), mode="bilinear").permute(0, 2, 3, 1).round().clamp(0, 255)
            img = (img + torch.randint(0, 12, img.shape, generator=g)).clamp(0, 255).to(torch.uint8).contiguous().to(dev)
            prob = ops.predict_maps(yl, 2, 1, size, size, 0.5, 0.2, 0.7, want_prob=True).prob
            ring.append((yl, img, prob))
        arms = [("crf_refine T=%d" % T, lambda i: ops.crf_refine(ring[i][2], ring[i][1], T, R, D)),
                ("crf_refine T=1", lambda i: ops.crf_refine(ring[i][2], ring[i][1], 1, R, D)),
                ("predict_maps", lambda i: ops.predict_maps(ring[i][0], 2, 1, size, size, 0.5, 0.2, 0.7)),
                ("prob_maps", lambda i: ops.prob_maps(ring[i][2], 0.5, 0.2, 0.7))]
        times = {name: [] for name, _ in arms}
        for rep in range(o.reps + 3):
            for name, fn in arms:
                i = rep % o.ring
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                filler @ filler
                a.record()
                fn(i)
                b.record()
                b.synchronize()
                if rep >= 3:
                    times[name].append(a.elapsed_time(b) * 1e3)
        log("%d x %d, R=%d D=%d, %d repetitions" % (size, size, R, D, o.reps))
        for name, _ in arms:
            t = sorted(times[name])
            log("  %-16s median %9.1f us  (min %9.1f, max %9.1f)" % (name, t[len(t) // 2], t[0], t[-1]))
        t5 = sorted(times["crf_refine T=%d" % T])[o.reps // 2]
        nb = size * size * ((2 * R + 1) ** 2 - 1)
        log("  per iteration %.1f us; %.3g neighbour evaluations per second" % (t5 / T, nb * T / (t5 * 1e-6)))
    if o.out:
        os.makedirs(os.path.dirname(os.path.abspath(o.out)), exist_ok=True)
        with open(o.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
