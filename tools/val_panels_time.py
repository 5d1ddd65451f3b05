"""Timing of the validation image panels on one GPU.

    python tools/val_panels_time.py [--out profiles/val_panels_time.txt]

1. iswm_val_panels (ops.val_panels, all outputs on) at N = 16, 513^2, C = 2 and, in the same process at the same
   shape, iswm_predict_maps (ops.predict_maps) as the yardstick: one pair of device events per launch after a warm-up,
   the median over the launches, algorithmic bytes and bytes/s of each;
2. the wall time of one save_validation_results pass over the synthetic validation split (deeplabv3plus_resnet50,
   crop 513, 8 tiles in batches of 4, --save_confidence_map), PNG encoding included.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops, train, val_results  # noqa: E402
from iswm_amd.network import modeling  # noqa: E402

H = W = 513
N = 16


def median_ms(fn, reps=50, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2], times[0], times[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    say("val_panels_time: %d x %dx%d, C = 2, %s" % (N, H, W, torch.cuda.get_device_name()))
    hl = wl = 33
    ld = 4
    yl = (torch.randn((N, hl, wl, ld), generator=g) * 3.0).to(dev)
    u8 = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8).to(dev)
    x = ops.predict_normalize(u8, val_results.MEAN, val_results.STD)
    lab = (torch.rand((N, H, W), generator=g) < 0.1).to(torch.uint8).to(dev)
    px = N * H * W
    logits = N * hl * wl * ld * 4
    t_v = median_ms(lambda: ops.val_panels(x, yl, lab, 2, val_results.MEAN, val_results.STD))
    t_p = median_ms(lambda: ops.predict_maps(yl, 2, 1, H, W, 0.5, 0.2, 0.7))
    b_v = logits + px * (12 + 1) + px * (5 * 3 + 2)           # x fp32 x 3 + label; five RGB panels + pred + conf
    b_p = logits + px * 3                                     # pred, conf, band
    say("1. median of 50 launches (min .. max), device events around each launch:")
    say("   val_panels   %8.3f ms (%.3f .. %.3f)  %6.1f MB  %7.1f GB/s" % (t_v + (b_v / 1e6, b_v / t_v[0] / 1e6)))
    say("   predict_maps %8.3f ms (%.3f .. %.3f)  %6.1f MB  %7.1f GB/s" % (t_p + (b_p / 1e6, b_p / t_p[0] / 1e6)))

    model = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16).to(dev)
    val = train.SyntheticBinarySegmentation(split='val', size=H, length=8, seed=1)
    loader = torch.utils.data.DataLoader(val, batch_size=4, shuffle=False, num_workers=0)
    with tempfile.TemporaryDirectory() as tmp:
        opts = types.SimpleNamespace(val_results_dir=tmp, save_confidence_map=True, num_workers=2, num_classes=2)
        for it in (0, 1):                                      # the first pass warms the model up
            with contextlib.redirect_stdout(io.StringIO()):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                n = val_results.save_validation_results(model, loader, dev, opts, it, 0.5)
                dt = time.perf_counter() - t0
        files = sum(len(f) for _, _, f in os.walk(tmp))
    say("2. save_validation_results, 8 synthetic %dx%d tiles in batches of 4, 2 encoder threads: %.2f s for %d frames "
        "(%d PNGs written in both passes)" % (H, W, dt, n, files))

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
