"""Inference timing on one GPU: deeplabv3plus_resnet101, output stride 16, 513^2 frames.

    python tools/predict_time.py [--out profiles/predict_time.txt] [--maps-only]

The event windows of part 1 cover back-to-back calls and include their enqueue; the kernels' own durations come from
a separate run of part 1 alone: rocprofv3 --kernel-trace --stats -d DIR -- python tools/predict_time.py --maps-only

1. the fused maps kernel (ops.predict_maps) against the unfused composition it replaces (the model's final upsample
   to NCHW logits -> torch.softmax -> [:, 1] -> > thr / * 255 -> uint8 / band compare), 16 x 513^2, device events;
   algorithmic bytes and GB/s against 8 TB/s for both;
2. device images/s of normalize + forward_lowres + maps + one copy back, batch 16 and batch 1, against the
   reference's per-image path on the same model (host-normalised fp32 upload, model(x), softmax, compare, .cpu());
3. end-to-end images/s of process_images (the CLI's loop) over 64 generated 513^2 PNGs, --workers 8, with and
   without --save_confidence --save_binary.
"""
import argparse
import contextlib
import io
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops, predict  # noqa: E402
from iswm_amd.network import modeling  # noqa: E402

PEAK = 8e12
H = W = 513


def timed(fn, reps, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def unfused(yl, nc, thr, lo, hi):
    logits = ops.bilinear_to_nchw_fwd(yl, nc, H, W)
    p = torch.softmax(logits, dim=1)[:, 1]
    pred = (p > thr).float()
    conf = (p * 255).to(torch.uint8)
    band = ((conf >= lo) & (conf <= hi)).to(torch.uint8) * 255
    return pred, conf, band


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--maps-only", action="store_true", help="part 1 only (for a kernel-trace run)")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = modeling.deeplabv3plus_resnet101(num_classes=2, output_stride=16).to(dev).eval()
    say("predict_time: deeplabv3plus_resnet101 os16, %dx%d, %s" % (H, W, torch.cuda.get_device_name()))

    # 1. maps kernel vs unfused
    n = 16
    rng = np.random.default_rng(0)
    u8 = torch.from_numpy(rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)).to(dev)
    with torch.no_grad():
        x = ops.predict_normalize(u8, predict.MEAN, predict.STD)
        yl = model.forward_lowres(x)
        lo, hi = ops.band_bounds(0.2, 0.7)
        t_f = timed(lambda: ops.predict_maps(yl, 2, 1, H, W, 0.5, 0.2, 0.7), 50)
        t_u = timed(lambda: unfused(yl, 2, 0.5, lo, hi), 20)
    _, hl, wl, ld = yl.shape
    px = n * H * W
    b_f = n * hl * wl * ld * 4 + 3 * px
    # unfused, per op: upsample (read yl, write 8 B/px), softmax (8 + 8), slice+compare (4 + 4 float), *255 (4 + 4),
    # cast (4 + 1), band compares / and / cast / *255 (1+1, 1+1, 2+1, 1+1, 1+1)
    b_u = n * hl * wl * ld * 4 + px * (8 + 16 + 8 + 8 + 5 + 11)
    say("1. maps, %d x %dx%d from %dx%dx%d logits:" % (n, H, W, hl, wl, ld))
    say("   fused predict_maps  %8.3f ms  %6.1f MB  %7.1f GB/s  (%.1f %% of 8 TB/s)" %
        (t_f, b_f / 1e6, b_f / t_f / 1e6, 100 * b_f / (t_f * 1e-3) / PEAK))
    say("   unfused composition %8.3f ms  %6.1f MB  %7.1f GB/s  (%.1f %% of 8 TB/s)   fused is %.1fx faster" %
        (t_u, b_u / 1e6, b_u / t_u / 1e6, 100 * b_u / (t_u * 1e-3) / PEAK, t_u / t_f))

    if args.maps_only:
        return

    # 2. device images/s
    def device_batch(bs):
        host = torch.from_numpy(rng.integers(0, 256, (bs, H, W, 3), dtype=np.uint8)).pin_memory()
        lay = ops.predict_maps_layout(bs, H, W)
        out = torch.empty(lay["end"], dtype=torch.uint8, pin_memory=True)

        def run():
            with torch.no_grad():
                xx = ops.predict_normalize(host.to(dev, non_blocking=True), predict.MEAN, predict.STD)
                m = ops.predict_maps(model.forward_lowres(xx), 2, 1, H, W, 0.5, 0.2, 0.7)
                out.copy_(m.packed, non_blocking=True)
        return run

    def reference_image():
        img = torch.from_numpy(rng.integers(0, 256, (H, W, 3), dtype=np.uint8))
        xh = img.permute(2, 0, 1).float().div(255)
        xh = xh.sub(torch.tensor(predict.MEAN)[:, None, None]).div(torch.tensor(predict.STD)[:, None, None])[None]

        def run():
            with torch.no_grad():
                logits = model(xh.to(dev))
                p = torch.softmax(logits, dim=1)[:, 1]
                pred = (p > 0.5).float()
                p.cpu()
                pred.cpu()
        return run

    say("2. device images/s (normalize + forward_lowres + maps + copy back):")
    for bs, reps in ((16, 6), (1, 30)):
        t = timed(device_batch(bs), reps, warm=2)
        say("   batch %2d: %8.2f ms/batch  %7.1f images/s" % (bs, t, bs * 1e3 / t))
    t = timed(reference_image(), 30, warm=2)
    say("   reference per-image path (fp32 upload, model(x), softmax, compare, .cpu()): %8.2f ms  %7.1f images/s" %
        (t, 1e3 / t))

    # 3. end to end
    say("3. process_images over 64 PNGs of %dx%d, --workers 8:" % (H, W))
    from PIL import Image
    with tempfile.TemporaryDirectory() as tmp:
        src = os.path.join(tmp, "in", "seq")
        os.makedirs(src)
        for k in range(64):
            base = rng.integers(0, 256, (H // 8 + 2, W // 8 + 2, 3), dtype=np.uint8)
            Image.fromarray(base).resize((W, H), Image.BILINEAR).save(os.path.join(src, "f%03d.png" % k))
        for bs in (1, 16):
            for extra in (False, True):
                pr = predict.DevicePredictor(model, dev, 2, 1, 0.5, 0.2, 0.7, extra, extra)
                with contextlib.redirect_stdout(io.StringIO()):
                    predict.process_images(os.path.dirname(src), os.path.join(tmp, "warm"), pr, extra, extra,
                                           batch_size=bs, workers=8, progress=False)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    done = predict.process_images(os.path.dirname(src), os.path.join(tmp, "out"), pr, extra, extra,
                                                  batch_size=bs, workers=8, progress=False)
                    dt = time.perf_counter() - t0
                say("   --batch_size %2d %-34s %6.2f s  %6.1f images/s" %
                    (bs, "--save_confidence --save_binary" if extra else "(predict masks only)", dt, done / dt))

    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
