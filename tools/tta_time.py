"""Flip and multi-scale test-time augmentation timing on one GPU: deeplabv3plus_resnet101, output
stride 16, 16 frames of 513^2, views (0.75, 1.0, 1.25) with flips: 6 views.

    python tools/tta_time.py [--out profiles/tta_time.txt] [--batch 16] [--side 513]

One process; every figure is the median (min - max) of ROUNDS device-event windows after a warm-up of the same shapes.
a. k_predict_view_normalize, one call per view, with algorithmic bytes (the uint8 taps read once, the fp32 view written)
   and GB/s against 8 TB/s;
b. k_predict_views_maps + k_predict_stats over the six views' logits against the unfused torch chain on the same
   logits -- per view interpolate, softmax, slice, flip, add; then divide, compare, x255, casts, band -- alternated
   round by round;
c. images/s through predict.TTAPredictor against predict.DevicePredictor on the same frames, alternated round by round;
d. peak device memory of the two predictors.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops, predict  # noqa: E402
from iswm_amd.network import modeling  # noqa: E402

PEAK = 8e12
SCALES, FLIP = (0.75, 1.0, 1.25), True
ROUNDS = 9


def windows(fn, reps, rounds=ROUNDS, warm=2):
    """ms per call: `rounds` event windows of `reps` calls each"""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return out


def mmm(v):
    return "%9.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


def unfused(yls, flips, H, W, thr, lo, hi):
    """the torch chain k_predict_views_maps replaces, on NHWC logits whose first two channels are the classes"""
    acc = None
    for y, f in zip(yls, flips):
        lg = F.interpolate(y[..., :2].permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=False)
        p = torch.softmax(lg, dim=1)[:, 1]
        if f:
            p = p.flip(-1)
        acc = p if acc is None else acc + p
    p = acc / float(len(yls))
    pred = (p > thr).to(torch.uint8) * 255
    conf = (p * 255).to(torch.uint8)
    band = ((conf >= lo) & (conf <= hi)).to(torch.uint8) * 255
    return pred, conf, band


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--side", type=int, default=513)
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:
            with open(args.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    dev = torch.device("cuda")
    torch.manual_seed(0)
    model = modeling.deeplabv3plus_resnet101(num_classes=2, output_stride=16).to(dev).eval()
    B, S = args.batch, args.side
    views = ops.tta_views(S, S, SCALES, FLIP)
    flips = [f for _, _, f in views]
    say("tta_time: deeplabv3plus_resnet101 os16, %d frames of %dx%d, views %s, %s" %
        (B, S, S, ", ".join("%dx%d%s" % (h, w, " flipped" if f else "") for h, w, f in views),
         torch.cuda.get_device_name()))
    rng = np.random.default_rng(0)
    from PIL import Image
    frames = np.stack([np.array(Image.fromarray(rng.integers(0, 256, (S // 8 + 2, S // 8 + 2, 3), dtype=np.uint8))
                                .resize((S, S), Image.BILINEAR)) for _ in range(B)])      # smooth content
    img = torch.from_numpy(frames).to(dev)

    # a. one view's network input
    say("a. predict_view_normalize, ms per call, median (min - max) of %d windows of 20 calls:" % ROUNDS)
    for hv, wv, f in views:
        t = windows(lambda: ops.predict_view_normalize(img, hv, wv, f, predict.MEAN, predict.STD), 20)
        nbytes = B * (3 * min(S * S, 4 * hv * wv) + 12 * hv * wv)
        med = statistics.median(t)
        say("   %4dx%-4d flip=%d  %s  %6.1f MB  %7.1f GB/s (%.1f %% of 8 TB/s)" %
            (hv, wv, f, mmm(t), nbytes / 1e6, nbytes / med / 1e6, 100 * nbytes / (med * 1e-3) / PEAK))

    # b. the gather against the unfused chain, on the network's own logits
    with torch.no_grad():
        yls = [model.forward_lowres(ops.predict_view_normalize(img, hv, wv, f, predict.MEAN, predict.STD))
               for hv, wv, f in views]
    lo, hi = ops.band_bounds(0.2, 0.7)
    fused = lambda: ops.predict_views_maps(yls, flips, 2, 1, S, S, 0.5, 0.2, 0.7)
    chain = lambda: unfused(yls, flips, S, S, 0.5, lo, hi)
    m = fused()
    pred, conf, band = chain()
    agree = [float((a == b).float().mean()) for a, b in ((m.pred, pred), (m.conf, conf), (m.band, band))]
    windows(fused, 5, rounds=1)
    windows(chain, 5, rounds=1)
    t_f, t_c = [], []
    for _ in range(ROUNDS):
        t_f += windows(fused, 10, rounds=1, warm=0)
        t_c += windows(chain, 10, rounds=1, warm=0)
    nbytes = sum(int(y.shape[0] * y.shape[1] * y.shape[2] * y.stride(2)) * 4 for y in yls) + 3 * B * S * S
    say("b. predict_views_maps + stats over %d views against the unfused torch chain, ms per call, %d alternated "
        "windows of 10 calls:" % (len(views), ROUNDS))
    say("   fused    %s  %6.1f MB  %7.1f GB/s" % (mmm(t_f), nbytes / 1e6, nbytes / statistics.median(t_f) / 1e6))
    say("   unfused  %s  = %.2fx the fused time; maps equal on %.4f / %.4f / %.4f of the pixels (pred / conf / band)" %
        (mmm(t_c), statistics.median(t_c) / statistics.median(t_f), agree[0], agree[1], agree[2]))

    # c., d. the predictors, alternated
    tta = predict.TTAPredictor(model, dev, 2, 1, 0.5, 0.2, 0.7, True, True, SCALES, FLIP)
    one = predict.DevicePredictor(model, dev, 2, 1, 0.5, 0.2, 0.7, True, True)
    torch.cuda.reset_peak_memory_stats()
    one(frames)()
    mem_o = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    tta(frames)()
    mem_t = torch.cuda.max_memory_allocated()
    for _ in range(2):
        one(frames)()
        tta(frames)()
    t_o, t_t = [], []
    for _ in range(ROUNDS):
        t_o += windows(lambda: one(frames)(), 1, rounds=1, warm=0)
        t_t += windows(lambda: tta(frames)(), 1, rounds=1, warm=0)
    mo, mt = statistics.median(t_o), statistics.median(t_t)
    work = sum(h * w for h, w, _ in views) / float(S * S)
    say("c. predictors on the same %d frames (upload, views, maps, copy back, wait), ms per batch, %d alternated windows:"
        % (B, ROUNDS))
    say("   DevicePredictor  %s  = %.1f images/s" % (mmm(t_o), 1e3 * B / mo))
    say("   TTAPredictor     %s  = %.1f images/s  = %.2fx the single-view time for %.2fx its pixels; the gather is "
        "%.2f %% of it" % (mmm(t_t), 1e3 * B / mt, mt / mo, work, 100 * statistics.median(t_f) / mt))
    say("d. peak device memory: DevicePredictor %.2f GB, TTAPredictor %.2f GB" % (mem_o / 1e9, mem_t / 1e9))
    say("kernel durations from a rocprofv3 kernel trace: not measured")


if __name__ == "__main__":
    main()
