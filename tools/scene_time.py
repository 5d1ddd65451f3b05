"""Sliding-window scene prediction timing on one GPU: deeplabv3plus_resnet101, output stride 16,
a synthetic 4096^2 scene in 513^2 windows with 64 pixels of overlap, 16 windows per device batch.

    python tools/scene_time.py [--out profiles/scene_time.txt] [--side 4096] [--skip-whole]

One process; every figure is the median (min - max) of ROUNDS device-event windows after a warm-up of the same shapes.
1. k_scene_tiles_normalize (one batch of 16 windows) and k_scene_maps (all windows of the scene) alone, each window
   covering REPS back-to-back calls (their enqueue included), with algorithmic bytes and GB/s against 8 TB/s;
2. scenes/s through predict.ScenePredictor (upload, every window batch, scene_maps, the copy back, wait()) and the
   share of k_scene_maps in it;
3. the same scene through predict.DevicePredictor -- the whole-frame path, which is what the command line did with a
   frame of any size before --tile_size -- alternated with ScenePredictor, round by round.  It comes last: a whole
   4096^2 frame is outside what the kernels' planners were measured for, and the lines above are written out first.
"""
import argparse
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops, predict  # noqa: E402
from iswm_amd.network import modeling  # noqa: E402

PEAK = 8e12
TILE, OVERLAP, TILE_BATCH = 513, 64, 16
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--side", type=int, default=4096)
    ap.add_argument("--skip-whole", action="store_true", help="leave out part 3")
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
    S = args.side
    plan = ops.scene_plan(S, S, TILE, OVERLAP)
    say("scene_time: deeplabv3plus_resnet101 os16, %dx%d scene, %dx%d windows of %dx%d every %d (overlap %d), "
        "%d windows per batch, %s" % (S, S, plan.nty, plan.ntx, plan.th, plan.tw, plan.sy, OVERLAP, TILE_BATCH,
                                      torch.cuda.get_device_name()))
    rng = np.random.default_rng(0)
    small = rng.integers(0, 256, (S // 8 + 2, S // 8 + 2, 3), dtype=np.uint8)
    from PIL import Image
    frame = np.array(Image.fromarray(small).resize((S, S), Image.BILINEAR))       # smooth content, a writable copy
    scene = torch.from_numpy(frame).to(dev)

    # 1. the two kernels alone
    count = min(TILE_BATCH, plan.ntiles)
    with torch.no_grad():
        yl = model.forward_lowres(ops.scene_tiles_normalize(scene, plan, 0, count, predict.MEAN, predict.STD))
    _, hl, wl, ld = yl.shape
    logits = torch.randn((plan.ntiles, hl, wl, ld), device=dev) * 3.0
    t_n = windows(lambda: ops.scene_tiles_normalize(scene, plan, 0, count, predict.MEAN, predict.STD), 20)
    t_m = windows(lambda: ops.scene_maps(logits, 2, 1, plan, 0.5, 0.2, 0.7), 20)
    b_n = count * plan.th * plan.tw * (3 + 12)
    b_m = plan.ntiles * hl * wl * ld * 4 + 3 * S * S
    say("1. kernels alone, ms per call, median (min - max) of %d windows of 20 calls:" % ROUNDS)
    say("   scene_tiles_normalize, %2d windows      %s  %6.1f MB  %7.1f GB/s (%.1f %% of 8 TB/s)" %
        (count, mmm(t_n), b_n / 1e6, b_n / statistics.median(t_n) / 1e6, 100 * b_n / (statistics.median(t_n) * 1e-3) / PEAK))
    say("   scene_maps, %3d windows of %dx%dx%d   %s  %6.1f MB  %7.1f GB/s (%.1f %% of 8 TB/s)" %
        (plan.ntiles, hl, wl, ld, mmm(t_m), b_m / 1e6, b_m / statistics.median(t_m) / 1e6,
         100 * b_m / (statistics.median(t_m) * 1e-3) / PEAK))

    # 2. scenes/s through ScenePredictor
    batch = frame[None]
    tiled = predict.ScenePredictor(model, dev, 2, 1, 0.5, 0.2, 0.7, True, True, TILE, OVERLAP, tile_batch=TILE_BATCH)
    t_s = windows(lambda: tiled(batch)(), 1, warm=2)
    med = statistics.median(t_s)
    say("2. ScenePredictor (upload, %d batches, scene_maps, copy back, wait), ms per scene: %s  = %.2f scenes/s; "
        "scene_maps is %.2f %% of it" % ((plan.ntiles + TILE_BATCH - 1) // TILE_BATCH, mmm(t_s), 1e3 / med,
                                        100 * statistics.median(t_m) / med))
    if args.skip_whole:
        return

    # 3. the whole-frame path on the same scene, alternated
    whole = predict.DevicePredictor(model, dev, 2, 1, 0.5, 0.2, 0.7, True, True)
    say("3. whole-frame DevicePredictor on the same scene, alternated with ScenePredictor:")
    torch.cuda.reset_peak_memory_stats()
    res_w = whole(batch)()
    mem_w = torch.cuda.max_memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res_t = tiled(batch)()
    mem_t = torch.cuda.max_memory_allocated()
    t_w, t_t = [], []
    for _ in range(ROUNDS):
        t_w += windows(lambda: whole(batch)(), 1, rounds=1, warm=0)
        t_t += windows(lambda: tiled(batch)(), 1, rounds=1, warm=0)
    say("   whole frame  %s ms  = %.2f scenes/s" % (mmm(t_w), 1e3 / statistics.median(t_w)))
    say("   tiled        %s ms  = %.2f scenes/s  (%.2fx the whole-frame time)" %
        (mmm(t_t), 1e3 / statistics.median(t_t), statistics.median(t_t) / statistics.median(t_w)))
    say("   peak device memory: whole frame %.1f GB, tiled %.1f GB; the masks of the two paths agree on %.2f %% of the "
        "pixels (random weights, and the paths see different context: they are not expected to agree)" %
        (mem_w / 1e9, mem_t / 1e9, 100.0 * float((res_w["pred"] == res_t["pred"]).mean())))


if __name__ == "__main__":
    main()
