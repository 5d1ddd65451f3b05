"""INT8 against FP32 inference timing on one GPU: output stride 16, 16 x 513^2 frames.

    python tools/quant_time.py [--out profiles/quant_time.txt] [--reps 10]

For r50 and r101 (DeepLabV3+, oracle.synth weights, calibrated on two 4 x 513^2 batches) the device images/s of
normalize + forward_lowres + predict_maps + one copy of the masks back, FP32 and INT8 alternated in one process,
timed with device events over back-to-back batches.  Per-kernel durations: a separate
rocprofv3 --kernel-trace --stats run of this script.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd import ops, quant  # noqa: E402
from iswm_amd.network import modeling  # noqa: E402
from iswm_amd.predict import MEAN, STD  # noqa: E402
from oracle.synth import ArchCfg, synth_state_dict  # noqa: E402

B, H, W = 16, 513, 513


def run(model, img, host):
    x = ops.predict_normalize(img, MEAN, STD)
    maps = ops.predict_maps(model.forward_lowres(x), 2, 1, H, W, 0.5, 0.2, 0.7)
    host.copy_(maps.pred.view(-1), non_blocking=True)


def time_it(model, img, host, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        run(model, img, host)
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    dev = torch.device("cuda")
    g = torch.Generator().manual_seed(0)
    img = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, generator=g).to(dev)
    host = torch.empty(B * H * W, dtype=torch.uint8, pin_memory=True)
    lines = []
    for bb in ("resnet50", "resnet101"):
        m = getattr(modeling, "deeplabv3plus_" + bb)(num_classes=2, output_stride=16, pretrained_backbone=False)
        m.load_state_dict(synth_state_dict(ArchCfg("deeplabv3plus", bb, 2, 16)), strict=True)
        m = m.to(dev).eval()
        with torch.no_grad():
            cal = [ops.predict_normalize(img[4 * i:4 * i + 4], MEAN, STD) for i in range(2)]
            qm = quant.quantize_model(m, quant.calibrate(m, cal))
            for model in (m, qm):                              # warm-up
                run(model, img, host)
            t = {"fp32": [], "int8": []}
            for _ in range(3):                                 # alternated
                t["fp32"].append(time_it(m, img, host, a.reps))
                t["int8"].append(time_it(qm, img, host, a.reps))
        best = {k: min(v) for k, v in t.items()}
        line = "deeplabv3plus_%s os16 %dx%d^2: fp32 %.2f ms/batch = %.0f images/s | int8 %.2f ms/batch = %.0f images/s | x%.2f" % (
            bb, B, H, best["fp32"], 1e3 * B / best["fp32"], best["int8"], 1e3 * B / best["int8"], best["fp32"] / best["int8"])
        print(line, flush=True)
        lines.append(line)
        del m, qm
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
