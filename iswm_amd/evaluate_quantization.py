"""FP32 against INT8 evaluation -- runnable counterpart of the reference's evaluate_quantization.py.

    python -m iswm_amd.evaluate_quantization --fp32_ckpt best.pth --eval_data_dir val/ \\
        [--num_images N] [--output_stride 16] [--num_visualizations 20] [--results_dir evaluation_results]

`--eval_data_dir` holds `imgs/` and `masks/`; the mask of `imgs/<base><ext>` is `masks/<base>_mask<ext>` (mask > 0 is
foreground; a missing mask is all background, with a warning).  The FP32 model is calibrated (iswm_amd.quant, MinMax)
on the first 25 batches of 4 images, quantized, saved as `<ckpt base>_int8<ext>`, and both models are evaluated at
batch 1 through ops.predict_maps (threshold 0.5) into two StreamMetrics(2).  The report has the reference's rows; the
average time skips the first image and each time ends in a device synchronise.

Same flags and defaults as the reference's get_argparser.  Differences, all deliberate:
  * ``--model`` takes this project's constructors (default deeplabv3plus_resnet50, the reference's only model), built
    with ``pretrained_backbone=False`` -- the weights come from ``--fp32_ckpt``;
  * both models run on the GPU (the reference runs fbgemm on the CPU, and its conversion fails for want of a
    QuantStub, so it prints the FP32 column only);
  * the INT8 model size is the real size of the saved `_int8` file, not "fp32 / 4 (est.)";
  * the comparison image is a 2 x 2 PNG composed with PIL (image, ground truth, FP32, INT8), not a matplotlib figure;
  * ``module.`` prefixes are stripped as the reference does; a checkpoint may also be a bare state dict;
  * images of different sizes are refused with a clear error before any work (the reference's batch-of-4 DataLoader
    fails on them in its collate step, and StreamMetrics' front and temporal evaluators compare consecutive frames).
"""
import argparse
import logging
import os
import sys
import time

import numpy as np
from PIL import Image, ImageDraw

logger = logging.getLogger(__name__)

IMAGE_EXTS = ('.png', '.jpg', '.jpeg')
CALIB_BATCHES, CALIB_BATCH = 25, 4
THRESHOLD = 0.5


def get_argparser():
    from .predict import _model_names
    parser = argparse.ArgumentParser(description="FP32 vs. INT8 Model Evaluation Script")
    parser.add_argument("--fp32_ckpt", required=True, type=str, help="Path to the trained FP32 model checkpoint (.pth)")
    parser.add_argument("--eval_data_dir", required=True, type=str,
                        help="Path to the validation data directory (should contain 'imgs' and 'masks' subfolders)")
    parser.add_argument("--num_images", type=int, default=0,
                        help="Number of images to evaluate on. Default: 0 (all images)")
    parser.add_argument("--output_stride", type=int, default=16, help="Output stride for DeepLabV3+")
    parser.add_argument("--num_visualizations", type=int, default=20, help="Number of comparison images to generate.")
    parser.add_argument("--results_dir", type=str, default="evaluation_results",
                        help="Directory to save visualization images.")
    parser.add_argument("--model", type=str, default='deeplabv3plus_resnet50', choices=_model_names(),
                        help="model name")
    parser.add_argument("--use_ema", action='store_true',
                        help="evaluate and quantize the checkpoint's EMA weights (a checkpoint of train --ema_decay)")
    return parser


def pair_files(image_dir, mask_dir, num_images=0):
    """[(image name, image path, mask path or None)] in sorted name order, the first num_images when > 0"""
    names = sorted(f for f in os.listdir(image_dir) if f.lower().endswith(IMAGE_EXTS))
    if num_images > 0:
        names = names[:num_images]
    out = []
    for name in names:
        base, ext = os.path.splitext(name)
        mp = os.path.join(mask_dir, "%s_mask%s" % (base, ext))
        out.append((name, os.path.join(image_dir, name), mp if os.path.exists(mp) else None))
    return out


def load_sample(img_path, mask_path):
    """(uint8 [H, W, 3] RGB, uint8 [H, W] mask with values 0 / 1)"""
    with Image.open(img_path) as im:
        img = np.asarray(im.convert('RGB'))
    if mask_path is not None:
        with Image.open(mask_path) as m:
            mask = (np.asarray(m.convert('L')) > 0).astype(np.uint8)
    else:
        logger.warning("no mask for '%s': using an empty mask", os.path.basename(img_path))
        mask = np.zeros(img.shape[:2], dtype=np.uint8)
    return img, mask


def save_visual_comparison(img, gt, fp32_pred, int8_pred, out_dir, img_name):
    """2 x 2 PNG: image, ground truth, FP32 prediction, INT8 prediction (masks shown as 0 / 255)"""
    h, w = img.shape[:2]
    title = 20
    canvas = Image.new('RGB', (2 * w, 2 * (h + title)), (255, 255, 255))
    panels = [(img, "Original Image"), (gt, "Ground Truth Mask"), (fp32_pred, "FP32 Prediction"),
              (int8_pred, "INT8 Prediction")]
    draw = ImageDraw.Draw(canvas)
    for k, (a, label) in enumerate(panels):
        x0, y0 = (k % 2) * w, (k // 2) * (h + title)
        pic = Image.fromarray(a) if a.ndim == 3 else Image.fromarray((a > 0).astype(np.uint8) * 255).convert('RGB')
        canvas.paste(pic, (x0, y0 + title))
        draw.text((x0 + 4, y0 + 4), label, fill=(0, 0, 0))
    path = os.path.join(out_dir, "%s_comparison.png" % os.path.splitext(img_name)[0])
    canvas.save(path)
    return path


def _calib_batches(images, dev):
    """the first 25 batches of 4 images (the last one may be shorter), normalised on the device"""
    import torch
    from . import ops
    from .predict import MEAN, STD
    for b in range(CALIB_BATCHES):
        chunk = images[b * CALIB_BATCH:(b + 1) * CALIB_BATCH]
        if not chunk:
            return
        yield ops.predict_normalize(torch.from_numpy(np.stack(chunk)).to(dev), MEAN, STD)


def main(argv=None):
    print("--- Script execution started. ---")
    opts = get_argparser().parse_args(argv)
    print("--- Parsed Arguments: %s ---" % opts)
    os.makedirs(opts.results_dir, exist_ok=True)

    import torch
    from . import network, ops, quant
    from .metrics import StreamMetrics
    from .predict import MEAN, STD, load_model
    if not torch.cuda.is_available():
        raise RuntimeError("iswm_amd.evaluate_quantization needs a GPU (there is no CPU path)")
    dev = torch.device("cuda")
    print("Evaluation device: %s" % dev)

    image_dir = os.path.join(opts.eval_data_dir, 'imgs')
    mask_dir = os.path.join(opts.eval_data_dir, 'masks')
    if not os.path.isdir(image_dir) or not os.path.isdir(mask_dir):
        print("Error: 'imgs' or 'masks' subfolder not found in %s" % opts.eval_data_dir)
        return None
    files = pair_files(image_dir, mask_dir, opts.num_images)
    if not files:
        print("Error: No images found in %s" % image_dir)
        return None
    if not os.path.isfile(opts.fp32_ckpt):
        raise FileNotFoundError(opts.fp32_ckpt)
    samples = [load_sample(p, m) for _, p, m in files]
    sizes = sorted({s[0].shape[:2] for s in samples})
    if len(sizes) > 1:
        raise ValueError("the evaluation images must share one size; found %s" % sizes[:4])

    print("Loading FP32 model...")
    model = network.modeling.__dict__[opts.model](num_classes=2, output_stride=opts.output_stride,
                                                  pretrained_backbone=False)
    model = load_model(model, opts.fp32_ckpt, use_ema=opts.use_ema).to(dev).eval()

    print("\nCreating INT8 model from FP32 model...")
    print("Running calibration for INT8 model...")
    amax = quant.calibrate(model, _calib_batches([s[0] for s in samples], dev))
    int8_model = quant.quantize_model(model, amax)
    base, ext = os.path.splitext(opts.fp32_ckpt)
    int8_path = "%s_int8%s" % (base, ext)
    int8_model.save_int8(int8_path)
    print("\nINT8 model checkpoint saved successfully to: %s" % int8_path)

    fp32_size = os.path.getsize(opts.fp32_ckpt) / (1024 * 1024)
    int8_size = os.path.getsize(int8_path) / (1024 * 1024)
    metrics = {"fp32": StreamMetrics(2, device=dev), "int8": StreamMetrics(2, device=dev)}
    models = {"fp32": model, "int8": int8_model}
    times = {"fp32": [], "int8": []}
    saved = 0
    print("\nStarting evaluation on %d images..." % len(files))
    with torch.no_grad():
        for (name, _, _), (img, mask) in zip(files, samples):
            h, w = mask.shape
            x = ops.predict_normalize(torch.from_numpy(np.ascontiguousarray(img[None])).to(dev), MEAN, STD)
            gt = torch.from_numpy(mask[None]).to(dev)
            preds = {}
            for k in ("fp32", "int8"):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                maps = ops.predict_maps(models[k].forward_lowres(x), 2, 1, h, w, THRESHOLD, 0.2, 0.7)
                torch.cuda.synchronize()
                times[k].append(time.perf_counter() - t0)
                preds[k] = (maps.pred > 0).to(torch.uint8)
                metrics[k].update(gt, preds[k])
            if saved < opts.num_visualizations:
                save_visual_comparison(img, mask, preds["fp32"][0].cpu().numpy(), preds["int8"][0].cpu().numpy(),
                                       opts.results_dir, name)
                saved += 1

    print("\n\n" + "=" * 25 + " Quantization Evaluation Report " + "=" * 25)
    print("Evaluated on %d images.\n" % len(files))
    print("%-30s | %-20s | %-20s | %-15s" % ("Metric", "FP32 Model (on GPU)", "INT8 Model (on GPU)", "Change"))
    print("-" * 90)
    avg = {k: float(np.mean(v[1:] if len(v) > 1 else v)) * 1000 for k, v in times.items()}
    speedup = avg["fp32"] / avg["int8"] if avg["int8"] > 0 else float('inf')
    print("%-30s | %-20.2f | %-20.2f | %.2fx Speedup" % ("Avg. Inference Time (ms)", avg["fp32"], avg["int8"], speedup))
    print("%-30s | %-20.2f | %-20.2f | %.2fx smaller" % ("Model Size (MB)", fp32_size, int8_size,
                                                          fp32_size / int8_size if int8_size > 0 else float('inf')))
    print("-" * 90)
    score = {k: m.get_results() for k, m in metrics.items()}
    for key, label in (("MIoU", "Mean IoU (mIoU)"), ("Foreground IoU", "Foreground IoU"),
                       ("Foreground F1", "Foreground F1")):
        a, b = score["fp32"].get(key, 0.0), score["int8"].get(key, 0.0)
        print("%-30s | %-20.4f | %-20.4f | %+.4f" % (label, a, b, b - a))
    print("-" * 90)
    print("Visualizations saved to: %s" % opts.results_dir)
    print("=" * 78)
    print("--- Script execution finished. ---")
    return {"scores": score, "times_ms": avg, "int8_ckpt": int8_path, "visualizations": saved}


if __name__ == "__main__":
    main(sys.argv[1:])
