"""Inference entry point -- runnable counterpart of the reference's predict.py.

    python -m iswm_amd.predict --input <dir> --ckpt <checkpoint> --save_val_results_to <out> \\
        [--save_confidence] [--save_binary] [--batch_size B] [--workers W] [--tile_size T [--tile_overlap O]]
        [--tta_scales S1,S2,... ] [--tta_flip] [--crf_iters T [--crf_radius R] [--crf_step D] ...]

Every subfolder of ``--input`` is walked (process_images, predict.py:292-368) and each frame gets
``<out>/<subfolder>/<name>_predict.png`` (0/255 foreground mask), plus ``_confidence.png`` (uint8(p * 255), p = the
softmax foreground probability) and ``_binary_mask.png`` (min_broken_prob <= conf / 255 <= max_broken_prob) when
asked for.  Per batch, the uint8 frames are uploaded once; ops.predict_normalize, the model's forward_lowres and
ops.predict_maps run on the device; one asynchronous copy brings the maps and the per-image statistics back; PNG
decoding and encoding run in a thread pool, overlapping the device work.

Same flags and defaults as the reference's get_argparser (predict.py:19-67).  Differences, all deliberate:
  * ``--model`` takes this project's constructors (train.py's choices); the reference builds resnet50 only;
  * models are built with ``pretrained_backbone=False`` -- the weights come from ``--ckpt`` (the reference's
    pretrained backbone is a download);
  * ``--save_val_results_to`` is required (the reference's default None crashes at os.makedirs);
  * ``--gpu_id`` selects ``cuda:<id>`` among the visible devices; the process does not rewrite
    CUDA_VISIBLE_DEVICES;
  * new ``--batch_size`` (default 1): consecutive frames of one subfolder with the same size share a batch;
  * new ``--workers`` (default 4): host threads for PNG decoding and encoding;
  * new ``--tile_size T`` (default 0: every frame goes through the network whole) and ``--tile_overlap O`` (default
    -1: T // 8): a frame larger than T is predicted in T x T windows every T - O pixels, the last window of each axis
    pulled back inside the frame, and the overlaps are blended with weights that ramp over O pixels (ScenePredictor;
    DESIGN.md section 13).  ``--batch_size`` then counts windows per device batch and frames are handed over one at
    a time.  A frame no larger than T is one window and gives the whole-frame path's bytes;
  * new ``--tta_scales S1,S2,...`` (default ``1.0``) and ``--tta_flip``: test-time augmentation.  The foreground
    probability is the mean over views of the frame, one per scale (the frame resampled bilinearly to
    int(H * s + 0.5) x int(W * s + 0.5)) and, with ``--tta_flip``, its mirror image after each; the maps are cut from
    that mean (TTAPredictor).  1 to 8 distinct scales in [0.25, 4.0].  With the defaults the
    whole-frame path runs unchanged.  Not combined with ``--tile_size``: TTA over windows is not built;
  * new ``--crf_iters T`` (default 0: off) with ``--crf_radius`` (5), ``--crf_step`` (2), ``--crf_bilateral_weight`` (10),
    ``--crf_spatial_weight`` (3), ``--crf_theta_alpha`` (80), ``--crf_theta_beta`` (13) and ``--crf_theta_gamma`` (3): T mean-field
    iterations of a locally connected dense CRF pull the foreground probability onto the edges of the frame itself before the
    maps are cut from it (ops.crf_refine, ops.prob_maps); the printed statistics are those of the refined
    probability.  It follows every path -- whole frames, ``--tile_size`` (the whole scene is refined, not its windows) and
    test-time augmentation -- and INT8 checkpoints.  The defaults are ConvCRF's published values and are unvalidated on
    internal-wave frames.  A ``--crf_*`` flag without ``--crf_iters`` >= 1 is an error; with 0 nothing changes;
  * ``--binary_threshold`` is accepted and unused, as in the reference (predict.py:223);
  * ``--enable_wave_processing`` is refused: its synthetic "broken area" generator is random and draws with
    OpenCV, which is not a dependency here.  Its flags still parse;
  * ``_predict.png`` is mode L with values 0 / 255 (this project's decode_target); the colour map of the
    reference's BinarySegmentation.decode_target is not in its tree and stays unpinned;
  * subfolders and files are walked in sorted order (the reference uses os.listdir order);
  * messages are in English;
  * ``--ckpt`` may name an INT8 checkpoint written by iswm_amd.quant (detected by its format tag): the frames then
    run through QuantizedSegmentationModel.forward_lowres, and ``--model`` / ``--output_stride`` are taken from the
    checkpoint.
"""
import argparse
import os
import sys
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg', '.tif')
MEAN = (0.485, 0.456, 0.406)        # predict.py:96
STD = (0.229, 0.224, 0.225)
WAVE_PROCESSING_REFUSED = ("--enable_wave_processing is not supported: the reference's synthetic broken-area "
                           "generator is random and draws with OpenCV, which this project does not depend on")


def _model_names():
    from . import network
    return sorted(name for name in network.modeling.__dict__ if name.islower() and
                  not (name.startswith("__") or name.startswith('_')) and callable(network.modeling.__dict__[name]))


def get_argparser():
    parser = argparse.ArgumentParser()

    # Dataset Options
    parser.add_argument("--input", type=str, required=True,
                        help="Directory whose subfolders hold the images")
    parser.add_argument("--dataset", type=str, default='binary', choices=['binary'], help='Name of dataset')

    # Model Options
    parser.add_argument("--model", type=str, default='deeplabv3plus_resnet50', choices=_model_names(),
                        help='Model name')
    parser.add_argument("--ckpt", default=None, type=str, help="Path to trained model")
    parser.add_argument("--gpu_id", type=str, default='0', help="GPU ID (index among the visible devices)")
    parser.add_argument("--save_val_results_to", default=None, required=True,
                        help="Directory to save segmentation results")

    # Additional Parameters
    parser.add_argument("--output_stride", type=int, default=16, help='Output stride for DeepLabV3+ (8 or 16)')

    # Confidence Map & Binary Mask Options
    parser.add_argument("--save_confidence", action='store_true', help="Save confidence maps")
    parser.add_argument("--save_binary", action='store_true', help="Save binary masks")
    parser.add_argument("--binary_threshold", type=int, default=200,
                        help="Threshold for binarizing confidence map (unused, as in the reference)")
    parser.add_argument("--pred_threshold", type=float, default=0.5,
                        help="Threshold for predicting foreground (default: 0.5)")

    # Internal-wave processing options (parsed; --enable_wave_processing is refused)
    parser.add_argument("--internal_wave_area_threshold", type=float, default=0.01,
                        help="Minimum foreground area ratio to consider image having internal waves")
    parser.add_argument("--synthetic_broken_prob", type=float, default=0.8,
                        help="Probability to generate synthetic broken areas for no-wave images")
    parser.add_argument("--synthetic_broken_ratio", type=float, default=0.05,
                        help="Ratio of image area to generate as synthetic broken areas")
    parser.add_argument("--enable_wave_processing", action='store_true',
                        help="Enable internal wave specific processing (not supported)")

    parser.add_argument("--min_broken_prob", type=float, default=0.2,
                        help="Minimum foreground probability to consider pixel as broken area (default: 0.2)")
    parser.add_argument("--max_broken_prob", type=float, default=0.7,
                        help="Maximum foreground probability to consider pixel as broken area (default: 0.7)")

    # this project's additions
    parser.add_argument("--batch_size", type=int, default=1,
                        help="frames per device batch (consecutive frames of one subfolder with the same size)")
    parser.add_argument("--workers", type=int, default=4, help="host threads for PNG decoding and encoding")
    parser.add_argument("--tile_size", type=int, default=0,
                        help="predict frames in windows of this size and blend the overlaps (0: whole frames); "
                             "--batch_size then counts windows per device batch")
    parser.add_argument("--tile_overlap", type=int, default=-1,
                        help="overlap of neighbouring windows in pixels (default: tile_size // 8)")
    parser.add_argument("--tta_scales", type=str, default="1.0",
                        help="test-time augmentation: comma list of 1 to 8 distinct scales in [0.25, 4.0] whose "
                             "foreground probabilities are averaged (default: 1.0)")
    parser.add_argument("--tta_flip", action='store_true',
                        help="test-time augmentation: add the horizontally mirrored view of every scale")
    parser.add_argument("--use_ema", action='store_true',
                        help="predict with the checkpoint's EMA weights (a checkpoint of train --ema_decay)")
    parser.add_argument("--crf_iters", type=int, default=0, metavar="T",
                        help="refine the foreground probability with T mean-field iterations of a locally connected dense CRF "
                             "on the frame (0: off; at most 20)")
    parser.add_argument("--crf_radius", type=int, default=None, metavar="R",
                        help="CRF window radius in steps, 1 to 7 (default: 5; needs --crf_iters)")
    parser.add_argument("--crf_step", type=int, default=None, metavar="D",
                        help="CRF window dilation in pixels, 1 to 4 (default: 2; needs --crf_iters)")
    parser.add_argument("--crf_bilateral_weight", type=float, default=None,
                        help="weight of the colour-and-position message (default: 10; needs --crf_iters)")
    parser.add_argument("--crf_spatial_weight", type=float, default=None,
                        help="weight of the position-only message (default: 3; needs --crf_iters)")
    parser.add_argument("--crf_theta_alpha", type=float, default=None,
                        help="position scale of the bilateral kernel in pixels (default: 80; needs --crf_iters)")
    parser.add_argument("--crf_theta_beta", type=float, default=None,
                        help="colour scale of the bilateral kernel in grey levels (default: 13; needs --crf_iters)")
    parser.add_argument("--crf_theta_gamma", type=float, default=None,
                        help="position scale of the spatial kernel in pixels (default: 3; needs --crf_iters)")
    return parser


CRF_FLAGS = (("crf_radius", "radius", 5), ("crf_step", "step", 2), ("crf_bilateral_weight", "w_bilateral", 10.0),
             ("crf_spatial_weight", "w_spatial", 3.0), ("crf_theta_alpha", "theta_alpha", 80.0),
             ("crf_theta_beta", "theta_beta", 13.0), ("crf_theta_gamma", "theta_gamma", 3.0))


def crf_options(parser, opts):
    """the keyword arguments of ops.crf_refine (iters included), or None when --crf_iters is 0; the flags left out are filled in
    with their defaults.  A --crf_* flag without --crf_iters >= 1 and values outside ops.crf_check's ranges are argparse errors"""
    from . import ops
    given = ["--" + flag for flag, _, _ in CRF_FLAGS if getattr(opts, flag) is not None]
    if not 0 <= opts.crf_iters <= ops.CRF_MAX_ITERS:
        parser.error("--crf_iters %d must lie in [0, %d]" % (opts.crf_iters, ops.CRF_MAX_ITERS))
    if opts.crf_iters == 0 and given:
        parser.error("%s needs --crf_iters of at least 1" % ", ".join(given))
    for flag, _, default in CRF_FLAGS:
        if getattr(opts, flag) is None:
            setattr(opts, flag, default)
    crf = dict(((name, getattr(opts, flag)) for flag, name, _ in CRF_FLAGS), iters=opts.crf_iters)
    try:
        ops.crf_check(**crf)
    except ValueError as e:
        parser.error("--crf_*: %s" % e)
    return crf if opts.crf_iters > 0 else None


def _crf_maps(maps, frames, crf, thr, min_prob, max_prob):
    """the maps of the probability of `maps` refined on the uint8 frames [N, H, W, 3] already on the device"""
    from . import ops
    return ops.prob_maps(ops.crf_refine(maps.prob, frames, **crf), thr, min_prob, max_prob)


def tta_options(parser, opts):
    """(scales, flip), or None for the defaults (one unflipped view at scale 1: the whole-frame path); bad lists and
    TTA together with --tile_size are argparse errors"""
    from . import ops
    scales = []
    for item in opts.tta_scales.split(","):
        try:
            scales.append(float(item))
        except ValueError:
            parser.error("--tta_scales %r: %r is no number" % (opts.tta_scales, item.strip()))
    try:
        ops.tta_views(1, 1, scales, opts.tta_flip)
    except ValueError as e:
        parser.error("--tta_scales %r: %s" % (opts.tta_scales, e))
    if scales == [1.0] and not opts.tta_flip:
        return None
    if opts.tile_size != 0:
        parser.error("--tta_scales / --tta_flip cannot be combined with --tile_size: test-time augmentation over "
                     "windows is not built")
    return scales, bool(opts.tta_flip)


def tile_options(parser, opts):
    """(tile_size, tile_overlap) with the default overlap filled in; bad combinations are argparse errors"""
    if opts.tile_size < 0:
        parser.error("--tile_size %d must not be negative" % opts.tile_size)
    if opts.tile_size == 0:
        if opts.tile_overlap != -1:
            parser.error("--tile_overlap %d needs --tile_size" % opts.tile_overlap)
        return 0, 0
    overlap = opts.tile_size // 8 if opts.tile_overlap == -1 else opts.tile_overlap
    if overlap < 0 or overlap > 1024 or overlap > opts.tile_size // 2:
        parser.error("--tile_overlap %d must lie in [0, min(1024, tile_size // 2 = %d)] for --tile_size %d" %
                     (overlap, opts.tile_size // 2, opts.tile_size))
    return opts.tile_size, overlap


def list_subdirs(input_base_path):
    return sorted(d for d in os.listdir(input_base_path) if os.path.isdir(os.path.join(input_base_path, d)))


def list_images(subdir_path):
    return sorted(f for f in os.listdir(subdir_path) if f.lower().endswith(IMAGE_EXTENSIONS)
                  and os.path.isfile(os.path.join(subdir_path, f)))


def decode_image(path):
    """uint8 [H, W, 3] RGB (predict.py:259)"""
    with Image.open(path) as im:
        return np.asarray(im.convert('RGB'))


def _decoded(pool, paths, ahead):
    """(path, array or exception) in order, keeping at most `ahead` decodes in flight"""
    q = deque()
    it = iter(paths)
    for p in it:
        q.append((p, pool.submit(decode_image, p)))
        if len(q) >= ahead:
            break
    while q:
        p, f = q.popleft()
        try:
            yield p, f.result()
        except Exception as e:          # noqa: BLE001 -- reported per image, like the reference
            yield p, e
        nxt = next(it, None)
        if nxt is not None:
            q.append((nxt, pool.submit(decode_image, nxt)))


def _batches(decoded, batch_size, on_error):
    """consecutive decoded frames with the same size, at most batch_size each: lists of (path, array)"""
    cur = []
    for path, img in decoded:
        if isinstance(img, Exception):
            on_error(path, img)
            continue
        if cur and (len(cur) >= batch_size or cur[0][1].shape != img.shape):
            yield cur
            cur = []
        cur.append((path, img))
    if cur:
        yield cur


def _save_png(arr, path):
    """uint8 [H, W] -> mode-L PNG"""
    Image.fromarray(np.ascontiguousarray(arr)).save(path)


def _stats_lines(st, npix, thr):
    """the reference's per-image log (predict.py:271-272)"""
    return ("Foreground probability: min=%.4f, max=%.4f, mean=%.4f\n"
            "Pixels below prediction threshold %s: %.2f%%" %
            (st[0], st[1], st[2] / npix, thr, 100.0 * st[3] / npix))


def process_images(input_base_path, output_path, predict_batch, save_confidence, save_binary, pred_threshold=0.5,
                   batch_size=1, workers=4, log=print, progress=True):
    """Walk the subfolders of input_base_path (predict.py:292-368) and write the masks of every image.

    predict_batch(uint8 [B, H, W, 3]) enqueues one batch and returns a callable; calling it waits for that batch and
    returns {"pred", "conf", "band": uint8 [B, H, W] (conf / band may be None when not asked for), "stats": [B, 5]}.
    Batch i+1 is enqueued before batch i is waited for, and the PNGs are encoded in the pool, so the device never
    waits on host encoding.  An exception on one image is printed and that image skipped.  Returns the number of
    images written."""
    from tqdm import tqdm

    os.makedirs(output_path, exist_ok=True)
    subdirs = list_subdirs(input_base_path)
    log("\nFound %d subfolders" % len(subdirs))
    files = {d: list_images(os.path.join(input_base_path, d)) for d in subdirs}
    total_images = sum(len(v) for v in files.values())
    log("Found %d images in total" % total_images)

    done = [0]
    workers = max(1, int(workers))
    batch_size = max(1, int(batch_size))

    def report(path, e):
        log("\nError while processing %s: %s" % (path, e))

    with ThreadPoolExecutor(max_workers=workers) as pool, \
            tqdm(total=total_images, desc="Total progress", disable=not progress) as pbar:
        encodes = deque()

        def drain(block):
            while encodes and (block or encodes[0][1].done()):
                path, f = encodes.popleft()
                try:
                    f.result()
                    done[0] += 1
                    pbar.update(1)
                except Exception as e:      # noqa: BLE001
                    report(path, e)

        def encode_one(res, k, out_base):
            _save_png(res["pred"][k], out_base + '_predict.png')
            if save_confidence:
                _save_png(res["conf"][k], out_base + '_confidence.png')
            if save_binary:
                _save_png(res["band"][k], out_base + '_binary_mask.png')

        def finish(pending):
            items, subdir, wait, last = pending
            try:
                res = wait()
            except Exception as e:          # noqa: BLE001
                for path, _ in items:
                    report(path, e)
                res = None
            for k, (path, img) in enumerate(items if res is not None else ()):
                log(_stats_lines(res["stats"][k], img.shape[0] * img.shape[1], pred_threshold))
                base = os.path.splitext(os.path.basename(path))[0]
                out_base = os.path.join(output_path, subdir, base)
                encodes.append((path, pool.submit(encode_one, res, k, out_base)))
            if last:
                log("Finished folder %s" % subdir)
            drain(False)

        # one pipeline across folders: the next folder's first batch is enqueued before the previous folder's last
        # batch is waited for, and nothing waits on the encodes until the end
        pending = None
        for subdir in subdirs:
            subdir_path = os.path.join(input_base_path, subdir)
            log("\nProcessing folder: %s" % subdir)
            log("Found %d images in %s" % (len(files[subdir]), subdir))
            os.makedirs(os.path.join(output_path, subdir), exist_ok=True)
            paths = [os.path.join(subdir_path, f) for f in files[subdir]]
            for items in _batches(_decoded(pool, paths, 2 * batch_size + workers), batch_size, report):
                try:
                    wait = predict_batch(np.stack([img for _, img in items]))
                except Exception as e:      # noqa: BLE001
                    for path, _ in items:
                        report(path, e)
                    continue
                if pending is not None:
                    finish(pending)
                pending = [items, subdir, wait, False]
            if pending is not None and pending[1] == subdir:
                pending[3] = True           # the folder is finished once its last batch is
            else:
                log("Finished folder %s" % subdir)
        if pending is not None:
            finish(pending)
        drain(True)

    log("\nPrediction finished, results saved to: %s" % output_path)
    return done[0]


class DevicePredictor:
    """predict_batch for process_images: upload -> predict_normalize -> forward_lowres -> predict_maps -> one copy of
    stats + the requested maps into pinned host memory.  With `crf` (crf_options) the probability is refined on the uploaded
    frames and the maps are cut from that: two more calls, the same single copy."""

    def __init__(self, model, device, num_classes, fg, pred_threshold, min_prob, max_prob, want_conf, want_band, crf=None):
        self.model, self.device = model, device
        self.num_classes, self.fg = num_classes, fg
        self.thr, self.min_prob, self.max_prob = pred_threshold, min_prob, max_prob
        self.want_conf, self.want_band = want_conf, want_band
        self.crf = crf

    def __call__(self, batch):
        import torch
        from . import ops
        n, h, w, _ = batch.shape
        pin = torch.from_numpy(np.ascontiguousarray(batch)).pin_memory()
        with torch.cuda.device(self.device), torch.no_grad():
            img = pin.to(self.device, non_blocking=True)
            x = ops.predict_normalize(img, MEAN, STD)
            yl = self.model.forward_lowres(x)
            maps = ops.predict_maps(yl, self.num_classes, self.fg, h, w, self.thr, self.min_prob, self.max_prob,
                                    want_prob=self.crf is not None)
            if self.crf is not None:
                maps = _crf_maps(maps, img, self.crf, self.thr, self.min_prob, self.max_prob)
            lay = ops.predict_maps_layout(n, h, w)
            end = lay["band"] + n * h * w if self.want_band else lay["conf"] + n * h * w if self.want_conf else \
                lay["pred"] + n * h * w
            host = torch.empty(end, dtype=torch.uint8, pin_memory=True)
            host.copy_(maps.packed[:end], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()

        def wait():
            ev.synchronize()
            a = host.numpy()
            stats = a[:40 * n].view(np.float64).reshape(n, 5)
            pick = (lambda k: a[lay[k]:lay[k] + n * h * w].reshape(n, h, w))
            return {"pred": pick("pred"), "conf": pick("conf") if self.want_conf else None,
                    "band": pick("band") if self.want_band else None, "stats": stats}
        return wait


class ScenePredictor:
    """predict_batch for process_images over frames larger than the training crops: per frame, one upload, then
    ops.scene_tiles_normalize -> forward_lowres per batch of windows into one logits buffer, ops.scene_maps over all
    windows, and one copy of stats + the requested maps into pinned host memory.  With `crf` (crf_options) the blended
    probability is refined on the whole scene before the maps are cut.  Nothing synchronises before wait()."""

    def __init__(self, model, device, num_classes, fg, pred_threshold, min_prob, max_prob, want_conf, want_band,
                 tile_size, tile_overlap, tile_batch=1, crf=None):
        self.crf = crf
        self.model, self.device = model, device
        self.num_classes, self.fg = num_classes, fg
        self.thr, self.min_prob, self.max_prob = pred_threshold, min_prob, max_prob
        self.want_conf, self.want_band = want_conf, want_band
        self.tile_size, self.tile_overlap, self.tile_batch = int(tile_size), int(tile_overlap), max(1, int(tile_batch))

    def __call__(self, batch):
        import torch
        from . import ops
        n, h, w, _ = batch.shape
        plan = ops.scene_plan(h, w, self.tile_size, self.tile_overlap)
        lay = ops.predict_maps_layout(1, h, w)
        end = lay["band"] + h * w if self.want_band else lay["conf"] + h * w if self.want_conf else lay["pred"] + h * w
        pin = torch.from_numpy(np.ascontiguousarray(batch)).pin_memory()
        host = torch.empty((n, end), dtype=torch.uint8, pin_memory=True)
        with torch.cuda.device(self.device), torch.no_grad():
            for f in range(n):
                scene = pin[f].to(self.device, non_blocking=True)
                logits = None
                for k0 in range(0, plan.ntiles, self.tile_batch):
                    count = min(self.tile_batch, plan.ntiles - k0)
                    yl = self.model.forward_lowres(ops.scene_tiles_normalize(scene, plan, k0, count, MEAN, STD))
                    if count == plan.ntiles:
                        logits = yl
                        break
                    if logits is None:      # sized once the first batch shows the low-resolution shape and pitch
                        logits = torch.empty((plan.ntiles,) + tuple(yl.shape[1:]), dtype=yl.dtype, device=yl.device)
                    logits[k0:k0 + count].copy_(yl)
                maps = ops.scene_maps(logits, self.num_classes, self.fg, plan, self.thr, self.min_prob, self.max_prob,
                                      want_prob=self.crf is not None)
                if self.crf is not None:
                    maps = _crf_maps(maps, scene.unsqueeze(0), self.crf, self.thr, self.min_prob, self.max_prob)
                host[f].copy_(maps.packed[:end], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()

        def wait():
            ev.synchronize()
            a = host.numpy()
            stats = np.ascontiguousarray(a[:, :40]).view(np.float64).reshape(n, 5)
            pick = (lambda k: a[:, lay[k]:lay[k] + h * w].reshape(n, h, w))
            return {"pred": pick("pred"), "conf": pick("conf") if self.want_conf else None,
                    "band": pick("band") if self.want_band else None, "stats": stats}
        return wait


class TTAPredictor:
    """predict_batch for process_images with test-time augmentation: one upload, then per view of ops.tta_views
    ops.predict_view_normalize -> forward_lowres on the whole frame batch with every view's logits kept, one
    ops.predict_views_maps over all of them, and one copy of stats + the requested maps into pinned host memory.
    With `crf` (crf_options) the mean probability is refined on the frames before the maps are cut.
    Nothing synchronises before wait()."""

    def __init__(self, model, device, num_classes, fg, pred_threshold, min_prob, max_prob, want_conf, want_band,
                 scales, flip, crf=None):
        self.crf = crf
        self.model, self.device = model, device
        self.num_classes, self.fg = num_classes, fg
        self.thr, self.min_prob, self.max_prob = pred_threshold, min_prob, max_prob
        self.want_conf, self.want_band = want_conf, want_band
        self.scales, self.flip = tuple(float(s) for s in scales), bool(flip)

    def __call__(self, batch):
        import torch
        from . import ops
        n, h, w, _ = batch.shape
        views = ops.tta_views(h, w, self.scales, self.flip)
        pin = torch.from_numpy(np.ascontiguousarray(batch)).pin_memory()
        with torch.cuda.device(self.device), torch.no_grad():
            img = pin.to(self.device, non_blocking=True)
            yls = [self.model.forward_lowres(ops.predict_view_normalize(img, hv, wv, f, MEAN, STD))
                   for hv, wv, f in views]
            maps = ops.predict_views_maps(yls, [f for _, _, f in views], self.num_classes, self.fg, h, w, self.thr,
                                          self.min_prob, self.max_prob, want_prob=self.crf is not None)
            if self.crf is not None:
                maps = _crf_maps(maps, img, self.crf, self.thr, self.min_prob, self.max_prob)
            lay = ops.predict_maps_layout(n, h, w)
            end = lay["band"] + n * h * w if self.want_band else lay["conf"] + n * h * w if self.want_conf else \
                lay["pred"] + n * h * w
            host = torch.empty(end, dtype=torch.uint8, pin_memory=True)
            host.copy_(maps.packed[:end], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()

        def wait():
            ev.synchronize()
            a = host.numpy()
            stats = a[:40 * n].view(np.float64).reshape(n, 5)
            pick = (lambda k: a[lay[k]:lay[k] + n * h * w].reshape(n, h, w))
            return {"pred": pick("pred"), "conf": pick("conf") if self.want_conf else None,
                    "band": pick("band") if self.want_band else None, "stats": stats}
        return wait


def load_model(model, ckpt_path, ck=None, use_ema=False):
    """predict.py:80-91 with the weights-only loader: {"model_state": ...} (this project's and the reference's
    checkpoints) or a bare state dict, `module.` prefixes stripped, strict load.  No file: initial weights.
    `ck`: the file's contents when the caller has read it already.  `use_ema`: load the checkpoint's EMA weights
    (optim.ema_model_state: parameters from "ema_state", BatchNorm statistics from "model_state"); a checkpoint
    without them, or no checkpoint, is an error."""
    if use_ema and not (ckpt_path is not None and os.path.isfile(ckpt_path)):
        raise FileNotFoundError("--use_ema needs a checkpoint (got %r)" % (ckpt_path,))
    if ckpt_path is not None and os.path.isfile(ckpt_path):
        if ck is None:
            from .train import load_checkpoint
            ck = load_checkpoint(ckpt_path)
        if use_ema:
            from .optim import ema_model_state
            if not (isinstance(ck, dict) and "model_state" in ck):
                raise KeyError("%s is a bare state dict: it has no 'ema_state'" % ckpt_path)
            ck = {"model_state": ema_model_state(ck)}
        state = ck["model_state"] if isinstance(ck, dict) and "model_state" in ck else ck
        state = {(k[7:] if k.startswith("module.") else k): v for k, v in state.items()}
        model.load_state_dict(state, strict=True)
        print("Model loaded from %s" % ckpt_path)
    else:
        print("[!] No checkpoint found")
    return model


def main(argv=None):
    parser = get_argparser()
    opts = parser.parse_args(argv)
    tile_size, tile_overlap = tile_options(parser, opts)
    tta = tta_options(parser, opts)
    crf = crf_options(parser, opts)
    if opts.enable_wave_processing:
        get_argparser().error(WAVE_PROCESSING_REFUSED)
    if opts.batch_size < 1 or opts.workers < 1:
        get_argparser().error("--batch_size and --workers must be at least 1")

    import torch
    from . import network
    if not torch.cuda.is_available():
        raise RuntimeError("iswm_amd.predict needs a GPU (there is no CPU path)")
    device = torch.device("cuda:%d" % int(opts.gpu_id))
    print("Device: %s" % device)

    num_classes, fg = 2, 1                       # --dataset binary: prob[:, 1] (predict.py:267)
    from . import quant
    q, ck = quant.read_checkpoint(opts.ckpt) if opts.ckpt is not None and os.path.isfile(opts.ckpt) else (None, None)
    if q is not None:
        if opts.use_ema:
            parser.error("--use_ema: %s is an INT8 checkpoint (export it from the EMA weights instead)" % opts.ckpt)
        model = quant.load_int8(q, device)
        print("INT8 model loaded from %s (%s, output stride %d)" % (opts.ckpt, q["arch"]["model"],
                                                                     q["arch"]["output_stride"]))
    else:
        model = network.modeling.__dict__[opts.model](num_classes=num_classes, output_stride=opts.output_stride,
                                                      pretrained_backbone=False)
        model = load_model(model, opts.ckpt, ck, use_ema=opts.use_ema).to(device)
    model.eval()

    if tile_size > 0:                            # windows share a device batch; frames go one at a time
        predictor = ScenePredictor(model, device, num_classes, fg, opts.pred_threshold, opts.min_broken_prob,
                                   opts.max_broken_prob, opts.save_confidence, opts.save_binary, tile_size,
                                   tile_overlap, tile_batch=opts.batch_size, crf=crf)
        frames = 1
    elif tta is not None:
        predictor = TTAPredictor(model, device, num_classes, fg, opts.pred_threshold, opts.min_broken_prob,
                                 opts.max_broken_prob, opts.save_confidence, opts.save_binary, tta[0], tta[1], crf=crf)
        frames = opts.batch_size
    else:
        predictor = DevicePredictor(model, device, num_classes, fg, opts.pred_threshold, opts.min_broken_prob,
                                    opts.max_broken_prob, opts.save_confidence, opts.save_binary, crf=crf)
        frames = opts.batch_size
    return process_images(opts.input, opts.save_val_results_to, predictor, opts.save_confidence, opts.save_binary,
                          pred_threshold=opts.pred_threshold, batch_size=frames, workers=opts.workers)


if __name__ == "__main__":
    main(sys.argv[1:])
