"""The best model's validation images -- counterpart of the reference's save_validation_results (train.py:461-523,
called at :733-737): for frame 0 of every validation batch

    NNNN_original.png  NNNN_target.png  NNNN_pred.png  NNNN_overlay.png  NNNN_error.png  [NNNN_confidence.png]

under ``<val_results_dir>/best_model_iter_<itr>_score_<weighted, 4 decimals>``.  The whole batch goes through
forward_lowres (as the reference runs the whole batch), ops.val_panels builds frame 0's panels in one kernel, one
asynchronous copy brings them to pinned host memory, and the PNGs are encoded in a thread pool while the next batch
runs.  Differences from the reference, all deliberate:

  * ``--save_val_results`` defaults to False here (the reference: True): without the flag a run writes what it wrote
    before this module existed;
  * ``_overlay.png`` is the 0.7-alpha composite of prediction over image at native resolution; the reference's file is
    a matplotlib figure whose size depends on the DPI, which is not reproduced;
  * ``_error.png`` is new (ops.val_panels);
  * for a class count other than 2 the masks are painted with the PASCAL VOC colour map (the reference paints
    everything black there);
  * files are numbered from 0 by the frames handed to the encoder pool; a frame whose batch fails on the device takes
    no number, as in the reference, but one whose PNG cannot be written leaves a gap (the next batch is already
    queued by then);
  * messages are in English.
"""
import os
import shutil
import time
from collections import deque
from concurrent.futures import ThreadPoolExecutor

import numpy as np
from PIL import Image

MEAN = (0.485, 0.456, 0.406)          # train.py:491
STD = (0.229, 0.224, 0.225)
RGB_KINDS = ("original", "target", "pred", "overlay", "error")
_PANEL_OF = {"original": "original", "target": "target_rgb", "pred": "pred_rgb", "overlay": "overlay", "error": "error",
             "confidence": "conf"}


def results_dirname(cur_itrs, weighted_score, prefix="best_model"):
    """train.py:463"""
    return "%s_iter_%d_score_%.4f" % (prefix, cur_itrs, weighted_score)


def panel_kinds(save_confidence_map):
    return RGB_KINDS + (("confidence",) if save_confidence_map else ())


def panel_filename(index, kind):
    """train.py:499-516"""
    return "%04d_%s.png" % (index, kind)


def write_panels(results_dir, index, panels, save_confidence_map=False):
    """one frame's files from uint8 arrays: panels[kind] is [H, W, 3] (mode RGB) for RGB_KINDS and [H, W] (mode L) for
    "confidence", which is written only when asked for.  Returns the paths written."""
    paths = []
    for kind in panel_kinds(save_confidence_map):
        arr = np.ascontiguousarray(panels[kind])
        want_shape = 2 if kind == "confidence" else 3
        if arr.dtype != np.uint8 or arr.ndim != want_shape or (want_shape == 3 and arr.shape[2] != 3):
            raise ValueError("%s panel: expected uint8 %s, got %s %s" %
                             (kind, "[H, W]" if want_shape == 2 else "[H, W, 3]", arr.dtype, arr.shape))
        path = os.path.join(results_dir, panel_filename(index, kind))
        Image.fromarray(arr).save(path)                 # uint8 [H, W, 3] -> mode RGB, [H, W] -> mode L
        paths.append(path)
    return paths


def _enqueue(model, images, labels, num_classes, kinds):
    """forward_lowres on the whole batch, the panels of frame 0, one copy to pinned memory; returns wait() ->
    {kind: array}"""
    import torch
    from . import ops
    yl = model.forward_lowres(images)
    want = tuple(_PANEL_OF[k] for k in kinds)
    panels = ops.val_panels(images[0:1], yl[0:1], labels[0:1], num_classes, MEAN, STD, want=want)
    h, w = images.shape[2:]
    lay = ops.val_panels_layout(1, h, w, want)
    host = torch.empty(lay["end"], dtype=torch.uint8, pin_memory=True)
    host.copy_(panels.packed[:lay["end"]], non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()

    def wait():
        ev.synchronize()
        a = host.numpy()
        out = {}
        for k in kinds:
            off = lay[_PANEL_OF[k]]
            out[k] = a[off:off + h * w].reshape(h, w) if k == "confidence" else a[off:off + 3 * h * w].reshape(h, w, 3)
        return out
    return wait


def save_validation_results(model, loader, device, opts, cur_itrs, weighted_score, prefix="best_model"):
    """train.py:461-523 on the device.  Batch i + 1 is enqueued before batch i is waited for; a failure on one frame is
    printed and that frame skipped.  Returns the number of frames saved."""
    import torch
    results_dir = os.path.join(opts.val_results_dir, results_dirname(cur_itrs, weighted_score, prefix))
    if os.path.exists(results_dir):
        shutil.rmtree(results_dir)
    os.makedirs(results_dir, exist_ok=True)
    save_conf = bool(getattr(opts, "save_confidence_map", False))
    kinds = panel_kinds(save_conf)
    workers = max(1, int(getattr(opts, "num_workers", 1) or 1))
    t0 = time.time()
    saved = [0]
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad(), ThreadPoolExecutor(max_workers=workers) as pool:
            encodes = deque()

            def drain(block):
                while encodes and (block or encodes[0][1].done()):
                    idx, f = encodes.popleft()
                    try:
                        f.result()
                        saved[0] += 1
                    except Exception as e:      # noqa: BLE001 -- reported per frame, like the reference (:518-520)
                        print("Error while saving validation image %04d: %s" % (idx, e))

            def finish(pending):
                idx, wait = pending
                try:
                    panels = wait()
                except Exception as e:          # noqa: BLE001
                    print("Error while saving validation image %04d: %s" % (idx, e))
                    return
                encodes.append((idx, pool.submit(write_panels, results_dir, idx, panels, save_conf)))
                drain(False)

            pending, count = None, 0
            for images, labels in loader:
                try:
                    wait = _enqueue(model, images.to(device, dtype=torch.float32), labels.to(device), opts.num_classes,
                                    kinds)
                except Exception as e:          # noqa: BLE001
                    print("Error while saving validation image %04d: %s" % (count, e))
                    continue
                if pending is not None:
                    finish(pending)
                pending = (count, wait)
                count += 1                      # files are numbered by frames handed over, from 0
            if pending is not None:
                finish(pending)
            drain(True)
    finally:
        model.train(was_training)
    print("Saved %d validation images of the best model to %s (%.2f s)" % (saved[0], results_dir, time.time() - t0))
    return saved[0]
