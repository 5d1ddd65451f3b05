"""Device-side counterpart of the confusion-matrix half of the reference's StreamMetrics
(metrics/stream_metrics.py:7-63,100-186): the 2x2 (n x n) histogram of (ground truth, prediction) is counted by
a HIP kernel straight from the label tensor and the argmax mask -- or from the logits, fusing the argmax
(train.py:644,659) -- and stays on the GPU as int64; only the n*n counts cross PCIe when results are read.

Kept from the reference: constructor arguments, `n_classes`, `confusion_matrix`, `FOREGROUND_CLASS`,
`_fast_hist`, `update(label_trues, label_preds, sequence_data)`, `get_results()` with all of the reference's keys and
formulas (eps = 1e-7), `best_score`, `reset()`.  The temporal, region and front-tracking evaluators are the device
counterparts of sequence_metrics.py; a sequence update feeds them exactly as the reference does (:100-137).
"Best Score" is the running maximum of the weighted score (:63-97) after every update and once more in get_results().

update() never synchronises: every per-update quantity (confusion-matrix snapshot, evaluator scalars) stays in device
logs, and get_results() copies them to the host in one transfer and replays the per-update weighted scores.
A batch [B, H, W] given with sequence_data=False counts all of it into the confusion matrix and feeds the region and
front evaluators one frame at a time (the reference passes such a batch to cv2 / its mask utilities, which only
handle single frames).
"""
import numpy as np
import torch

from .. import ops
from .sequence_metrics import (FrameView, FrontTrackingMetrics, RegionMetrics, TemporalMetrics, as_device_masks,
                               first_preprocess)

WEIGHTS = {"MIoU": 0.05, "Foreground IoU": 0.25, "Foreground F1": 0.25, "Front Tracking Error": 0.25,
           "Temporal Consistency": 0.10, "Region Continuity": 0.10}     # :65-73 (train.py:842-850 get_metric_weights)


class StreamMetrics(object):
    def __init__(self, n_classes, sequence_length=7, temporal_stride=1, threshold=0.005, device=None):
        self.n_classes = n_classes
        self.FOREGROUND_CLASS = 1
        self.sequence_length, self.temporal_stride, self.threshold = sequence_length, temporal_stride, threshold
        self.device = torch.device(device if device is not None else "cuda")
        self._hist = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=self.device)
        self.best_score = {'weighted_score': 0.0}
        self.temporal_evaluator = TemporalMetrics(sequence_length=sequence_length, threshold=threshold,
                                                  device=self.device)
        self.region_evaluator = RegionMetrics(device=self.device)
        self.front_tracking_evaluator = FrontTrackingMetrics(device=self.device)
        self._steps = []          # per update: confusion-matrix snapshot + evaluator log lengths (device)
        self._replayed = 0        # updates already folded into best_score

    # ---- counting -------------------------------------------------------------------------------------
    def _dev(self, a, what):
        return as_device_masks(a, self.device, what)

    def _fast_hist(self, label_true, label_pred):
        """n x n int64 histogram (device tensor) of one batch: reference :24-31"""
        return ops.confusion_matrix(self._dev(label_true, "label_true"), self._dev(label_pred, "label_pred"),
                                    self.n_classes)

    def update(self, label_trues, label_preds, sequence_data=True):
        """reference :100-137: a sequence feeds the temporal evaluator and contributes its LAST frame to the region and
        front evaluators and the confusion matrix; a batch contributes all of it"""
        gts, preds = self._dev(label_trues, "label_trues"), self._dev(label_preds, "label_preds")
        if sequence_data:
            # TemporalMetrics stores preprocess(preds[-1]); calculate_error preprocesses preds[-1]: one view serves both
            pv, gv = FrameView(first_preprocess(preds)), FrameView(first_preprocess(gts))
            self.temporal_evaluator._update_views(pv, gv)
            self.region_evaluator.update(preds[-1], gts[-1])
            self.front_tracking_evaluator._update_views(pv, gv)
            gts, preds = gts[-1], preds[-1]
        else:
            frames_p = preds if preds.dim() == 3 else preds.unsqueeze(0)
            frames_g = gts if gts.dim() == 3 else gts.unsqueeze(0)
            for p, g in zip(frames_p, frames_g):
                self.region_evaluator.update(p, g)
                self.front_tracking_evaluator.update(p, g)
        ops.confusion_matrix(gts, preds, self.n_classes, hist=self._hist)
        counts = [torch.full((1,), len(e._rows), dtype=torch.int64, device=self.device)       # fills, no copies
                  for e in (self.temporal_evaluator, self.front_tracking_evaluator, self.region_evaluator)]
        self._steps.append(torch.cat([self._hist.flatten()] + counts))

    def update_logits(self, label_trues, logits):
        """prediction = logits.max(1)[1] fused into the counting kernel; logits [B, C, H, W] fp32 on the device"""
        ops.confusion_matrix_logits(self._dev(label_trues, "label_trues"), logits, self.n_classes, hist=self._hist)

    # ---- results ---------------------------------------------------------------------------------------
    @property
    def confusion_matrix(self):
        """host copy, float64 like the reference's np.zeros accumulator (:12)"""
        return self._hist.cpu().numpy().astype(np.float64)

    def _calculate_foreground_metrics(self, hist):
        """reference :33-63 (without its debug prints)"""
        fg = self.FOREGROUND_CLASS
        true_positives = hist[fg, fg]
        false_positives = hist[:, fg].sum() - true_positives
        false_negatives = hist[fg, :].sum() - true_positives
        eps = 1e-7
        foreground_iou = true_positives / (true_positives + false_positives + false_negatives + eps)
        precision = true_positives / (true_positives + false_positives + eps)
        recall = true_positives / (true_positives + false_negatives + eps)
        f1_score = 2 * precision * recall / (precision + recall + eps)
        background_tp = hist[0, 0]
        background_fp = hist[:, 0].sum() - background_tp
        background_fn = hist[0, :].sum() - background_tp
        background_iou = background_tp / (background_tp + background_fp + background_fn + eps)
        miou = (background_iou + foreground_iou) / 2.0
        return miou, foreground_iou, precision, recall, f1_score

    def _calculate_weighted_score(self, results):
        """reference :63-97"""
        norm_front_error = 1.0 - min(results["Front Tracking Error"] / 10.0, 1.0)
        return (WEIGHTS["MIoU"] * results["MIoU"] + WEIGHTS["Foreground IoU"] * results["Foreground IoU"] +
                WEIGHTS["Foreground F1"] * results["Foreground F1"] +
                WEIGHTS["Front Tracking Error"] * norm_front_error +
                WEIGHTS["Temporal Consistency"] * results["Temporal Consistency"] +
                WEIGHTS["Region Continuity"] * results["Region Continuity"])

    def _fetch(self):
        """the one device-to-host copy: every pending log, the confusion matrix included"""
        evals = (self.temporal_evaluator, self.front_tracking_evaluator, self.region_evaluator)
        parts = [self._hist.flatten().to(torch.float64)]
        parts += [e._pending().flatten() for e in evals if e._rows]
        if self._steps:
            parts.append(torch.stack(self._steps).flatten().to(torch.float64))
        host = torch.cat(parts).cpu().numpy()
        nc2 = self.n_classes ** 2
        hist, off = host[:nc2].reshape(self.n_classes, self.n_classes), nc2
        for e in evals:
            if e._rows:
                n = len(e._rows) * e.WIDTH
                e._set_host(host[off:off + n])
                off += n
        steps = host[off:].reshape(len(self._steps), nc2 + 3)
        return hist, steps

    def _results(self, hist, n_temporal=None, n_front=None, n_region=None):
        """reference :139-188 (without the best-score bookkeeping) over the first n_* records of each evaluator"""
        miou, foreground_iou, precision, recall, f1_score = self._calculate_foreground_metrics(hist)
        n_windows = None if n_temporal is None else max(0, n_temporal - self.sequence_length + 1)
        temporal = self.temporal_evaluator._statistics(n_windows)
        region_mean, region_ratio = self.region_evaluator._stats(n_region)
        return {"MIoU": miou, "Foreground IoU": foreground_iou, "Foreground F1": f1_score,
                "Temporal Consistency": temporal["mean_score"],
                "Front Tracking Error": self.front_tracking_evaluator._mean_error(n_front),
                "Region Continuity": region_mean, "Precision": precision, "Recall": recall,
                "Transition Accuracy": temporal["mean_transition"], "Stability Score": temporal["mean_stability"],
                "Motion Consistency": temporal["mean_motion"], "Wave Segment Score": temporal["mean_wave_segment"],
                "Region Valid Ratio": region_ratio}

    def _replay(self, steps):
        """the weighted score the reference computes after each update (:124-137), for the updates not folded yet"""
        nc2 = self.n_classes ** 2
        for row in steps[self._replayed:]:
            hist = row[:nc2].reshape(self.n_classes, self.n_classes)
            nt, nf, nr = (int(v) for v in row[nc2:])
            w = self._calculate_weighted_score(self._results(hist, nt, nf, nr))
            if w > self.best_score['weighted_score']:
                self.best_score['weighted_score'] = w
        self._replayed = len(steps)

    def get_results(self, update_best=True):
        hist, steps = self._fetch()
        self._replay(steps)
        results = self._results(hist)
        if update_best:
            w = self._calculate_weighted_score(results)
            if w > self.best_score['weighted_score']:
                self.best_score['weighted_score'] = w
        results["Best Score"] = self.best_score['weighted_score']
        return results

    def reset(self):
        """reference :190-195; the best score survives, so pending updates are folded into it first"""
        if self._replayed < len(self._steps):
            self._replay(self._fetch()[1])
        self._hist.zero_()
        self.temporal_evaluator.reset()
        self.region_evaluator.reset()
        self.front_tracking_evaluator.reset()
        self._steps, self._replayed = [], 0
