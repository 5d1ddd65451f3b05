"""Boundary validation metrics: how far the contour of a predicted mask lies from the contour of its label mask, per image and
class, from exact distances computed on the device (ops.boundary_metrics, include/iswm_hip_bm.h).

Per image, class c of K ('foreground': 1 .. C-1, 'all': 0 .. C-1) and direction (predicted contour -> label contour, label contour
-> predicted contour) the kernel leaves n (contour pixels), within (those at most `tolerance` pixels from the other contour), the
largest squared distance, the squared distance of the `percent`-th nearest rank, and the sum of the distances.  get_results()
aggregates on the host in float64 over every (image, class) pair seen:

    Boundary Precision = sum withinP / sum nP      Boundary Recall = sum withinG / sum nG      Boundary F1 = 2PR / (P + R)
    (each 0 where its denominator is 0), and over the M matched pairs (both contours present):
    ASSD = mean (dsumP + dsumG) / (nP + nG)     HD = mean sqrt(max(max2P, max2G))     HD95 = mean sqrt(max(q2P, q2G))
    (each nan when M = 0; the key stays HD95 whatever `percent` is),
    Boundary Pairs = M      Boundary Missed = #{nG > 0, nP = 0}      Boundary Spurious = #{nP > 0, nG = 0}

update() never synchronises: the two result tensors of each call stay in a device log, and get_results() copies the log to the
host in one transfer.  Batches of different H x W may be mixed; each update is one call.
"""
import math

import torch

from .. import ops
from .sequence_metrics import as_device_masks


class BoundaryMetrics(object):
    def __init__(self, n_classes, classes='foreground', ignore_index=255, tolerance=2, percent=95, device=None):
        self.n_classes, self.classes, self.ignore_index = int(n_classes), classes, int(ignore_index)
        self.tolerance, self.percent = tolerance, percent
        self.device = torch.device(device if device is not None else "cuda")
        self._log = []            # per update: (stats [B,|K|,2,4] int64, dsum [B,|K|,2] float64), device tensors

    def update(self, label_trues, label_preds):
        """the argument order of StreamMetrics.update: labels first"""
        gts, preds = as_device_masks(label_trues, self.device, "label_trues"), as_device_masks(label_preds, self.device, "label_preds")
        if gts.dim() == 2:
            gts, preds = gts.unsqueeze(0), preds.unsqueeze(0)
        self._log.append(ops.boundary_metrics(preds, gts, self.n_classes, self.classes, self.ignore_index, self.tolerance,
                                              self.percent))

    def update_logits(self, label_trues, logits):
        """prediction = logits.max(1)[1]; logits [B, C, H, W] fp32 on the device"""
        self.update(label_trues, ops.argmax_nchw(logits))

    def _fetch(self):
        """the one device-to-host copy -> (stats [M, 2, 4] as Python ints, dsum [M, 2] as Python floats) of every pair seen.  The
        integers travel as float64: every one of them is below 2^25, exact there."""
        if not self._log:
            return [], []
        stats = torch.cat([s.reshape(-1, 8) for s, _ in self._log])
        dsum = torch.cat([d.reshape(-1, 2) for _, d in self._log])
        host = torch.cat([stats.to(torch.float64), dsum], 1).cpu().tolist()
        return [[[int(v) for v in row[0:4]], [int(v) for v in row[4:8]]] for row in host], [row[8:10] for row in host]

    def get_results(self):
        stats, dsum = self._fetch()
        n_p = sum(s[0][0] for s in stats)
        n_g = sum(s[1][0] for s in stats)
        precision = sum(s[0][1] for s in stats) / n_p if n_p else 0.0
        recall = sum(s[1][1] for s in stats) / n_g if n_g else 0.0
        f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
        matched = [(s, d) for s, d in zip(stats, dsum) if s[0][0] > 0 and s[1][0] > 0]
        m = len(matched)
        nan = float("nan")
        assd = math.fsum((d[0] + d[1]) / (s[0][0] + s[1][0]) for s, d in matched) / m if m else nan
        hd = math.fsum(math.sqrt(max(s[0][2], s[1][2])) for s, _ in matched) / m if m else nan
        hd95 = math.fsum(math.sqrt(max(s[0][3], s[1][3])) for s, _ in matched) / m if m else nan
        return {"Boundary Precision": float(precision), "Boundary Recall": float(recall), "Boundary F1": float(f1),
                "ASSD": float(assd), "HD": float(hd), "HD95": float(hd95), "Boundary Pairs": float(m),
                "Boundary Missed": float(sum(1 for s in stats if s[1][0] > 0 and s[0][0] == 0)),
                "Boundary Spurious": float(sum(1 for s in stats if s[0][0] > 0 and s[1][0] == 0))}

    def reset(self):
        self._log = []
