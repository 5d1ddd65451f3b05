"""CPU restatement of the reference's sequence-validation metrics -- the parity pin of iswm_amd/csrc/mask_metrics.hip
and iswm_amd/metrics/{sequence,stream}_metrics.py.

numpy + scipy.ndimage.label only (cv2 is not needed): cv2's 3x3 MORPH_RECT close / open / dilate / erode are restated
with a neutral border, and cv2.connectedComponentsWithStats with an 8-connected scipy labelling, whose numbering
follows the raster order of each component's first pixel -- so np.argmax over the areas breaks ties towards the
component whose first pixel comes first, the rule the device path implements.

Line numbers cite the reference tree: metrics/utils/mask_utils.py (MU), metrics/temporal_metrics.py (TM),
metrics/front_tracking_metrics.py (FT), metrics/region_metrics.py (RM), metrics/stream_metrics.py (SM).
"""
import numpy as np
from scipy.ndimage import label as _label

EIGHT = np.ones((3, 3), dtype=int)


def _shift_stack(m, r, fill):
    """the (2r+1)^2 shifted copies of m, outside pixels = fill"""
    h, w = m.shape
    p = np.full((h + 2 * r, w + 2 * r), fill, dtype=m.dtype)
    p[r:r + h, r:r + w] = m
    return [p[dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)]


def dilate(m, r=1):
    """cv2.dilate, rect (2r+1)^2 kernel, default border (never dilates)"""
    return np.maximum.reduce(_shift_stack(m.astype(np.uint8), r, 0))


def erode(m, r=1):
    """cv2.erode, rect (2r+1)^2 kernel, default border (never erodes)"""
    return np.minimum.reduce(_shift_stack(m.astype(np.uint8), r, 1))


def close3(m):
    return erode(dilate(m))


def open3(m):
    return dilate(erode(m))


def components(m):
    """8-connected labelling: (labels 0 = background, 1.. in raster order of first pixel; areas per label)"""
    lab, n = _label(m > 0, structure=EIGHT)
    areas = np.bincount(lab.ravel(), minlength=n + 1)[1:]
    return lab, n, areas


def canonical_labels(m):
    """labels as the device numbers them: the smallest raster index of the component, -1 for background; areas at
    the root"""
    lab, n, areas = components(m)
    flat = lab.ravel()
    _, first = np.unique(flat, return_index=True)               # first raster index of labels 0..n
    first = first[1:] if flat[first[0]] == 0 else first
    root = np.concatenate([[-1], first]).astype(np.int64)
    root_area = np.zeros(m.size, dtype=np.int64)
    root_area[first] = areas
    return root[flat].reshape(m.shape), root_area.reshape(m.shape)


def preprocess_mask(mask):
    """MU:7-50.  Returns the reference's array: uint8 0/1 for one valid component, float64 mask*weight for several,
    zeros for none."""
    mask = np.asarray(mask)
    if mask.ndim == 3:                                           # MU:11-12
        mask = mask[-1]
    m = (mask > 0).astype(np.uint8)                              # MU:14
    m = open3(close3(m))                                         # MU:18-20
    lab, n, areas = components(m)                                # MU:23
    if n == 0:                                                   # MU:25 (num_labels > 1 fails): the cleaned mask
        return m
    valid = np.flatnonzero(areas >= m.size * 0.001) + 1          # MU:28-32
    if len(valid) == 0:                                          # MU:44-45
        return np.zeros_like(m)
    largest = valid[np.argmax(areas[valid - 1])]                 # MU:36
    base = (lab == largest).astype(np.uint8)
    if len(valid) > 1:                                           # MU:39-42
        return base * max(0.4, 1.0 - 0.2 * (len(valid) - 1))
    return base


def find_front_positions(mask):
    """MU:52-72: preprocess again, then the leftmost pixel equal to 1 of each row"""
    m = preprocess_mask(mask)
    if not np.any(m):
        return []
    out = []
    for i in range(m.shape[0]):
        cols = np.flatnonzero(m[i] == 1)
        if len(cols):
            out.append((i, cols[0]))
    return out


def calculate_motion(curr, prev):
    """MU:74-101"""
    cf, pf = find_front_positions(curr), find_front_positions(prev)
    if not cf or not pf:
        return 0.0
    cy, cx = np.mean([p[0] for p in cf]), np.mean([p[1] for p in cf])
    py, px = np.mean([p[0] for p in pf]), np.mean([p[1] for p in pf])
    d = np.sqrt((cy - py) ** 2 + (cx - px) ** 2)
    return 1.0 / (1.0 + d / (curr.shape[0] * 0.1))


def calculate_stability(curr, prev):
    """MU:103-135: rows of the (re-)preprocessed current frame, searched in [c-ws, c+ws) of the previous one"""
    c, p = preprocess_mask(curr), preprocess_mask(prev)
    ws = int(c.shape[1] * 0.1)
    scores = []
    for i in range(c.shape[0]):
        cols = np.flatnonzero(c[i] == 1)
        if len(cols) == 0:
            continue
        front = cols[0]
        s0, s1 = max(0, front - ws), min(c.shape[1], front + ws)
        hit = np.flatnonzero(p[i, s0:s1] == 1)
        if len(hit):
            scores.append(1.0 / (1.0 + abs(front - (hit[0] + s0)) / ws))
    return np.mean(scores) if scores else 0.0


def check_wave_presence(mask, threshold=0.005):
    """MU:137-141"""
    m = preprocess_mask(mask)
    return np.sum(m) / m.size >= threshold


class TemporalMetrics:
    """TM:5-181 (the score path; history lists as in the reference)"""

    def __init__(self, sequence_length=7, threshold=0.005):
        self.sequence_length, self.threshold = sequence_length, threshold
        self.reset()

    def reset(self):
        self.preds, self.gts = [], []
        self.temporal_scores, self.transition_scores, self.stability_scores = [], [], []
        self.motion_scores, self.wave_segment_scores = [], []

    def _transitions(self, gt_w, pred_w):                       # TM:19-40
        gt_t, pr_t = np.diff(gt_w).astype(int), np.diff(pred_w).astype(int)
        if not np.any(gt_t):
            s = 1.0 if not np.any(pr_t) else 0.0
        else:
            gi, pi = np.flatnonzero(gt_t), np.flatnonzero(pr_t)
            s = 0.0 if len(gi) != len(pi) else 1.0 / (1.0 + np.mean(np.abs(gi - pi)))
        self.transition_scores.append(s)
        return s

    def _wave(self, preds):                                      # TM:42-66
        st = [calculate_stability(preds[t], preds[t - 1]) for t in range(1, len(preds))]
        mo = [calculate_motion(preds[t], preds[t - 1]) for t in range(1, len(preds))]
        self.stability_scores.append(np.mean(st) if st else 0.0)
        self.motion_scores.append(np.mean(mo) if mo else 0.0)
        return np.mean([0.5 * s + 0.5 * m for s, m in zip(st, mo)]) if st else 0.0

    def _segments(self, preds, gts, gt_w):                       # TM:73-99
        sc = [0.5 * calculate_stability(preds[t], preds[t - 1]) + 0.5 * calculate_stability(preds[t], gts[t])
              for t in range(1, len(preds)) if gt_w[t]]
        s = np.mean(sc) if sc else 0.0
        self.wave_segment_scores.append(s)
        return s

    def _consistency(self, preds, gts):                          # TM:110-125
        gt_w = [check_wave_presence(f, self.threshold) for f in gts]
        pr_w = [check_wave_presence(f, self.threshold) for f in preds]
        if not any(gt_w):
            return 1.0 - sum(pr_w) / len(pr_w)                   # TM:68-71
        if all(gt_w):
            return self._wave(preds)
        return 0.6 * self._transitions(gt_w, pr_w) + 0.4 * self._segments(preds, gts, gt_w)   # TM:101-108

    def update(self, pred, gt):                                  # TM:127-151
        pred, gt = np.asarray(pred), np.asarray(gt)
        self.preds.append(preprocess_mask(pred) if pred.ndim > 2 else pred)
        self.gts.append(preprocess_mask(gt) if gt.ndim > 2 else gt)
        if len(self.preds) == self.sequence_length:
            self.temporal_scores.append(self._consistency(self.preds, self.gts))
            self.preds, self.gts = self.preds[1:], self.gts[1:]

    def get_mean_score(self):
        return np.mean(self.temporal_scores) if self.temporal_scores else 0.0

    def get_detailed_statistics(self):                           # TM:163-172
        m = lambda v: np.mean(v) if v else 0.0
        return {"mean_score": self.get_mean_score(), "mean_transition": m(self.transition_scores),
                "mean_stability": m(self.stability_scores), "mean_motion": m(self.motion_scores),
                "mean_wave_segment": m(self.wave_segment_scores), "score_count": len(self.temporal_scores)}


class FrontTrackingMetrics:
    """FT:6-133"""

    def __init__(self):
        self.max_distance_threshold = None
        self.tracking_errors = []

    def calculate_error(self, pred, gt):                          # FT:18-113
        tau = self.max_distance_threshold
        pf = find_front_positions(preprocess_mask(pred))
        gf = find_front_positions(preprocess_mask(gt))
        if gf and not pf:
            return tau * 2.0
        if pf and not gf:
            return tau * 1.5
        if not gf and not pf:
            return 0.0

        def one_way(src, dst):
            err = wsum = 0
            nv = 0
            for sy, sx in src:
                best, bdx = float("inf"), float("inf")
                for dy, dx in dst:
                    d = np.sqrt((sy - dy) ** 2 + (sx - dx) ** 2)
                    if d < best:
                        best, bdx = d, abs(sx - dx)
                if best < tau:
                    w = 1.0 / (bdx + 1e-6)
                    err += best * w
                    wsum += w
                    nv += 1
            return err, wsum, nv

        pe, pw, pn = one_way(pf, gf)
        ge, gw, gn = one_way(gf, pf)
        if pn == 0 or gn == 0:
            return tau * 2.0
        cover = gn / len(gf)
        return max(pe / pw, ge / gw) + (1.0 - cover) * tau * 0.5

    def update(self, pred, gt):                                   # FT:115-124
        if self.max_distance_threshold is None:
            self.max_distance_threshold = np.asarray(pred).shape[1] * 0.1
        self.tracking_errors.append(self.calculate_error(pred, gt))

    def get_mean_error(self):                                     # FT:126-133
        v = [x for x in self.tracking_errors if not np.isinf(x)]
        if not v:
            return self.max_distance_threshold * 2.0 if self.max_distance_threshold is not None else float("inf")
        return np.mean(v)

    def reset(self):
        self.tracking_errors = []


def repair_small_gaps(m):
    """RM:7-12: 3 x dilate then 2 x erode, 3x3"""
    for _ in range(3):
        m = dilate(m)
    for _ in range(2):
        m = erode(m)
    return m


def fragmentation(areas):
    """RM:20-36 over the areas of the components >= 50 px"""
    if not len(areas):
        return 0.0
    a = sorted(areas, reverse=True)
    total = sum(a)
    ratios = [x / total for x in a]
    s = ratios[0]
    if len(a) > 1:
        s -= sum(r * (i + 1) / len(a) for i, r in enumerate(ratios[1:])) * 0.5
    return max(0.0, min(1.0, s))


def region_metrics(pred, gt):
    """RM:78-121: None when either frame is empty, else final_score"""
    p, g = (np.asarray(pred) > 0).astype(np.uint8), (np.asarray(gt) > 0).astype(np.uint8)
    if p.sum() == 0 or g.sum() == 0:
        return None
    p = repair_small_gaps(p)
    sim = np.logical_and(p, g).sum() / np.logical_or(p, g).sum()
    _, _, areas = components(p)
    frag = float(fragmentation([int(a) for a in areas if a >= 50]))
    return float(0.7 * frag + 0.3 * float(sim))


class RegionMetrics:
    """RM:14-157 (score path)"""

    def __init__(self):
        self.reset()

    def reset(self):
        self.valid_scores, self.total_cases, self.invalid_cases = [], 0, 0

    def update(self, pred, gt):
        self.total_cases += 1
        s = region_metrics(pred, gt)
        if s is None:
            self.invalid_cases += 1
        else:
            self.valid_scores.append(s)

    def get_mean_score(self):
        return np.mean(self.valid_scores) if self.valid_scores else 0.0

    def valid_ratio(self):
        return len(self.valid_scores) / self.total_cases if self.valid_scores else 0.0


WEIGHTS = {"MIoU": 0.05, "Foreground IoU": 0.25, "Foreground F1": 0.25, "Front Tracking Error": 0.25,
           "Temporal Consistency": 0.10, "Region Continuity": 0.10}     # SM:65-73, train.py:842-850


def weighted_score(r):
    """SM:63-97"""
    nfe = 1.0 - min(r["Front Tracking Error"] / 10.0, 1.0)
    return (WEIGHTS["MIoU"] * r["MIoU"] + WEIGHTS["Foreground IoU"] * r["Foreground IoU"] +
            WEIGHTS["Foreground F1"] * r["Foreground F1"] + WEIGHTS["Front Tracking Error"] * nfe +
            WEIGHTS["Temporal Consistency"] * r["Temporal Consistency"] +
            WEIGHTS["Region Continuity"] * r["Region Continuity"])


def foreground_metrics(h):
    """SM:33-61"""
    tp = h[1, 1]
    fp, fn = h[:, 1].sum() - tp, h[1, :].sum() - tp
    eps = 1e-7
    iou = tp / (tp + fp + fn + eps)
    prec, rec = tp / (tp + fp + eps), tp / (tp + fn + eps)
    f1 = 2 * prec * rec / (prec + rec + eps)
    btp = h[0, 0]
    biou = btp / (btp + h[:, 0].sum() - btp + h[0, :].sum() - btp + eps)
    return (biou + iou) / 2.0, iou, prec, rec, f1


class StreamMetrics:
    """SM:7-195 for two classes (the metric half; debug prints dropped)"""

    def __init__(self, n_classes=2, sequence_length=7, threshold=0.005):
        self.n = n_classes
        self.hist = np.zeros((n_classes, n_classes))
        self.best = 0.0
        self.temporal = TemporalMetrics(sequence_length, threshold)
        self.region = RegionMetrics()
        self.front = FrontTrackingMetrics()

    def _fast_hist(self, t, p):                                   # SM:24-31
        t, p = np.asarray(t).ravel().astype(np.int64), np.asarray(p).ravel().astype(np.int64)
        k = (t >= 0) & (t < self.n)
        return np.bincount(self.n * t[k] + p[k], minlength=self.n ** 2).reshape(self.n, self.n)

    def update(self, gts, preds, sequence_data=True):             # SM:100-137
        gts, preds = np.asarray(gts), np.asarray(preds)
        if sequence_data:
            self.temporal.update(preds, gts)
            self.region.update(preds[-1], gts[-1])
            self.front.update(preds[-1], gts[-1])
            self.hist += self._fast_hist(gts[-1], preds[-1])
        else:
            self.region.update(preds, gts)
            self.front.update(preds, gts)
            self.hist += self._fast_hist(gts, preds)
        self.best = max(self.best, weighted_score(self.get_results(update_best=False)))

    def get_results(self, update_best=True):                      # SM:139-188
        miou, iou, prec, rec, f1 = foreground_metrics(self.hist)
        ts = self.temporal.get_detailed_statistics()
        r = {"MIoU": miou, "Foreground IoU": iou, "Foreground F1": f1,
             "Temporal Consistency": self.temporal.get_mean_score(),
             "Front Tracking Error": self.front.get_mean_error(),
             "Region Continuity": self.region.get_mean_score(), "Precision": prec, "Recall": rec,
             "Transition Accuracy": ts["mean_transition"], "Stability Score": ts["mean_stability"],
             "Motion Consistency": ts["mean_motion"], "Wave Segment Score": ts["mean_wave_segment"],
             "Region Valid Ratio": self.region.valid_ratio()}
        if update_best:
            self.best = max(self.best, weighted_score(r))
        r["Best Score"] = self.best
        return r


def is_best_score(current, best, weights=WEIGHTS):
    """train.py:760-797 (best None -> True)"""
    if best is None:
        return True
    cur = bst = 0.0
    for k in ("MIoU", "Foreground IoU", "Foreground F1", "Temporal Consistency", "Region Continuity"):
        if weights.get(k, 0) > 0:
            v = float(current[k])
            if not np.isnan(v):
                cur += weights[k] * v
                bst += weights[k] * float(best.get(k, 0.0))
    if "Front Tracking Error" in current:
        w = abs(weights.get("Front Tracking Error", 0.03))
        cur += w * max(0, 1 - float(current["Front Tracking Error"]) / 10.0)
        bst += w * max(0, 1 - float(best.get("Front Tracking Error", 10.0)) / 10.0)
    return cur > bst
