"""Restatement of the boundary validation metrics of csrc/boundary_metrics.hip (include/iswm_hip_bm.h), with the label and
prediction builders and the case table that tests/test_boundary_metrics_cpu.py (no GPU: the restatements against each other and
against tests/boundary_ref.py's signed map, hand-worked planes, the rank rule, the degenerate values, eight mutants) and
tests/test_boundary_metrics_gpu.py (the kernels, the metrics object, the trainer) share.

Nothing here calls the product: numpy, scipy and math on the CPU only.  The definition, written out again:

    pred [B,H,W], labels [B,H,W]; K = {1 .. C-1} ('foreground') or {0 .. C-1} ('all'); a pixel is valid when its LABEL is
    (y != ignore_index and 0 <= y < C); the prediction's value plays no part in validity, and a predicted value outside [0, C) is in
    no class's mask.  Per image and class c of K:
        G = {p valid : y_p == c}          P = {p valid : pred_p == c}
        S(A) = {p in A : some 4-neighbour q inside the image is valid and q not in A}
    Invalid pixels and the image edge make no contour.  Distances run in the plain pixel grid and pass through invalid pixels.
    For X -> Y in (S(P) -> S(G), S(G) -> S(P)), d2(p) = min over q in Y of |p - q|^2:
        n = |X|;  within = #{d2 <= tau^2};  max2 = max d2;  q2 = the d2 of 1-based ascending rank (percent * n + 99) // 100;
        dsum = sum of sqrt(d2);   Y empty: within 0, max2 -1, q2 -1, dsum 0 (n as counted);  X empty: the same with n = 0.
    Aggregation over every (image, class) pair seen, in float64:
        Boundary Precision = sum withinP / sum nP, Boundary Recall = sum withinG / sum nG, Boundary F1 = 2PR / (P + R), each 0
        where its denominator is 0; over the M matched pairs (nP > 0 and nG > 0): ASSD = mean (dsumP + dsumG) / (nP + nG),
        HD = mean sqrt(max(max2P, max2G)), HD95 = mean sqrt(max(q2P, q2G)), each nan when M = 0; Boundary Pairs = M,
        Boundary Missed = #{nG > 0, nP = 0}, Boundary Spurious = #{nP > 0, nG = 0}.

The contour has two restatements (the 4-neighbour rule written out; A & ~binary_erosion(A | invalid, cross, border_value=1)) and so
have the distances (brute force in numpy integers over the contour pixels of both sets; scipy's distance_transform_edt of the
array whose zeros are the other contour, squared and rounded: a squared distance between grid points is an integer and scipy's
float64 distance is within 1e-9 of its root at these sizes).  test_boundary_metrics_cpu.py shows each pair equal.

Predictions are perturbed copies of the labels (shifted, dilated, eroded, a blob added, a part dropped), so distances span 0 to
tens of pixels: independent random masks would put every distance at 2 or less and test nothing.  Every case that is not labelled
degenerate has nP >= 20 and nG >= 20 on each of its planes that is not listed as a degenerate plane; build() asserts it.
"""
import functools
import math

import numpy as np

from tests.boundary_ref import pattern

IGNORE = 255
PATTERNS = ("blobs", "bands", "corner_fg", "one_bg", "full_row", "checker", "ignore_frame", "out_of_range")
CONTOUR_MUTANTS = ("eight_neighbours", "edge_is_contour", "invalid_is_outside")
DISTANCE_MUTANTS = ("cityblock", "column_only")
STAT_MUTANTS = ("directions_swapped", "rank_floor", "strict_tolerance")
MIN_CONTOUR = 20
KEYS = ("Boundary Precision", "Boundary Recall", "Boundary F1", "ASSD", "HD", "HD95", "Boundary Pairs", "Boundary Missed",
        "Boundary Spurious")


def selected(c, classes):
    assert classes in ("foreground", "all")
    return list(range(1 if classes == "foreground" else 0, c))


def valid_of(lab, c, ignore_index):
    return (lab != ignore_index) & (lab >= 0) & (lab < c)


def masks(lab, pred, c, cls, ignore_index):
    """(G, P, valid) of one image (int64 [H,W]) and class"""
    valid = valid_of(lab, c, ignore_index)
    return valid & (lab == cls), valid & (pred == cls), valid


def _shifted(a, dy, dx, fill):
    """b[y, x] = a[y + dy, x + dx] where that lies inside the image, `fill` elsewhere"""
    h, w = a.shape
    out = np.full_like(a, fill)
    ys, yd = (slice(dy, h), slice(0, h - dy)) if dy >= 0 else (slice(0, h + dy), slice(-dy, h))
    xs, xd = (slice(dx, w), slice(0, w - dx)) if dx >= 0 else (slice(0, w + dx), slice(-dx, w))
    if abs(dy) < h and abs(dx) < w:
        out[yd, xd] = a[ys, xs]
    return out


def contour_rule(a, valid, mutant=None):
    """S(A), the rule written out: p in A with a 4-neighbour q inside the image that is valid and not in A"""
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if mutant == "eight_neighbours":
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    outside = (valid & ~a) if mutant != "invalid_is_outside" else ~a
    hit = np.zeros_like(a)
    for dy, dx in steps:
        hit |= _shifted(outside, dy, dx, mutant == "edge_is_contour")
    return a & hit


def contour_erosion(a, valid):
    """S(A), the second way: A without the erosion of A | invalid by the cross, the outside of the image counted as inside"""
    from scipy.ndimage import binary_erosion
    cross = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]], bool)
    return a & ~binary_erosion(a | ~valid, cross, border_value=1)


def d2_brute(x, y, mutant=None):
    """int64 [|X|]: for each pixel of the set X (bool [H,W], row-major order) the least squared distance to the set Y (not empty)"""
    py, px = np.nonzero(x)
    qy, qx = np.nonzero(y)
    assert qy.size
    out = np.empty(py.size, np.int64)
    step = max(1, (1 << 22) // qy.size)
    for s in range(0, py.size, step):
        dy, dx = np.abs(py[s:s + step, None] - qy[None]), np.abs(px[s:s + step, None] - qx[None])
        if mutant == "cityblock":
            d = (dy + dx) ** 2
        elif mutant == "column_only":
            d = dy * dy + (dx != 0) * (1 << 20)
        else:
            d = dy * dy + dx * dx
        out[s:s + step] = d.min(1)
    return out


def d2_scipy(x, y):
    from scipy.ndimage import distance_transform_edt
    assert y.any()
    d = distance_transform_edt(~y)[x]
    return np.rint(d * d).astype(np.int64)


def rank_of(n, percent, mutant=None):
    """the 1-based nearest rank, in integers"""
    if mutant == "rank_floor":
        return max(1, (percent * n) // 100)
    return (percent * n + 99) // 100


def direction_stats(d2, n, tolerance, percent, mutant=None):
    """([n, within, max2, q2], dsum) of one direction; d2: the int64 distances of X's pixels, or None when Y is empty"""
    if d2 is None or n == 0:
        return [n, 0, -1, -1], 0.0
    assert d2.size == n
    d = sorted(int(v) for v in d2)
    tau2 = tolerance * tolerance
    within = sum(1 for v in d if (v < tau2 if mutant == "strict_tolerance" else v <= tau2))
    return [n, within, d[-1], d[rank_of(n, percent, mutant) - 1]], math.fsum(math.sqrt(v) for v in d)


def plane_stats(lab, pred, c, cls, ignore_index, tolerance, percent, how="brute", contour="rule", mutant=None):
    """([[n, within, max2, q2] of S(P) -> S(G), the same of S(G) -> S(P)], [dsum, dsum]) of one image and class"""
    g, p, valid = masks(lab, pred, c, cls, ignore_index)
    cm = mutant if mutant in CONTOUR_MUTANTS else None
    sg, sp = (contour_rule(g, valid, cm), contour_rule(p, valid, cm)) if contour == "rule" else \
        (contour_erosion(g, valid), contour_erosion(p, valid))
    dm = mutant if mutant in DISTANCE_MUTANTS else None
    assert dm is None or how == "brute"
    dist = (lambda x, y: d2_brute(x, y, dm)) if how == "brute" else d2_scipy
    sm = mutant if mutant in STAT_MUTANTS else None
    pairs = [(sp, sg), (sg, sp)]
    if sm == "directions_swapped":
        pairs.reverse()
    stats, dsum = [], []
    for x, y in pairs:
        s, d = direction_stats(dist(x, y) if x.any() and y.any() else None, int(x.sum()), tolerance, percent, sm)
        stats.append(s)
        dsum.append(d)
    return stats, dsum


def reference(pred, labels, c, classes="foreground", ignore_index=IGNORE, tolerance=2, percent=95, how="auto", contour="rule",
              mutant=None):
    """(stats int64 [B,|K|,2,4], dsum float64 [B,|K|,2]) of pred and labels (integer arrays [B,H,W])"""
    pred, labels = np.asarray(pred).astype(np.int64), np.asarray(labels).astype(np.int64)
    assert pred.shape == labels.shape and pred.ndim == 3
    ks = selected(c, classes)
    stats = np.zeros((pred.shape[0], len(ks), 2, 4), np.int64)
    dsum = np.zeros((pred.shape[0], len(ks), 2), np.float64)
    for n in range(pred.shape[0]):
        for j, cls in enumerate(ks):
            hw = how
            if hw == "auto":                                           # brute force while the two contours are small
                g, p, valid = masks(labels[n], pred[n], c, cls, ignore_index)
                small = int(contour_rule(g, valid).sum()) * int(contour_rule(p, valid).sum()) <= 1 << 24
                hw = "brute" if small else "scipy"
            stats[n, j], dsum[n, j] = plane_stats(labels[n], pred[n], c, cls, ignore_index, tolerance, percent, hw, contour, mutant)
    return stats, dsum


def aggregate(runs):
    """the dict of KEYS over runs = [(stats [B,|K|,2,4], dsum [B,|K|,2]), ...]: every (image, class) pair of every run"""
    st = [s for stats, _ in runs for s in np.asarray(stats).reshape(-1, 2, 4).tolist()]
    ds = [d for _, dsum in runs for d in np.asarray(dsum).reshape(-1, 2).tolist()]
    n_p, n_g = sum(s[0][0] for s in st), sum(s[1][0] for s in st)
    precision = sum(s[0][1] for s in st) / n_p if n_p else 0.0
    recall = sum(s[1][1] for s in st) / n_g if n_g else 0.0
    f1 = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    matched = [(s, d) for s, d in zip(st, ds) if s[0][0] > 0 and s[1][0] > 0]
    m = len(matched)
    mean = lambda values: math.fsum(values) / m if m else float("nan")
    return {"Boundary Precision": precision, "Boundary Recall": recall, "Boundary F1": f1,
            "ASSD": mean([(d[0] + d[1]) / (s[0][0] + s[1][0]) for s, d in matched]),
            "HD": mean([math.sqrt(max(s[0][2], s[1][2])) for s, _ in matched]),
            "HD95": mean([math.sqrt(max(s[0][3], s[1][3])) for s, _ in matched]),
            "Boundary Pairs": float(m),
            "Boundary Missed": float(sum(1 for s in st if s[1][0] > 0 and s[0][0] == 0)),
            "Boundary Spurious": float(sum(1 for s in st if s[0][0] > 0 and s[1][0] == 0))}


# ---- predictions: perturbed copies of the labels ---------------------------------------------------------------------
def shift(lab, dy, dx):
    """the labels moved down by dy and right by dx; background (0) comes in at the edge"""
    return _shifted(lab, -dy, -dx, 0)


def dilate(lab):
    """every foreground class grown by a pixel (the cross) into the background"""
    out = lab.copy()
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        s = _shifted(lab, dy, dx, 0)
        out = np.where((out == 0) & (s > 0) & (s < IGNORE), s, out)
    return out


def erode(lab):
    """every foreground pixel with a 4-neighbour of another value becomes background"""
    out = lab.copy()
    rim = np.zeros(lab.shape, bool)
    for dy, dx in ((-1, 0), (1, 0), (0, -1), (0, 1)):
        s = _shifted(lab, dy, dx, -7)                                   # (-7: outside the image, no neighbour)
        rim |= (s != lab) & (s != -7)
    out[rim & (lab > 0) & (lab < IGNORE)] = 0
    return out


def add_blob(lab, cls=1):
    """a disc of class `cls` near the bottom right corner"""
    h, w = lab.shape
    yy, xx = np.mgrid[0:h, 0:w]
    r = max(2.0, 0.12 * min(h, w))
    out = lab.copy()
    out[(yy - 0.8 * h) ** 2 + (xx - 0.8 * w) ** 2 <= r * r] = cls
    return out


def drop_left(lab):
    """the foreground of the left third dropped"""
    out = lab.copy()
    part = out[:, :lab.shape[1] // 3]
    part[(part > 0) & (part < IGNORE)] = 0
    return out


PERTURB = {"shift": lambda a: shift(a, 2, 3), "shift_far": lambda a: shift(a, -1, 17), "dilate": dilate, "erode": erode,
           "add_blob": add_blob, "drop_left": drop_left, "same": lambda a: a.copy()}


def rect_labels(h, w, c=2, seed=0):
    """rectangles of the foreground classes in turn, each with a border of at least 20 pixels where the plane allows one, away
    from the image edge: the generic labels of the shape cases"""
    lab = np.zeros((h, w), np.int64)
    n = max(c - 1, 1)
    for k in range(n):
        x0 = 1 + (k * (w - 2)) // n + (seed % 2)
        x1 = max(x0 + 1, 1 + ((k + 1) * (w - 2)) // n - 2)
        y0, y1 = 1 + (seed % 3 if h > 8 else 0), max(2, h - 2)
        lab[y0:y1, x0:min(x1, w - 1)] = (1 + k) if c > 1 else 0
    return lab


# ---- the cases -----------------------------------------------------------------------------------------------------------
# name -> dict(shape = (B, C, H, W), labels = how each image's labels are made, perturb = the predictions of the images in turn,
#              classes, ignore_index, degenerate = the whole case is exempt from the 20-pixel condition (planes too small for it,
#              single pixels, empty contours), degenerate_planes = class-plane indices exempt from it)
def _case(shape, labels="rect", perturb=("shift",), classes="foreground", ignore_index=IGNORE, degenerate=False,
          degenerate_planes=(), kinds=("u8", "u8")):
    return dict(shape=shape, labels=labels, perturb=tuple(perturb), classes=classes, ignore_index=ignore_index,
                degenerate=degenerate, degenerate_planes=tuple(degenerate_planes), kinds=kinds)


CASES = {
    # planes too small for 20 contour pixels: every pattern is run on them
    "1x1": _case((1, 2, 1, 1), "checker", ("same",), degenerate=True),
    "1x9": _case((1, 2, 1, 9), "checker", ("shift_1x",), degenerate=True),
    "9x1": _case((1, 2, 9, 1), "checker", ("shift_1y",), degenerate=True),
    "2x2": _case((1, 2, 2, 2), "checker", ("shift_1x",), degenerate=True),
    # the row block's thread stride
    "6x255": _case((1, 2, 6, 255), "bands", ("shift",)),
    "6x256": _case((1, 2, 6, 256), "bands", ("shift",)),
    "6x257": _case((1, 2, 6, 257), "bands", ("shift",)),
    # the column batch
    "7x40": _case((1, 2, 7, 40)), "8x40": _case((1, 2, 8, 40)), "9x40": _case((1, 2, 9, 40)),
    "15x40": _case((1, 2, 15, 40), perturb=("dilate",)), "16x40": _case((1, 2, 16, 40), perturb=("erode",)),
    "17x40": _case((1, 2, 17, 40), perturb=("shift_far",)),
    # three images, three classes, both class selections: leaks across images and class planes
    "b3c3_fg": _case((3, 3, 33, 61), "rect", ("shift", "dilate", "add_blob")),
    "b3c3_all": _case((3, 3, 33, 61), "rect", ("shift", "erode", "add_blob"), classes="all"),
    "33x300": _case((2, 2, 33, 300), "blobs300", ("shift", "drop_left")),
    "3x2897": _case((1, 2, 3, 2897), "row", ("shift_1y",)),
    "2897x3": _case((1, 2, 2897, 3), "column", ("shift_1x",)),
    # the two contours at opposite ends (d2 = 4076^2 + .. : the largest a two-pixel-wide plane reaches is 4095^2 + 1 < 2^24) and,
    # for the select's top bit, at opposite corners of the largest plane (d2 > 2^24)
    "2x4096": _case((1, 2, 2, 4096), "ends_x", ("ends",)),
    "4096x2": _case((1, 2, 4096, 2), "ends_y", ("ends",)),
    "4096x4096": _case((1, 2, 4096, 4096), "corners", ("ends",)),
    # the four label / prediction width pairs
    "u8_i64": _case((2, 2, 19, 47), "rect", ("shift", "dilate"), kinds=("u8", "i64")),
    "i64_u8": _case((2, 2, 19, 47), "rect", ("shift", "dilate"), kinds=("i64", "u8")),
    "i64_i64": _case((2, 2, 19, 47), "rect", ("shift", "dilate"), kinds=("i64", "i64")),
    # ignore_index inside [0, C): the plane of class 3 has no label contour (degenerate), its predictions are spurious
    "ig_inside": _case((2, 4, 33, 91), "rect_ig", ("shift", "dilate"), ignore_index=3, degenerate_planes=(2,)),
    # a predicted value outside [0, C): in no class's mask, still a valid "other" pixel that makes contour
    "pred_outside": _case((2, 2, 23, 57), "rect", ("outside", "outside"), kinds=("u8", "i64")),
    # a segment whose distances are all equal: two full rows 5 apart
    "all_equal": _case((1, 2, 17, 64), "row8", ("shift_5y",)),
    # a pixel on both contours, and the same mask both ways
    "same": _case((2, 2, 21, 45), "rect", ("same", "same")),
    # degenerate planes
    "no_pred": _case((1, 2, 13, 31), "rect", ("zeros",), degenerate=True),
    "no_label": _case((1, 2, 13, 31), "zeros", ("rect",), degenerate=True),
    "neither": _case((1, 2, 13, 31), "zeros", ("zeros",), degenerate=True),
    "all_ignored": _case((1, 2, 13, 31), "ignored", ("rect",), degenerate=True),
    "all_foreground": _case((1, 2, 13, 31), "ones", ("ones",), degenerate=True),
}
# every pattern of tests/boundary_ref.py as it is; the single foreground pixel and the single background pixel have 1 and 4 contour
# pixels and are labelled degenerate
PATTERN_CASES = {"pat_" + p: _case((2, 2, 33, 47), "pattern:" + p, ("shift", "shift_far"), degenerate=p in ("corner_fg", "one_bg"))
                 for p in PATTERNS}
CASES.update(PATTERN_CASES)
TOLERANCES = (0, 2, 5)
PERCENTS = (1, 50, 95, 100)
BIG = dict(shape=(16, 2, 513, 513), tolerance=2, percent=95)          # the dsum bound at n > 4096: band labels, shifted by 3


def _labels_of(how, h, w, c, seed, ignore_index):
    if how == "rect":
        return rect_labels(h, w, c, seed)
    if how == "rect_ig":                                                # class 3 is the ignore value: a frame of it, as a padded crop
        lab = rect_labels(h, w, 3, seed)
        lab[:2], lab[-2:], lab[:, :2], lab[:, -2:] = 3, 3, 3, 3
        return lab
    if how == "zeros":
        return np.zeros((h, w), np.int64)
    if how == "ones":
        return np.ones((h, w), np.int64)
    if how == "ignored":
        return np.full((h, w), ignore_index, np.int64)
    if how == "checker":
        return pattern("checker", h, w, c, seed)
    if how == "bands":                                                  # the thin wavy band, and a rectangle for the far end
        lab = pattern("bands", h, w, c, seed)
        lab[h - 3:h - 1, w // 2:w // 2 + 9] = 1
        return lab
    if how == "blobs300":
        return pattern("blobs", h, w, c, seed)
    if how in ("row", "row8"):
        lab = np.zeros((h, w), np.int64)
        lab[8 if how == "row8" else 0, :] = 1
        return lab
    if how == "column":
        lab = np.zeros((h, w), np.int64)
        lab[:, 0] = 1
        return lab
    if how in ("ends_x", "ends_y", "corners"):                          # a checkerboard patch at the near end: every pixel contour
        lab = np.zeros((h, w), np.int64)
        yy, xx = np.mgrid[0:min(h, 24), 0:min(w, 24)]
        lab[:min(h, 24), :min(w, 24)] = (yy + xx) % 2
        return lab
    if how.startswith("pattern:"):
        return pattern(how[8:], h, w, c, seed, ignore_index)
    raise KeyError(how)


def _pred_of(how, lab, h, w, c, seed, ignore_index):
    if how in PERTURB:
        return PERTURB[how](lab)
    if how == "shift_1x":
        return shift(lab, 0, 1)
    if how == "shift_1y":
        return shift(lab, 1, 0)
    if how == "shift_5y":
        return shift(lab, 5, 0)
    if how == "zeros":
        return np.zeros((h, w), np.int64)
    if how == "ones":
        return np.ones((h, w), np.int64)
    if how == "rect":
        return rect_labels(h, w, c, seed)
    if how == "ends":                                                   # the labels' patch, at the far end
        return lab[::-1, ::-1].copy()
    if how == "outside":                                                # a stripe of a value that is no class, through the masks
        out = shift(lab, 1, 2)
        out[:, w // 2 - 1:w // 2 + 2] = c + 5
        return out
    raise KeyError(how)


@functools.lru_cache(maxsize=None)
def build(name):
    """(pred, labels) of a case, numpy [B,H,W] of the case's two dtypes; shared and cached: do not write into them.  Asserts the
    20-pixel condition of the module docstring with the restatement alone."""
    cs = CASES[name]
    b, c, h, w = cs["shape"]
    labs = [_labels_of(cs["labels"], h, w, c, i, cs["ignore_index"]) for i in range(b)]
    preds = [_pred_of(cs["perturb"][i % len(cs["perturb"])], labs[i], h, w, c, i, cs["ignore_index"]) for i in range(b)]
    lab, pred = np.stack(labs), np.stack(preds)
    lk, pk = cs["kinds"]
    if lk == "i64" and lab.size >= 8:
        lab.reshape(-1)[lab.size // 3] = -1                                 # an int64 label below the class range
    if pk == "i64" and pred.size >= 8:
        pred.reshape(-1)[pred.size // 5] = -3                               # and such a prediction
    lab = lab.astype(np.uint8 if lk == "u8" else np.int64)
    pred = pred.astype(np.uint8 if pk == "u8" else np.int64)
    if not cs["degenerate"]:
        for n, cls, np_, ng in contour_counts(pred, lab, c, cs["classes"], cs["ignore_index"]):
            j = cls - selected(c, cs["classes"])[0]
            if j not in cs["degenerate_planes"]:
                assert np_ >= MIN_CONTOUR and ng >= MIN_CONTOUR, (name, n, cls, np_, ng)
    return pred, lab


def contour_counts(pred, labels, c, classes, ignore_index):
    """[(image, class, |S(P)|, |S(G)|)] by the restatement alone"""
    out = []
    pred, labels = pred.astype(np.int64), labels.astype(np.int64)
    for n in range(pred.shape[0]):
        for cls in selected(c, classes):
            g, p, valid = masks(labels[n], pred[n], c, cls, ignore_index)
            out.append((n, cls, int(contour_rule(p, valid).sum()), int(contour_rule(g, valid).sum())))
    return out


@functools.lru_cache(maxsize=None)
def expected(name, tolerance=2, percent=95):
    """(stats, dsum) of a case by the restatement; shared and cached: do not write into them"""
    cs = CASES[name]
    pred, lab = build(name)
    return reference(pred, lab, cs["shape"][1], cs["classes"], cs["ignore_index"], tolerance, percent)


@functools.lru_cache(maxsize=None)
def big_case():
    """(pred, labels, stats, dsum) of BIG: the band labels of the boundary loss's timing and a prediction shifted by 3 pixels"""
    b, c, h, w = BIG["shape"]
    lab = np.stack([pattern("bands", h, w, c, seed=i) for i in range(b)])
    pred = np.stack([shift(l, 3, 0) if i % 2 else shift(l, 0, 3) for i, l in enumerate(lab)])
    stats, dsum = reference(pred, lab, c, "foreground", IGNORE, BIG["tolerance"], BIG["percent"], how="scipy")
    return pred.astype(np.uint8), lab.astype(np.uint8), stats, dsum
