"""CPU restatement of sliding-window scene prediction -- the parity pin of iswm_scene_plan_make, k_scene_maps and
iswm_amd.predict.ScenePredictor.  numpy only; the maps that follow the blended probability
are tests/predict_ref.py's, unchanged.

A scene of length L per axis is cut into windows of t = min(T, L) every s = t - O pixels, the last one pulled back
to L - t; overlapping windows are blended with weights that ramp over R = max(O, 1) pixels from each window edge.
"""
import numpy as np


def plan_axis(L, T, O):
    """(t, s, n, origins) of one axis; ValueError for what iswm_scene_plan_make refuses"""
    if L < 1 or T < 1 or O < 0 or O > 1024:
        raise ValueError("bad plan: length %d, tile %d, overlap %d" % (L, T, O))
    t = min(T, L)
    if L <= t:
        return t, t, 1, [0]
    if O > t // 2:
        raise ValueError("overlap %d exceeds half of the %d-pixel window" % (O, t))
    s = t - O
    n = -(-(L - t) // s) + 1
    return t, s, n, [min(k * s, L - t) for k in range(n)]


class Plan:
    """both axes; oy / ox are the window origins (they may be replaced, e.g. mirrored, as long as they stay sorted:
    windows are numbered k = ty * ntx + tx and visited in that order)"""

    def __init__(self, H, W, T, O):
        self.H, self.W = H, W
        self.th, self.sy, self.nty, self.oy = plan_axis(H, T, O)
        self.tw, self.sx, self.ntx, self.ox = plan_axis(W, T, O)
        self.ramp = max(O, 1)

    def astuple(self):
        return (self.H, self.W, self.th, self.tw, self.sy, self.sx, self.nty, self.ntx, self.ramp)

    def windows(self):
        """(k, oy, ox) in visiting order"""
        return [(ty * self.ntx + tx, oy, ox) for ty, oy in enumerate(self.oy) for tx, ox in enumerate(self.ox)]


def w1d(length, R):
    i = np.arange(length)
    return np.minimum(np.minimum(i + 1, length - i), R).astype(np.int64)


def weights(plan):
    """(w, total): w int64 [th, tw], the weight of a window's pixel (the same for every window), and total int64
    [H, W], the sum over the windows covering each scene pixel"""
    w = np.outer(w1d(plan.th, plan.ramp), w1d(plan.tw, plan.ramp))
    total = np.zeros((plan.H, plan.W), dtype=np.int64)
    for _, oy, ox in plan.windows():
        total[oy:oy + plan.th, ox:ox + plan.tw] += w
    return w, total


def blend(p_tiles, plan, dtype):
    """per-window foreground probabilities [ntiles, th, tw] -> the scene's [H, W].
    float64: the definition, sum_t (w_t / W) p_t with integer weights w_t and W = sum_t w_t.
    float32: the kernel's order -- wn_t = float32(w_t) / float32(W), p = fma(wn_t, p_t, p) over the covering windows
    in ascending k (the fma as a float64 product and sum rounded to float32 once), then min(p, 1)."""
    p_tiles = np.asarray(p_tiles)
    w, total = weights(plan)
    assert (total > 0).all() and p_tiles.shape == (plan.nty * plan.ntx, plan.th, plan.tw)
    if dtype == np.float64:
        acc = np.zeros((plan.H, plan.W), dtype=np.float64)
        for k, oy, ox in plan.windows():
            sl = (slice(oy, oy + plan.th), slice(ox, ox + plan.tw))
            acc[sl] += (w / total[sl]) * p_tiles[k].astype(np.float64)       # w / total = 1.0 under one window
        return acc
    assert dtype == np.float32
    p = np.zeros((plan.H, plan.W), dtype=np.float32)
    w32, tot32 = w.astype(np.float32), total.astype(np.float32)          # exact: below 2^24
    for k, oy, ox in plan.windows():
        sl = (slice(oy, oy + plan.th), slice(ox, ox + plan.tw))
        wn = w32 / tot32[sl]
        p[sl] = (wn.astype(np.float64) * p_tiles[k].astype(np.float32).astype(np.float64) +
                 p[sl].astype(np.float64)).astype(np.float32)
    return np.minimum(p, np.float32(1.0))
