"""CPU restatement of flip and multi-scale test-time augmentation -- the parity pin of ops.tta_views,
k_predict_view_normalize, k_predict_views_maps and iswm_amd.predict.TTAPredictor, and the inputs
and bounds shared by tests/test_tta_cpu.py and tests/test_tta_gpu.py.  numpy only; the maps that follow the averaged
probability are tests/predict_ref.py's, unchanged.

The probability of a frame is the mean over views of it.  A view is the frame resampled to Hv x Wv (bilinear,
align_corners=False) and, when flipped, mirrored left to right; the network's low-resolution logits of a view are
sampled at the frame's pixels in one bilinear step and a flipped view is read at the mirrored column.
"""
import numpy as np

from tests import predict_ref as R
from tests import scene_cases as SC

MAX_VIEWS = 16
MAX_SCALES = 8
SCALE_RANGE = (0.25, 4.0)


def views(H, W, scales, flip):
    """the ordered views (Hv, Wv, flip): per scale in the order given the unflipped view, then with `flip` the
    flipped one; Hv = max(1, int(H * s + 0.5)) in Python floats.  ValueError for what ops.tta_views refuses."""
    scales = list(scales)
    if H < 1 or W < 1:
        raise ValueError("bad frame size %r x %r" % (H, W))
    if not 1 <= len(scales) <= MAX_SCALES:
        raise ValueError("%d scales" % len(scales))
    out = []
    for i, s in enumerate(scales):
        s = float(s)
        if not SCALE_RANGE[0] <= s <= SCALE_RANGE[1]:
            raise ValueError("scale %r outside the range" % s)
        if s in [float(t) for t in scales[:i]]:
            raise ValueError("scale %r twice" % s)
        hv, wv = max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))
        out.append((hv, wv, False))
        if flip:
            out.append((hv, wv, True))
    if len(out) > MAX_VIEWS:
        raise ValueError("%d views" % len(out))
    return out


def view_normalize64(img_u8, Hv, Wv, flip):
    """uint8 [N, H, W, 3] -> fp64 [N, 3, Hv, Wv]: the taps and weights of bilinear.h's src_index in fp32
    (scene_cases._taps), the bilinear value and (v / 255 - mean) / std in fp64 on the float32 constants the kernel is
    given, then the mirror"""
    img = np.asarray(img_u8)
    assert img.ndim == 4 and img.shape[3] == 3 and img.dtype == np.uint8
    x = img.astype(np.float64)
    a0, a1, la0, la1 = SC._taps(img.shape[1], Hv)
    b0, b1, lb0, lb1 = SC._taps(img.shape[2], Wv)
    lb0, lb1 = lb0[None, None, :, None], lb1[None, None, :, None]
    top = x[:, a0][:, :, b0] * lb0 + x[:, a0][:, :, b1] * lb1
    bot = x[:, a1][:, :, b0] * lb0 + x[:, a1][:, :, b1] * lb1
    v = top * la0[None, :, None, None] + bot * la1[None, :, None, None]
    m = np.asarray(R.MEAN, dtype=np.float32).astype(np.float64)
    s = np.asarray(R.STD, dtype=np.float32).astype(np.float64)
    out = ((v / 255.0 - m) / s).transpose(0, 3, 1, 2)
    return (out[..., ::-1] if flip else out).copy()


def combine(p_views, dtype):
    """per-view foreground probabilities at the frame's pixels [V, ...] (flipped views already mirrored back) -> p.
    float64: the definition, the mean.  float32: the kernel's order -- acc = 0, acc += p_v in list order, each sum
    rounded to float32, then one float32 division by V."""
    p_views = np.asarray(p_views)
    V = p_views.shape[0]
    assert 1 <= V <= MAX_VIEWS
    if dtype == np.float64:
        return p_views.astype(np.float64).mean(axis=0)
    assert dtype == np.float32
    acc = np.zeros(p_views.shape[1:], dtype=np.float32)
    for v in range(V):
        acc = (acc + p_views[v].astype(np.float32)).astype(np.float32)
    return (acc / np.float32(V)).astype(np.float32)


def unflip(p, flip):
    """a view's probability map at the frame's size [..., H, W] as the gather reads it"""
    return p[..., ::-1] if flip else p


# ---- the cases of the views_maps tests ----------------------------------------------------------------------------
# W no multiple of 16: 16-pixel chunks straddle the boundary between the two images
FRAMES = [(37, 53), (33, 48), (65, 65)]
EIGHT = (0.5, 0.625, 0.75, 0.875, 1.0, 1.25, 1.5, 2.0)
VIEW_SETS = [((1.0,), True), ((0.5, 1.0, 1.5), True), ((0.75, 1.0, 1.25), False), (EIGHT, True)]
N = 2


def bound(V):
    """|p - p64| of V views: the pinned per-view bound of predict_maps (1e-6; a mean of V values within 1e-6 is within
    1e-6), half an ulp per add of a partial sum <= k (at most 2^-24 * k; summed over k = 1..V and divided by V:
    (V + 1) / 2 * 2^-24), and the rounding of the division (at most 2^-24 on a value <= 1)"""
    return 1e-6 + ((V + 1) / 2.0 + 1.0) * 2.0 ** -24


def view_logits(H, W, scales, flip, c, fg, ld):
    """[(yl [N, ceil(Hv / 4), ceil(Wv / 4), ld] torch fp32, flip)] per view of the frame, scene_cases.logits"""
    out = []
    for v, (hv, wv, f) in enumerate(views(H, W, scales, flip)):
        hl, wl = -(-hv // 4), -(-wv // 4)
        out.append((SC.logits(N, hl, wl, c, ld, seed=hl * 31 + wl * 17 + c * 7 + fg + 101 * v), f))
    return out
