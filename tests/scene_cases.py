"""Inputs and bounds shared by tests/test_scene_cpu.py and tests/test_scene_gpu.py: the logits generator of
test_predict_maps_against_restatement, the scenes, class layouts and cuts, and the derived error bound of the
blended probability."""
import numpy as np
import torch

# |p - p64|: the pinned per-window bound of predict_maps (1e-6) plus one rounding per wn_t and one per fma over at
# most 9 windows, each at most 2^-24 of a value <= 1
BOUND = 1e-6 + 18 * 2.0 ** -24

# (C, fg, pitch): 1, 2, 2 float4 groups in registers and the two-pass path
CLASSES = [(2, 1, 4), (3, 2, 8), (5, 4, 8), (17, 16, 20)]
# (H, W, tile, overlap, low-res side): ragged last windows in both axes; overlap = half a window (3 x 3 windows cover
# a pixel); no overlap (ramp 1) with a pulled-back last window; a low-res grid that is no divisor of the window
SCENES = [(37, 53, 16, 4, 5), (40, 40, 16, 8, 4), (33, 48, 16, 0, 5), (97, 129, 65, 16, 17)]
CUTS = [(0.5, 0.2, 0.7), (0.2, 0.0, 1.0)]


def logits(n, h, w, c, ld, seed):
    """low-res NHWC logits with saturated pixels (+-30) and exact ties between the foreground and another class"""
    g = torch.Generator().manual_seed(seed)
    yl = torch.randn((n, h, w, ld), generator=g) * 3.0
    sat = torch.rand((n, h, w), generator=g) < 0.1
    yl[..., 0][sat] = 30.0
    yl[..., 1][sat] = -30.0
    flip = torch.rand((n, h, w), generator=g) < 0.05
    yl[..., 0][flip] = -30.0
    yl[..., 1][flip] = 30.0
    tie = torch.rand((n, h, w), generator=g) < 0.1
    yl[..., c - 1][tie] = yl[..., 0][tie]
    yl[..., 1][tie] = yl[..., 0][tie]
    return yl


def scene_logits(ntiles, side, c, fg, ld):
    return logits(ntiles, side, side, c, ld, seed=side * 31 + c * 7 + fg + ntiles)


def _taps(insz, outsz):
    """bilinear.h's src_index: fp32 scale, source coordinate and weights"""
    scale = np.float32(insz) / np.float32(outsz)
    src = scale * (np.arange(outsz, dtype=np.float32) + np.float32(0.5)) - np.float32(0.5)
    src = np.maximum(src, np.float32(0)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), insz - 1)
    i1 = i0 + (i0 < insz - 1)
    l1 = (src - i0.astype(np.float32)).astype(np.float32)
    return i0, i1, (np.float32(1) - l1).astype(np.float64), l1.astype(np.float64)


def upsample64(yl, c, H, W):
    """[n, h, w, ld] NHWC -> fp64 NCHW [n, c, H, W]: bilinear, align_corners=False, the kernel's taps, fp64 sums"""
    y = np.asarray(yl, dtype=np.float64)[..., :c]
    a0, a1, la0, la1 = _taps(y.shape[1], H)
    b0, b1, lb0, lb1 = _taps(y.shape[2], W)
    top = y[:, a0][:, :, b0] * lb0[None, None, :, None] + y[:, a0][:, :, b1] * lb1[None, None, :, None]
    bot = y[:, a1][:, :, b0] * lb0[None, None, :, None] + y[:, a1][:, :, b1] * lb1[None, None, :, None]
    out = top * la0[None, :, None, None] + bot * la1[None, :, None, None]
    return out.transpose(0, 3, 1, 2)
