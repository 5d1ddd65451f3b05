"""TEST INFRASTRUCTURE ONLY -- numpy restatement of the arithmetic behind the device forms of ExtRandomRotation,
ExtRandomVerticalFlip and ExtColorJitter: Pillow's Image.rotate (nearest), convert('L'),
Image.blend as ImageEnhance calls it, and the RGB <-> HSV conversions of Convert.c.  tests/test_augment_ext_cpu.py proves
every function here against Pillow itself; tests/test_augment_ext_gpu.py compares the kernels with `chain`, which takes
resize, pad, crop and horizontal flip from oracle/augment.py.  Never imported by the product."""
import math

import numpy as np
import torch

from oracle import augment as oaug

BRIGHTNESS, CONTRAST, SATURATION, HUE = 0, 1, 2, 3


# ---- rotation ---------------------------------------------------------------------------------------------------
def _fix(v):
    v = v * 65536.0
    return int(v + 0.5) if v >= 0 else int(v - 0.5)


def rotation_coeffs(angle, w, h):
    """the six 16.16 integers of Geometry.c affine_fixed for Image.rotate(angle) of a w x h image (general case)"""
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    m[2], m[5] = m[0] * -cx + m[1] * -cy + m[2], m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]),
            _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate_nearest(arr, angle):
    """Image.rotate(angle, NEAREST, expand=False, center=None) of a uint8 [H,W] or [H,W,C] array"""
    h, w = arr.shape[:2]
    angle = angle % 360.0
    if angle == 0:
        return arr.copy()
    if angle == 180:
        return arr[::-1, ::-1].copy()
    if angle in (90, 270) and w == h:
        return np.rot90(arr, 1 if angle == 90 else 3).copy()
    a0, a1, a2, a3, a4, a5 = rotation_coeffs(angle, w, h)
    y, x = np.mgrid[0:h, 0:w].astype(np.int64)
    xin = (a2 + y * a1 + x * a0) >> 16                         # numpy's >> on int64 is arithmetic
    yin = (a5 + y * a4 + x * a3) >> 16
    inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    out = np.zeros_like(arr)
    out[inside] = arr[yin[inside], xin[inside]]
    return out


# ---- grey, blends -------------------------------------------------------------------------------------------------
def gray(rgb):
    """convert('L') of uint8 [..., 3] -> uint8 [...]"""
    v = rgb.astype(np.int64)
    return ((v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16).astype(np.uint8)


def blend(degenerate, image, factor):
    """Image.blend(degenerate, image, factor): uint8 arrays (broadcastable), fp32 arithmetic"""
    f = np.float32(factor)
    d = np.broadcast_to(degenerate, image.shape)
    if f == 0:
        return d.astype(np.uint8).copy()
    if f == 1:
        return image.copy()
    t = d.astype(np.float32) + f * (image.astype(np.float32) - d.astype(np.float32))     # every operand is fp32
    assert t.dtype == np.float32
    if 0 <= f <= 1:
        return t.astype(np.int32).astype(np.uint8)
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.clip(t, 0, 255).astype(np.int32)))
    return out.astype(np.uint8)


def brightness(img, factor):
    return blend(np.zeros_like(img), img, factor)


def saturation(img, factor):
    return blend(gray(img)[..., None], img, factor)


def contrast_mean(img):
    l = gray(img)
    return int(float(int(l.astype(np.int64).sum())) / float(l.size) + 0.5)


def contrast(img, factor):
    return blend(np.full_like(img, contrast_mean(img)), img, factor)


# ---- HSV ------------------------------------------------------------------------------------------------------------
def rgb_to_hsv(rgb):
    """convert('HSV') of uint8 [..., 3] (Convert.c rgb2hsv_row: fp32 quotients, the hue term and fmod in fp64)"""
    r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
    maxc, minc = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    grey = maxc == minc
    f32 = np.float32
    cr = np.where(grey, 1, maxc - minc).astype(f32)
    mx = np.where(grey, 1, maxc).astype(f32)
    s = cr / mx
    rc, gc, bc = (maxc - r).astype(f32) / cr, (maxc - g).astype(f32) / cr, (maxc - b).astype(f32) / cr
    assert s.dtype == f32 and rc.dtype == f32
    d = np.float64
    h = np.where(r == maxc, bc.astype(d) - gc.astype(d),
                 np.where(g == maxc, 2.0 + rc.astype(d) - bc.astype(d), 4.0 + gc.astype(d) - rc.astype(d))).astype(f32)
    h = np.fmod(h.astype(d) / 6.0 + 1.0, 1.0).astype(f32)
    uh = np.clip((h.astype(d) * 255.0).astype(np.int64), 0, 255)
    us = np.clip((s.astype(d) * 255.0).astype(np.int64), 0, 255)
    out = np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), maxc], axis=-1)
    return out.astype(np.uint8)


def _round_half_up(x):
    fl = np.floor(x)
    return (fl + (x - fl >= 0.5)).astype(np.int64)


def hsv_to_rgb(hsv):
    """convert('RGB') of a uint8 [..., 3] HSV array (Convert.c hsv2rgb: fp64 with f and fs stored as fp32)"""
    f32, d = np.float32, np.float64
    h, s, v = (hsv[..., k].astype(np.int64) for k in range(3))
    hh = h.astype(d) * 6.0 / 255.0
    i = np.floor(hh).astype(np.int64)
    f = (hh - i.astype(d)).astype(f32).astype(d)
    fs = (s.astype(d) / 255.0).astype(f32).astype(d)
    vd = v.astype(d)
    p = np.clip(_round_half_up(vd * (1.0 - fs)), 0, 255)
    q = np.clip(_round_half_up(vd * (1.0 - fs * f)), 0, 255)
    t = np.clip(_round_half_up(vd * (1.0 - fs * (1.0 - f))), 0, 255)
    sel = i % 6
    r = np.choose(sel, [v, q, p, p, t, v])
    g = np.choose(sel, [t, v, v, q, p, p])
    b = np.choose(sel, [p, p, t, v, v, q])
    grey = s == 0
    out = np.stack([np.where(grey, v, r), np.where(grey, v, g), np.where(grey, v, b)], axis=-1)
    return out.astype(np.uint8)


def hue_shift(hue_factor):
    """what `np_h += np.uint8(hue_factor * 255)` adds: truncated toward zero, modulo 256"""
    return int(hue_factor * 255) % 256


def hue(img, hue_factor):
    hsv = rgb_to_hsv(img).astype(np.int64)
    hsv[..., 0] = (hsv[..., 0] + hue_shift(hue_factor)) % 256
    return hsv_to_rgb(hsv.astype(np.uint8))


# ---- the whole chain --------------------------------------------------------------------------------------------
def crop_u8(img_u8, lbl_u8, params, crop):
    """uint8 [th,tw,3] image and [th,tw] label after resize, pad, crop and horizontal flip (oracle/augment.py's PIL
    calls, read back before ToTensor: mean 0 / std 1 / 255 makes its output v / 255 exactly invertible)"""
    t, lab = oaug.augment_sample(img_u8, lbl_u8, tuple(params[:6]), crop, [0.0, 0.0, 0.0], [1.0, 1.0, 1.0])
    u8 = torch.round(t * 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    assert torch.equal(torch.from_numpy(u8).permute(2, 0, 1).to(torch.float32).div(255), t)
    return u8, lab.numpy()


def chain(img, lbl, params, crop, mean, std):
    """img uint8 [H,W,3], lbl uint8 [H,W]; params (rs_h, rs_w, pad, crop_i, crop_j, flip[, angle, vflip, ops, factors])
    -> (float32 [3,th,tw] tensor, uint8 [th,tw] tensor), the reference chain rotation -> scale -> crop -> flips ->
    jitter -> ToTensor -> Normalize"""
    angle, vflip, ops, factors = (None, 0, (), (None,) * 4) if len(params) == 6 else params[6:10]
    if angle is not None:
        img, lbl = rotate_nearest(img, angle), rotate_nearest(lbl, angle)
    u8, lab = crop_u8(np.ascontiguousarray(img), np.ascontiguousarray(lbl), params, crop)
    if vflip:
        u8, lab = u8[::-1].copy(), lab[::-1].copy()
    for op in ops:
        if op == BRIGHTNESS:
            u8 = brightness(u8, factors[BRIGHTNESS])
        elif op == CONTRAST:
            u8 = contrast(u8, factors[CONTRAST])
        elif op == SATURATION:
            u8 = saturation(u8, factors[SATURATION])
        elif op == HUE:
            u8 = hue(u8, factors[HUE])
        else:
            raise ValueError("op %r" % (op,))
    t = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    m = torch.as_tensor(mean, dtype=torch.float32)[:, None, None]
    s = torch.as_tensor(std, dtype=torch.float32)[:, None, None]
    t.sub_(m).div_(s)
    return t, torch.from_numpy(lab.copy())
