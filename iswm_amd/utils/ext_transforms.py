"""Device-side training-input pipeline -- counterpart of the transforms the reference composes in
train.py:355-362 (utils/ext_transforms.py: ExtRandomScale :94-115, ExtRandomCrop :327-396,
ExtRandomHorizontalFlip :212-233, ExtToTensor :273-296, ExtNormalize :298-324, ExtCompose :39-64).

The reference runs them per sample on PIL images inside DataLoader workers.  Here the classes keep their names
and constructor arguments but only CARRY parameters; `ExtCompose.batch(images, labels)` draws the random
parameters of every sample on the host -- with Python's `random`, in the same order the reference's chain
consumes it (uniform scale; randint i, randint j unless the sizes already match; random() < p for the flip), so a
single-process loader with the same seed produces the same augmentations -- and runs the whole batch in ONE HIP
kernel (csrc/augment.hip) from uint8 source tiles resident on the GPU.

ExtRandomRotation (:147-210), ExtRandomVerticalFlip (:236-259) and ExtColorJitter (:429-519), which the reference
defines without composing them, have a device form too: the rotation as a nearest copy of the
source tile before the scale (iswm_aug_rotate), the vertical flip and the jitter's randomly ordered brightness /
contrast / saturation / hue operations per output pixel (iswm_augment_batch_ex).  `draw` walks the transforms in composed
order, so `random` is consumed as the reference chain would consume it.  A pipeline without them takes the route, and
issues the library calls, it always did.

Bit-exactness with Pillow's resize is obtained by computing Pillow's own per-column / per-row resampling tables
here in double precision (`_resample_tables` follows Resample.c precompute_coeffs + normalize_coeffs_8bpc,
`_nearest_table` follows Geometry.c ImagingScaleAffine) and letting the kernel do only the integer arithmetic.
"""
import ctypes
import math
import numbers
import random

import numpy as np

from .. import _lib
from .._lib import call

PRECISION_BITS = 32 - 8 - 2      # Pillow Resample.c


class ExtRandomScale(object):
    def __init__(self, scale_range, interpolation="bilinear"):
        self.scale_range = scale_range
        self.interpolation = interpolation


class ExtRandomCrop(object):
    def __init__(self, size, padding=0, pad_if_needed=False):
        self.size = (int(size), int(size)) if isinstance(size, numbers.Number) else tuple(size)
        if padding:
            raise NotImplementedError("ExtRandomCrop(padding>0) is not used by train.py and not built")
        self.padding = padding
        self.pad_if_needed = pad_if_needed


class ExtRandomHorizontalFlip(object):
    def __init__(self, p=0.5):
        self.p = p


class ExtRandomVerticalFlip(object):
    def __init__(self, p=0.5):
        self.p = p


class ExtRandomRotation(object):
    """Angle range of the reference's ExtRandomRotation (:147-210): a number d means (-d, d), a pair is taken as it is.
    Only the nearest filter about the image centre without `expand` has a device form (ExtCompose checks that)."""

    def __init__(self, degrees, resample=False, expand=False, center=None):
        if isinstance(degrees, numbers.Number):
            if degrees < 0:
                raise ValueError("ExtRandomRotation: a single angle stands for (-angle, angle) and cannot be negative "
                                 "(got %r)" % (degrees,))
            degrees = (-degrees, degrees)
        elif len(degrees) != 2:
            raise ValueError("ExtRandomRotation: degrees is a number or a (min, max) pair (got %d values)" % len(degrees))
        self.degrees = degrees
        self.resample, self.expand, self.center = resample, expand, center


def _jitter_range(name, value, neutral, lowest, highest, clip):
    """[min, max] a colour-jitter factor is drawn from, or None when the range is the neutral value alone.  A number v
    means neutral -/+ v, with `clip` cut off at `lowest`; a pair is taken as given.  The reference accepts a single hue
    above 0.5 and fails in adjust_hue at the first sample drawn beyond it; here every range is held to [lowest, highest]
    when it is built."""
    if isinstance(value, numbers.Number):
        if value < 0:
            raise ValueError("ExtColorJitter: %s=%r: a single number is a half-width and cannot be negative" % (name, value))
        rng = [max(neutral - value, lowest) if clip else neutral - value, neutral + value]
    elif isinstance(value, (tuple, list)) and len(value) == 2:
        rng = value
    else:
        raise TypeError("ExtColorJitter: %s is a number or a (min, max) pair (got %r)" % (name, value))
    if not lowest <= rng[0] <= rng[1] <= highest:
        raise ValueError("ExtColorJitter: %s range %r leaves [%s, %s] or is not ordered" % (name, list(rng), lowest, highest))
    return None if rng[0] == rng[1] == neutral else rng


class ExtColorJitter(object):
    """Factor ranges of the reference's ExtColorJitter (:429-519): brightness, contrast and saturation around 1 and never
    below 0, hue around 0 within [-0.5, 0.5]; an attribute is None when its factor is off."""

    def __init__(self, brightness=0, contrast=0, saturation=0, hue=0):
        self.brightness = _jitter_range("brightness", brightness, 1, 0, float("inf"), True)
        self.contrast = _jitter_range("contrast", contrast, 1, 0, float("inf"), True)
        self.saturation = _jitter_range("saturation", saturation, 1, 0, float("inf"), True)
        self.hue = _jitter_range("hue", hue, 0, -0.5, 0.5, False)


class ExtToTensor(object):
    def __init__(self, normalize=True, target_type='uint8'):
        if not normalize or target_type != 'uint8':
            raise NotImplementedError("only ExtToTensor(normalize=True, target_type='uint8') (train.py:359) is built")
        self.normalize, self.target_type = normalize, target_type


class ExtNormalize(object):
    def __init__(self, mean, std):
        self.mean, self.std = list(mean), list(std)


# ---- Pillow's tables ---------------------------------------------------------------------------------------
def _resample_tables(in_size, out_size):
    """Pillow Resample.c precompute_coeffs (BILINEAR, box = whole axis) + normalize_coeffs_8bpc.
    Returns (bounds int32 [out,2] = (first source index, count), weights int32 [out, ksize], ksize)."""
    scale = float(in_size) / float(out_size)
    filterscale = scale if scale >= 1.0 else 1.0
    support = 1.0 * filterscale                              # bilinear support = 1
    ksize = int(math.ceil(support)) * 2 + 1
    xx = np.arange(out_size, dtype=np.float64)
    center = 0.0 + (xx + 0.5) * scale
    ss = 1.0 / filterscale
    xmin = (center - support + 0.5).astype(np.int64)          # C (int) cast: truncation
    xmin = np.maximum(xmin, 0)
    xmax = (center + support + 0.5).astype(np.int64)
    xmax = np.minimum(xmax, in_size) - xmin
    k = np.zeros((out_size, ksize), dtype=np.float64)
    ww = np.zeros(out_size, dtype=np.float64)
    for x in range(ksize):                                    # sequential accumulation, as the C loop
        arg = np.abs((float(x) + xmin - center + 0.5) * ss)
        w = np.where(arg < 1.0, 1.0 - arg, 0.0)
        w = np.where(x < xmax, w, 0.0)
        k[:, x] = w
        ww = ww + w
    nz = ww != 0.0
    k[nz] = k[nz] / ww[nz, None]
    kk = np.floor(0.5 + k * float(1 << PRECISION_BITS)).astype(np.int32)     # weights are never negative
    bounds = np.stack([xmin, xmax], axis=1).astype(np.int32)
    return bounds, kk, ksize


def _nearest_table(in_size, out_size):
    """Pillow Geometry.c ImagingScaleAffine: xo = a*0.5, then xo += a per output index; index = (int)xo."""
    a = float(in_size) / float(out_size)
    steps = np.full(out_size, a, dtype=np.float64)
    steps[0] = 0.0 + a * 0.5
    xo = np.cumsum(steps)                                     # sequential double additions
    idx = np.where(xo < 0.0, -1, xo.astype(np.int64))
    return np.clip(idx, 0, in_size - 1).astype(np.int32)       # (indices outside the source cannot occur for a resize)


# the header's records, and the same bytes as numpy records for filling a pinned buffer without a Python object per field
_AUG_SAMPLE = _lib.STRUCTS["iswm_aug_sample"]
_AUG_DTYPE, _AUG_EXTRA_DTYPE = np.dtype(_AUG_SAMPLE), np.dtype(_lib.STRUCTS["iswm_aug_extra"])

OP_BRIGHTNESS, OP_CONTRAST, OP_SATURATION, OP_HUE = (_lib.CONSTANTS["ISWM_AUG_OP_" + n] for n in
                                                     ("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE"))
ROT_MAX_SIDE = 8192     # keeps Pillow's 32-bit fixed-point walk (Geometry.c affine_fixed) clear of overflow


def _rotation_coeffs(angle, w, h):
    """Image.rotate(angle, NEAREST, expand=False, center=None) of a w x h image as the six 16.16 fixed-point integers
    Geometry.c affine_fixed walks, or None when Pillow returns a copy.  Output pixel (x, y) reads source
    ((a2 + y*a1 + x*a0) >> 16, (a5 + y*a4 + x*a3) >> 16).  Pillow's exact transposes have whole-pixel coefficients."""
    angle = angle % 360.0
    one = 65536
    if angle == 0:
        return None
    if angle == 180:                                           # ROTATE_180: out[y][x] = in[h-1-y][w-1-x]
        return (-one, 0, (w - 1) * one, 0, -one, (h - 1) * one)
    if angle == 90 and w == h:                                 # ROTATE_90: out[y][x] = in[x][w-1-y]
        return (0, -one, (w - 1) * one, one, 0, 0)
    if angle == 270 and w == h:                                # ROTATE_270: out[y][x] = in[h-1-x][y]
        return (0, one, 0, -one, 0, (h - 1) * one)
    t = -math.radians(angle)
    m = [round(math.cos(t), 15), round(math.sin(t), 15), 0.0, round(-math.sin(t), 15), round(math.cos(t), 15), 0.0]
    cx, cy = w / 2.0, h / 2.0
    x, y = -cx, -cy
    m[2], m[5] = m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy

    def fix(v):
        v = v * 65536.0
        return int(v + 0.5) if v >= 0 else int(v - 0.5)
    return (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]),
            fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _hue_shift(hue_factor):
    """what `np_h += np.uint8(hue_factor * 255)` adds to the uint8 H channel: truncated toward zero, modulo 256"""
    return int(hue_factor * 255) % 256


def _align16(n):
    return (n + 15) // 16 * 16


def _fill_extra(e, p, sh, sw, rot_img_off, rot_lbl_off):
    """one iswm_aug_extra from extended parameters p (or a 6-tuple: neutral); returns (rotated, has a contrast op)"""
    e["rot_mode"] = 0
    e["n_ops"] = 0
    if len(p) == 6:
        return False, False
    angle, ops, factors = p[6], p[8], p[9]
    coeffs = None if angle is None else _rotation_coeffs(angle, sw, sh)
    if coeffs is not None:
        if max(sh, sw) > ROT_MAX_SIDE:
            raise ValueError("rotation of a %dx%d tile: sides above %d are not built" % (sh, sw, ROT_MAX_SIDE))
        a0, a1, a2, a3, a4, a5 = coeffs
        e["rot_mode"], e["a"] = 1, (a0, a1, a2, a3, a4, a5)
        e["rot_img_off"], e["rot_lbl_off"] = rot_img_off, rot_lbl_off
    if len(ops) > 4 or len(set(ops)) != len(ops) or any(o not in (0, 1, 2, 3) for o in ops):
        raise ValueError("op list %r: at most one each of brightness 0, contrast 1, saturation 2, hue 3" % (ops,))
    missing = [o for o in ops if factors[o] is None]
    if missing:
        raise ValueError("op list %r names op %d, whose factor is None in %r" % (ops, missing[0], factors))
    e["n_ops"] = len(ops)
    e["ops"] = tuple(ops) + (0,) * (4 - len(ops))
    e["factor"] = tuple(0.0 if (f is None or i == OP_HUE) else f for i, f in enumerate(factors))
    e["hue_shift"] = _hue_shift(factors[OP_HUE]) if OP_HUE in ops else 0
    return coeffs is not None, OP_CONTRAST in ops


def _ksize(in_size, out_size):
    """taps per output index, as _resample_tables computes them (one division and one ceil: stays on the host)"""
    scale = float(in_size) / float(out_size)
    support = 1.0 * (scale if scale >= 1.0 else 1.0)
    return int(math.ceil(support)) * 2 + 1


class ExtCompose(object):
    """Same constructor as the reference (a list of the Ext* transforms above).  `batch()` is the device path;
    `batch_resident()` is the same path fed from a DeviceTileStore, with the tables computed on the device.
    `ring_depth`: pinned parameter buffers `batch_resident` rotates through (how many batches the host may run ahead
    of the device before it waits for the oldest parameter copy)."""

    def __init__(self, transforms, ring_depth=4):
        self.transforms = transforms
        if int(ring_depth) < 1:
            raise ValueError("ring_depth must be at least 1 (got %r)" % (ring_depth,))
        self.ring_depth = int(ring_depth)
        self._ring = [[None, None] for _ in range(self.ring_depth)]     # [pinned uint8 buffer, event behind its last copy]
        self._ring_pos = 0
        self.scale = self.crop = self.hflip = self.norm = self.rotation = self.vflip = self.jitter = None
        for t in transforms:
            if isinstance(t, ExtRandomScale):
                self.scale = t
            elif isinstance(t, ExtRandomCrop):
                self.crop = t
            elif isinstance(t, ExtRandomHorizontalFlip):
                self.hflip = t
            elif isinstance(t, ExtNormalize):
                self.norm = t
            elif isinstance(t, ExtRandomRotation):
                if t.resample not in (False, None, 0):             # 0 == PIL.Image.NEAREST
                    raise NotImplementedError("ExtRandomRotation: only the NEAREST filter is built (resample=%r): the "
                                              "reference hands the same filter to the label" % (t.resample,))
                if t.expand or t.center is not None:
                    raise NotImplementedError("ExtRandomRotation: expand=True and a rotation centre are not built")
                if self.scale is not None or self.crop is not None or self.rotation is not None:
                    raise NotImplementedError("ExtRandomRotation must stand once, before ExtRandomScale and "
                                              "ExtRandomCrop: it acts on the source tile")
                self.rotation = t
            elif isinstance(t, (ExtRandomVerticalFlip, ExtColorJitter)):
                if self.crop is None:
                    raise NotImplementedError("%s must stand after ExtRandomCrop" % type(t).__name__)
                if (self.vflip if isinstance(t, ExtRandomVerticalFlip) else self.jitter) is not None:
                    raise NotImplementedError("%s must stand once: two of them are two transforms in the reference, "
                                              "and the device pipeline applies one" % type(t).__name__)
                if isinstance(t, ExtRandomVerticalFlip):
                    self.vflip = t
                else:
                    self.jitter = t
            elif not isinstance(t, ExtToTensor):
                raise NotImplementedError("transform %s has no device implementation" % type(t).__name__)
        self.extended = not (self.rotation is None and self.vflip is None and self.jitter is None)
        if self.crop is None:
            raise NotImplementedError("the device pipeline needs an ExtRandomCrop (fixed output size per batch)")
        if self.norm is None:
            self.norm = ExtNormalize([0.0, 0.0, 0.0], [1.0, 1.0, 1.0])

    # ---- random parameters, consumed in the reference's order -------------------------------------------------
    def draw(self, src_h, src_w):
        """(rs_h, rs_w, pad, crop_i, crop_j, flip) of one sample; with a rotation, vertical flip or colour jitter
        composed: (..., flip, angle or None, vflip, ops, factors) -- ops = the jitter's op codes in the order they
        are applied, factors = (brightness, contrast, saturation, hue), None where a factor is off"""
        if self.extended:
            return self._draw_extended(src_h, src_w)
        return self._draw_geometry(src_h, src_w)

    def _draw_extended(self, src_h, src_w):
        """walks the transforms in composed order, as the reference chain consumes `random`"""
        angle, geom, flip, vflip, ops, factors = None, None, 0, 0, (), (None, None, None, None)
        for t in self.transforms:
            if isinstance(t, ExtRandomRotation):
                angle = random.uniform(t.degrees[0], t.degrees[1])                       # :186
            elif isinstance(t, ExtRandomCrop):
                geom = self._draw_geometry(src_h, src_w, with_flip=False)                # scale (if any) and crop
            elif isinstance(t, ExtRandomHorizontalFlip):
                flip = 1 if random.random() < t.p else 0                                 # :228
            elif isinstance(t, ExtRandomVerticalFlip):
                vflip = 1 if random.random() < t.p else 0                                # :254
            elif isinstance(t, ExtColorJitter):                                          # get_params :472-500
                ranges = (t.brightness, t.contrast, t.saturation, t.hue)
                factors = tuple(None if r is None else random.uniform(r[0], r[1]) for r in ranges)
                order = [op for op, r in enumerate(ranges) if r is not None]
                random.shuffle(order)
                ops = tuple(order)
        return geom + (flip, angle, vflip, ops, factors)

    def _draw_geometry(self, src_h, src_w, with_flip=True):
        rs_h, rs_w = src_h, src_w
        if self.scale is not None:
            s = random.uniform(self.scale.scale_range[0], self.scale.scale_range[1])      # :109
            rs_h, rs_w = int(src_h * s), int(src_w * s)                                   # :110
            if rs_h < 1 or rs_w < 1:
                raise ValueError("rescaled size %dx%d is empty" % (rs_h, rs_w))
        th, tw = self.crop.size
        h, w, pad = rs_h, rs_w, 0
        if self.crop.pad_if_needed and w < tw:                 # :380-382 pads ALL four sides
            p = int((1 + tw - w) / 2)
            pad, h, w = pad + p, h + 2 * p, w + 2 * p
        if self.crop.pad_if_needed and h < th:                 # :385-387
            p = int((1 + th - h) / 2)
            pad, h, w = pad + p, h + 2 * p, w + 2 * p
        if h < th or w < tw:
            raise ValueError("image %dx%d smaller than the crop %dx%d (pad_if_needed=False)" % (h, w, th, tw))
        if w == tw and h == th:                                # get_params :352-360
            i, j = 0, 0
        else:
            i = random.randint(0, h - th)
            j = random.randint(0, w - tw)
        if not with_flip:
            return rs_h, rs_w, pad, i, j
        flip = 0
        if self.hflip is not None:
            flip = 1 if random.random() < self.hflip.p else 0   # :228
        return rs_h, rs_w, pad, i, j, flip

    # ---- one launch for the whole batch -------------------------------------------------------------------
    def batch(self, images, labels, params=None):
        """images: list of uint8 [H,W,3] CUDA tensors; labels: list of uint8 [H,W] CUDA tensors (sizes may differ per
        sample).  Returns (float32 [B,3,th,tw], uint8 [B,th,tw]) on the same device.  `params` overrides the random
        draw with explicit (rs_h, rs_w, pad, crop_i, crop_j, flip) tuples (tests)."""
        if len(images) != len(labels) or not images:
            raise ValueError("need equally many images and labels (got %d, %d)" % (len(images), len(labels)))
        import torch
        dev = images[0].device
        th, tw = self.crop.size
        B = len(images)
        samples = (_AUG_SAMPLE * B)()
        extras = np.zeros(B, dtype=_AUG_EXTRA_DTYPE) if self.extended else None
        rot_img, rot_lbl, any_contrast = 0, 0, False
        tabs, tab_off, img_off, lbl_off = [], 0, 0, 0
        for b, (im, lb) in enumerate(zip(images, labels)):
            if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3 or not im.is_cuda:
                raise ValueError("image %d: expected a uint8 [H,W,3] CUDA tensor, got %s %s" % (b, tuple(im.shape), im.dtype))
            if lb.dtype != torch.uint8 or tuple(lb.shape) != tuple(im.shape[:2]) or not lb.is_cuda:
                raise ValueError("label %d: expected a uint8 %s CUDA tensor, got %s %s" % (b, tuple(im.shape[:2]), tuple(lb.shape), lb.dtype))
            sh, sw = int(im.shape[0]), int(im.shape[1])
            p = params[b] if params is not None else self.draw(sh, sw)
            rs_h, rs_w, pad, ci, cj, flip = p[:6]
            if self.extended:
                rotated, contrast = _fill_extra(extras[b], p, sh, sw, rot_img, rot_lbl)
                flip |= 2 if len(p) > 6 and p[7] else 0
                any_contrast |= contrast
                if rotated:
                    rot_img, rot_lbl = rot_img + _align16(sh * sw * 3), rot_lbl + _align16(sh * sw)
            elif len(p) != 6:
                raise ValueError("extended parameters need a rotation, vertical flip or colour jitter in the pipeline")
            hb, hk, ksh = _resample_tables(sw, rs_w)
            vb, vk, ksv = _resample_tables(sh, rs_h)
            t = np.concatenate([_nearest_table(sw, rs_w), _nearest_table(sh, rs_h), hb.reshape(-1), hk.reshape(-1),
                                vb.reshape(-1), vk.reshape(-1)])
            s = samples[b]
            s.img_off, s.lbl_off = img_off, lbl_off
            s.src_h, s.src_w, s.rs_h, s.rs_w = sh, sw, rs_h, rs_w
            s.pad, s.crop_i, s.crop_j, s.flip = pad, ci, cj, flip
            s.tab_off, s.ksize_h, s.ksize_v = tab_off, ksh, ksv
            tabs.append(t)
            tab_off += t.size
            img_off += sh * sw * 3
            lbl_off += sh * sw
        img_buf = torch.cat([im.reshape(-1) for im in images])
        lbl_buf = torch.cat([lb.reshape(-1) for lb in labels])
        tables = torch.from_numpy(np.concatenate(tabs).astype(np.int32)).to(dev)
        sbuf = torch.frombuffer(bytearray(bytes(samples)), dtype=torch.uint8).to(dev)
        out = torch.empty((B, 3, th, tw), dtype=torch.float32, device=dev)
        out_lbl = torch.empty((B, th, tw), dtype=torch.uint8, device=dev)
        mean = (ctypes.c_float * 3)(*[float(np.float32(m)) for m in self.norm.mean])
        std = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in self.norm.std])
        _lib.load()
        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
        if self.extended:
            ebuf = torch.from_numpy(extras.view(np.uint8)).to(dev)
            self._launch_extended(img_buf, lbl_buf, sbuf.data_ptr(), ebuf.data_ptr(), tables, B, rot_img, rot_lbl,
                                  max(int(im.shape[0]) * int(im.shape[1]) for im in images), any_contrast, mean, std, out,
                                  out_lbl, stream)
            return out, out_lbl
        call("iswm_augment_batch", img_buf.data_ptr(), lbl_buf.data_ptr(), sbuf.data_ptr(), tables.data_ptr(), B, th, tw,
             mean, std, out.data_ptr(), out_lbl.data_ptr(), stream)
        return out, out_lbl

    def _launch_extended(self, img_arena, lbl_arena, samples_ptr, extras_ptr, tables, B, rot_img, rot_lbl, max_hw,
                         any_contrast, mean, std, out, out_lbl, stream):
        """iswm_aug_rotate into scratch arenas of rot_img / rot_lbl bytes (skipped when no sample rotates), then
        iswm_augment_batch_ex; every buffer comes from torch's caching allocator on the current stream"""
        import torch
        th, tw = self.crop.size
        dev = out.device
        rimg = rlbl = None
        if rot_img:
            rimg = torch.empty(rot_img, dtype=torch.uint8, device=dev)
            rlbl = torch.empty(rot_lbl, dtype=torch.uint8, device=dev)
            call("iswm_aug_rotate", img_arena.data_ptr(), lbl_arena.data_ptr(), samples_ptr, extras_ptr, B, max_hw,
                 rimg.data_ptr(), rot_img, rlbl.data_ptr(), rot_lbl, stream)
        ws_bytes = _lib.load().iswm_augment_batch_ex_workspace(B, th, tw)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        call("iswm_augment_batch_ex", img_arena.data_ptr(), lbl_arena.data_ptr(),
             rimg.data_ptr() if rimg is not None else None, rlbl.data_ptr() if rlbl is not None else None, samples_ptr,
             extras_ptr, tables.data_ptr(), B, th, tw, mean, std, 1 if any_contrast else 0, out.data_ptr(),
             out_lbl.data_ptr(), ws.data_ptr(), ws_bytes, stream)

    def batch_resident(self, store, indices, params=None):
        """`batch()` over tiles `indices` of a datasets.DeviceTileStore, without the host touching a table or a pixel:
        the parameters are drawn in index order (the `random` stream is consumed exactly as `batch` consumes it), the
        64-byte records go up from a ring of pinned buffers with a non-blocking copy, iswm_aug_tables fills Pillow's
        tables on the device and iswm_augment_batch reads the store's arenas in place.  Nothing here waits for the
        device, except that a pinned buffer is rewritten only after the event behind its previous copy has completed:
        a caller more than `ring_depth` batches ahead waits there for the oldest copy.  Same results as `batch`, bit
        for bit."""
        B = len(indices)
        if B < 1:
            raise ValueError("need at least one tile index")
        import torch
        th, tw = self.crop.size
        rec = np.zeros(B, dtype=_AUG_DTYPE)
        extras = np.zeros(B, dtype=_AUG_EXTRA_DTYPE) if self.extended else None
        rot_img, rot_lbl, max_hw, any_contrast = 0, 0, 0, False
        tab_off = max_rs = 0
        for b, i in enumerate(indices):
            img_off, lbl_off, sh, sw = store.meta[int(i)]
            p = params[b] if params is not None else self.draw(sh, sw)
            rs_h, rs_w, pad, ci, cj, flip = p[:6]
            if self.extended:
                rotated, contrast = _fill_extra(extras[b], p, sh, sw, rot_img, rot_lbl)
                flip |= 2 if len(p) > 6 and p[7] else 0
                any_contrast |= contrast
                max_hw = max(max_hw, sh * sw)
                if rotated:
                    rot_img, rot_lbl = rot_img + _align16(sh * sw * 3), rot_lbl + _align16(sh * sw)
            elif len(p) != 6:
                raise ValueError("extended parameters need a rotation, vertical flip or colour jitter in the pipeline")
            ksh, ksv = _ksize(sw, rs_w), _ksize(sh, rs_h)
            rec[b] = (img_off, lbl_off, sh, sw, rs_h, rs_w, pad, ci, cj, flip, tab_off, ksh, ksv, 0)
            tab_off += rs_w * (3 + ksh) + rs_h * (3 + ksv)
            max_rs = max(max_rs, rs_h, rs_w)
        if tab_off >= 2 ** 31:
            raise ValueError("the batch's tables need %d ints (tab_off is an int32)" % tab_off)
        rec_bytes = B * _AUG_DTYPE.itemsize
        nbytes = rec_bytes + (B * _AUG_EXTRA_DTYPE.itemsize if self.extended else 0)   # the extra records ride behind
        slot = self._ring[self._ring_pos % self.ring_depth]
        self._ring_pos += 1
        if slot[1] is not None:
            slot[1].synchronize()                          # the copy that last read this buffer (back-pressure)
        if slot[0] is None or slot[0].numel() < nbytes:
            slot[0] = torch.empty(max(nbytes, 4096), dtype=torch.uint8, pin_memory=True)
        slot[0].numpy()[:rec_bytes] = rec.view(np.uint8)
        if self.extended:
            slot[0].numpy()[rec_bytes:nbytes] = extras.view(np.uint8)
        dev = store.device
        _lib.load()
        with torch.cuda.device(dev):
            sbuf = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            sbuf.copy_(slot[0][:nbytes], non_blocking=True)
            if slot[1] is None:
                slot[1] = torch.cuda.Event()
            slot[1].record()
            tables = torch.empty(tab_off, dtype=torch.int32, device=dev)
            out = torch.empty((B, 3, th, tw), dtype=torch.float32, device=dev)
            out_lbl = torch.empty((B, th, tw), dtype=torch.uint8, device=dev)
            mean = (ctypes.c_float * 3)(*[float(np.float32(m)) for m in self.norm.mean])
            std = (ctypes.c_float * 3)(*[float(np.float32(v)) for v in self.norm.std])
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            call("iswm_aug_tables", sbuf.data_ptr(), B, max_rs, tables.data_ptr(), tab_off * 4, stream)
            if self.extended:
                self._launch_extended(store.img_arena, store.lbl_arena, sbuf.data_ptr(), sbuf.data_ptr() + rec_bytes,
                                      tables, B, rot_img, rot_lbl, max_hw, any_contrast, mean, std, out, out_lbl, stream)
                return out, out_lbl
            call("iswm_augment_batch", store.img_arena.data_ptr(), store.lbl_arena.data_ptr(), sbuf.data_ptr(),
                 tables.data_ptr(), B, th, tw, mean, std, out.data_ptr(), out_lbl.data_ptr(), stream)
        return out, out_lbl

    def __call__(self, img, lbl):
        """single-sample form of the reference's ExtCompose.__call__: (float32 [3,th,tw], uint8 [th,tw])"""
        out, out_lbl = self.batch([img], [lbl])
        return out[0], out_lbl[0]
