"""Rotation, vertical flip and colour jitter of the device input pipeline, without a GPU: the
numpy restatement tests/augment_ext_ref.py against Pillow itself, the order random numbers are consumed in against a
literal replay of the reference's calls, the composition rules, and that a pipeline without the new transforms issues
the library calls it always issued."""
import itertools
import os
import random
import re

import numpy as np
import pytest
from PIL import Image, ImageEnhance

from tests import augment_ext_ref as R

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILES = [(1, 1), (2, 3), (7, 5), (37, 53), (64, 64), (97, 129)]                         # (h, w)
ANGLES = [float(a) for a in np.linspace(-180.0, 180.0, 73)] + [0, 1e-3, 44.999, 45, 90, 180, 270, 359.99, 360, -33.3]
FACTORS = [0, 0.31, 0.5, 0.9, 1, 1.13, 1.5, 1.9]


# ---- rotation -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", TILES)
def test_rotate_nearest_equals_pillow(h, w):
    from iswm_amd.utils.ext_transforms import _rotation_coeffs
    rng = np.random.default_rng(h * 1000 + w)
    img = rng.integers(1, 256, (h, w, 3), dtype=np.uint8)                  # no zero: the fill is told from the source
    lbl = rng.integers(1, 3, (h, w), dtype=np.uint8)
    pim, plb = Image.fromarray(img, mode="RGB"), Image.fromarray(lbl, mode="L")
    assert 90 in ANGLES and 270 in ANGLES and -90.0 in ANGLES
    for angle in ANGLES:
        want = np.array(pim.rotate(angle, Image.NEAREST, False, None))
        want_l = np.array(plb.rotate(angle, Image.NEAREST, False, None))
        got, got_l = R.rotate_nearest(img, angle), R.rotate_nearest(lbl, angle)
        assert np.array_equal(got, want), "image %dx%d angle %r: %d pixels differ" % (h, w, angle, int((got != want).any(-1).sum()))
        assert np.array_equal(got_l, want_l), "label %dx%d angle %r" % (h, w, angle)
        # the product's six integers (exact transposes included) give the same picture through the kernel's one formula
        c = _rotation_coeffs(angle, w, h)
        if c is None:
            assert np.array_equal(want, img)
            continue
        y, x = np.mgrid[0:h, 0:w].astype(np.int64)
        xin, yin = (c[2] + y * c[1] + x * c[0]) >> 16, (c[5] + y * c[4] + x * c[3]) >> 16
        inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
        k = np.zeros_like(img)
        k[inside] = img[yin[inside], xin[inside]]
        assert np.array_equal(k, want), "product coefficients %dx%d angle %r" % (h, w, angle)
        assert all(-2 ** 31 <= v < 2 ** 31 for v in c)


# ---- grey and HSV over every colour ------------------------------------------------------------------------------
def _all_colours(lo, hi):
    """uint8 [hi - lo, 256, 3]: every (r, g, b) with lo <= r < hi"""
    r, g, b = np.meshgrid(np.arange(lo, hi), np.arange(256), np.arange(256), indexing="ij")
    return np.stack([r, g, b], -1).reshape(hi - lo, 256 * 256, 3).astype(np.uint8)


def test_gray_and_hsv_equal_pillow_on_all_colours():
    bad = {"gray": 0, "rgb2hsv": 0, "hsv2rgb": 0}
    for lo in range(0, 256, 32):
        c = _all_colours(lo, lo + 32)
        rgb, hsv = Image.fromarray(c, mode="RGB"), Image.fromarray(c, mode="HSV")
        bad["gray"] += int((R.gray(c) != np.array(rgb.convert("L"))).sum())
        bad["rgb2hsv"] += int((R.rgb_to_hsv(c) != np.array(rgb.convert("HSV"))).any(-1).sum())
        bad["hsv2rgb"] += int((R.hsv_to_rgb(c) != np.array(hsv.convert("RGB"))).any(-1).sum())
    assert bad == {"gray": 0, "rgb2hsv": 0, "hsv2rgb": 0}, bad


# ---- blends against ImageEnhance ---------------------------------------------------------------------------------
def _every_value_image():
    """[256, 256, 3]: every value 0..255 in every channel, in three different arrangements"""
    a = np.arange(256, dtype=np.uint8)
    return np.stack([np.broadcast_to(a[:, None], (256, 256)), np.broadcast_to(a[None, :], (256, 256)),
                     (a[:, None] * 7 + a[None, :] * 13).astype(np.uint8)], -1).copy()


@pytest.mark.parametrize("factor", FACTORS)
def test_blends_equal_image_enhance(factor):
    img = _every_value_image()
    assert all(len(np.unique(img[..., k])) == 256 for k in range(3))
    pim = Image.fromarray(img, mode="RGB")
    assert np.array_equal(R.brightness(img, factor), np.array(ImageEnhance.Brightness(pim).enhance(factor)))
    assert np.array_equal(R.saturation(img, factor), np.array(ImageEnhance.Color(pim).enhance(factor)))
    assert np.array_equal(R.contrast(img, factor), np.array(ImageEnhance.Contrast(pim).enhance(factor)))
    dark = (img // 3).astype(np.uint8)                                     # another mean
    assert np.array_equal(R.contrast(dark, factor),
                          np.array(ImageEnhance.Contrast(Image.fromarray(dark, mode="RGB")).enhance(factor)))


@pytest.mark.parametrize("hue_factor", [-0.5, -0.1, 0, 0.1, 0.5])
def test_hue_equals_the_shift_through_pillow_hsv(hue_factor):
    """the reference's adjust_hue: convert('HSV'), np_h += np.uint8(hue_factor * 255) (wrapping), convert('RGB')"""
    rng = np.random.default_rng(5)
    img = np.concatenate([_every_value_image(), rng.integers(0, 256, (64, 256, 3), dtype=np.uint8)])
    h, s, v = Image.fromarray(img, mode="RGB").convert("HSV").split()
    np_h = np.array(h, dtype=np.uint8)
    shift = np.array(int(hue_factor * 255)).astype(np.uint8)               # C conversion: toward zero, then modulo 256
    assert int(shift) == R.hue_shift(hue_factor)
    np_h = (np_h.astype(np.int64) + int(shift)).astype(np.uint8)
    want = np.array(Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB"))
    assert np.array_equal(R.hue(img, hue_factor), want)
    from iswm_amd.utils.ext_transforms import _hue_shift
    assert _hue_shift(hue_factor) == int(shift)


# ---- draw order -------------------------------------------------------------------------------------------------------
def _replay(src_h, src_w, crop, deg, ranges, jitter_first):
    """the reference chain's calls on `random`, literally: rotation :186, scale :109, crop :352-360, flips :228 :254,
    jitter get_params :472-500 (a shuffle of a k-list)"""
    angle = random.uniform(-deg, deg)
    s = random.uniform(0.5, 2.0)
    rs_h, rs_w = int(src_h * s), int(src_w * s)
    th, tw = crop
    w, h, pad = rs_w, rs_h, 0
    if w < tw:
        p = int((1 + tw - w) / 2)
        w, h, pad = w + 2 * p, h + 2 * p, pad + p
    if h < th:
        p = int((1 + th - h) / 2)
        w, h, pad = w + 2 * p, h + 2 * p, pad + p
    if w == tw and h == th:
        i, j = 0, 0
    else:
        i = random.randint(0, h - th)
        j = random.randint(0, w - tw)

    def jitter():
        factors = [None if r is None else random.uniform(r[0], r[1]) for r in ranges]
        lst = [op for op, r in enumerate(ranges) if r is not None]
        random.shuffle(lst)
        return tuple(lst), tuple(factors)
    if jitter_first:
        ops, factors = jitter()
    flip = 1 if random.random() < 0.5 else 0
    vflip = 1 if random.random() < 0.5 else 0
    if not jitter_first:
        ops, factors = jitter()
    return rs_h, rs_w, pad, i, j, flip, angle, vflip, ops, factors


@pytest.mark.parametrize("jitter_first", [True, False])
def test_random_draw_order_matches_a_replay_of_the_reference_calls(jitter_first):
    from iswm_amd.utils import ext_transforms as et
    jit = et.ExtColorJitter(brightness=0.4, contrast=0.3, saturation=(0.5, 1.5), hue=0)      # three enabled factors
    assert jit.hue is None and jit.brightness == [0.6, 1.4] and jit.saturation == (0.5, 1.5)
    flips = [et.ExtRandomHorizontalFlip(), et.ExtRandomVerticalFlip()]
    tail = [jit] + flips if jitter_first else flips + [jit]
    comp = et.ExtCompose([et.ExtRandomRotation(30), et.ExtRandomScale((0.5, 2.0)),
                          et.ExtRandomCrop(size=(65, 65), pad_if_needed=True)] + tail +
                         [et.ExtToTensor(), et.ExtNormalize(MEAN, STD)])
    random.seed(17)
    got = [comp.draw(60, 90) for _ in range(200)]
    after = random.random()
    random.seed(17)
    ranges = (jit.brightness, jit.contrast, jit.saturation, jit.hue)
    want = [_replay(60, 90, (65, 65), 30, ranges, jitter_first) for _ in range(200)]
    assert random.random() == after
    assert got == want
    assert {p[8] for p in got} == set(itertools.permutations((0, 1, 2)))                   # every op order occurs
    assert {p[5] for p in got} == {0, 1} == {p[7] for p in got} and any(p[2] > 0 for p in got)


def test_pipeline_without_new_transforms_draws_six_values():
    from iswm_amd.utils import ext_transforms as et
    comp = et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(size=(65, 65), pad_if_needed=True),
                          et.ExtRandomHorizontalFlip(), et.ExtToTensor(), et.ExtNormalize(MEAN, STD)])
    assert not comp.extended and len(comp.draw(60, 90)) == 6


# ---- composition errors -------------------------------------------------------------------------------------------------
def test_composition_rules_and_argument_checks():
    from iswm_amd.utils import ext_transforms as et
    crop = et.ExtRandomCrop(size=(65, 65), pad_if_needed=True)
    with pytest.raises(NotImplementedError, match="before ExtRandomScale"):
        et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtRandomRotation(10), crop])
    with pytest.raises(NotImplementedError, match="before ExtRandomScale"):
        et.ExtCompose([crop, et.ExtRandomRotation(10)])
    with pytest.raises(NotImplementedError, match="after ExtRandomCrop"):
        et.ExtCompose([et.ExtColorJitter(brightness=0.2), crop])
    with pytest.raises(NotImplementedError, match="after ExtRandomCrop"):
        et.ExtCompose([et.ExtRandomVerticalFlip(), crop])
    with pytest.raises(NotImplementedError, match="NEAREST"):
        et.ExtCompose([et.ExtRandomRotation(10, resample=Image.BILINEAR), crop])
    with pytest.raises(NotImplementedError, match="expand"):
        et.ExtCompose([et.ExtRandomRotation(10, expand=True), crop])
    with pytest.raises(NotImplementedError, match="centre"):
        et.ExtCompose([et.ExtRandomRotation(10, center=(3, 3)), crop])
    et.ExtCompose([et.ExtRandomRotation(10, resample=Image.NEAREST), crop])                 # NEAREST by name is accepted
    for twice in (et.ExtRandomVerticalFlip(), et.ExtColorJitter(brightness=0.2)):            # one of each, like the rotation
        with pytest.raises(NotImplementedError, match="must stand once"):
            et.ExtCompose([crop, twice, et.ExtRandomHorizontalFlip(), twice])
    with pytest.raises(NotImplementedError, match="must stand once"):
        et.ExtCompose([et.ExtRandomRotation(10), et.ExtRandomRotation(10), crop])
    # the constructors accept and refuse what the reference's do (exception types; the messages are this project's),
    # except that a single hue above 0.5 is refused here when the range is built
    with pytest.raises(ValueError, match=r"hue range \[-0.6, 0.6\] leaves \[-0.5, 0.5\]"):
        et.ExtColorJitter(hue=0.6)
    with pytest.raises(ValueError, match="hue range"):
        et.ExtColorJitter(hue=(-0.6, 0.1))
    with pytest.raises(ValueError, match="brightness=-0.1.*cannot be negative"):
        et.ExtColorJitter(brightness=-0.1)
    with pytest.raises(ValueError, match="brightness range.*not ordered"):
        et.ExtColorJitter(brightness=(1.2, 0.8))
    with pytest.raises(ValueError, match="saturation range"):
        et.ExtColorJitter(saturation=(-0.5, 1.0))
    for bad in ("much", (1, 2, 3), None):
        with pytest.raises(TypeError, match="contrast is a number or a"):
            et.ExtColorJitter(contrast=bad)
    with pytest.raises(ValueError, match="cannot be negative"):
        et.ExtRandomRotation(-5)
    with pytest.raises(ValueError, match="got 3 values"):
        et.ExtRandomRotation((1, 2, 3))
    assert et.ExtColorJitter(saturation=(0.5, 1.5)).saturation == (0.5, 1.5) and et.ExtColorJitter(hue=[0, 0]).hue is None
    assert et.ExtColorJitter(contrast=(1, 1)).contrast is None and et.ExtColorJitter(contrast=0.25).contrast == [0.75, 1.25]
    assert et.ExtRandomRotation(15).degrees == (-15, 15) and et.ExtRandomRotation((-5, 20)).degrees == (-5, 20)
    j = et.ExtColorJitter()
    assert j.brightness is None and j.contrast is None and j.saturation is None and j.hue is None
    assert et.ExtColorJitter(brightness=2).brightness == [0, 3] and et.ExtColorJitter(hue=0.5).hue == [-0.5, 0.5]
    assert et.ExtRandomVerticalFlip().p == 0.5


# ---- the untouched pipeline -------------------------------------------------------------------------------------------
class _FakeTensor(object):
    """stands in for the device buffers of batch_resident: the calls are recorded, never made"""

    def data_ptr(self):
        return 4096


def test_untouched_pipeline_issues_the_calls_it_always_issued(monkeypatch):
    import contextlib

    import torch

    from iswm_amd.utils import ext_transforms as et
    names = []
    monkeypatch.setattr(et, "call", lambda name, *a: names.append(name))
    monkeypatch.setattr(et._lib, "load", lambda: None)

    class Store(object):
        meta = [(0, 0, 40, 56), (6720, 2240, 64, 48)]
        device = "cpu"
        img_arena = lbl_arena = _FakeTensor()

    class Ev(object):
        def record(self):
            pass

        def synchronize(self):
            pass

    class Stream(object):
        cuda_stream = 0
    real_empty = torch.empty
    monkeypatch.setattr(torch, "empty", lambda *a, **k: real_empty(*a, **{kk: v for kk, v in k.items()
                                                                          if kk not in ("pin_memory", "device")}))
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.cuda, "Event", Ev)
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: Stream())
    comp = et.ExtCompose([et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(size=(65, 65), pad_if_needed=True),
                          et.ExtRandomHorizontalFlip(), et.ExtToTensor(), et.ExtNormalize(MEAN, STD)])
    random.seed(1)
    out, lbl = comp.batch_resident(Store(), [1, 0])
    assert names == ["iswm_aug_tables", "iswm_augment_batch"] and tuple(out.shape) == (2, 3, 65, 65)
    # with a new transform composed, the same harness sees the new entry points: the recorder does tell them apart
    names.clear()
    comp = et.ExtCompose([et.ExtRandomRotation(20), et.ExtRandomScale((0.5, 2.0)),
                          et.ExtRandomCrop(size=(65, 65), pad_if_needed=True), et.ExtRandomHorizontalFlip(),
                          et.ExtRandomVerticalFlip(), et.ExtColorJitter(0.3, 0.3, 0.3, 0.1)])

    class Lib(object):
        @staticmethod
        def iswm_augment_batch_ex_workspace(b, h, w):
            return 1024
    monkeypatch.setattr(et._lib, "load", lambda: Lib)
    comp.batch_resident(Store(), [1, 0])
    assert names == ["iswm_aug_tables", "iswm_aug_rotate", "iswm_augment_batch_ex"]


# ---- records and exports -----------------------------------------------------------------------------------------------
def test_extra_record_layout_and_exports():
    import ctypes

    from iswm_amd import _lib
    from iswm_amd.utils import ext_transforms as et
    extra = _lib.STRUCTS["iswm_aug_extra"]
    assert ctypes.sizeof(extra) == et._AUG_EXTRA_DTYPE.itemsize == 96
    for name, _ in extra._fields_:
        assert getattr(extra, name).offset == et._AUG_EXTRA_DTYPE.fields[name][1], name
    header = open(os.path.join(ROOT, "include", "iswm_hip.h")).read()
    declared = set(re.findall(r"\b(iswm_[a-z0-9_]+)\s*\(", header))
    for n in ("iswm_aug_rotate", "iswm_augment_batch_ex_workspace", "iswm_augment_batch_ex"):
        assert n in declared and n in _lib.EXPORTS, n
    assert declared == set(_lib.EXPORTS)
    for code, name in enumerate(("BRIGHTNESS", "CONTRAST", "SATURATION", "HUE")):
        assert re.search(r"^#define\s+ISWM_AUG_OP_%s\s+%d\s*$" % (name, code), header, re.M)
        assert getattr(et, "OP_" + name) == code == getattr(R, name)
    # _fill_extra: a 6-tuple is neutral; extended parameters land in the fields the kernel reads
    rec = np.zeros(2, dtype=et._AUG_EXTRA_DTYPE)
    assert et._fill_extra(rec[0], (65, 65, 0, 0, 0, 1), 40, 56, 0, 0) == (False, False)
    assert int(rec[0]["rot_mode"]) == 0 and int(rec[0]["n_ops"]) == 0
    p = (65, 65, 0, 0, 0, 1, 33.3, 1, (3, 1, 0), (0.5, 1.5, None, -0.1))
    assert et._fill_extra(rec[1], p, 40, 56, 32, 16) == (True, True)
    assert int(rec[1]["rot_mode"]) == 1 and tuple(rec[1]["a"]) == R.rotation_coeffs(33.3, 56, 40)
    assert tuple(rec[1]["ops"][:3]) == (3, 1, 0) and int(rec[1]["n_ops"]) == 3 and int(rec[1]["hue_shift"]) == 231
    assert tuple(rec[1]["factor"]) == (np.float32(0.5), np.float32(1.5), 0.0, 0.0)
    assert (int(rec[1]["rot_img_off"]), int(rec[1]["rot_lbl_off"])) == (32, 16)
    with pytest.raises(ValueError, match="factor is None"):                 # an op without its factor is not "factor 0"
        et._fill_extra(rec[0], (65, 65, 0, 0, 0, 0, None, 0, (0,), (None, 1.2, None, None)), 40, 56, 0, 0)
    with pytest.raises(ValueError, match="at most one each"):
        et._fill_extra(rec[0], (65, 65, 0, 0, 0, 0, None, 0, (0, 0), (1.1, None, None, None)), 40, 56, 0, 0)


def test_new_entry_points_validate_on_the_host():
    import ctypes

    from iswm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    assert lib.iswm_augment_batch_ex_workspace(0, 5, 5) == 0
    assert lib.iswm_augment_batch_ex_workspace(3, 65, 65) == 3 * 64 * 8 + 3 * 4
    assert lib.iswm_aug_rotate(None, p, p, p, 1, 4, p, 16, p, 16, None) == 1 and "null" in err()
    assert lib.iswm_aug_rotate(p, p, p, p, 0, 4, p, 16, p, 16, None) == 1 and "B" in err()
    assert lib.iswm_aug_rotate(p, p, p, p, 1, 4, p, 0, p, 16, None) == 1 and "scratch" in err()
    assert lib.iswm_augment_batch_ex(p, p, None, None, p, p, p, 1, 4, 4, f3, f3, 0, p, p, None, 0, None) == 1 and "null" in err()
    assert lib.iswm_augment_batch_ex(p, p, p, None, p, p, p, 1, 4, 4, f3, f3, 0, p, p, p, 512, None) == 1 and "both" in err()
    assert lib.iswm_augment_batch_ex(p, p, None, None, p, p, p, 1, 0, 4, f3, f3, 0, p, p, p, 512, None) == 1 and "size" in err()
    assert lib.iswm_augment_batch_ex(p, p, None, None, p, p, p, 1, 32768, 32769, f3, f3, 0, p, p, p, 512, None) == 1 and "2^30" in err()
    assert lib.iswm_augment_batch_ex(p, p, None, None, p, p, p, 1, 4, 4, f3, f3, 0, p, p, p, 8, None) == 1 and "workspace" in err()
    # iswm_augment_batch keeps its signature
    assert lib.iswm_augment_batch(p, p, p, p, 0, 4, 4, f3, f3, p, p, None) == 1 and "size" in err()


# ---- command line -------------------------------------------------------------------------------------------------------
def test_train_flags_compose_the_new_transforms():
    from iswm_amd import train
    from iswm_amd.utils import ext_transforms as et
    parser = train.get_argparser()
    names = lambda comp: [type(t).__name__ for t in comp.transforms]
    base = ["ExtRandomScale", "ExtRandomCrop", "ExtRandomHorizontalFlip", "ExtToTensor", "ExtNormalize"]
    opts = parser.parse_args(["--device_augment"])
    assert names(train._train_transform(opts, et)) == base and not train._train_transform(opts, et).extended
    opts = parser.parse_args(["--device_augment", "--aug_rotate", "15", "--aug_vflip", "--aug_color_jitter", "0.4,0.3,0.2,0.1"])
    comp = train._train_transform(opts, et)
    assert names(comp) == ["ExtRandomRotation", "ExtRandomScale", "ExtRandomCrop", "ExtRandomHorizontalFlip",
                           "ExtRandomVerticalFlip", "ExtColorJitter", "ExtToTensor", "ExtNormalize"]
    assert comp.rotation.degrees == (-15.0, 15.0) and comp.jitter.hue == [-0.1, 0.1] and comp.jitter.brightness == [0.6, 1.4]
    for bad in ("0.4,0.3,0.2", "0.4,0.3,0.2,0.6", "-0.1,0,0,0", "a,b,c,d"):
        with pytest.raises(ValueError, match="aug_color_jitter"):
            train._train_transform(parser.parse_args(["--device_augment", "--aug_color_jitter=" + bad]), et)
    with pytest.raises(ValueError, match="aug_rotate"):
        train._train_transform(parser.parse_args(["--device_augment", "--aug_rotate", "-3"]), et)
    # the synthetic DataLoader path without --device_augment has no device pipeline to put them in
    with pytest.raises(ValueError, match="--device_augment"):
        train.check_augment_flags(parser.parse_args(["--aug_vflip"]))
    train.check_augment_flags(parser.parse_args([]))
    train.check_augment_flags(parser.parse_args(["--aug_vflip", "--device_augment"]))
    train.check_augment_flags(parser.parse_args(["--aug_rotate", "5", "--dataset", "binary"]))
