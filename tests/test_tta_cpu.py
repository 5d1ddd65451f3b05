"""Flip and multi-scale test-time augmentation without a GPU: the view list of ops.tta_views against the restatement
tests/tta_ref.py and every refusal, the command line's flags, the view limit of the C header, the exported entry points
and their host validation, and the error caps of tests/test_tta_gpu.py checked on that test's inputs before a GPU sees
them."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import predict_ref as R
from tests import scene_cases as SC
from tests import tta_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_views_sizes_and_order():
    from iswm_amd import ops
    assert ops.tta_views(97, 129, [1.0], False) == [(97, 129, False)]
    assert ops.tta_views(97, 129, [1.0], True) == [(97, 129, False), (97, 129, True)]
    # int(x + 0.5): 97 * 0.75 = 72.75 -> 73, 129 * 0.75 = 96.75 -> 97, 97 * 1.25 = 121.25 -> 121, 129 * 1.25 = 161.25
    assert ops.tta_views(97, 129, (0.75, 1.0, 1.25), True) == [
        (73, 97, False), (73, 97, True), (97, 129, False), (97, 129, True), (121, 161, False), (121, 161, True)]
    # exact halves round up, not to even: 5 * 0.5 = 2.5 -> 3, 9 * 0.5 = 4.5 -> 5, 2 * 1.25 = 2.5 -> 3, 6 * 0.25 = 1.5 -> 2
    assert ops.tta_views(5, 9, [0.5], False) == [(3, 5, False)]
    assert ops.tta_views(2, 6, [1.25, 0.25], False) == [(3, 8, False), (1, 2, False)]
    # the order given is kept; never below one pixel; no deduplication of sizes
    assert ops.tta_views(1, 1, [0.25, 1.0, 0.5], True) == [(1, 1, False), (1, 1, True)] * 3
    assert ops.tta_views(8, 8, [2.0, 0.5], False) == [(16, 16, False), (4, 4, False)]
    assert ops.tta_views(513, 513, [0.25, 4.0], False) == [(128, 128, False), (2052, 2052, False)]
    assert ops.PREDICT_MAX_VIEWS == T.MAX_VIEWS == 16
    assert len(ops.tta_views(37, 53, T.EIGHT, True)) == 16
    rng = np.random.default_rng(0)
    for _ in range(300):
        H, W = (int(v) for v in rng.integers(1, 700, 2))
        scales = [float(s) for s in rng.choice(np.arange(25, 401) / 100.0, int(rng.integers(1, 9)), replace=False)]
        flip = bool(rng.integers(0, 2))
        assert ops.tta_views(H, W, scales, flip) == T.views(H, W, scales, flip)


@pytest.mark.parametrize("args,names", [
    ((37, 53, [], False), "0 scales"),
    ((37, 53, [0.3 + 0.1 * i for i in range(9)], False), "9 scales"),
    ((37, 53, [1.0, 0.2], False), "0.2"),
    ((37, 53, [4.5], True), "4.5"),
    ((37, 53, [1.0, float("nan")], True), "nan"),
    ((37, 53, [1.0, 0.5, 1.0], False), "1.0 is given twice"),
    ((37, 53, [1.0, "2"], False), "'2'"),
    ((37, 53, [True], False), "True"),
    ((37, 53, 1.0, False), "1.0"),
    ((0, 53, [1.0], False), "0 x 53"),
    ((37, -2, [1.0], False), "37 x -2"),
    ((37.0, 53, [1.0], False), "37.0"),
    ((37, 53, [1.0], 2), "flip 2"),
    ((37, 53, [1.0], None), "flip None"),
])
def test_views_refusals_name_the_value(args, names):
    from iswm_amd import ops
    with pytest.raises(ValueError, match=re.escape(names)):
        ops.tta_views(*args)


def test_max_views_of_the_header_is_the_python_limit():
    from iswm_amd import _lib, ops
    header = open(os.path.join(ROOT, "include", "iswm_hip.h")).read()
    m = re.search(r"^#define\s+ISWM_PREDICT_MAX_VIEWS\s+(\d+)\s*$", header, re.M)
    assert m, "ISWM_PREDICT_MAX_VIEWS is not defined in the header"
    assert int(m.group(1)) == ops.PREDICT_MAX_VIEWS == 2 * ops.TTA_MAX_SCALES
    assert ctypes.sizeof(_lib.PredictView) == 24                       # pointer, three ints, padded to 8


def test_tta_flags_parse_and_refuse_bad_combinations(capsys):
    from iswm_amd import predict
    parser = predict.get_argparser()
    base = ["--input", "x", "--save_val_results_to", "y"]
    parse = lambda *a: parser.parse_args(base + list(a))
    opt = lambda *a: predict.tta_options(parser, parse(*a))
    d = parse()
    assert d.tta_scales == "1.0" and d.tta_flip is False
    assert opt() is None                                              # the defaults: DevicePredictor, as before
    assert opt("--tta_scales", "1.0") is None and opt("--tta_scales", "1") is None
    assert opt("--tile_size", "513") is None                          # tiles without TTA stay allowed
    assert opt("--tta_flip") == ([1.0], True)
    assert opt("--tta_scales", "0.75,1.0,1.25") == ([0.75, 1.0, 1.25], False)
    assert opt("--tta_scales", " 0.5, 2", "--tta_flip") == ([0.5, 2.0], True)
    assert opt("--tta_scales", "0.5") == ([0.5], False)
    for bad, word in ((("--tta_scales", "1.0,abc"), "abc"), (("--tta_scales", ""), "''"),
                      (("--tta_scales", "1.0,,2.0"), "''"), (("--tta_scales", "0.1,1.0"), "0.1"),
                      (("--tta_scales", "1.0,5"), "5.0"), (("--tta_scales", "1.0,1.00"), "twice"),
                      (("--tta_scales", "nan"), "nan"),
                      (("--tta_scales", ",".join("%g" % (0.3 + 0.1 * i) for i in range(9))), "9 scales")):
        with pytest.raises(SystemExit):
            opt(*bad)
        err = capsys.readouterr().err
        assert "--tta_scales" in err and word in err, (bad, err)
    for bad in (("--tta_flip", "--tile_size", "64"), ("--tta_scales", "0.5,1.0", "--tile_size", "64")):
        with pytest.raises(SystemExit):
            opt(*bad)
        err = capsys.readouterr().err
        assert "--tile_size" in err and "over windows is not built" in err.replace("\n", " "), err


def _aligned(buf):
    a = ctypes.addressof(buf)
    return ctypes.c_void_p((a + 15) // 16 * 16)


def test_tta_entry_points_are_exported_and_validate_on_the_host():
    from iswm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    for n in ("iswm_predict_view_normalize", "iswm_predict_views_maps_workspace", "iswm_predict_views_maps"):
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    for n, h, w in ((1, 37, 53), (2, 65, 65), (16, 513, 513), (0, 5, 5)):
        assert lib.iswm_predict_views_maps_workspace(n, h, w) == lib.iswm_predict_maps_workspace(n, h, w)
    buf = (ctypes.c_char * 256)()
    p = _aligned(buf)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    # null pointers and bad ranges: status 1 and a message, nothing launched
    assert lib.iswm_predict_view_normalize(None, 1, 4, 4, 4, 4, 0, f3, f3, p, None) == 1 and "null" in err()
    assert lib.iswm_predict_view_normalize(p, 1, 4, 4, 0, 4, 0, f3, f3, p, None) == 1 and "0 x 4" in err()
    assert lib.iswm_predict_view_normalize(p, 1, 4, 4, 4, 4, 2, f3, f3, p, None) == 1 and "flip 2" in err()
    assert lib.iswm_predict_view_normalize(p, 0, 4, 4, 4, 4, 0, f3, f3, p, None) == 1
    ws = lib.iswm_predict_views_maps_workspace(1, 37, 53)

    def call(nviews=2, yl=p.value, Hi=5, flip=1, ldx=4, C=2, fg=1, out=p, wsb=ws, views=True):
        arr = (_lib.PredictView * 17)(*[_lib.PredictView(p.value, 5, 5, 0) for _ in range(17)])
        arr[1] = _lib.PredictView(yl, Hi, 5, flip)
        return lib.iswm_predict_views_maps(arr if views else None, nviews, 1, ldx, C, fg, 37, 53, 0.5, 51, 178, out, p, p,
                                           None, p, p, wsb, None)
    assert call(views=False) == 1 and "null" in err()
    assert call(nviews=0) == 1 and "0 views" in err()
    assert call(nviews=17) == 1 and "17 views" in err() and "16" in err()
    assert call(yl=None) == 1 and "view 1" in err() and "null" in err()
    assert call(yl=p.value + 4) == 1 and "view 1" in err() and "aligned" in err()
    assert call(Hi=0) == 1 and "view 1" in err() and "0 x 5" in err()
    assert call(flip=2) == 1 and "view 1" in err() and "flip 2" in err()
    assert call(wsb=ws - 1) == 1 and "workspace" in err()
    assert call(fg=2) == 1 and "foreground class 2" in err()
    assert call(ldx=6) == 1 and "ldx" in err()
    assert call(C=5) == 1 and "ldx" in err()
    assert call(out=ctypes.c_void_p(p.value + 4)) == 1 and "aligned" in err()


def test_combine_properties():
    rng = np.random.default_rng(3)
    p = rng.random((1, 7, 9))
    assert np.array_equal(T.combine(p, np.float64), p[0])
    p32 = p.astype(np.float32)
    assert np.array_equal(T.combine(p32, np.float32), p32[0])
    assert np.array_equal(T.combine(np.stack([p32[0], p32[0]]), np.float32), p32[0])       # (p + p) / 2 = p
    for V in (2, 3, 6, 16):                                            # ones stay one: no clamp is needed
        assert np.array_equal(T.combine(np.ones((V, 4, 4), dtype=np.float32), np.float32), np.ones((4, 4), np.float32))
        top = np.full((V, 64), np.float32(1.0)) - rng.integers(0, 2, (V, 64)).astype(np.float32) * np.float32(2.0 ** -24)
        assert T.combine(top.astype(np.float32), np.float32).max() <= 1.0


@pytest.mark.parametrize("frame", T.FRAMES)
@pytest.mark.parametrize("c,fg,ld", SC.CLASSES)
def test_combine_fp32_respects_the_gpu_tests_caps(c, fg, ld, frame):
    """the kernel's order of operations in float32 against the mean in float64, on the GPU test's logits with each
    view's probability correctly rounded: the bound and both pixel caps of test_views_maps_against_restatement hold"""
    H, W = frame
    for scales, flip in T.VIEW_SETS:
        vl = T.view_logits(H, W, scales, flip, c, fg, ld)
        V = len(vl)
        p_v = np.stack([T.unflip(R.softmax_fg(SC.upsample64(yl.numpy(), c, H, W), fg), f) for yl, f in vl])
        p64 = T.combine(p_v, np.float64)
        p32 = T.combine(p_v.astype(np.float32), np.float32)
        assert p32.max() <= 1.0
        assert np.abs(p32.astype(np.float64) - p64).max() <= T.bound(V)
        for thr, mn, mx in SC.CUTS:
            pred, conf = R.predict_mask(p32, thr)
            band = R.binarize_confidence_map(conf, mn, mx)
            pred_r, conf_r = R.predict_mask(p64, thr)
            band_r = R.binarize_confidence_map(conf_r, mn, mx)
            bad = (pred != pred_r) | (conf != conf_r) | (band != band_r)
            edge = R.near_boundary(p64, thr, 2 * T.bound(V))
            assert not (bad & ~edge).any()
            assert (bad & ~(p32 == 1.0)).sum() <= 1e-3 * p64.size + 2
            if c == 2 and thr == 0.5:
                assert 0.05 <= float((p64 > thr).mean()) <= 0.95


def test_view_normalize64_identity_and_flip_are_the_reference_normalize():
    rng = np.random.default_rng(5)
    img = rng.integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    want = np.stack([R.normalize(f).double().numpy() for f in img])
    got = T.view_normalize64(img, 7, 9, False)
    assert got.shape == (2, 3, 7, 9) and np.abs(got - want).max() <= 4e-7      # fp32 chain against fp64
    assert np.array_equal(T.view_normalize64(img, 7, 9, True), got[..., ::-1])
    assert np.array_equal(T.view_normalize64(img, 7, 9, True), T.view_normalize64(img[:, :, ::-1], 7, 9, False))
    # torch's own resampling of the frame, in fp64
    import torch
    import torch.nn.functional as F
    x = torch.from_numpy(img).permute(0, 3, 1, 2).double()
    for hv, wv in ((4, 5), (11, 13), (14, 18)):
        y = F.interpolate(x, size=(hv, wv), mode="bilinear", align_corners=False).flip(-1).numpy()
        m = np.asarray(R.MEAN, np.float32).astype(np.float64)[None, :, None, None]
        s = np.asarray(R.STD, np.float32).astype(np.float64)[None, :, None, None]
        assert np.abs(T.view_normalize64(img, hv, wv, True) - (y / 255.0 - m) / s).max() <= 1e-4
