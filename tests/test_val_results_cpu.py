"""Host side of the validation image panels (iswm_amd/val_results.py, ops.val_palette / val_panels_layout) and the
restatement tests/val_results_ref.py itself, without a GPU."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import predict_ref as P
from tests import val_results_ref as R


def test_restatement_round_trip_is_off_by_one_for_224_pairs():
    """ToTensor + Normalize, then the reference's Denormalize -> * 255 -> astype(uint8), over all 256 values of all 3
    channels: inside [0, 255] (so numpy never wraps and the clamp never acts), and value - 1 instead of value for
    224 of the 768 pairs -- 104 / 26 / 94 per channel.  That is the reference's arithmetic; its files carry those bytes."""
    img = np.repeat(np.arange(256, dtype=np.uint8)[None, :, None], 3, axis=2)          # [1, 256, 3]: value v in every channel
    x = P.normalize(img)
    t = R.denormalize_f32(x)
    assert t.dtype == np.float32 and t.shape == (1, 256, 3)
    assert t.min() >= 0.0 and t.max() <= 255.0
    u8 = t.astype(np.uint8)
    assert np.array_equal(u8, R.denormalize_u8(x))
    diff = img.astype(int) - u8.astype(int)
    assert set(np.unique(diff)) == {0, 1}
    assert int(diff.sum()) == 224
    assert tuple(int(diff[..., c].sum()) for c in range(3)) == (104, 26, 94)


def test_denormalize_clamps_what_no_image_produces():
    x = torch.zeros(3, 1, 4)
    x[:, 0, 0] = float("nan")
    x[:, 0, 1] = 1e9
    x[:, 0, 2] = -1e9
    x[:, 0, 3] = torch.tensor([(1.0 - m) / s + 0.01 for m, s in zip(R.MEAN, R.STD)])          # t a little above 255
    u8 = R.denormalize_u8(x)
    assert u8[0, :, 0].tolist() == [0, 255, 0, 255] and np.array_equal(u8[..., 0], u8[..., 2])


def test_palette_binary_and_voc():
    from iswm_amd import ops
    b = ops.val_palette(2)
    assert b.shape == (256, 3) and b.dtype == np.uint8
    assert b[1].tolist() == [255, 255, 255] and not b[0].any() and not b[2:].any()         # 255 (ignore) is black too
    assert np.array_equal(b, R.palette(2))
    lab = np.array([[0, 1, 255, 2]], dtype=np.uint8)
    assert np.array_equal(b[lab], R.decode_target(lab, 2))
    v = ops.val_palette(21)
    assert v[:8].tolist() == [[0, 0, 0], [128, 0, 0], [0, 128, 0], [128, 128, 0], [0, 0, 128], [128, 0, 128],
                              [0, 128, 128], [128, 128, 128]]
    assert v[8].tolist() == [64, 0, 0] and v[15].tolist() == [192, 128, 128] and v[255].tolist() == [224, 224, 192]
    for nc in (3, 5, 21, 256):
        assert np.array_equal(ops.val_palette(nc), R.palette(nc))
    assert len({tuple(c) for c in v.tolist()}) == 256


def test_error_map_truth_table():
    label = np.array([[255, 255, 0, 0, 1, 1, 1, 2, 2, 3]], dtype=np.uint8)
    pred = np.array([[0, 1, 0, 2, 1, 0, 2, 2, 0, 1]], dtype=np.uint8)
    want = [R.GREY, R.GREY, R.BLACK, R.RED, R.WHITE, R.BLUE, R.MAGENTA, R.WHITE, R.BLUE, R.MAGENTA]
    assert R.error_map(label, pred)[0].tolist() == [list(c) for c in want]
    assert R.error_map(label.astype(np.int64), pred.astype(np.int64))[0].tolist() == [list(c) for c in want]
    assert (R.GREY, R.RED, R.BLUE, R.MAGENTA) == ((128, 128, 128), (255, 0, 0), (0, 0, 255), (255, 0, 255))


def test_overlay_and_confidence_restatement():
    o = np.array([[[0, 255, 100]]], dtype=np.uint8)
    p = np.array([[[255, 255, 0]]], dtype=np.uint8)
    assert R.overlay(o, p)[0, 0].tolist() == [179, 255, 30]               # (1785 + 5) // 10, 255, (300 + 5) // 10
    assert R.conf_u8(np.array([1.0, 0.5, 0.999999, 1 / 255 - 1e-9])).tolist() == [255, 127, 254, 0]
    lg = np.array([[[[0.0]], [[0.0]]]])
    assert R.max_prob(lg)[0, 0, 0] == 0.5
    assert R.near_boundary(np.array([100 / 255.0, 100.5 / 255.0]), 2e-6).tolist() == [True, False]


def test_directory_and_file_names():
    from iswm_amd import val_results as V
    assert V.results_dirname(1500, 0.87654321) == "best_model_iter_1500_score_0.8765"
    assert V.results_dirname(0, 0.5, prefix="test_only") == "test_only_iter_0_score_0.5000"
    assert V.panel_filename(0, "original") == "0000_original.png" and V.panel_filename(123, "error") == "0123_error.png"
    assert V.panel_kinds(False) == ("original", "target", "pred", "overlay", "error")
    assert V.panel_kinds(True) == ("original", "target", "pred", "overlay", "error", "confidence")


@pytest.mark.parametrize("save_conf", [False, True])
def test_writer_files_modes_and_sizes(tmp_path, save_conf):
    from iswm_amd import val_results as V
    rng = np.random.default_rng(7)
    h, w = 37, 53
    panels = {k: rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for k in V.RGB_KINDS}
    panels["confidence"] = rng.integers(0, 256, (h, w), dtype=np.uint8)
    paths = V.write_panels(str(tmp_path), 3, panels, save_conf)
    kinds = list(V.RGB_KINDS) + (["confidence"] if save_conf else [])
    assert sorted(os.listdir(str(tmp_path))) == sorted("0003_%s.png" % k for k in kinds)
    assert [os.path.basename(p) for p in paths] == ["0003_%s.png" % k for k in kinds]
    for k in kinds:
        im = Image.open(os.path.join(str(tmp_path), "0003_%s.png" % k))
        assert im.size == (w, h) and im.mode == ("L" if k == "confidence" else "RGB"), k
        assert np.array_equal(np.asarray(im), panels[k]), k
    with pytest.raises(ValueError, match="target panel"):
        V.write_panels(str(tmp_path), 4, dict(panels, target=panels["confidence"]), save_conf)


def test_packed_layout():
    from iswm_amd import ops
    assert ops.VAL_PANELS == ("original", "target_rgb", "pred_rgb", "overlay", "error", "pred", "conf")
    lay = ops.val_panels_layout(3, 33, 33)
    rgb, grey = (3 * 33 * 33 * 3 + 15) // 16 * 16, (3 * 33 * 33 + 15) // 16 * 16
    assert [lay[k] for k in ops.VAL_PANELS] == [0, rgb, 2 * rgb, 3 * rgb, 4 * rgb, 5 * rgb, 5 * rgb + grey]
    assert lay["end"] == 5 * rgb + 2 * grey and all(lay[k] % 16 == 0 for k in ops.VAL_PANELS)
    part = ops.val_panels_layout(1, 65, 65, ("conf", "original"))                # packed order, whatever the order asked in
    assert part == {"original": 0, "conf": (65 * 65 * 3 + 15) // 16 * 16, "end": (65 * 65 * 3 + 15) // 16 * 16 + 4240}
    m, s = ops.denorm_constants(R.MEAN, R.STD)
    rm, rs = R.denorm_constants()
    assert m.dtype == np.float32 and np.array_equal(m, rm.numpy()) and np.array_equal(s, rs.numpy())


def test_argparser_keeps_the_reference_flags_off_by_default():
    from iswm_amd import train
    opts = train.get_argparser().parse_args([])
    assert opts.save_val_results is False and opts.save_confidence_map is False and opts.val_results_dir == "val_results"
    opts = train.get_argparser().parse_args(["--save_val_results", "--save_confidence_map", "--val_results_dir", "x"])
    assert opts.save_val_results is True and opts.save_confidence_map is True and opts.val_results_dir == "x"
    assert train.save_validation_results.__module__ == "iswm_amd.val_results"


def test_val_panels_validates_on_the_host():
    """status 1 and a message for missing inputs, nothing launched"""
    import ctypes

    from iswm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_char * 256)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) // 16 * 16)
    q = ctypes.c_void_p(p.value + 4)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    none = [None] * 8

    def call(x, yl, lab, code, n, hi, wi, ldx, c, h, w, pal, outs):
        return lib.iswm_val_panels(x, yl, lab, code, n, hi, wi, ldx, c, h, w, f3, f3, pal, *(outs + [None]))
    assert call(p, p, p, 0, 1, 1, 1, 4, 2, 1, 1, p, none) == 1 and "no output" in err()
    only = lambda i: [p if k == i else None for k in range(8)]          # original pred conf prob target pred_rgb overlay error
    assert call(None, p, p, 0, 1, 1, 1, 4, 2, 1, 1, p, only(0)) == 1 and "need x" in err()
    assert call(p, None, p, 0, 1, 1, 1, 4, 2, 1, 1, p, only(1)) == 1 and "logits" in err()
    assert call(p, p, None, 0, 1, 1, 1, 4, 2, 1, 1, p, only(4)) == 1 and "labels" in err()
    assert call(p, p, p, 0, 1, 1, 1, 4, 2, 1, 1, None, only(5)) == 1 and "palette" in err()
    assert call(p, p, p, 2, 1, 1, 1, 4, 2, 1, 1, p, only(7)) == 1 and "dtype" in err()
    assert call(p, p, p, 0, 1, 1, 1, 4, 5, 1, 1, p, only(1)) == 1 and "pad4" in err()
    assert call(p, p, p, 0, 1, 1, 1, 6, 2, 1, 1, p, only(1)) == 1 and "pad4" in err()
    assert call(p, p, p, 0, 0, 1, 1, 4, 2, 1, 1, p, only(1)) == 1 and "bad size" in err()
    assert call(p, p, p, 0, 1, 1, 1, 4, 2, 1, 1, p, [q if k == 1 else None for k in range(8)]) == 1 and "aligned" in err()
