"""INT8 inference host side (iswm_amd/quant.py) against the restatement tests/quant_ref.py, and the C ABI's argument
checks of csrc/qconv.hip / csrc/quant.hip.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quant_ref as R


def test_fold_matches_restatement():
    from iswm_amd import quant
    from iswm_amd.network import _hip
    g = torch.Generator().manual_seed(0)
    conv = _hip.Conv2d(64, 32, 3, padding=1, bias=False)
    bn = _hip.BatchNorm2d(32)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(conv.weight.shape, generator=g))
        conv.weight[5].zero_()                                   # an all-zero output channel: s_w = 1, q = 0
        bn.weight.copy_(torch.rand(32, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(32, generator=g))
        bn.running_mean.copy_(torch.randn(32, generator=g))
        bn.running_var.copy_(torch.rand(32, generator=g) + 0.1)
    wf, b = quant.fold_bn(conv.weight, bn)
    wr, br = R.fold_bn(conv.weight.detach().double().numpy(), bn.weight.detach().numpy(), bn.bias.detach().numpy(),
                       bn.running_mean.numpy(), bn.running_var.numpy(), bn.eps)
    assert np.array_equal(wf, wr) and np.array_equal(b, br)
    q, s = quant.quantize_weight(wf)
    qr, sr = R.quantize_weight(wr)
    assert np.array_equal(q, qr) and np.array_equal(s, sr)
    assert s[5] == 1.0 and not q[5].any()
    assert np.abs(q).max() == 127 and q.min() >= -127


def test_quantize_weight_clamp_and_ties():
    from iswm_amd import quant
    wf = np.zeros((2, 1, 1, 4))
    wf[0, 0, 0] = [127.0, 2.5, 3.5, -2.5]        # s = 1: rint rounds halves to even
    wf[1, 0, 0] = [-254.0, 1.0, 0.5, 253.0]      # s = 2: -127 stays, 0.25 -> 0, 126.5 -> 126
    q, s = quant.quantize_weight(wf)
    assert list(s) == [1.0, 2.0]
    assert q[0, 0, 0].tolist() == [127, 2, 4, -2]
    assert q[1, 0, 0].tolist() == [-127, 0, 0, 126]
    assert quant.act_scale(0.0) == 1.0 and quant.act_scale(254.0) == 2.0


def test_refuses_separable_conv():
    from iswm_amd import quant
    from iswm_amd.network import modeling
    from iswm_amd.network._deeplab import convert_to_separable_conv
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16, pretrained_backbone=False)
    convert_to_separable_conv(m.classifier)
    with pytest.raises(NotImplementedError, match="separable"):
        quant.calibrate(m, [])
    with pytest.raises(NotImplementedError, match="separable"):
        quant.quantize_model(m, {})


def test_int8_checkpoint_tag():
    from iswm_amd import quant
    assert quant.is_int8_checkpoint({"format": quant.FORMAT})
    assert not quant.is_int8_checkpoint({"model_state": {}})
    assert not quant.is_int8_checkpoint(torch.zeros(1))
    with pytest.raises(ValueError, match="not an iswm_amd INT8 checkpoint"):
        quant.load_int8({"model_state": {}})


def test_read_checkpoint_detects_the_format_tag(tmp_path):
    """INT8 files are recognised; FP32 checkpoints with numpy scalars in their score dictionaries (the reference's and
    train.py's best_*.pth) still load through the weights-only loader and come back unchanged"""
    from iswm_amd import quant
    from iswm_amd.train import load_checkpoint
    p8, p32 = str(tmp_path / "m_int8.pth"), str(tmp_path / "m.pth")
    torch.save({"format": quant.FORMAT, "arch": {"model": "deeplabv3_resnet50"}}, p8)
    ck = {"model_state": {"module.w": torch.arange(3.0)}, "best_score": {"Mean IoU": np.float64(0.5)},
          "val_score": {"Overall Acc": np.float32(0.25), "n": np.int64(3)}}
    torch.save(ck, p32)
    q8, d8 = quant.read_checkpoint(p8)
    assert q8 is d8 and q8["arch"]["model"] == "deeplabv3_resnet50"
    q32, d32 = quant.read_checkpoint(p32)
    assert q32 is None and d32["best_score"]["Mean IoU"] == 0.5
    assert torch.equal(d32["model_state"]["module.w"], load_checkpoint(p32)["model_state"]["module.w"])


def test_predict_load_model_accepts_a_read_checkpoint(tmp_path):
    from iswm_amd import predict, quant
    conv = torch.nn.Conv2d(2, 3, 1)
    p = str(tmp_path / "best.pth")
    torch.save({"model_state": {"module." + k: v + 1 for k, v in conv.state_dict().items()},
                "best_score": {"Mean IoU": np.float64(0.7)}}, p)
    q, ck = quant.read_checkpoint(p)
    assert q is None
    m = predict.load_model(torch.nn.Conv2d(2, 3, 1), p, ck)
    assert torch.equal(m.weight, conv.weight + 1)


def _touch_png(path, h, w, value=0):
    from PIL import Image
    Image.fromarray(np.full((h, w, 3), value, np.uint8)).save(path)


def test_evaluator_file_pairing(tmp_path, caplog):
    from PIL import Image

    from iswm_amd import evaluate_quantization as E
    imgs, masks = tmp_path / "imgs", tmp_path / "masks"
    imgs.mkdir()
    masks.mkdir()
    for n in ("c.png", "a.jpg", "b.PNG", "d.jpeg"):
        _touch_png(str(imgs / n), 4, 5)
    (imgs / "notes.txt").write_text("x")
    Image.fromarray(np.array([[0, 3, 255, 0, 1]] * 4, np.uint8)).save(str(masks / "a_mask.jpg"), quality=100)
    Image.fromarray(np.array([[0, 3, 255, 0, 1]] * 4, np.uint8)).save(str(masks / "c_mask.png"))
    (masks / "b_mask.png").write_bytes(b"")                   # wrong suffix case: b.PNG pairs with b_mask.PNG only
    got = E.pair_files(str(imgs), str(masks))
    assert [g[0] for g in got] == ["a.jpg", "b.PNG", "c.png", "d.jpeg"]
    assert [g[2] is not None for g in got] == [True, False, True, False]
    assert got[2][2] == str(masks / "c_mask.png")
    assert [g[0] for g in E.pair_files(str(imgs), str(masks), num_images=2)] == ["a.jpg", "b.PNG"]
    img, mask = E.load_sample(got[2][1], got[2][2])
    assert img.shape == (4, 5, 3) and mask.dtype == np.uint8
    assert mask[0].tolist() == [0, 1, 1, 0, 1]
    with caplog.at_level("WARNING"):
        img, mask = E.load_sample(got[3][1], None)
    assert mask.shape == (4, 5) and not mask.any() and "no mask" in caplog.text


def test_evaluator_arguments():
    from iswm_amd import evaluate_quantization as E
    p = E.get_argparser()
    o = p.parse_args(["--fp32_ckpt", "a.pth", "--eval_data_dir", "d"])
    assert (o.num_images, o.output_stride, o.num_visualizations, o.results_dir, o.model) == \
        (0, 16, 20, "evaluation_results", "deeplabv3plus_resnet50")
    o = p.parse_args(["--fp32_ckpt", "a.pth", "--eval_data_dir", "d", "--num_images", "7", "--output_stride", "8",
                      "--model", "deeplabv3_resnet101"])
    assert (o.num_images, o.output_stride, o.model) == (7, 8, "deeplabv3_resnet101")
    with pytest.raises(SystemExit):
        p.parse_args(["--eval_data_dir", "d"])
    with pytest.raises(SystemExit):
        p.parse_args(["--fp32_ckpt", "a.pth"])


def test_evaluator_comparison_png(tmp_path):
    from PIL import Image

    from iswm_amd import evaluate_quantization as E
    img = np.zeros((6, 8, 3), np.uint8)
    m = np.zeros((6, 8), np.uint8)
    m[2:4] = 1
    path = E.save_visual_comparison(img, m, m, 1 - m, str(tmp_path), "x.png")
    assert path.endswith("x_comparison.png")
    out = np.asarray(Image.open(path))
    assert out.shape == (2 * (6 + 20), 16, 3)
    assert (out[20 + 2, 8:] == 255).all() and (out[2 * 20 + 6 + 2, 8:] == 0).all()     # GT row 2 fg, INT8 row 2 bg


def test_calibration_hook_is_off_by_default():
    from iswm_amd.network import _hip
    assert _hip.CALIB_RECORDER is None


def test_c_abi_argument_checks():
    from iswm_amd import _lib
    lib = _lib.load()
    d = _lib.QConvDesc(1, 8, 8, 64, 8, 8, 16, 3, 3, 1, 1, 1, 64, 16, 0, 1, 0, 0, 16)
    assert lib.iswm_qconv_weight_bytes(ctypes.byref(d)) == 16 * 9 * 64
    assert lib.iswm_qconv_fwd(ctypes.byref(d), None, None, None, None, None, 0.0, 1.0, None, None) == 1
    assert b"null pointer" in lib.iswm_last_error()
    assert lib.iswm_qconv_fwd(None, None, None, None, None, None, 0.0, 1.0, None, None) == 1
    bad = _lib.QConvDesc(1, 8, 8, 48, 8, 8, 16, 3, 3, 1, 1, 1, 64, 16, 0, 1, 0, 0, 16)        # Cin % 64 != 0
    assert lib.iswm_qconv_weight_bytes(ctypes.byref(bad)) == 0
    assert lib.iswm_qconv_fwd(ctypes.byref(bad), None, None, None, None, None, 0.0, 1.0, None, None) == 1
    assert b"Cin" in lib.iswm_last_error()
    bad = _lib.QConvDesc(1, 8, 8, 64, 7, 8, 16, 3, 3, 1, 1, 1, 64, 16, 0, 1, 0, 0, 16)        # Ho inconsistent
    assert lib.iswm_qconv_fwd(ctypes.byref(bad), None, None, None, None, None, 0.0, 1.0, None, None) == 1
    assert b"output size" in lib.iswm_last_error()
    assert lib.iswm_absmax(None, 0, 4, 4, 4, None, 0, None, None) == 1
    assert lib.iswm_absmax_workspace(0, 4) == 0 and lib.iswm_absmax_workspace(100, 4) > 0
    assert lib.iswm_quantize_i8(None, 0, 4, 4, 4, 1.0, 0, None, 4, None) == 1
    assert lib.iswm_qgap(None, 1, 4, 64, 64, 1.0, 1.0, None, 64, None) == 1
    assert lib.iswm_qbcast(None, 1, 4, 64, 64, None, 64, None) == 1
    assert lib.iswm_qbilinear(None, 1, 4, 4, 64, 64, 1.0, 8, 8, 1.0, None, 64, None) == 1
    assert b"null pointer" in lib.iswm_last_error()


def test_restatement_conv_int_matches_direct_sum():
    rng = np.random.default_rng(1)
    x = rng.integers(-127, 128, (1, 5, 6, 3)).astype(np.int8)
    w = rng.integers(-127, 128, (2, 3, 3, 3)).astype(np.int8)
    got = R.conv_int(x, w, 2, 2, 2)
    ho, wo = got.shape[1:3]
    for oh in range(ho):
        for ow in range(wo):
            for c in range(2):
                s = 0
                for i in range(3):
                    for j in range(3):
                        ih, iw = oh * 2 - 2 + 2 * i, ow * 2 - 2 + 2 * j
                        if 0 <= ih < 5 and 0 <= iw < 6:
                            s += int(np.dot(x[0, ih, iw].astype(np.int64), w[c, :, i, j].astype(np.int64)))
                assert got[0, oh, ow, c] == s
