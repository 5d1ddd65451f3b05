"""INT8 inference host side (iswm_amd/quant.py) against the restatement tests/quant_ref.py, and the C ABI's argument
checks of csrc/qconv.hip / csrc/quant.hip.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from tests import quant_cases as Q
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
    # forms the ABI refuses by design: an output pitch that is no multiple of 4 (so cstore % 4 != 0 needs a padded
    # pitch), a source pitch that is no multiple of 16, a pitch below the channels it holds
    for ldx, ldy, cstore, msg in ((64, 3, 3, b"ldy >= cstore, ldy % 4 == 0"), (64, 18, 16, b"ldy % 4 == 0"),
                                  (72, 16, 16, b"ldx >= Cin, ldx % 16 == 0"), (48, 16, 16, b"ldx >= Cin"),
                                  (64, 12, 16, b"ldy >= cstore"), (64, 16, 17, b"0 < cstore <= Cout")):
        bad = _lib.QConvDesc(1, 8, 8, 64, 8, 8, 16, 3, 3, 1, 1, 1, ldx, ldy, 0, 1, 0, 0, cstore)
        assert lib.iswm_qconv_fwd(ctypes.byref(bad), None, None, None, None, None, 0.0, 1.0, None, None) == 1
        assert msg in lib.iswm_last_error(), lib.iswm_last_error()
    assert lib.iswm_absmax(ctypes.c_void_p(16), 0, 4, 3, 3, ctypes.c_void_p(16), 4, ctypes.c_void_p(16), None) == 1
    assert b"ld % 4 == 0, ld >= pad4(C)" in lib.iswm_last_error()
    assert lib.iswm_quantize_i8(ctypes.c_void_p(16), 0, 4, 3, 4, 1.0, 0, ctypes.c_void_p(16), 3, None) == 1
    assert b"ldy % 4 == 0, ldy >= C" in lib.iswm_last_error()
    assert lib.iswm_qgap(ctypes.c_void_p(16), 1, 4, 64, 63, 1.0, 1.0, ctypes.c_void_p(16), 64, None) == 1
    assert b"qgap: bad size" in lib.iswm_last_error()
    assert lib.iswm_qbcast(ctypes.c_void_p(16), 1, 4, 6, 8, ctypes.c_void_p(16), 8, None) == 1
    assert b"qbcast: need C, ldv, ldy multiples of 4" in lib.iswm_last_error()
    assert lib.iswm_qbilinear(ctypes.c_void_p(16), 1, 4, 4, 6, 8, 1.0, 8, 8, 1.0, ctypes.c_void_p(16), 8, None) == 1
    assert b"qbilinear: need C, ldx, ldy multiples of 4" in lib.iswm_last_error()
    assert lib.iswm_absmax(None, 0, 4, 4, 4, None, 0, None, None) == 1
    assert lib.iswm_absmax_workspace(0, 4) == 0 and lib.iswm_absmax_workspace(100, 4) > 0
    assert lib.iswm_quantize_i8(None, 0, 4, 4, 4, 1.0, 0, None, 4, None) == 1
    assert lib.iswm_qgap(None, 1, 4, 64, 64, 1.0, 1.0, None, 64, None) == 1
    assert lib.iswm_qbcast(None, 1, 4, 64, 64, None, 64, None) == 1
    assert lib.iswm_qbilinear(None, 1, 4, 4, 64, 64, 1.0, 8, 8, 1.0, None, 64, None) == 1
    assert b"null pointer" in lib.iswm_last_error()


# (H, W, k, stride, pad, dil): the first geometry, stride 2 on an even map, no padding, a rate at least the map, and
# padding wider than the filter (whole output pixels inside the padding)
DIRECT_SUM_GEOMETRIES = [(5, 6, 3, 2, 2, 2), (8, 10, 3, 2, 1, 1), (8, 10, 1, 2, 0, 1), (6, 7, 3, 1, 0, 1),
                         (5, 7, 3, 1, 18, 18), (9, 11, 3, 1, 6, 6), (4, 5, 3, 1, 3, 1), (1, 1, 3, 1, 2, 2)]


def test_restatement_conv_int_matches_direct_sum():
    rng = np.random.default_rng(1)
    for (h, wd, k, stride, pad, dil) in DIRECT_SUM_GEOMETRIES:
        x = rng.integers(-128, 128, (2, h, wd, 3)).astype(np.int8)
        w = rng.integers(-128, 128, (2, 3, k, k)).astype(np.int8)
        got = R.conv_int(x, w, stride, pad, dil)
        ho, wo = got.shape[1:3]
        assert (ho, wo) == (Q.conv_out(h, k, stride, pad, dil), Q.conv_out(wd, k, stride, pad, dil))
        dead = 0
        for n in range(2):
            for oh in range(ho):
                for ow in range(wo):
                    taps = 0
                    for c in range(2):
                        s = 0
                        for i in range(k):
                            for j in range(k):
                                ih, iw = oh * stride - pad + dil * i, ow * stride - pad + dil * j
                                if 0 <= ih < h and 0 <= iw < wd:
                                    taps += 1
                                    s += int(np.dot(x[n, ih, iw].astype(np.int64), w[c, :, i, j].astype(np.int64)))
                        assert got[n, oh, ow, c] == s
                    dead += taps == 0
        assert (dead > 0) == ((h, wd, pad) == (4, 5, 3))


def test_restatement_conv_int_is_exact_at_the_int32_limit():
    """2048 * 9 products of magnitude 2^14: the fp64 partial sums stay below 2^31 and are exact"""
    for cid, want in (("extreme_pos", 128 * 128 * 18432), ("extreme_neg", -128 * 127 * 18432)):
        c = Q.QCONV_BY_ID[cid]
        o = Q.qconv_operands(c)
        acc = R.conv_int(o["xbuf"], o["w"], c.stride, c.pad, c.dil)
        assert acc.dtype == np.int64 and (acc[0, 1, 1] == want).all() and (acc[0, 0, 0] == want * 4 // 9).all()
        assert 2 ** 28 < abs(want) < 2 ** 31
        y = Q.qconv_expected(c, o)
        assert y.dtype == np.float32 and (y[0, 1, 1].astype(np.int64) == want).all()     # exact in fp32 too


# ---- the edge cases of tests/quant_cases.py: each case's property, from the restated geometry and quant_ref alone ----
def test_case_ids_are_unique_and_seeded_without_hash():
    for table in (Q.QCONV, Q.ABSMAX, Q.QUANTIZE, Q.QGAP, Q.QBCAST, Q.QBILINEAR):
        ids = [c.id for c in table]
        assert len(ids) == len(set(ids))
    a, b = Q.rng_of("one_pixel").integers(0, 1 << 30), Q.rng_of("one_pixel").integers(0, 1 << 30)
    import zlib
    assert a == b == np.random.default_rng(zlib.crc32(b"one_pixel")).integers(0, 1 << 30)
    assert "hash(" not in open(Q.__file__).read().replace("Python's hash()", "")


@pytest.mark.parametrize("cid", [c.id for c in Q.QCONV])
def test_qconv_case_property(cid):
    c = Q.QCONV_BY_ID[cid]
    t = Q.qconv_tiles(c)
    taps = Q.qconv_taps(c)
    o = Q.qconv_operands(c)
    want = Q.qconv_expected(c, o)
    assert want.shape == (c.N, t["Ho"], t["Wo"], c.Cout) and want.dtype == (np.float32 if c.f32 else np.int8)
    assert c.Cin % 64 == 0 and t["Cout_p"] % 16 == 0 and t["grid"][0] == (t["M"] + 255) // 256
    special = cid.startswith("ties") or cid.startswith("extreme")
    if not special:
        assert o["xbuf"].min() == -128 and o["w"].min() == -128
    centre = np.zeros((c.k, c.k), bool)
    centre[c.k // 2, c.k // 2] = True
    if cid == "one_pixel":
        assert t["M"] == 1 and t["steps"] == 1
    elif cid == "pooled":
        assert t["M"] == 3 and t["wide"] and t["grid"] == (1, 4)
    elif cid == "centre_only_1x1":
        assert t["M"] == 2 and (taps == centre).all() and taps.sum(axis=(2, 3)).max() == 1
    elif cid == "rate_ge_map":
        assert (taps == centre).all() and c.dil >= max(c.H, c.W)
        assert t["M"] == 35 and t["waves"] == 1 and t["row_blocks"] == 3 and t["ragged_rows"] == 3
        one = R.epilogue(R.conv_int(o["xbuf"], o["w"][:, :, 1:2, 1:2], 1, 0, 1), o["mul"], o["add"], c.relu, o["inv_s"],
                         o["lo"])
        assert np.array_equal(want, one)
    elif cid == "rate_partial":
        per_tap = taps.reshape(-1, 9)                   # the centre tap (pad = dil) is inside at every pixel
        assert per_tap.any(axis=0).all() and per_tap.all(axis=0).tolist() == [False] * 4 + [True] + [False] * 4
        assert set(per_tap.sum(axis=1).tolist()) == {1, 2, 4}
    elif cid == "s2_even":
        assert (t["Ho"], t["Wo"]) == (4, 5) and c.H % 2 == 0 and c.W % 2 == 0
        assert taps[-1, :, 2, 1].all() and taps[:, -1, 1, 2].all()          # the bottom and right taps are inside
        assert not taps[0, :, 0, :].any() and not taps[:, 0, :, 0].any()    # the top and left ones are padding
        assert (c.stride * (t["Ho"] - 1) - c.pad + 2, c.stride * (t["Wo"] - 1) - c.pad + 2) == (c.H - 1, c.W - 1)
    elif cid == "s2_1x1_even":
        assert (t["Ho"], t["Wo"], t["M"]) == (4, 5, 40) and t["wide"] and taps.all()
    elif cid == "valid_pad0":
        assert (t["Ho"], t["Wo"]) == (4, 5) and taps.all() and c.pad == 0
    elif cid == "over_pad":
        assert (t["Ho"], t["Wo"]) == (8, 9) and c.pad != c.dil * (c.k - 1) // 2
        dead = ~taps.any(axis=(2, 3))
        ring = np.ones((8, 9), bool)
        ring[1:-1, 1:-1] = False
        assert np.array_equal(dead, ring)
        zero = R.epilogue(np.zeros(want.shape, np.int64), o["mul"], o["add"], c.relu, o["inv_s"], o["lo"], o["res"],
                          o["s_res"])
        assert np.array_equal(want[0][dead], zero[0][dead]) and not np.array_equal(want[0][~dead], zero[0][~dead])
    elif cid == "m256":
        assert t["M"] == 256 and t["grid"][0] == 1 and t["waves"] == 4 and t["ragged_rows"] == 0
    elif cid == "m257":
        assert t["M"] == 257 and t["grid"][0] == 2 and t["M"] - Q.QC_WG_ROWS == 1
    elif cid == "chunks3":
        assert t["chunks"] == 3 and t["steps"] == 27 and t["chunks"] & (t["chunks"] - 1)
    elif cid == "x_slice":
        k3 = Q.QCONV_BY_ID["chunks3"]
        assert c[1:4] + c[5:10] == k3[1:4] + k3[5:10] and c.Cin == 128
        ld, x0 = Q.X_SLICE
        assert o["xbuf"].shape[3] == ld == 256 and o["x0"] == x0 == 64 and x0 + c.Cin == 192
        assert (o["xbuf"][..., :x0] == 127).all() and (o["xbuf"][..., x0 + c.Cin:] == 127).all()
        other = dict(o, xbuf=o["xbuf"].copy())
        other["xbuf"][..., :x0] = -77
        other["xbuf"][..., x0 + c.Cin:] = 31
        assert np.array_equal(Q.qconv_expected(c, other), want)
        leak = R.epilogue(R.conv_int(o["xbuf"][..., :c.Cin], o["w"], c.stride, c.pad, c.dil), o["mul"], o["add"], c.relu,
                          o["inv_s"], o["lo"])
        assert not np.array_equal(leak, want)                               # reading from channel 0 would show
    elif cid.startswith("extreme"):
        wv = -128 if cid == "extreme_pos" else 127
        assert (o["xbuf"] == -128).all() and (o["w"] == wv).all() and c.f32 and (o["mul"] == 1).all() and not o["add"].any()
        acc = -128 * wv * 9 * c.Cin
        assert 2 ** 28 < abs(acc) < 2 ** 31 and (want[0, 1, 1] == np.float32(acc)).all() and float(np.float32(acc)) == acc
    elif cid.startswith("cstore"):
        n = int(cid.split("_")[1])
        assert c.Cout == n and t["M"] == 15 and t["tail_len"] == n % 4 != 0
        if n < 16:
            assert not t["wide"] and t["Cout_p"] == 16 and (t["tail_block"], t["tail_group"]) == (0, 0)
        elif n == 17:
            assert not t["wide"] and t["Cout_p"] == 32 and t["grid"][1] == 2 and t["tail_block"] == 1
        else:
            assert t["wide"] and t["Cout_p"] == 64 and t["grid"][1] == 1 and (t["tail_block"], t["tail_group"]) == (0, 3)
        assert c.residual == cid.endswith("res") and c.f32 == cid.endswith("f32")
    elif cid.startswith("ties"):
        acc = R.conv_int(o["xbuf"], o["w"], 1, 0, 1)
        assert acc.min() == -300 and acc.max() == 300 and set(np.unique(acc)) == set(range(-300, 301))
        assert (o["mul"] == 0.5).all() and not o["add"].any() and o["inv_s"] == 1.0
        v = Q.qconv_v(c, o)
        if c.relu:
            assert o["lo"] == 0 and (v < 0).sum() >= 20 and (want[v < 0] == 0).all()
            n = Q.tie_counts(np.maximum(v, 0), 1.0, 0)
            assert min(n["down_pos"], n["up_pos"], n["clamp_hi"]) >= 20
        else:
            assert o["lo"] == -127 and (o["res"] is not None) == (cid == "ties_res")
            n = Q.tie_counts(v, 1.0, -127)
            assert min(n.values()) >= 20, n
            assert (want == 127).sum() >= n["clamp_hi"] and (want == -127).sum() >= n["clamp_lo"]
        print(cid, n)
    else:
        raise AssertionError("no property for " + cid)


def test_rint_differs_from_floor_half_up_on_the_tie_cases():
    """what the tie cases exist for: floor(v + 0.5) in place of rint gives other bytes on each of them"""
    for cid in ("ties", "ties_res", "ties_relu"):
        c = Q.QCONV_BY_ID[cid]
        o = Q.qconv_operands(c)
        v = Q.qconv_v(c, o)
        v = np.maximum(v, 0) if c.relu else v
        wrong = np.clip(np.floor(v + 0.5), o["lo"], 127).astype(np.int8)
        assert (wrong != Q.qconv_expected(c, o)).sum() >= 20


@pytest.mark.parametrize("cid", [c.id for c in Q.ABSMAX])
def test_absmax_case_property(cid):
    c = next(a for a in Q.ABSMAX if a.id == cid)
    buf = Q.absmax_operands(c)
    x = buf[..., c.c0:c.c0 + c.C]
    n, h, w, ld = c.shape
    assert ld % 4 == 0 and ld >= c.c0 + Q.pad4(c.C) and c.c0 % 4 == 0
    outside = np.ones(ld, bool)
    outside[c.c0:c.c0 + c.C] = False
    assert (buf[..., outside] == 1e6).all() and outside.any() == (cid[:3] != "cap")
    if c.C % 4:
        assert outside[c.c0 + c.C:c.c0 + Q.pad4(c.C)].all()                   # 1e6 inside the last group of four
    want = R.absmax(x, None, c.amax0)
    groups = n * h * w * ((c.C + 3) // 4)
    if cid.startswith("cap"):
        assert groups == 526336 > Q.STREAM_CAP * Q.STREAM_BLOCK and Q.stream_grid(groups) == Q.STREAM_CAP > Q.STREAM_BLOCK
        assert Q.stream_grid(Q.STREAM_CAP * Q.STREAM_BLOCK) == Q.STREAM_CAP == Q.stream_grid(groups - 2048)
        assert want == 7.3125
        flat = np.abs(x).reshape(-1, 32)
        row = int(np.argmax(flat.max(axis=1)))
        assert row == (n * h * w - 1 if c.peak == "last" else 0)
    elif cid == "preset":
        assert want == np.float32(1e4) > np.abs(x).max()
    else:
        assert Q.stream_grid(groups) < Q.STREAM_CAP
        assert want == 7.3125 and x.min() == -7.3125 and x.max() <= 4        # the maximum is a negative value
        assert (np.abs(x[..., c.C - 1]) == 7.3125).any()                     # in the last real channel


@pytest.mark.parametrize("cid", [c.id for c in Q.QUANTIZE])
def test_quantize_case_property(cid):
    c = next(a for a in Q.QUANTIZE if a.id == cid)
    x = Q.quantize_operands(c)
    want = R.quantize(x, c.inv_s, c.lo)
    n, h, w = c.shape
    assert x.shape == (n, h, w, c.C) and c.ldy % 4 == 0 and c.ldy >= c.C
    words = n * h * w * (c.ldy // 4)
    assert (Q.stream_grid(words) == Q.STREAM_CAP and words > Q.STREAM_CAP * Q.STREAM_BLOCK) == (cid == "cap")
    if cid == "cap":
        assert words == 528384
    if cid.startswith("tie_rows"):
        rows = want[0, :, :, :].reshape(8, -1)
        assert (rows == rows[:, :1]).all()
        lo = c.lo
        assert rows[:, 0].tolist() == [0, 2, 2, max(lo, 0), max(lo, -2), max(lo, -2), 127, lo]
    if cid == "near_ties_planes":
        v = torch.tensor(Q.NEAR_TIES, dtype=torch.float32)
        assert v.double().tolist() == Q.NEAR_TIES                             # the values are fp32 numbers
        hi = v.bfloat16().double().numpy()
        assert hi.tolist() == [0.5, 0.5, 1.5, 1.5, -2.5, -2.5]                # the hi plane sits on the tie
        planes = Q.planes_by_rounding(x)
        assert np.array_equal(planes[0, 0, :, 0, 0].double().numpy(), hi) and planes[1].abs().max() == 2.0 ** -20
        full = R.quantize(np.array(Q.NEAR_TIES), 1.0, -127).tolist()
        assert full == [1, 0, 2, 1, -2, -3]                                   # each pair goes to different integers
        assert R.quantize(hi, 1.0, -127).tolist() == [0, 0, 2, 2, -2, -2]     # the hi plane alone does not separate them
        assert want[0, :, 0, 0].tolist() == full


@pytest.mark.parametrize("cid", [c.id for c in Q.QGAP])
def test_qgap_case_property(cid):
    c = next(a for a in Q.QGAP if a.id == cid)
    buf = Q.qgap_operands(c)
    x = buf[..., :c.C]
    assert buf.shape[3] == c.C + 8 and (buf[..., c.C:] == 99).all() and c.ldy >= c.C
    want = R.qgap(x, c.s_in)
    assert want.shape == (c.N, 1, 1, c.C)
    assert c.H * c.W in (1, 2, 35) and c.N in (1, 5) and c.C in (1, 255, 256, 257, 600)
    if c.fill == "ties":
        assert c.H * c.W == 2 and c.s_in == 2.0 ** -5
        s = x.astype(np.int64).sum(axis=(1, 2))
        u = s.astype(np.float64) * c.s_in / 2.0 * (1.0 / c.s_in)
        assert set(u.ravel().tolist()) == {0.5, 1.5, -0.5, -1.5}
        assert set(zip(u.ravel().tolist(), want.ravel().tolist())) == {(0.5, 0), (1.5, 2), (-0.5, 0), (-1.5, -2)}
    if c.fill == "min":
        assert (x == -128).all() and (want == -127).all()
    # a pitch taken for a width reads other bytes: the restatement of the buffer read with ldx = C differs
    if c.H * c.W > 1 or c.N > 1:
        flat = buf.reshape(-1)[:c.N * c.H * c.W * c.C].reshape(c.N, c.H, c.W, c.C)
        assert not np.array_equal(R.qgap(flat, c.s_in), want)


def test_qgap_cases_cover_the_issue():
    assert {c.C for c in Q.QGAP} == {1, 255, 256, 257, 600} and {c.H * c.W for c in Q.QGAP} == {1, 2, 35}
    assert {c.N for c in Q.QGAP} == {1, 5} and any(c.ldy > c.C for c in Q.QGAP)
    assert [(c.C + 255) // 256 for c in Q.QGAP] == [1, 1, 1, 2, 3, 3]        # blocks along the channels


@pytest.mark.parametrize("cid", [c.id for c in Q.QBCAST])
def test_qbcast_case_property(cid):
    c = next(a for a in Q.QBCAST if a.id == cid)
    words = c.N * c.H * c.W * (c.C // 4)
    assert c.C % 4 == 0 and c.ldv % 4 == 0 and c.ldv >= c.C
    assert (words > Q.STREAM_CAP * Q.STREAM_BLOCK) == (cid == "cap")
    assert {"c4": c.C == 4, "ldv": c.ldv > c.C, "hw1": c.H * c.W == 1, "cap": words == 528384}[cid]


@pytest.mark.parametrize("cid", [c.id for c in Q.QBILINEAR])
def test_qbilinear_case_property(cid):
    c = next(a for a in Q.QBILINEAR if a.id == cid)
    x = Q.qbilinear_operands(c)
    want = R.qbilinear(x, c.s_in, c.Ho, c.Wo, c.inv_s)
    assert want.shape == (c.N, c.Ho, c.Wo, c.C) and c.C in (4, 260)
    if cid == "identity":
        assert (c.Hi, c.Wi) == (c.Ho, c.Wo) and c.s_in * c.inv_s == 1.0 and x.min() == -127 and np.array_equal(want, x)
    else:
        assert x.min() == -128
    if cid.startswith("down"):
        assert c.Ho < c.Hi and c.Wo < c.Wi
    if cid == "mixed_5x9_13x4":
        assert c.Ho > c.Hi and c.Wo < c.Wi and c.Hi * c.Wo != c.Wi * c.Ho
    if cid == "src_1x6":
        assert c.Hi == 1 and (want == want[:, :1]).all()
    if cid == "src_6x1":
        assert c.Wi == 1 and (want == want[:, :, :1]).all()
    if cid == "src_1x1":
        assert np.array_equal(want, np.broadcast_to(R.quantize(x.astype(np.float64) * c.s_in, c.inv_s, -127), want.shape))
    if cid == "dst_1x1":
        assert (c.Ho, c.Wo) == (1, 1)


def test_network_and_scene_cases():
    assert {(os_, n) for os_, n, _, _ in Q.NETWORK} == {(16, 1), (16, 3), (8, 1), (8, 3)}
    for os_, n, h, w in Q.NETWORK:
        side = lambda v: (v - 1) // os_ + 1                                  # noqa: E731
        if os_ == 16:                                                        # the layer4 map: 3 x 3 or 3 x 4
            assert side(h) == 3 and side(w) in (3, 4) and n * side(h) * side(w) <= 36
            assert 12 >= side(w) and 18 >= side(w)                           # rates 12 and 18 are centre-only
    from tests import scene_ref as S
    p = S.Plan(Q.SCENE["H"], Q.SCENE["W"], Q.SCENE["tile"], Q.SCENE["overlap"])
    nwin = len(list(p.windows()))
    assert nwin == Q.SCENE["windows"] == 6 and (p.th, p.tw) == (65, 65)
    # window batches of 1: six one-window calls; 4: a full batch and a short one; 6: the whole scene at once
    assert [(nwin + b - 1) // b for b in Q.SCENE["tile_batches"]] == [6, 2, 1] and nwin % 4 == 2
