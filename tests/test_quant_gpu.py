"""INT8 inference on the GPU (csrc/qconv.hip, csrc/quant.hip, iswm_amd/quant.py) against the numpy restatement
tests/quant_ref.py: every kernel and the whole network bit-exact, calibration against torch on captured tensors, and
the int8-vs-fp32 agreement reported and bounded."""
import numpy as np
import pytest
import torch

from tests import quant_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def _qconv(x, w, mul, add, k, stride, pad, dil, relu, lo, inv_s, **kw):
    from iswm_amd import ops
    cout_p = (w.shape[0] + 15) // 16 * 16
    wp = np.zeros((cout_p, k, k, x.shape[3]), np.int8)
    wp[:w.shape[0], :, :, :w.shape[1]] = w.transpose(0, 2, 3, 1)
    m = np.zeros(cout_p)
    a = np.zeros(cout_p)
    m[:w.shape[0]], a[:w.shape[0]] = mul, add
    t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev())     # noqa: E731
    return ops.qconv_fwd(t(x), t(wp.reshape(cout_p, -1)), t(m), t(a), k, stride, pad, dil, relu, lo, inv_s,
                         cstore=w.shape[0], **kw)


def test_mfma_lane_map():
    """identity weights return the input channels; an asymmetric integer B catches any row / column swap"""
    rng = np.random.default_rng(0)
    x = rng.integers(-100, 101, (1, 5, 7, 64)).astype(np.int8)
    w = np.zeros((16, 64, 1, 1), np.int8)
    for c in range(16):
        w[c, 3 * c + 1, 0, 0] = 1
    got = _qconv(x, w, np.ones(16), np.zeros(16), 1, 1, 0, 1, False, -127, 1.0, out_f32=True).cpu().numpy()
    assert np.array_equal(got, x[..., 1:48:3].astype(np.float32))
    w = (np.arange(16)[:, None] * 7 + np.arange(64)[None, :] * 3) % 11 - 5
    w = w.astype(np.int8)[:, :, None, None]
    got = _qconv(x, w, np.ones(16), np.zeros(16), 1, 1, 0, 1, False, -127, 1.0, out_f32=True).cpu().numpy()
    assert np.array_equal(got, R.conv_int(x, w, 1, 0, 1).astype(np.float32))


GRID = [  # (N, H, W, Cin, Cout, k, stride, dil, relu, residual, f32)
    (1, 33, 33, 64, 16, 1, 1, 1, True, False, False),
    (3, 33, 33, 256, 256, 1, 1, 1, True, True, False),
    (1, 65, 65, 64, 48, 3, 1, 1, True, False, False),
    (3, 33, 33, 256, 256, 3, 1, 2, True, False, False),
    (1, 33, 33, 256, 256, 3, 1, 6, True, False, False),
    (1, 33, 33, 320, 256, 3, 1, 18, True, False, False),
    (3, 65, 65, 64, 256, 3, 2, 1, True, False, False),
    (1, 97, 129, 256, 256, 1, 2, 1, False, False, False),
    (1, 97, 129, 320, 256, 3, 1, 1, True, False, False),
    (3, 65, 65, 256, 16, 1, 1, 1, False, False, True),
    (1, 33, 33, 256, 48, 1, 1, 1, True, True, False),
    (3, 97, 129, 64, 256, 3, 1, 1, False, True, False),
    (1, 33, 33, 256, 10, 1, 1, 1, False, False, True),      # cstore % 4 != 0: the per-element tail stores
    (3, 33, 33, 64, 6, 3, 1, 2, True, True, False),
]


@pytest.mark.parametrize("case", GRID)
def test_qconv_bit_exact(case):
    n, h, w_, cin, cout, k, stride, dil, relu, has_res, f32 = case
    rng = np.random.default_rng(hash(case) & 0xFFFF)
    x = rng.integers(-127, 128, (n, h, w_, cin)).astype(np.int8)
    if relu:
        x = np.abs(x).astype(np.int8)
    w = rng.integers(-127, 128, (cout, cin, k, k)).astype(np.int8)
    pad = dil * (k - 1) // 2
    mul = rng.uniform(1e-6, 1e-5, cout)
    add = rng.normal(0, 0.05, cout)
    ho = (h + 2 * pad - dil * (k - 1) - 1) // stride + 1
    wo = (w_ + 2 * pad - dil * (k - 1) - 1) // stride + 1
    acc = R.conv_int(x, w, stride, pad, dil)
    lo = 0 if relu else -127
    inv = 127.0 / 2.0
    res = rng.integers(-127, 128, (n, ho, wo, cout)).astype(np.int8) if has_res else None
    if has_res:                                                  # a pitched residual: ldr % 4 == 0
        rbuf = np.zeros((n, ho, wo, (cout + 3) // 4 * 4), np.int8)
        rbuf[..., :cout] = res
    want = R.epilogue(acc, mul, add, relu, None if f32 else inv, lo, res, 0.013)
    # into a pitched slice with sentinels in the neighbouring channels
    ld = (cout + 3) // 4 * 4 + 32
    if f32:
        buf = torch.full((n, ho, wo, ld), 7.0, device=dev())
    else:
        buf = torch.full((n, ho, wo, ld), 55, dtype=torch.int8, device=dev())
    out = buf[..., 16:16 + cout]
    tres = torch.from_numpy(rbuf).to(dev())[..., :cout] if has_res else None
    _qconv(x, w, mul, add, k, stride, pad, dil, relu, lo, inv, out=out, res=tres, s_res=0.013, out_f32=f32)
    b = buf.cpu().numpy()
    assert np.array_equal(b[..., 16:16 + cout], want)
    sentinel = 7.0 if f32 else 55
    assert (b[..., :16] == sentinel).all() and (b[..., 16 + cout:] == sentinel).all()


def test_absmax_matches_torch():
    from iswm_amd import ops
    g = torch.Generator().manual_seed(3)
    x = (torch.randn((2, 17, 19, 304), generator=g) * 3).to(dev())
    buf = torch.zeros((2, 17, 19, 320), device=dev())
    buf[..., :304] = x
    buf[..., 304:] = 1e6                                       # past the real channels: ignored
    a = torch.zeros((1,), device=dev())
    ops.absmax(buf, a, 304)
    assert a.item() == x.abs().max().item()
    p = ops.split_planes(torch.randn((2, 9, 11, 256), generator=g).to(dev()) * 5)
    a2 = torch.zeros((1,), device=dev())
    ops.absmax(p, a2)
    assert a2.item() == p.f32().abs().max().item()
    ops.absmax(p, a)                                           # max-accumulates
    assert a.item() == max(x.abs().max().item(), a2.item())


def test_small_kernels_bit_exact():
    from iswm_amd import ops
    rng = np.random.default_rng(5)
    xf = torch.from_numpy(rng.normal(0, 2, (2, 13, 15, 64)).astype(np.float32))
    xf[0, 0, 0, :4] = torch.tensor([0.5, 1.5, -2.5, 1e3])      # ties at scale 1 and a clamp
    inv = 1.0
    q = ops.quantize_i8(xf.to(dev()), inv, -127).cpu().numpy()
    assert np.array_equal(q, R.quantize(xf.numpy(), inv, -127))
    inv = 127.0 / 5.3
    q = ops.quantize_i8(ops.split_planes(xf.to(dev())), inv, 0, ldy=128).cpu().numpy()
    assert np.array_equal(q[..., :64], R.quantize(xf.numpy(), inv, 0)) and not q[..., 64:].any()
    xi = rng.integers(0, 128, (3, 9, 11, 256)).astype(np.int8)
    s_in = 0.037
    g = ops.qgap(torch.from_numpy(xi).to(dev()), s_in, 1.0 / s_in).cpu().numpy()
    assert np.array_equal(g, R.qgap(xi, s_in))
    v = torch.from_numpy(rng.integers(-127, 128, (3, 1, 1, 256)).astype(np.int8)).to(dev())
    buf = torch.full((3, 9, 11, 320), 9, dtype=torch.int8, device=dev())
    ops.qbcast(v, buf[..., 32:288])
    b = buf.cpu().numpy()
    assert (b[..., 32:288] == v.cpu().numpy()).all() and (b[..., :32] == 9).all() and (b[..., 288:] == 9).all()
    for (hi, wi, ho, wo) in [(9, 11, 33, 41), (17, 17, 65, 65), (25, 33, 97, 129)]:
        xa = rng.integers(0, 128, (2, hi, wi, 256)).astype(np.int8)
        dst = torch.full((2, ho, wo, 320), 3, dtype=torch.int8, device=dev())
        ops.qbilinear(torch.from_numpy(xa).to(dev()), 0.021, 127.0 / 2.9, dst[..., 48:304])
        d = dst.cpu().numpy()
        assert np.array_equal(d[..., 48:304], R.qbilinear(xa, 0.021, ho, wo, 127.0 / 2.9))
        assert (d[..., :48] == 3).all() and (d[..., 304:] == 3).all()


def _model(name, bb, os_, seed=0):
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    cfg = ArchCfg(name, bb, 2, os_)
    m = getattr(modeling, "%s_%s" % (name, bb))(num_classes=2, output_stride=os_, pretrained_backbone=False)
    m.load_state_dict(synth_state_dict(cfg, salt=seed), strict=True)
    return m.to(dev()).eval()


def _images(n, h, w, seed):
    from oracle.synth import synth_images
    return synth_images(n, h, w, seed=seed).to(dev())


@pytest.mark.parametrize("name,bb,os_,hw", [("deeplabv3plus", "resnet50", 16, (65, 65)),
                                            ("deeplabv3plus", "resnet50", 16, (97, 129)),
                                            ("deeplabv3", "resnet50", 8, (97, 129)),
                                            ("deeplabv3plus", "resnet101", 16, (65, 65))])
def test_network_bit_exact(name, bb, os_, hw, tmp_path):
    from iswm_amd import quant
    m = _model(name, bb, os_)
    amax = quant.calibrate(m, [_images(2, hw[0], hw[1], s) for s in (1, 2)])
    qm = quant.quantize_model(m, amax)
    x = _images(2, hw[0], hw[1], 7)
    with torch.no_grad():
        q = qm.stem(x)
        yl = qm.body(q)
        assert torch.equal(qm.forward_lowres(x), yl)
        one = torch.cat([qm.forward_lowres(x[i:i + 1]) for i in range(2)])
    assert torch.equal(one, yl)                                   # batch 2 == two batch-1 calls
    st = qm.state_int8()
    want = R.forward_body(st, q.cpu().numpy())
    got = yl.cpu().numpy()
    assert got.shape[:3] == want.shape[:3] and got.shape[3] == 4
    assert np.array_equal(got[..., :2], want), np.abs(got[..., :2] - want).max()
    # the fold restated from the fp32 module for every conv
    for k, r in st["convs"].items():
        conv = m.get_submodule(k)
        bn = quant._bn_of(m, k)
        if bn is None:
            wr, br = conv.weight.detach().cpu().double().numpy(), conv.bias.detach().cpu().double().numpy()
        else:
            wr, br = R.fold_bn(conv.weight.detach().cpu().double().numpy(), bn.weight.detach().cpu().numpy(),
                               bn.bias.detach().cpu().numpy(), bn.running_mean.cpu().numpy(), bn.running_var.cpu().numpy(),
                               bn.eps)
        qr, sr = R.quantize_weight(wr)
        assert np.array_equal(r["w"].numpy(), qr) and np.array_equal(r["s_w"].numpy(), sr) and np.array_equal(r["b"].numpy(), br)
    # save / load round trip
    p = tmp_path / "m_int8.pth"
    qm.save_int8(str(p))
    q2 = quant.load_int8(str(p))
    with torch.no_grad():
        assert torch.equal(q2.forward_lowres(x), yl)
    assert qm.forward(x).shape == (2, 2) + hw


def test_calibration_equals_captured_tensors():
    from iswm_amd import ops, quant
    m = _model("deeplabv3plus", "resnet50", 16)
    seen = {}

    class Capture(quant.AmaxRecorder):
        def record(self, module, t, c=None):
            super().record(module, t, c)
            name = self.names[module] + (".cat" if isinstance(module, (quant.ASPP, quant.DeepLabHeadV3Plus)) else "")
            if c is None and isinstance(module, torch.nn.Conv2d):
                c = module.out_channels
            v = ops.as_f32(t)[..., :c].abs().max().item()
            seen[name] = max(seen.get(name, 0.0), v)

    rec = Capture(m)
    with torch.no_grad(), quant.calibrating(m, rec):
        for s in (1, 2):
            m.forward_lowres(_images(2, 65, 65, s))
    got = rec.result()
    assert set(got) == set(seen) and "classifier.aspp.cat" in got and "classifier.cat" in got and "backbone.maxpool" in got
    for k in got:
        assert got[k] == np.float32(seen[k]), k


def test_quantization_error_bounded():
    """int8 vs fp32 on the same frames: pred agreement next to the foreground fraction, and logits SQNR"""
    from iswm_amd import ops, quant
    m = _model("deeplabv3plus", "resnet50", 16)
    amax = quant.calibrate(m, [_images(4, 129, 129, s) for s in range(3)])
    qm = quant.quantize_model(m, amax)
    x = _images(4, 129, 129, 11)
    with torch.no_grad():
        lf = m.forward_lowres(x)[..., :2]
        lq = qm.forward_lowres(x)[..., :2]
        pf = ops.predict_maps(m.forward_lowres(x), 2, 1, 129, 129, 0.5, 0.2, 0.7).pred
        pq = ops.predict_maps(qm.forward_lowres(x), 2, 1, 129, 129, 0.5, 0.2, 0.7).pred
    agree = (pf == pq).float().mean().item()
    fg = (pf > 0).float().mean().item()
    fg_iou = ((pf > 0) & (pq > 0)).sum().item() / max(1, ((pf > 0) | (pq > 0)).sum().item())
    sqnr = 10 * np.log10((lf.double() ** 2).sum().item() / ((lf.double() - lq.double()) ** 2).sum().item())
    print("int8 vs fp32: pred agreement %.4f (fp32 foreground fraction %.4f), foreground IoU %.4f, logits SQNR %.2f dB" %
          (agree, fg, fg_iou, sqnr))
    # first MI355X run: agreement 0.9935 at a foreground fraction of 0.0204, foreground IoU 0.7116, SQNR 24.05 dB
    # (DESIGN.md section 10); the
    # foreground IoU bound catches an INT8 model that loses the (small) foreground, which the agreement alone would not
    assert fg > 0.01 and agree > 0.98 and sqnr > 20.0 and fg_iou > 0.65


def test_predict_cli_with_int8_checkpoint(tmp_path, capsys):
    """predict --ckpt <x>_int8.pth runs the quantized model and writes the same masks as forward_lowres + predict_maps"""
    import os

    from PIL import Image

    from iswm_amd import ops, predict, quant
    from iswm_amd.predict import decode_image
    from tests import predict_ref as P
    m = _model("deeplabv3plus", "resnet50", 16)
    qm = quant.quantize_model(m, quant.calibrate(m, [_images(2, 65, 65, 1)]))
    ckpt = str(tmp_path / "m_int8.pth")
    qm.save_int8(ckpt)
    inp = tmp_path / "in" / "s1"
    inp.mkdir(parents=True)
    rng = np.random.default_rng(2)
    for k, (h, w) in enumerate([(65, 65), (70, 90)]):
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(inp / ("f%d.png" % k)))
    out = str(tmp_path / "out")
    n = predict.main(["--input", str(tmp_path / "in"), "--ckpt", ckpt, "--save_val_results_to", out])
    text = capsys.readouterr().out
    assert n == 2 and "INT8 model loaded from" in text
    for k in range(2):
        im = decode_image(str(inp / ("f%d.png" % k)))
        x = P.normalize(im)[None].to(dev())
        with torch.no_grad():
            want = ops.predict_maps(qm.forward_lowres(x), 2, 1, im.shape[0], im.shape[1], 0.5, 0.2, 0.7).pred
        got = np.asarray(Image.open(os.path.join(out, "s1", "f%d_predict.png" % k)))
        assert np.array_equal(got, want[0].cpu().numpy())


def test_calibration_hook_inert_when_off(monkeypatch):
    """with no calibration running, an FP32 eval forward makes the same library calls before and after a calibration,
    none of them a range measurement, and the classifier stays fused into its BatchNorm pass"""
    from iswm_amd import ops, quant
    m = _model("deeplabv3plus", "resnet50", 16)
    x = _images(2, 65, 65, 4)
    with torch.no_grad():
        m.forward_lowres(x)                                    # one-time setup (plans, packers) out of the comparison
    real = ops.call
    seq = []

    def spy(name, *a):
        seq.append(name)
        return real(name, *a)

    monkeypatch.setattr(ops, "call", spy)
    with torch.no_grad():
        y0 = m.forward_lowres(x)
        before = list(seq)
        seq.clear()
        quant.calibrate(m, [x])
        during = list(seq)
        seq.clear()
        y1 = m.forward_lowres(x)
        after = list(seq)
    assert before == after and torch.equal(y0, y1)
    assert "iswm_absmax" not in before and "iswm_bn_apply_classify" in before
    assert "iswm_absmax" in during and "iswm_bn_apply_classify" not in during


def test_evaluator_cli_end_to_end(tmp_path, capsys):
    import os

    from PIL import Image

    from iswm_amd import evaluate_quantization as E
    from iswm_amd import quant
    from oracle.synth import ArchCfg, synth_state_dict
    sd = synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, 16))
    ckpt = str(tmp_path / "best.pth")
    torch.save({"model_state": {"module." + k: v for k, v in sd.items()}, "best_score": {"Mean IoU": np.float64(0.1)}},
               ckpt)
    d = tmp_path / "val"
    (d / "imgs").mkdir(parents=True)
    (d / "masks").mkdir()
    rng = np.random.default_rng(9)
    for k in range(6):
        h, w = 65, 81
        Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(str(d / "imgs" / ("f%d.png" % k)))
        if k != 2:
            Image.fromarray((rng.random((h, w)) < 0.3).astype(np.uint8) * 255).save(str(d / "masks" / ("f%d_mask.png" % k)))
    res = str(tmp_path / "res")
    r = E.main(["--fp32_ckpt", ckpt, "--eval_data_dir", str(d), "--num_images", "5", "--num_visualizations", "3",
                "--results_dir", res])
    text = capsys.readouterr().out
    print(text)
    for row in ("Avg. Inference Time (ms)", "Model Size (MB)", "Mean IoU (mIoU)", "Foreground IoU", "Foreground F1",
                "Evaluated on 5 images."):
        assert row in text
    assert r["int8_ckpt"] == str(tmp_path / "best_int8.pth") and os.path.isfile(r["int8_ckpt"])
    assert quant.read_checkpoint(r["int8_ckpt"])[0] is not None
    assert sorted(os.listdir(res)) == ["f0_comparison.png", "f1_comparison.png", "f2_comparison.png"]
    for k in ("fp32", "int8"):
        assert 0.0 <= r["scores"][k]["MIoU"] <= 1.0
    Image.fromarray(np.zeros((30, 40, 3), np.uint8)).save(str(d / "imgs" / "f9.png"))
    with pytest.raises(ValueError, match="share one size"):
        E.main(["--fp32_ckpt", ckpt, "--eval_data_dir", str(d), "--results_dir", res])
