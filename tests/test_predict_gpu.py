"""Inference on the GPU (iswm_amd/csrc/predict.hip, forward_lowres, iswm_amd/predict.py) against the CPU restatement
tests/predict_ref.py: normalisation bit-exact, the fused maps against the restatement on the device's own unfused
logits, the low-resolution hook against forward(), and the command line end to end against the fp64 oracle."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import predict_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


@pytest.mark.parametrize("hw", [(1, 1), (37, 53), (97, 129)])
def test_predict_normalize_bit_exact(hw):
    from iswm_amd import ops
    rng = np.random.default_rng(hw[0])
    img = rng.integers(0, 256, (2,) + hw + (3,), dtype=np.uint8)
    img[0, 0, 0] = (0, 255, 128)
    got = ops.predict_normalize(torch.from_numpy(img).to(dev()), R.MEAN, R.STD).cpu()
    want = torch.stack([R.normalize(im) for im in img])
    assert got.shape == want.shape and torch.equal(got, want)


def _logits(n, h, w, c, ld, seed):
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


SHAPES = [((1, 1), (1, 1)), ((9, 9), (33, 33)), ((17, 23), (65, 93)), ((33, 33), (129, 129))]
CUTS = [(0.5, 0.2, 0.7), (0.5, 0.5, 0.5), (0.3, 0.7, 0.2), (0.2, 0.0, 1.0)]


# (C, fg, pitch): C <= 3 are the binary model's shapes; C = 5, 16 keep 2 and 4 float4 groups of logits in registers
# (G = 2, 4) and C = 17 takes the two-pass path (G = 0)
CASES = [(c, fg, 8, lo_hi) for c, fg in [(2, 1), (3, 1), (3, 2)] for lo_hi in SHAPES] + \
        [(c, fg, ld, lo_hi) for c, fg, ld in [(5, 4, 8), (16, 3, 16), (17, 16, 20)] for lo_hi in SHAPES[1:3]]


@pytest.mark.parametrize("c,fg,ld,lo_hi", CASES)
def test_predict_maps_against_restatement(c, fg, ld, lo_hi):
    from iswm_amd import ops
    (hl, wl), (H, W) = lo_hi
    n = 3
    yl = _logits(n, hl, wl, c, ld, seed=hl * 31 + c * 7 + fg).to(dev())
    lg = ops.bilinear_to_nchw_fwd(yl, c, H, W).cpu().double().numpy()      # the unfused path's own logits
    p64 = R.softmax_fg(lg, fg)
    npix = n * H * W
    for thr, mn, mx in CUTS:
        m = ops.predict_maps(yl, c, fg, H, W, thr, mn, mx, want_prob=True)
        m2 = ops.predict_maps(yl, c, fg, H, W, thr, mn, mx, want_prob=True)
        assert all(torch.equal(a, b) for a, b in zip(m[:5], m2[:5])), "not reproducible"
        prob = m.prob.cpu().numpy()
        pred, conf, band = (t.cpu().numpy() for t in (m.pred, m.conf, m.band))
        stats = m.stats.cpu().numpy()
        assert np.abs(prob.astype(np.float64) - p64).max() <= 1e-6
        pred_r, conf_r = R.predict_mask(p64, thr)
        band_r = R.binarize_confidence_map(conf_r, mn, mx)
        edge = R.near_boundary(p64, thr, 2e-6)
        bad = (pred != pred_r) | (conf != conf_r) | (band != band_r)
        assert not (bad & ~edge).any(), "mismatch away from a decision boundary"
        # p -> 1: the fp32 sum 1 + e rounds to 1 once e < 2^-24, so the kernel (like any fp32 softmax) gives p = 1 where
        # the correctly rounded fp64 p is 1 - 2^-24 (conf 255 against 254); counted apart.  The rest is the rounding of
        # the fp32 sum next to an integer of p * 255: observed at most 7 of 49 923 pixels (1.4e-4) for C = 3; a sum of
        # more classes rounds more often
        absorbed = bad & (prob == 1.0)
        print("predict_maps C=%d fg=%d %dx%d->%dx%d thr=%g band=[%g,%g]: %d boundary pixels, %d differ "
              "(%d of them p = 1 in fp32)" % (c, fg, hl, wl, H, W, thr, mn, mx, int(edge.sum()), int(bad.sum()),
                                              int(absorbed.sum())))
        assert (bad & ~absorbed).sum() <= (2e-4 if c <= 3 else 1e-3) * npix + 2
        # the kernel's maps follow from its own p exactly
        p32 = prob.astype(np.float32)
        assert np.array_equal(pred, R.predict_mask(p32, thr)[0])
        assert np.array_equal(conf, R.predict_mask(p32, thr)[1])
        assert np.array_equal(band, R.binarize_confidence_map(conf, mn, mx))
        for k in range(n):
            ref = R.prob_stats(p64[k], thr)
            own = R.prob_stats(p32[k], thr)
            assert stats[k, 0] == own[0] and stats[k, 1] == own[1]
            # 1 ulp of fp64, or 1e-5 relative in the saturated tail (p ~ 1e-14: l - m ~ -60 carries fp32 rounding)
            for j in (0, 1):
                assert abs(stats[k, j] - ref[j]) <= max(np.spacing(np.float32(ref[j])), 1e-5 * abs(ref[j])), (k, j)
            assert abs(stats[k, 2] - ref[2]) <= 1e-6 * abs(ref[2]) + 1e-12
            assert stats[k, 3] == own[3] and stats[k, 4] == own[4] == (pred[k] == 255).sum()
            nb = int(edge[k].sum())
            assert abs(stats[k, 3] - ref[3]) <= nb and abs(stats[k, 4] - ref[4]) <= nb


def _r50():
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    sd = synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, 16))
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval(), sd


def test_forward_lowres_pin():
    from iswm_amd import ops
    m, _ = _r50()
    x = torch.from_numpy(np.random.default_rng(5).standard_normal((2, 3, 97, 129)).astype(np.float32)).to(dev())
    with torch.no_grad():
        full = m(x)
        yl = m.forward_lowres(x)
        again = ops.bilinear_to_nchw_fwd(yl, 2, 97, 129)
    assert yl.shape[0] == 2 and yl.shape[3] == 4 and yl.stride(3) == 1
    assert torch.equal(full, again)
    with pytest.raises(RuntimeError, match="no_grad"):
        m.forward_lowres(x)


def _spread_head(m, sd, x):
    """scale and centre the final 1x1 classifier so that p spreads over (0, 1) on x: std(l1 - l0) = 3"""
    with torch.no_grad():
        yl = m.forward_lowres(x)
    d = (yl[..., 1] - yl[..., 0]).double()
    s = 3.0 / float(d.std())
    sd = dict(sd)
    w, b = sd["classifier.classifier.6.weight"].clone(), sd["classifier.classifier.6.bias"].clone()
    sd["classifier.classifier.6.weight"] = w * s
    b = b * s
    b[1] -= float(d.mean()) * s
    sd["classifier.classifier.6.bias"] = b
    return sd


def _frames(root):
    inp = os.path.join(root, "frames")
    rng = np.random.default_rng(11)
    files = {"s1": [("a.png", 65, 65), ("b.jpg", 65, 65), ("c.png", 97, 129)],
             "s2": [("d.jpg", 97, 129), ("e.png", 97, 129)]}
    for sub, items in files.items():
        os.makedirs(os.path.join(inp, sub))
        for name, h, w in items:
            base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
            im = Image.fromarray(base).resize((w, h), Image.BILINEAR)          # smooth content, like a frame
            im.save(os.path.join(inp, sub, name))
    with open(os.path.join(inp, "s2", "broken.png"), "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n truncated")
    return inp, files


def test_predict_cli_end_to_end(tmp_path, capsys):
    from iswm_amd import predict
    from iswm_amd.predict import decode_image
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg
    m, sd = _r50()
    inp, files = _frames(str(tmp_path))
    x0 = R.normalize(decode_image(os.path.join(inp, "s1", "c.png")))[None].to(dev())
    sd = _spread_head(m, sd, x0)
    ckpt = os.path.join(str(tmp_path), "ref_format.pth")
    torch.save({"model_state": {"module." + k: v for k, v in sd.items()}}, ckpt)

    outs = {}
    for bs in (2, 1):
        out = os.path.join(str(tmp_path), "out%d" % bs)
        n = predict.main(["--input", inp, "--ckpt", ckpt, "--save_val_results_to", out, "--save_confidence",
                          "--save_binary", "--batch_size", str(bs), "--workers", "2"])
        text = capsys.readouterr().out
        assert n == 5
        assert "Model loaded from" in text and "broken.png" in text and "Error while processing" in text
        assert text.count("Foreground probability: min=") == 5
        outs[bs] = out

    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = OracleDeepLab(ArchCfg("deeplabv3plus", "resnet50", 2, 16), sd64, dropout_p=0.0).eval()
    npix = nedge = nbad = nfg = 0
    same_maps = True
    for sub, items in files.items():
        for name, h, w in items:
            base = os.path.splitext(name)[0]
            maps = {}
            for bs, out in outs.items():
                for kind in ("predict", "confidence", "binary_mask"):
                    im = Image.open(os.path.join(out, sub, "%s_%s.png" % (base, kind)))
                    assert im.mode == "L" and im.size == (w, h)
                    maps[bs, kind] = np.asarray(im)
            same_maps &= all(np.array_equal(maps[1, k], maps[2, k]) for k in ("predict", "confidence", "binary_mask"))
            x = R.normalize(decode_image(os.path.join(inp, sub, name)))[None]
            with torch.no_grad():
                lg = oracle(x.double()).numpy()
            p64 = R.softmax_fg(lg, 1)[0]
            pred_r, conf_r = R.predict_mask(p64, 0.5)
            band_r = R.binarize_confidence_map(conf_r, 0.2, 0.7)
            pred, conf, band = maps[2, "predict"], maps[2, "confidence"], maps[2, "binary_mask"]
            assert np.abs(conf.astype(int) - conf_r.astype(int)).max() <= 1, (sub, name)
            edge = R.near_boundary(p64, 0.5, 1e-4)
            bad = (pred != pred_r) | (band != band_r)
            assert not (bad & ~edge).any(), (sub, name)
            nfg += int((pred == 255).sum())
            npix += p64.size
            nedge += int(edge.sum())
            nbad += int(bad.sum())
    print("predict CLI vs fp64 oracle: %d pixels, %d near a boundary, %d differ; batch 1 and 2 maps %s" %
          (npix, nedge, nbad, "bit-identical" if same_maps else "differ"))
    assert nbad <= 1e-3 * npix
    assert 0.05 < nfg / npix < 0.95, "probabilities do not spread"

    # the same frames through the model directly: batch 2 against batch 1
    m.load_state_dict(sd, strict=True)
    from iswm_amd import ops
    pair = [decode_image(os.path.join(inp, "s2", f)) for f in ("d.jpg", "e.png")]
    img = torch.from_numpy(np.stack(pair)).to(dev())
    with torch.no_grad():
        x = ops.predict_normalize(img, R.MEAN, R.STD)
        y2 = m.forward_lowres(x)[..., :2].cpu()
        y1 = torch.cat([m.forward_lowres(x[k:k + 1])[..., :2].cpu() for k in range(2)])
    err = float((y2 - y1).abs().max())
    print("forward_lowres batch 2 vs batch 1: max |diff| %.3e (%s)" % (err, "bit-identical" if err == 0 else "differ"))
    assert err <= 1e-5 * float(y1.abs().max())


def test_predict_without_checkpoint(tmp_path, capsys):
    from iswm_amd import predict
    inp = os.path.join(str(tmp_path), "in", "seq")
    os.makedirs(inp)
    Image.fromarray(np.random.default_rng(3).integers(0, 256, (33, 33, 3), dtype=np.uint8)).save(
        os.path.join(inp, "f.png"))
    out = os.path.join(str(tmp_path), "out")
    n = predict.main(["--input", os.path.dirname(inp), "--save_val_results_to", out])
    assert n == 1
    assert "[!] No checkpoint found" in capsys.readouterr().out
    assert os.listdir(os.path.join(out, "seq")) == ["f_predict.png"]
