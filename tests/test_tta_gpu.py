"""Flip and multi-scale test-time augmentation on the GPU (k_predict_view_normalize, k_predict_views_maps,
iswm_amd.predict.TTAPredictor) against the CPU restatements tests/tta_ref.py and tests/predict_ref.py: the identity
and mirror views bit-exact, resampled views against float64 at a derived bound, the averaged maps against the
restatement on the device's own unfused per-view logits, one identity view against predict_maps byte for byte, and
the command line end to end against the fp64 oracle run per view."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from PIL import Image

from tests import predict_ref as R
from tests import scene_cases as SC
from tests import tta_ref as T
from tests.test_scene_gpu import KINDS, _frames, _r50, _spread_head

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def _images(n, h, w):
    rng = np.random.default_rng(h * 7 + w)
    img = rng.integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    img[0, 0, 0] = (0, 255, 128)
    img[-1, -1, -1] = (255, 0, 255)
    return img


VIEW_FRAMES = [(1, 1), (37, 53), (97, 129)]
# the largest source extent of VIEW_FRAMES: the product scale * (dst + 0.5) of src_index stays below 256
VIEW_BOUND = (6 * 2.0 ** -17 / 255 + 2 * 2.0 ** -25) / 0.224 + 2.0 ** -23 + 2 * 2.0 ** -16 / 0.224


@pytest.mark.parametrize("hw", VIEW_FRAMES)
def test_view_normalize_identity_and_mirror_bit_exact(hw):
    from iswm_amd import ops
    H, W = hw
    img = _images(2, H, W)
    d = torch.from_numpy(img).to(dev())
    want = ops.predict_normalize(d, R.MEAN, R.STD)
    assert torch.equal(want.cpu(), torch.stack([R.normalize(f) for f in img]))
    got = ops.predict_view_normalize(d, H, W, False, R.MEAN, R.STD)
    assert got.shape == want.shape and torch.equal(got, want)
    mirrored = ops.predict_normalize(torch.from_numpy(img[:, :, ::-1].copy()).to(dev()), R.MEAN, R.STD)
    got = ops.predict_view_normalize(d, H, W, True, R.MEAN, R.STD)
    assert torch.equal(got, mirrored) and torch.equal(got, want.flip(-1))


@pytest.mark.parametrize("hw", VIEW_FRAMES)
def test_view_normalize_against_float64(hw):
    """Resampled views against tta_ref.view_normalize64 (the taps of scene_cases._taps in fp32, the rest in fp64).
    The bound, from the operations k_predict_view_normalize writes, for frames up to 129 pixels a side:
      * the three lerps: each is two products and a sum of values <= 255, at most three roundings of half an ulp
        (2^-17) each, fewer where the compiler contracts; the errors of the two horizontal lerps enter the vertical
        one with weights that sum to 1, so v is within 6 * 2^-17 of the fp64 value on the same taps; divided by 255 and
        by the smallest std, 0.224;
      * v / 255 and the subtraction of the mean, one rounding each of a value <= 1 (2^-25), divided by 0.224, and the
        rounding of the last division on |x| <= 2.7 (2^-23);
      * the source coordinate: src_index writes scale * (dst + 0.5f) - 0.5f and hipcc contracts it to one fma, while
        _taps rounds the product first.  Both are within half an ulp of the exact value -- the product's ulp for
        _taps, the result's for the fma -- so they differ by at most one ulp of a product below 256, 2^-16, per axis.
        The bilinear surface of values <= 255 changes by at most 255 per unit of either coordinate (continuously
        across integer coordinates and the clamp), so v moves by at most 2 * 255 * 2^-16, again over 255 * 0.224.
    (6 * 2^-17 / 255 + 2 * 2^-25) / 0.224 + 2^-23 + 2 * 2^-16 / 0.224 = 1.07e-6 + 1.19e-7 + 1.362e-4 = 1.374e-4.  The
    third term is reached only where a tap weight differs; the measured maximum is in DESIGN.md section 14."""
    from iswm_amd import ops
    H, W = hw
    img = _images(2, H, W)
    d = torch.from_numpy(img).to(dev())
    worst = 0.0
    for s in (0.5, 0.75, 1.25, 2.0):
        for hv, wv, f in T.views(H, W, [s], True):
            got = ops.predict_view_normalize(d, hv, wv, f, R.MEAN, R.STD)
            assert got.shape == (2, 3, hv, wv) and got.dtype == torch.float32
            err = float(np.abs(got.cpu().double().numpy() - T.view_normalize64(img, hv, wv, f)).max())
            print("view_normalize %dx%d -> %dx%d flip=%d: max |x - x64| %.3e (bound %.3e)" %
                  (H, W, hv, wv, f, err, VIEW_BOUND))
            worst = max(worst, err)
            assert err <= VIEW_BOUND
            again = ops.predict_view_normalize(d, hv, wv, f, R.MEAN, R.STD)
            assert torch.equal(got, again)
            if not f:                                                # the flipped view is the mirror of the plain one
                flipped = ops.predict_view_normalize(d, hv, wv, True, R.MEAN, R.STD)
                assert torch.equal(flipped, got.flip(-1))
    print("view_normalize %dx%d: largest error %.3e" % (H, W, worst))


def _same_packed(a, b, n, H, W):
    from iswm_amd import ops
    lay = ops.predict_maps_layout(n, H, W)
    parts = [(0, 40 * n)] + [(lay[k], lay[k] + n * H * W) for k in ("pred", "conf", "band")]
    return a.shape == b.shape == (lay["end"],) and all(torch.equal(a[i:j], b[i:j]) for i, j in parts)


@pytest.mark.parametrize("view_set", range(len(T.VIEW_SETS)))
@pytest.mark.parametrize("frame", T.FRAMES)
@pytest.mark.parametrize("c,fg,ld", SC.CLASSES)
def test_views_maps_against_restatement(c, fg, ld, frame, view_set):
    """k_predict_views_maps against the float64 mean of the per-view probabilities, each from the device's own unfused
    upsample of that view's logits (the route predict_maps is pinned on at 1e-6).  The foreground share is asserted
    for C = 2 at threshold 0.5 only: at 0.2 it is 100 %, and with more classes the foreground class seldom wins."""
    from iswm_amd import ops
    H, W = frame
    scales, flip = T.VIEW_SETS[view_set]
    vl = [(yl.to(dev()), f) for yl, f in T.view_logits(H, W, scales, flip, c, fg, ld)]
    V, n = len(vl), T.N
    yls, flips = [y for y, _ in vl], [f for _, f in vl]
    p_v = [T.unflip(R.softmax_fg(ops.bilinear_to_nchw_fwd(y, c, H, W).cpu().double().numpy(), fg), f) for y, f in vl]
    p64 = T.combine(np.stack(p_v), np.float64)
    bound = T.bound(V)
    npix = n * H * W
    for thr, mn, mx in SC.CUTS:
        m = ops.predict_views_maps(yls, flips, c, fg, H, W, thr, mn, mx, want_prob=True)
        m2 = ops.predict_views_maps(yls, flips, c, fg, H, W, thr, mn, mx, want_prob=True)
        assert all(torch.equal(a, b) for a, b in zip(m[:5], m2[:5])), "not reproducible"
        assert _same_packed(m.packed, ops.predict_views_maps(yls, flips, c, fg, H, W, thr, mn, mx).packed, n, H, W)
        prob = m.prob.cpu().numpy()
        pred, conf, band = (t.cpu().numpy() for t in (m.pred, m.conf, m.band))
        stats = m.stats.cpu().numpy()
        assert prob.shape == pred.shape == conf.shape == band.shape == (n, H, W) and stats.shape == (n, 5)
        err = np.abs(prob.astype(np.float64) - p64).max()
        pred_r, conf_r = R.predict_mask(p64, thr)
        band_r = R.binarize_confidence_map(conf_r, mn, mx)
        edge = R.near_boundary(p64, thr, 2 * bound)
        bad = (pred != pred_r) | (conf != conf_r) | (band != band_r)
        absorbed = bad & (prob == 1.0)                              # fp32's 1 + e = 1 (test_predict_maps_against_restatement)
        share = float((p64 > thr).mean())
        print("views_maps C=%d fg=%d %dx%d %d views thr=%g band=[%g,%g]: max |p - p64| %.3e (bound %.3e), %d boundary "
              "pixels, %d differ (%d of them p = 1 in fp32), foreground share %.3f" %
              (c, fg, H, W, V, thr, mn, mx, err, bound, int(edge.sum()), int(bad.sum()), int(absorbed.sum()), share))
        assert prob.max() <= 1.0
        assert err <= bound
        assert not (bad & ~edge).any(), "mismatch away from a decision boundary"
        assert (bad & ~absorbed).sum() <= 1e-3 * npix + 2
        if c == 2 and thr == 0.5:
            assert 0.05 <= share <= 0.95
        # the kernel's maps follow from its own p exactly
        p32 = prob.astype(np.float32)
        assert np.array_equal(pred, R.predict_mask(p32, thr)[0])
        assert np.array_equal(conf, R.predict_mask(p32, thr)[1])
        assert np.array_equal(band, R.binarize_confidence_map(conf, mn, mx))
        for k in range(n):
            own = R.prob_stats(p32[k], thr)
            assert stats[k, 0] == own[0] and stats[k, 1] == own[1]
            assert abs(stats[k, 2] - own[2]) <= 1e-12 * abs(own[2])     # the same fp32 values, another fixed fp64 order
            assert stats[k, 3] == own[3] and stats[k, 4] == own[4] == (pred[k] == 255).sum()


@pytest.mark.parametrize("c,fg,ld", SC.CLASSES)
@pytest.mark.parametrize("lo_hi", [((9, 9), (33, 33)), ((17, 23), (65, 93))])
def test_one_identity_view_is_predict_maps(lo_hi, c, fg, ld):
    """A list of one unflipped view runs k_predict_maps itself: predict_maps's bytes for every class layout.  Two
    identical unflipped views go through k_predict_views_maps: (p + p) / 2 = p, so for one float4 group of logits
    (C <= 4, every model this project builds) the bytes are predict_maps's again, which pins the per-pixel form; with
    more groups the compiler may contract bilerp4 differently per inlining site and the pair
    is held to the float64 bound of two views."""
    from iswm_amd import ops
    (hl, wl), (H, W) = lo_hi
    n = 2
    yl = SC.logits(n, hl, wl, c, ld, seed=hl * 31 + c * 7 + fg).to(dev())
    p64 = R.softmax_fg(ops.bilinear_to_nchw_fwd(yl, c, H, W).cpu().double().numpy(), fg)   # the mean of two equal views
    for thr, mn, mx in SC.CUTS:
        b = ops.predict_maps(yl, c, fg, H, W, thr, mn, mx, want_prob=True)
        a = ops.predict_views_maps([yl], [False], c, fg, H, W, thr, mn, mx, want_prob=True)
        assert torch.equal(a.prob, b.prob) and _same_packed(a.packed, b.packed, n, H, W), (c, fg, thr)
        two = ops.predict_views_maps([yl, yl], [False, False], c, fg, H, W, thr, mn, mx, want_prob=True)
        pa, pb = two.prob.cpu().numpy().ravel(), b.prob.cpu().numpy().ravel()
        ulp = np.abs(pa.view(np.int32).astype(np.int64) - pb.view(np.int32).astype(np.int64))
        print("two identity views C=%d %dx%d thr=%g: %d of %d probabilities differ from predict_maps, at most %d ulp" %
              (c, H, W, thr, int((pa != pb).sum()), pa.size, int(ulp.max())))
        if c <= 4:
            assert torch.equal(two.prob, b.prob) and _same_packed(two.packed, b.packed, n, H, W), (c, fg, thr)
        else:
            assert np.abs(pa.astype(np.float64) - p64.ravel()).max() <= T.bound(2)


TTA_FLAGS = ["--tta_scales", "0.75,1.0,1.25", "--tta_flip"]
TTA_SCALES = (0.75, 1.0, 1.25)
CLI_FRAMES = [("a.png", 65, 65), ("b.png", 65, 65), ("c.png", 97, 129)]


def _tta_frames(root):
    """test_scene_gpu's two frames and a second 65 x 65 one, so that --batch_size 2 batches two frames"""
    inp = _frames(root)
    a = np.asarray(Image.open(os.path.join(inp, "s1", "a.png")).convert("RGB"))
    Image.fromarray(a[::-1, :, ::-1].copy()).save(os.path.join(inp, "s1", "b.png"))
    return inp


def _maps_of(out, base, h, w):
    got = {}
    for kind in KINDS:
        im = Image.open(os.path.join(out, "s1", "%s_%s.png" % (base, kind)))
        assert im.mode == "L" and im.size == (w, h)
        got[kind] = np.asarray(im)
    return got


def test_tta_cli_end_to_end(tmp_path, capsys):
    from iswm_amd import ops, predict
    from iswm_amd.predict import DevicePredictor, TTAPredictor, decode_image
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg
    m, sd = _r50()
    inp = _tta_frames(str(tmp_path))
    big = decode_image(os.path.join(inp, "s1", "c.png"))
    with torch.no_grad():
        x0 = ops.predict_normalize(torch.from_numpy(big.copy()).to(dev())[None], R.MEAN, R.STD)
    sd = _spread_head(m, sd, x0)
    ckpt = os.path.join(str(tmp_path), "ref_format.pth")
    torch.save({"model_state": {"module." + k: v for k, v in sd.items()}}, ckpt)

    common = ["--input", inp, "--ckpt", ckpt, "--save_confidence", "--save_binary", "--workers", "2"]
    runs = {"tta1": TTA_FLAGS + ["--batch_size", "1"], "tta2": TTA_FLAGS + ["--batch_size", "2"],
            "plain": ["--batch_size", "2"], "explicit": ["--batch_size", "2", "--tta_scales", "1.0"]}
    outs = {}
    for tag, extra in runs.items():
        outs[tag] = os.path.join(str(tmp_path), tag)
        n = predict.main(common + ["--save_val_results_to", outs[tag]] + extra)
        text = capsys.readouterr().out
        assert n == 3 and text.count("Foreground probability: min=") == 3 and "Error while processing" not in text

    # the default flags: DevicePredictor's maps, and the same files whether the default is spelled out or not; one
    # identity view through TTAPredictor gives those bytes too
    m.load_state_dict(sd, strict=True)
    args = (m, dev(), 2, 1, 0.5, 0.2, 0.7, True, True)
    for name, h, w in CLI_FRAMES:
        base = os.path.splitext(name)[0]
        frame = decode_image(os.path.join(inp, "s1", name))[None]
        want = DevicePredictor(*args)(frame)()
        one = TTAPredictor(*args, (1.0,), False)(frame)()
        got = _maps_of(outs["plain"], base, h, w)
        for kind, k in zip(KINDS, ("pred", "conf", "band")):
            assert np.array_equal(got[kind], want[k][0]), (name, kind)
            assert np.array_equal(one[k], want[k]), (name, kind)
            a, b = (open(os.path.join(outs[tag], "s1", "%s_%s.png" % (base, kind)), "rb").read()
                    for tag in ("plain", "explicit"))
            assert a == b, (name, kind)
        assert one["stats"].tobytes() == want["stats"].tobytes()

    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = OracleDeepLab(ArchCfg("deeplabv3plus", "resnet50", 2, 16), sd64, dropout_p=0.0).eval()
    refs = {}
    for name, h, w in CLI_FRAMES:
        img = decode_image(os.path.join(inp, "s1", name))
        p_v = []
        for hv, wv, f in T.views(h, w, TTA_SCALES, True):
            x = torch.from_numpy(T.view_normalize64(img[None], hv, wv, f))
            with torch.no_grad():
                low = oracle.head(oracle.backbone(x))
                lg = F.interpolate(low, size=(h, w), mode="bilinear", align_corners=False).numpy()
            p_v.append(T.unflip(R.softmax_fg(lg, 1), f)[0])
        refs[name] = T.combine(np.stack(p_v), np.float64)
    same_maps = True
    for tag in ("tta1", "tta2"):
        npix = nedge = nbad = nfg = 0
        for name, h, w in CLI_FRAMES:
            base = os.path.splitext(name)[0]
            got = _maps_of(outs[tag], base, h, w)
            other = _maps_of(outs["tta1"], base, h, w)
            same_maps &= all(np.array_equal(got[k], other[k]) for k in KINDS)
            p64 = refs[name]
            pred_r, conf_r = R.predict_mask(p64, 0.5)
            band_r = R.binarize_confidence_map(conf_r, 0.2, 0.7)
            pred, conf, band = got["predict"], got["confidence"], got["binary_mask"]
            assert np.abs(conf.astype(int) - conf_r.astype(int)).max() <= 1, (tag, name)
            edge = R.near_boundary(p64, 0.5, 1e-4)
            bad = (pred != pred_r) | (band != band_r)
            assert not (bad & ~edge).any(), (tag, name)
            nfg += int((pred == 255).sum())
            npix += p64.size
            nedge += int(edge.sum())
            nbad += int(bad.sum())
        print("TTA CLI (%s) vs fp64 oracle per view: %d pixels, %d near a boundary, %d differ, foreground share %.3f" %
              (tag, npix, nedge, nbad, nfg / npix))
        assert nbad <= 1e-3 * npix
        assert 0.05 < nfg / npix < 0.95, "probabilities do not spread"
    print("TTA CLI: frame batch 1 and 2 maps %s" % ("bit-identical" if same_maps else "differ"))


def test_tta_predictor_on_an_int8_model(tmp_path):
    """TTAPredictor over a QuantizedSegmentationModel (test_scene_predictor_on_an_int8_model's): only forward_lowres is
    used, so the packed result is the bytes of predict_views_maps over per-view forward_lowres calls."""
    from iswm_amd import ops, quant
    from iswm_amd.predict import TTAPredictor, decode_image
    from oracle.synth import synth_images
    from tests import quant_cases as Q
    H, W, side = Q.SCENE["H"], Q.SCENE["W"], Q.SCENE["tile"]
    m, sd = _r50()
    inp = _frames(str(tmp_path))
    big = decode_image(os.path.join(inp, "s1", "c.png"))
    assert big.shape == (H, W, 3) and big.dtype == np.uint8
    img = torch.from_numpy(big.copy()).to(dev())[None]
    with torch.no_grad():
        x0 = ops.predict_normalize(img, R.MEAN, R.STD)
    m.load_state_dict(_spread_head(m, sd, x0), strict=True)            # spread before calibration
    qm = quant.quantize_model(m, quant.calibrate(m, [synth_images(2, side, side, seed=s).to(dev()) for s in (1, 2)]))
    views = ops.tta_views(H, W, TTA_SCALES, True)
    assert len(views) == 6
    with torch.no_grad():
        yls = [qm.forward_lowres(ops.predict_view_normalize(img, hv, wv, f, R.MEAN, R.STD)) for hv, wv, f in views]
    ref = ops.predict_views_maps(yls, [f for _, _, f in views], 2, 1, H, W, 0.5, 0.2, 0.7, want_prob=True)
    share = float((ref.prob > 0.5).float().mean())
    assert 0.05 <= share <= 0.95, share
    ref_stats = ref.stats.cpu().numpy()
    got = TTAPredictor(qm, dev(), 2, 1, 0.5, 0.2, 0.7, True, True, TTA_SCALES, True)(big.copy()[None])()
    assert got["stats"].tobytes() == ref_stats.tobytes()
    for k in ("pred", "conf", "band"):
        assert got[k].shape == (1, H, W) and np.array_equal(got[k], getattr(ref, k).cpu().numpy()), k
    assert ref_stats[0, 4] == (got["pred"] == 255).sum()
    print("INT8 TTA: foreground share %.4f over 6 views; predictor and per-view calls identical" % share)
