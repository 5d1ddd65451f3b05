"""Sliding-window scene prediction on the GPU (k_scene_tiles_normalize, k_scene_maps, iswm_amd.predict.ScenePredictor)
against the CPU restatements tests/scene_ref.py and tests/predict_ref.py: the window gather bit-exact, the blended
maps against the restatement on the device's own unfused per-window logits, a one-window scene against predict_maps
byte for byte, and the command line end to end against the fp64 oracle run per window."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import predict_ref as R
from tests import scene_cases as SC
from tests import scene_ref as S

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


@pytest.mark.parametrize("hwto", [(1, 1, 16, 0), (37, 53, 16, 4), (16, 53, 16, 8), (33, 48, 16, 0)])
def test_scene_tiles_normalize_bit_exact(hwto):
    from iswm_amd import ops
    H, W, T, O = hwto
    rng = np.random.default_rng(H * 7 + W)
    img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img[0, 0] = (0, 255, 128)
    plan = ops.scene_plan(H, W, T, O)
    rp = S.Plan(H, W, T, O)
    assert plan.astuple() == rp.astuple()
    want = torch.stack([R.normalize(img[oy:oy + rp.th, ox:ox + rp.tw]) for _, oy, ox in rp.windows()])
    scene = torch.from_numpy(img).to(dev())
    n = plan.ntiles
    got = ops.scene_tiles_normalize(scene, plan, 0, n, R.MEAN, R.STD).cpu()
    assert got.shape == want.shape and torch.equal(got, want)
    if n > 1:                                                   # two calls split at an odd window index
        cut = n // 2 if (n // 2) % 2 else n // 2 + 1
        assert 0 < cut < n and cut % 2 == 1
        two = torch.cat([ops.scene_tiles_normalize(scene, plan, 0, cut, R.MEAN, R.STD),
                         ops.scene_tiles_normalize(scene, plan, cut, n - cut, R.MEAN, R.STD)]).cpu()
        assert torch.equal(two, want)


def _same_packed(a, b, H, W):
    """two packed buffers of predict_maps_layout(1, H, W), byte for byte over the bytes the layout defines (the
    alignment gaps between its parts are never written)"""
    from iswm_amd import ops
    lay = ops.predict_maps_layout(1, H, W)
    parts = [(0, 40)] + [(lay[k], lay[k] + H * W) for k in ("pred", "conf", "band")]
    return a.shape == b.shape == (lay["end"],) and all(torch.equal(a[i:j], b[i:j]) for i, j in parts)


@pytest.mark.parametrize("scene", SC.SCENES)
@pytest.mark.parametrize("c,fg,ld", SC.CLASSES)
def test_scene_maps_against_restatement(c, fg, ld, scene):
    from iswm_amd import ops
    H, W, T, O, side = scene
    plan = ops.scene_plan(H, W, T, O)
    rp = S.Plan(H, W, T, O)
    assert plan.astuple() == rp.astuple()
    yl = SC.scene_logits(plan.ntiles, side, c, fg, ld).to(dev())
    lg = ops.bilinear_to_nchw_fwd(yl, c, plan.th, plan.tw).cpu().double().numpy()    # the unfused path's own logits
    p64 = S.blend(R.softmax_fg(lg, fg), rp, np.float64)[None]
    npix = H * W
    for thr, mn, mx in SC.CUTS:
        m = ops.scene_maps(yl, c, fg, plan, thr, mn, mx, want_prob=True)
        m2 = ops.scene_maps(yl, c, fg, plan, thr, mn, mx, want_prob=True)
        assert all(torch.equal(a, b) for a, b in zip(m[:5], m2[:5])), "not reproducible"
        assert _same_packed(m.packed, ops.scene_maps(yl, c, fg, plan, thr, mn, mx).packed, H, W)
        prob = m.prob.cpu().numpy()
        pred, conf, band = (t.cpu().numpy() for t in (m.pred, m.conf, m.band))
        stats = m.stats.cpu().numpy()
        assert prob.shape == pred.shape == conf.shape == band.shape == (1, H, W) and stats.shape == (1, 5)
        err = np.abs(prob.astype(np.float64) - p64).max()
        pred_r, conf_r = R.predict_mask(p64, thr)
        band_r = R.binarize_confidence_map(conf_r, mn, mx)
        edge = R.near_boundary(p64, thr, 2 * SC.BOUND)
        bad = (pred != pred_r) | (conf != conf_r) | (band != band_r)
        absorbed = bad & (prob == 1.0)                          # fp32's 1 + e = 1 (test_predict_maps_against_restatement)
        print("scene_maps C=%d fg=%d %dx%d T=%d O=%d (%d windows of %dx%d logits) thr=%g band=[%g,%g]: max |p - p64| "
              "%.3e, %d boundary pixels, %d differ (%d of them p = 1 in fp32)" %
              (c, fg, H, W, T, O, plan.ntiles, side, side, thr, mn, mx, err, int(edge.sum()), int(bad.sum()),
               int(absorbed.sum())))
        assert err <= SC.BOUND
        assert not (bad & ~edge).any(), "mismatch away from a decision boundary"
        assert (bad & ~absorbed).sum() <= 1e-3 * npix + 2
        # the kernel's maps follow from its own p exactly
        p32 = prob.astype(np.float32)
        assert np.array_equal(pred, R.predict_mask(p32, thr)[0])
        assert np.array_equal(conf, R.predict_mask(p32, thr)[1])
        assert np.array_equal(band, R.binarize_confidence_map(conf, mn, mx))
        ref = R.prob_stats(p64[0], thr)
        own = R.prob_stats(p32[0], thr)
        assert stats[0, 0] == own[0] and stats[0, 1] == own[1]
        for j in (0, 1):
            assert abs(stats[0, j] - ref[j]) <= max(np.spacing(np.float32(ref[j])), 1e-5 * abs(ref[j])), j
        assert abs(stats[0, 2] - own[2]) <= 1e-12 * abs(own[2])         # the same fp32 values, another fixed fp64 order
        assert abs(stats[0, 2] - ref[2]) <= 1e-6 * abs(ref[2]) + 1e-12
        assert stats[0, 3] == own[3] and stats[0, 4] == own[4] == (pred[0] == 255).sum()
        nb = int(edge[0].sum())
        assert abs(stats[0, 3] - ref[3]) <= nb and abs(stats[0, 4] - ref[4]) <= nb


# every path of fg_prob: logits of 1, 2 and 4 float4 groups held in registers (G = 1, 2, 4) and the two-pass path
ONE_WINDOW_CLASSES = [(2, 1, 4), (3, 1, 8), (5, 4, 8), (16, 3, 16), (17, 16, 20)]


@pytest.mark.parametrize("c,fg,ld", ONE_WINDOW_CLASSES)
@pytest.mark.parametrize("lo_hi", [((9, 9), (33, 33)), ((17, 23), (65, 93))])
def test_one_window_scene_is_predict_maps(lo_hi, c, fg, ld):
    """A scene of one window against predict_maps, byte for byte, on every path of fg_prob.  iswm_scene_maps runs a
    one-window plan through k_predict_maps itself: k_scene_maps samples with the same source, but hipcc contracts
    bilerp4's a * b + c * d per inlining site, and for 5 <= C <= 16 its p differed from k_predict_maps's in up to 544
    of 6 045 pixels by at most 62 ulp when it ran these scenes."""
    from iswm_amd import ops
    (hl, wl), (H, W) = lo_hi
    plan = ops.scene_plan(H, W, 513, 64)
    assert plan.ntiles == 1 and (plan.th, plan.tw) == (H, W)
    yl = SC.logits(1, hl, wl, c, ld, seed=hl * 31 + c * 7 + fg).to(dev())
    for thr, mn, mx in SC.CUTS:
        a = ops.scene_maps(yl, c, fg, plan, thr, mn, mx, want_prob=True)
        b = ops.predict_maps(yl, c, fg, H, W, thr, mn, mx, want_prob=True)
        pa, pb = a.prob.cpu().numpy().ravel(), b.prob.cpu().numpy().ravel()
        ulp = np.abs(pa.view(np.int32).astype(np.int64) - pb.view(np.int32).astype(np.int64))
        print("one window C=%d %dx%d thr=%g: %d of %d probabilities differ, at most %d ulp" %
              (c, H, W, thr, int((pa != pb).sum()), pa.size, int(ulp.max())))
        assert torch.equal(a.prob, b.prob), (c, fg, thr)
        assert _same_packed(a.packed, b.packed, H, W), (c, fg, thr)


# one float4 group of logits: what every model this project builds hands to the maps kernels (num_classes = 2 or 3,
# padded to 4) -- the layouts the command line can reach
ONE_GROUP_CLASSES = [(2, 1, 4), (3, 2, 8)]


@pytest.mark.parametrize("scene", SC.SCENES[:3])
@pytest.mark.parametrize("c,fg,ld", ONE_GROUP_CLASSES)
def test_pixels_under_one_window_carry_that_windows_probability(c, fg, ld, scene):
    """In a scene of several windows, a pixel that one window covers has wn = 1: k_scene_maps gives it predict_maps's
    probability of that window, bit for bit.  Pinned for one float4 group of logits.  With two to four groups
    (5 <= C <= 16) k_scene_maps's p_t is within 62 ulp of predict_maps's and not its bits (the compiler contracts
    bilerp4 per inlining site); those layouts are held to the fp64 bound only."""
    from iswm_amd import ops
    H, W, T, O, side = scene
    plan = ops.scene_plan(H, W, T, O)
    rp = S.Plan(H, W, T, O)
    yl = SC.scene_logits(plan.ntiles, side, c, fg, ld).to(dev())
    got = ops.scene_maps(yl, c, fg, plan, 0.5, 0.2, 0.7, want_prob=True).prob.cpu().numpy()[0]
    cover = np.zeros((H, W), dtype=int)
    for _, oy, ox in rp.windows():
        cover[oy:oy + rp.th, ox:ox + rp.tw] += 1
    assert (cover == 1).any() and (cover > 1).any()          # the scene has both kinds of pixels
    per_window = ops.predict_maps(yl, c, fg, rp.th, rp.tw, 0.5, 0.2, 0.7, want_prob=True).prob.cpu().numpy()
    for k, oy, ox in rp.windows():
        sl = (slice(oy, oy + rp.th), slice(ox, ox + rp.tw))
        alone = cover[sl] == 1
        assert np.array_equal(got[sl][alone], per_window[k][alone]), k


def _r50():
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    sd = synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, 16))
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    m.load_state_dict(sd, strict=True)
    return m.to(dev()).eval(), sd


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


FRAMES = [("a.png", 65, 65), ("c.png", 97, 129)]
KINDS = ("predict", "confidence", "binary_mask")


def _frames(root):
    inp = os.path.join(root, "frames")
    os.makedirs(os.path.join(inp, "s1"))
    rng = np.random.default_rng(11)
    for name, h, w in FRAMES:
        base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
        Image.fromarray(base).resize((w, h), Image.BILINEAR).save(os.path.join(inp, "s1", name))   # smooth content
    return inp


def test_scene_cli_end_to_end(tmp_path, capsys):
    from iswm_amd import ops, predict
    from iswm_amd.predict import decode_image
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg
    T, O = 65, 16
    m, sd = _r50()
    inp = _frames(str(tmp_path))
    big = decode_image(os.path.join(inp, "s1", "c.png"))
    plan = ops.scene_plan(97, 129, T, O)
    assert plan.ntiles == 6
    with torch.no_grad():
        x0 = ops.scene_tiles_normalize(torch.from_numpy(big.copy()).to(dev()), plan, 0, 6, R.MEAN, R.STD)
    sd = _spread_head(m, sd, x0)
    ckpt = os.path.join(str(tmp_path), "ref_format.pth")
    torch.save({"model_state": {"module." + k: v for k, v in sd.items()}}, ckpt)

    common = ["--input", inp, "--ckpt", ckpt, "--save_confidence", "--save_binary", "--workers", "2"]
    runs = {"tiled4": ["--tile_size", str(T), "--tile_overlap", str(O), "--batch_size", "4"],
            "tiled1": ["--tile_size", str(T), "--tile_overlap", str(O), "--batch_size", "1"],
            "whole": ["--batch_size", "1"]}
    outs = {}
    for tag, extra in runs.items():
        outs[tag] = os.path.join(str(tmp_path), tag)
        n = predict.main(common + ["--save_val_results_to", outs[tag]] + extra)
        text = capsys.readouterr().out
        assert n == 2 and text.count("Foreground probability: min=") == 2 and "Error while processing" not in text

    def maps_of(tag, base, h, w):
        got = {}
        for kind in KINDS:
            im = Image.open(os.path.join(outs[tag], "s1", "%s_%s.png" % (base, kind)))
            assert im.mode == "L" and im.size == (w, h)
            got[kind] = np.asarray(im)
        return got

    # the 65 x 65 frame is one window: the whole-frame path's files, byte for byte
    for kind in KINDS:
        a, b = (open(os.path.join(outs[tag], "s1", "a_%s.png" % kind), "rb").read() for tag in ("tiled4", "whole"))
        assert a == b, kind

    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    oracle = OracleDeepLab(ArchCfg("deeplabv3plus", "resnet50", 2, 16), sd64, dropout_p=0.0).eval()
    same_maps = True
    for tag in ("tiled4", "tiled1"):
        npix = nedge = nbad = nfg = 0
        for name, h, w in FRAMES:
            base = os.path.splitext(name)[0]
            got = maps_of(tag, base, h, w)
            other = maps_of("tiled4", base, h, w)
            same_maps &= all(np.array_equal(got[k], other[k]) for k in KINDS)
            img = decode_image(os.path.join(inp, "s1", name))
            rp = S.Plan(h, w, T, O)
            x = torch.stack([R.normalize(img[oy:oy + rp.th, ox:ox + rp.tw]) for _, oy, ox in rp.windows()])
            with torch.no_grad():
                lg = oracle(x.double()).numpy()
            p64 = S.blend(R.softmax_fg(lg, 1), rp, np.float64)
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
        print("scene CLI (%s) vs fp64 oracle per window: %d pixels, %d near a boundary, %d differ" %
              (tag, npix, nedge, nbad))
        assert nbad <= 1e-3 * npix
        assert 0.05 < nfg / npix < 0.95, "probabilities do not spread"
    print("scene CLI: window batch 1 and 4 maps %s" % ("bit-identical" if same_maps else "differ"))


def test_scene_predictor_on_an_int8_model(tmp_path, capsys):
    """ScenePredictor over a QuantizedSegmentationModel: the packed result is the same bytes for window batches of 1
    (six one-window calls), 4 (an assembled logits buffer with a short last batch) and 6 (the single-batch shortcut),
    and the bytes of scene_maps over six one-window forward_lowres calls, each of which equals the numpy restatement
    of the INT8 network bit for bit; the command line on the INT8 checkpoint writes the same three maps.  scene_maps
    itself is held to float64 by test_scene_maps_against_restatement: this pins the route into it."""
    from iswm_amd import ops, predict, quant
    from iswm_amd.predict import ScenePredictor, decode_image
    from oracle.synth import synth_images
    from tests import quant_cases as Q
    from tests import quant_ref as QR
    H, W, T, O = (Q.SCENE[k] for k in ("H", "W", "tile", "overlap"))
    m, sd = _r50()
    inp = _frames(str(tmp_path))
    os.remove(os.path.join(inp, "s1", "a.png"))
    big = decode_image(os.path.join(inp, "s1", "c.png"))
    assert big.shape == (H, W, 3) and big.dtype == np.uint8
    plan = ops.scene_plan(H, W, T, O)
    rp = S.Plan(H, W, T, O)
    assert plan.ntiles == Q.SCENE["windows"] and plan.astuple() == rp.astuple()
    scene = torch.from_numpy(big.copy()).to(dev())
    with torch.no_grad():
        x0 = ops.scene_tiles_normalize(scene, plan, 0, plan.ntiles, R.MEAN, R.STD)
    m.load_state_dict(_spread_head(m, sd, x0), strict=True)            # spread before calibration
    qm = quant.quantize_model(m, quant.calibrate(m, [synth_images(2, T, T, seed=s).to(dev()) for s in (1, 2)]))
    st = qm.state_int8()

    # the reference route: one window per call, each pinned to the restatement
    tiles = []
    for k in range(plan.ntiles):
        with torch.no_grad():
            xk = ops.scene_tiles_normalize(scene, plan, k, 1, R.MEAN, R.STD)
            assert torch.equal(xk, x0[k:k + 1])
            yk = qm.forward_lowres(xk)
            want = QR.forward_body(st, qm.stem(xk).cpu().numpy())
        assert np.array_equal(yk.cpu().numpy()[..., :2], want), k
        tiles.append(yk)
    stacked = torch.cat(tiles)
    ref = ops.scene_maps(stacked, 2, 1, plan, 0.5, 0.2, 0.7)
    lay = ops.predict_maps_layout(1, H, W)
    ref_maps = {k: ref.packed[lay[k]:lay[k] + H * W].view(H, W).cpu().numpy() for k in ("pred", "conf", "band")}
    ref_stats = ref.stats.cpu().numpy()

    # the restated probabilities spread: the maps are no constant
    p64 = S.blend(R.softmax_fg(SC.upsample64(stacked.cpu().numpy(), 2, T, T), 1), rp, np.float64)
    share = float((p64 > 0.5).mean())
    assert 0.05 <= share <= 0.95, share

    for b in Q.SCENE["tile_batches"]:
        got = ScenePredictor(qm, dev(), 2, 1, 0.5, 0.2, 0.7, True, True, T, O, tile_batch=b)(big.copy()[None])()
        assert got["stats"].tobytes() == ref_stats.tobytes(), b
        for k in ("pred", "conf", "band"):
            assert got[k].shape == (1, H, W) and np.array_equal(got[k][0], ref_maps[k]), (b, k)
    assert ref_stats[0, 4] == (ref_maps["pred"] == 255).sum()

    ckpt = os.path.join(str(tmp_path), "m_int8.pth")
    qm.save_int8(ckpt)
    out = os.path.join(str(tmp_path), "out")
    n = predict.main(["--input", inp, "--ckpt", ckpt, "--save_val_results_to", out, "--save_confidence", "--save_binary",
                      "--tile_size", str(T), "--tile_overlap", str(O), "--batch_size", "4"])
    text = capsys.readouterr().out
    assert n == 1 and "INT8 model loaded from" in text and "Error while processing" not in text
    for kind, k in zip(KINDS, ("pred", "conf", "band")):
        im = Image.open(os.path.join(out, "s1", "c_%s.png" % kind))
        assert im.mode == "L" and np.array_equal(np.asarray(im), ref_maps[k]), kind
    print("INT8 scene: foreground share of the restated probabilities %.4f; batches %s and the command line identical" %
          (share, list(Q.SCENE["tile_batches"])))
