"""The CRF refinement on the GPU (csrc/crf.hip, ops.crf_refine / ops.prob_maps, the three predictors and the command line) against
the numpy restatement of tests/crf_ref.py in float64.

The bound of the refinement is written in units of E32 = max|q32 - q64|, the distance between the float32 and the float64 restatement
on the same input, which the test computes itself: max|q_dev - q64| <= 16 E32 + 2.4e-7.  The factor 16 pays for the hardware
exponential and another order over up to 224 terms; 2.4e-7 is four fp32 spacings below 1.0.  Nothing in it comes from the kernel.
Every case has w_b + w_s <= 2, where one iteration does not amplify the error of the one before, and none saturates
(tests/test_crf_cpu.py asserts both on the reference)."""
import functools
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import crf_ref as R
from tests import predict_ref as P

pytestmark = pytest.mark.gpu

MEAN, STD = P.MEAN, P.STD


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def bound(e32):
    return 16.0 * e32 + 2.4e-7


@functools.lru_cache(maxsize=None)
def _reference(shape, k):
    """(prob, frames, q64, E32) of case (shape, PARAMS[k]), computed once; nobody writes to them"""
    p, img = R.case_inputs(shape, k)
    q64 = R.refine_case(p, img, R.PARAMS[k])
    q32 = R.refine_case(p, img, R.PARAMS[k], dtype=np.float32)
    return p, img, q64, float(np.abs(q32.astype(np.float64) - q64).max())


def _refine(p, img, params):
    from iswm_amd import ops
    r, d, t, w_b, w_s, ta, tb, tg = params
    return ops.crf_refine(torch.from_numpy(p).to(dev()), torch.from_numpy(img).to(dev()), t, r, d, w_b, w_s, ta, tb, tg)


@pytest.mark.parametrize("k", range(len(R.PARAMS)))
@pytest.mark.parametrize("shape", R.SHAPES)
def test_refine_against_float64(shape, k):
    p, img, q64, e32 = _reference(shape, k)
    assert 0.015 < q64.min() and q64.max() < 0.99
    q = _refine(p, img, R.PARAMS[k])
    assert q.shape == p.shape and q.dtype == torch.float32
    err = float(np.abs(q.cpu().numpy().astype(np.float64) - q64).max())
    print("crf %s R=%d D=%d T=%d: max|q - q64| %.3e, E32 %.3e, ratio %s, bound %.3e, moved %.3f" %
          ((shape,) + R.PARAMS[k][:3] + (err, e32, "%.2f" % (err / e32) if e32 else "-", bound(e32),
                                         np.abs(q64 - R.clamp(p)).max())))
    assert err <= bound(e32)


def _defaults():
    return {("step_" if k == "step" else k): v for k, v in R.DEFAULTS.items()}


def test_defaults_on_the_wavy_edge():
    from iswm_amd import ops
    truth, frame, prob = R.wavy_edge()
    q64 = R.refine(prob, frame, 5, **_defaults())
    e32 = float(np.abs(R.refine(prob, frame, 5, dtype=np.float32, **_defaults()).astype(np.float64) - q64).max())
    q = ops.crf_refine(torch.from_numpy(prob[None]).to(dev()), torch.from_numpy(frame[None]).to(dev()), 5)[0].cpu().numpy()
    err = float(np.abs(q.astype(np.float64) - q64).max())
    before, after = R.misclassified(prob, truth), R.misclassified(q, truth)
    print("crf wavy edge, defaults, T=5: max|q - q64| %.3e, E32 %.3e, ratio %.2f; misclassified %d -> %d (float64: %d)" %
          (err, e32, err / e32, before, after, R.misclassified(q64, truth)))
    assert err <= bound(e32)
    assert after <= before // 4


def test_two_calls_give_identical_bits_and_zero_iterations_return_the_input():
    from iswm_amd import ops
    p, img, _, _ = _reference((2, 37, 53), 1)
    a, b = _refine(p, img, R.PARAMS[1]), _refine(p, img, R.PARAMS[1])
    assert torch.equal(a, b)
    tp, ti = torch.from_numpy(p).to(dev()), torch.from_numpy(img).to(dev())
    assert ops.crf_refine(tp, ti, 0) is tp
    c, d = ops.crf_refine(tp, ti, 4), ops.crf_refine(tp, ti, 4)          # the defaults, an even count: both planes in play
    assert torch.equal(c, d) and not torch.equal(c, tp)
    with pytest.raises(ValueError):
        ops.crf_refine(tp, ti[:1], 1)
    with pytest.raises(ValueError):
        ops.crf_refine(tp, ti.cpu(), 1)


GOOD = dict(radius=3, step=1, iters=2, w_b=1.0, w_s=1.0, ta=4.0, tb=20.0, tg=2.0)


@pytest.mark.parametrize("change,word", [(dict(radius=0), "radius"), (dict(radius=8), "radius"), (dict(step=5), "step"),
                                         (dict(iters=0), "iterations"), (dict(iters=21), "iterations"), (dict(ta=0.0), "theta"),
                                         (dict(tb=0.0), "theta"), (dict(tg=0.0), "theta"), (dict(w_b=-1.0), "weights"),
                                         (dict(w_s=-0.5), "weights"), (dict(alias=True), "alias"), (dict(short=True), "workspace"),
                                         (dict(null=True), "null")])
def test_c_abi_refusals_set_an_error_and_leave_out_untouched(change, word):
    from iswm_amd import _lib
    from iswm_amd.ops import _p, _stream
    lib = _lib.load()
    n, h, w = 1, 9, 11
    prob = torch.full((n, h, w), 0.25, device=dev())
    img = torch.zeros((n, h, w, 3), dtype=torch.uint8, device=dev())
    out = torch.full((n, h, w), -7.0, device=dev())
    nbytes = lib.iswm_crf_refine_workspace(n, h, w)
    work = torch.zeros(nbytes // 4, device=dev())
    a = dict(GOOD)
    a.update({k: v for k, v in change.items() if k in GOOD})
    rc = lib.iswm_crf_refine(_p(prob), None if change.get("null") else _p(img), n, h, w, a["radius"], a["step"], a["iters"], a["w_b"],
                             a["w_s"], a["ta"], a["tb"], a["tg"], _p(prob) if change.get("alias") else _p(out), _p(work),
                             nbytes - 1 if change.get("short") else nbytes, _stream())
    msg = lib.iswm_last_error().decode()
    torch.cuda.synchronize()
    assert rc != 0 and word in msg, msg
    assert bool((out == -7.0).all()) and bool((prob == 0.25).all())
    # the same call with nothing wrong runs
    assert lib.iswm_crf_refine(_p(prob), _p(img), n, h, w, GOOD["radius"], GOOD["step"], GOOD["iters"], 1.0, 1.0, 4.0, 20.0, 2.0,
                               _p(out), _p(work), nbytes, _stream()) == 0
    torch.cuda.synchronize()
    assert bool(((out > 0) & (out < 1)).all())


# ---- prob_maps --------------------------------------------------------------------------------------------------------------------

def _logits(n, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    yl = torch.randn((n, h, w, 4), generator=g) * 3.0
    sat = torch.rand((n, h, w), generator=g) < 0.1
    yl[..., 0][sat] = 30.0
    yl[..., 1][sat] = -30.0
    return yl


def _same_packed(a, b, n, H, W):
    """two packed buffers byte for byte over the bytes predict_maps_layout defines (its alignment gaps are never written)"""
    from iswm_amd import ops
    lay = ops.predict_maps_layout(n, H, W)
    parts = [(0, 40 * n)] + [(lay[k], lay[k] + n * H * W) for k in ("pred", "conf", "band")]
    return a.shape == b.shape == (lay["end"],) and all(torch.equal(a[i:j], b[i:j]) for i, j in parts)


@pytest.mark.parametrize("thr,mn,mx", [(0.5, 0.2, 0.7), (0.3, 0.1, 0.9), (0.7, 0.7, 0.2)])
@pytest.mark.parametrize("lo,hi", [((1, 10, 14), (2, 37, 53)), ((1, 2, 2), (1, 5, 7)), ((1, 33, 33), (3, 129, 129))])
def test_prob_maps_reproduces_predict_maps(lo, hi, thr, mn, mx):
    from iswm_amd import ops
    n, H, W = hi
    yl = _logits(n, lo[1], lo[2], seed=H * 3 + W).to(dev())
    want = ops.predict_maps(yl, 2, 1, H, W, thr, mn, mx, want_prob=True)
    got = ops.prob_maps(want.prob, thr, mn, mx)
    assert got.prob is want.prob
    assert _same_packed(got.packed, want.packed, n, H, W)
    assert torch.equal(got.stats, want.stats) and torch.equal(got.pred, want.pred) and torch.equal(got.band, want.band)
    assert 0 < int((want.pred == 255).sum()) < n * H * W


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 37, 53), (3, 16, 16)])
def test_prob_maps_on_an_arbitrary_map_follows_the_rules_exactly(shape):
    """values on the 2^-24 grid, so that their float64 sum is exact in any order and the statistics can be held to equality"""
    from iswm_amd import ops
    n, h, w = shape
    rng = np.random.RandomState(h * w)
    p = (np.floor(rng.uniform(0, 1, size=shape) * 2 ** 24) / 2 ** 24).astype(np.float32)
    thr = float(np.float32(0.3))
    flat = p.reshape(-1)
    special = [0.0, 1.0, np.float32(thr), np.nextafter(np.float32(thr), np.float32(1)), np.nextafter(np.float32(thr), np.float32(0)),
               np.float32(51 / 255), np.float32(1 - 2.0 ** -24)]
    flat[:min(len(special), flat.size)] = special[:flat.size]
    for mn, mx in ((0.2, 0.7), (0.0, 1.0)):
        m = ops.prob_maps(torch.from_numpy(p).to(dev()), thr, mn, mx)
        pred_r, conf_r = P.predict_mask(p, thr)
        assert np.array_equal(m.pred.cpu().numpy(), pred_r) and np.array_equal(m.conf.cpu().numpy(), conf_r)
        assert np.array_equal(m.band.cpu().numpy(), P.binarize_confidence_map(conf_r, mn, mx))
        stats = m.stats.cpu().numpy()
        for k in range(n):
            assert tuple(stats[k]) == tuple(float(v) for v in P.prob_stats(p[k], thr)), k


# ---- the predictors and the command line ------------------------------------------------------------------------------------------

CRF = dict(iters=2, radius=3, step=1, w_bilateral=6.0, w_spatial=2.0, theta_alpha=30.0, theta_beta=20.0, theta_gamma=2.0)
CUT = (0.5, 0.2, 0.7)


def _smooth(rng, h, w):
    base = rng.integers(0, 256, (h // 8 + 2, w // 8 + 2, 3), dtype=np.uint8)
    return np.asarray(Image.fromarray(base).resize((w, h), Image.BILINEAR))


def _calibration_pair():
    """the 97 x 97 frame the classifier is spread on, and its mirror image upside down: the probability of both spreads over (0, 1)"""
    a = _smooth(np.random.default_rng(11), 97, 97)
    return np.stack([a, a[::-1, ::-1].copy()])


@pytest.fixture(scope="module")
def model():
    """r50 os16 V3+ with seeded synthetic weights, its classifier scaled so that p spreads over (0, 1) on a smooth frame"""
    from iswm_amd import ops
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    sd = synth_state_dict(ArchCfg("deeplabv3plus", "resnet50", 2, 16))
    m = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev()).eval()
    x = ops.predict_normalize(torch.from_numpy(_calibration_pair()[:1]).to(dev()), MEAN, STD)
    with torch.no_grad():
        yl = m.forward_lowres(x)
    d = (yl[..., 1] - yl[..., 0]).double()
    s = 3.0 / float(d.std())
    sd = dict(sd)
    b = sd["classifier.classifier.6.bias"].clone() * s
    b[1] -= float(d.mean()) * s
    sd["classifier.classifier.6.weight"] = sd["classifier.classifier.6.weight"] * s
    sd["classifier.classifier.6.bias"] = b
    m.load_state_dict(sd, strict=True)
    return m, sd


def _check(got, want, plain, n, h, w):
    """a predictor's result against the hand-made maps, and the refinement against doing nothing"""
    assert got["stats"].tobytes() == want.stats.cpu().numpy().tobytes()
    for k in ("pred", "conf", "band"):
        assert got[k].shape == (n, h, w) and np.array_equal(got[k], getattr(want, k).cpu().numpy()), k
    assert not torch.equal(want.conf, plain.conf), "the refinement changed nothing"
    assert 0 < int((want.pred == 255).sum()) < n * h * w


def test_device_predictor_is_the_composition(model):
    from iswm_amd import ops
    from iswm_amd.predict import DevicePredictor
    m, _ = model
    rng = np.random.default_rng(21)
    batch = np.stack([_smooth(rng, 65, 93), _smooth(rng, 65, 93)])
    got = DevicePredictor(m, dev(), 2, 1, *CUT, True, True, crf=CRF)(batch)()
    img = torch.from_numpy(batch).to(dev())
    with torch.no_grad():
        plain = ops.predict_maps(m.forward_lowres(ops.predict_normalize(img, MEAN, STD)), 2, 1, 65, 93, *CUT, want_prob=True)
    want = ops.prob_maps(ops.crf_refine(plain.prob, img, **CRF), *CUT)
    _check(got, want, plain, 2, 65, 93)
    off = DevicePredictor(m, dev(), 2, 1, *CUT, True, True)(batch)()                     # crf=None: the maps call's own bytes
    assert off["stats"].tobytes() == plain.stats.cpu().numpy().tobytes() and np.array_equal(off["conf"], plain.conf.cpu().numpy())


def test_scene_predictor_is_the_composition(model):
    from iswm_amd import ops
    from iswm_amd.predict import ScenePredictor
    m, _ = model
    frame = _smooth(np.random.default_rng(22), 97, 97)
    plan = ops.scene_plan(97, 97, 65, 16)
    assert (plan.nty, plan.ntx) == (2, 2)
    got = ScenePredictor(m, dev(), 2, 1, *CUT, True, True, 65, 16, tile_batch=3, crf=CRF)(frame[None].copy())()
    scene = torch.from_numpy(frame.copy()).to(dev())
    with torch.no_grad():
        yl = m.forward_lowres(ops.scene_tiles_normalize(scene, plan, 0, plan.ntiles, MEAN, STD))
        plain = ops.scene_maps(yl, 2, 1, plan, *CUT, want_prob=True)
    want = ops.prob_maps(ops.crf_refine(plain.prob, scene.unsqueeze(0), **CRF), *CUT)       # the whole scene, not its windows
    _check(got, want, plain, 1, 97, 97)


def test_tta_predictor_is_the_composition(model):
    from iswm_amd import ops
    from iswm_amd.predict import TTAPredictor
    m, _ = model
    batch = _calibration_pair()
    got = TTAPredictor(m, dev(), 2, 1, *CUT, True, True, (1.0, 0.75), True, crf=CRF)(batch)()
    img = torch.from_numpy(batch).to(dev())
    views = ops.tta_views(97, 97, (1.0, 0.75), True)
    with torch.no_grad():
        yls = [m.forward_lowres(ops.predict_view_normalize(img, hv, wv, f, MEAN, STD)) for hv, wv, f in views]
        plain = ops.predict_views_maps(yls, [f for _, _, f in views], 2, 1, 97, 97, *CUT, want_prob=True)
    want = ops.prob_maps(ops.crf_refine(plain.prob, img, **CRF), *CUT)
    _check(got, want, plain, 2, 97, 97)


def test_cli_with_and_without_the_refinement(model, tmp_path, capsys):
    from iswm_amd import predict
    from iswm_amd.predict import DevicePredictor, decode_image
    m, sd = model
    inp = os.path.join(str(tmp_path), "frames")
    os.makedirs(os.path.join(inp, "s1"))
    for name, frame in zip(("a.png", "b.png"), _calibration_pair()):
        Image.fromarray(frame).save(os.path.join(inp, "s1", name))
    ckpt = os.path.join(str(tmp_path), "m.pth")
    torch.save({"model_state": sd}, ckpt)
    common = ["--input", inp, "--ckpt", ckpt, "--save_confidence", "--save_binary", "--batch_size", "2"]
    runs = {"plain": [], "zero": ["--crf_iters", "0"],
            "crf": ["--crf_iters", "2", "--crf_radius", "3", "--crf_step", "1", "--crf_bilateral_weight", "6", "--crf_spatial_weight",
                    "2", "--crf_theta_alpha", "30", "--crf_theta_beta", "20", "--crf_theta_gamma", "2"]}
    text = {}
    for tag, extra in runs.items():
        assert predict.main(common + ["--save_val_results_to", os.path.join(str(tmp_path), tag)] + extra) == 2
        text[tag] = capsys.readouterr().out
        assert "Error while processing" not in text[tag]
    files = sorted(os.listdir(os.path.join(str(tmp_path), "plain", "s1")))
    assert files == ["%s_%s.png" % (b, k) for b in "ab" for k in ("binary_mask", "confidence", "predict")]
    read = (lambda tag, f: open(os.path.join(str(tmp_path), tag, "s1", f), "rb").read())
    for f in files:
        assert sorted(os.listdir(os.path.join(str(tmp_path), "zero", "s1"))) == files
        assert read("zero", f) == read("plain", f), f
    stats_lines = (lambda t: [line for line in t.splitlines() if line.startswith(("Foreground probability", "Pixels below"))])
    assert stats_lines(text["zero"]) == stats_lines(text["plain"]) != stats_lines(text["crf"])

    batch = np.stack([decode_image(os.path.join(inp, "s1", n)) for n in ("a.png", "b.png")])
    want = DevicePredictor(m, dev(), 2, 1, 0.5, 0.2, 0.7, True, True, crf=CRF)(batch)()
    differs = False
    for i, b in enumerate("ab"):
        for kind, k in (("predict", "pred"), ("confidence", "conf"), ("binary_mask", "band")):
            im = Image.open(os.path.join(str(tmp_path), "crf", "s1", "%s_%s.png" % (b, kind)))
            assert im.mode == "L" and im.size == (97, 97)
            assert np.array_equal(np.asarray(im), want[k][i]), (b, kind)
            differs |= read("crf", "%s_%s.png" % (b, kind)) != read("plain", "%s_%s.png" % (b, kind))
        assert predict._stats_lines(want["stats"][i], 97 * 97, 0.5) in text["crf"]        # the refined probability's statistics
    assert differs
