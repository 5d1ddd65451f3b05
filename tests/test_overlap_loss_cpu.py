"""No GPU: the restatement of the overlap criteria (tests/overlap_loss_ref.py) against float64 autograd of the plain formula, its
stated values on the degenerate label patterns, the fp32 floors measured again, six mutants that the 4 x FLOOR bounds must see,
the new C entry points' host-side refusals, and the trainer's options."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import overlap_loss_ref as R

CHECKS = ("sums", "loss", "grad")


def plain_autograd(logits, labels, weight, ignore_index, lce, lov, alpha, beta, gamma, smooth, classes):
    """the loss written the way a user would with torch ops, float64, differentiated by autograd"""
    z = logits.double().requires_grad_(True)
    c = z.shape[1]
    y = labels.long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    p = torch.softmax(z, 1)
    onehot = F.one_hot(torch.where(valid, y, torch.zeros_like(y)), c).permute(0, 3, 1, 2).double() * valid[:, None]
    pv = p * valid[:, None]
    tp, fp, fn = (pv * onehot).sum((0, 2, 3)), (pv * (1 - onehot)).sum((0, 2, 3)), ((1 - pv) * onehot).sum((0, 2, 3))
    tversky = (tp + smooth) / (tp + alpha * fp + beta * fn + smooth)
    ell = (1 - tversky).clamp(min=0) ** gamma
    loss = lov * (ell[1:] if classes == "foreground" else ell).mean()
    if lce != 0:
        target = torch.where(valid, y, torch.full_like(y, -100))
        loss = loss + lce * F.cross_entropy(z, target, weight=None if weight is None else weight.double(), ignore_index=-100)
    loss.backward()
    return loss.detach(), z.grad


def min_one_minus_t(sums, c, alpha, beta, gamma, smooth, classes):
    """the smallest 1 - T_c over the chosen classes, from float64 sums"""
    big_i, big_p, big_g = sums[2:2 + c], sums[2 + c:2 + 2 * c], sums[2 + 2 * c:]
    om = 1 - (big_i + smooth) / (big_i + alpha * (big_p - big_i) + beta * (big_g - big_i) + smooth)
    return float((om[1:] if classes == "foreground" else om).min())


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_restatement_equals_float64_autograd(case):
    shape, kind, scale = case
    logits, labels, weight = R.inputs(shape, kind, R.SCALES[scale])
    for combo in R.COMBOS:
        wt, args = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], combo)
        loss, grad = plain_autograd(logits, labels, wt, R.IGNORE, *args)
        assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))), R.combo_id(combo)
        if min_one_minus_t(ref["sums"], logits.shape[1], *args[2:]) <= 0 and args[4] < 1:
            # the degenerate point (one saturated pixel: T == 1): autograd's 0 * inf is nan, the definition's guard gives 0
            assert bool(torch.isnan(grad).any()) and bool(torch.isfinite(ref["grad"]).all()), R.combo_id(combo)
            continue
        assert float((ref["grad"] - grad).abs().max()) <= 1e-12, R.combo_id(combo)


def test_restatement_equals_autograd_with_an_ignore_index_inside_the_class_range():
    logits, labels, weight = R.inputs(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    wt, args = R.combo_args(R.IG2_COMBO, weight)
    ref = R.reference(R.IG2_SHAPE, "u8", 1.0, R.IG2_COMBO, R.IG2_IGNORE)
    loss, grad = plain_autograd(logits, labels, wt, R.IG2_IGNORE, *args)
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 and float((ref["grad"] - grad).abs().max()) <= 1e-12
    assert float(ref["sums"][2 + 2 * 3 + 2]) == 0.0 and int((labels == 2).sum()) > 20          # G_2: none of them counted


@pytest.mark.parametrize("gamma", [0.75, 1.0, 2.0])
def test_all_ignored_is_zero_with_zero_gradient(gamma):
    logits, labels, _ = R.degenerate_inputs("all_ignored")
    for classes in ("foreground", "all"):
        r = R.overlap_ref(logits, labels, None, R.IGNORE, 0.0, 1.0, 0.3, 0.7, gamma, 1.0, classes)
        assert float(r["loss"]) == 0.0 and not bool(r["grad"].any()) and not bool(r["sums"].any())


@pytest.mark.parametrize("gamma", [0.75, 1.0, 2.0])
def test_no_foreground_and_all_foreground_values(gamma):
    """with smooth s, N valid pixels and P1 = sum of the foreground probabilities:
         no foreground pixel:  I = G = 0      -> T = s / (alpha P1 + s)
         all foreground:       I = P1, G = N  -> T = (P1 + s) / (P1 + beta (N - P1) + s)"""
    alpha, beta, s = 0.3, 0.7, 1.0
    logits, lab0, _ = R.degenerate_inputs("no_foreground")
    p1 = float(torch.softmax(logits.double(), 1)[:, 1].sum())
    n = lab0.numel()
    r = R.overlap_ref(logits, lab0, None, R.IGNORE, 0.0, 1.0, alpha, beta, gamma, s, "foreground")
    assert math.isfinite(float(r["loss"])) and bool(torch.isfinite(r["grad"]).all())
    assert abs(float(r["loss"]) - (1 - s / (alpha * p1 + s)) ** gamma) <= 1e-12
    _, lab1, _ = R.degenerate_inputs("all_foreground")
    r = R.overlap_ref(logits, lab1, None, R.IGNORE, 0.0, 1.0, alpha, beta, gamma, s, "foreground")
    assert bool(torch.isfinite(r["grad"]).all())
    assert abs(float(r["loss"]) - (1 - (p1 + s) / (p1 + beta * (n - p1) + s)) ** gamma) <= 1e-12
    for pattern in ("no_foreground", "all_foreground"):                       # and autograd agrees where it is defined
        lg, lb, w = R.degenerate_inputs(pattern)
        for combo in R.degenerate_combos(pattern):
            wt, args = R.combo_args(combo, w)
            loss, grad = plain_autograd(lg, lb, wt, R.IGNORE, *args)
            ref = R.degenerate_reference(pattern, combo)
            assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 and float((ref["grad"] - grad).abs().max()) <= 1e-12


def _errs(logits, labels, wt, ignore_index, args, ref):
    low = R.overlap_ref(logits, labels, wt, ignore_index, *args, dtype=torch.float32)
    return {k: R.rel_err(low[k], ref[k]) for k in CHECKS}


@functools.lru_cache(maxsize=None)
def measure_floors():
    """{key: largest fp32-vs-float64 error of the group's cases} -- the figures FLOOR records (before the 2^-24 minimum)"""
    torch.set_num_threads(1)
    out = {}

    def take(group, errs):
        for k, e in errs.items():
            key = R.floor_key(k, group)
            out[key] = max(out.get(key, 0.0), e)
    for shape, kind, scale in R.INPUT_CASES:
        logits, labels, weight = R.inputs(shape, kind, R.SCALES[scale])
        for combo in R.COMBOS:
            wt, args = R.combo_args(combo, weight)
            take(R.group(shape, scale), _errs(logits, labels, wt, R.IGNORE, args, R.reference(shape, kind, R.SCALES[scale], combo)))
    for name, shape in R.BIG.items():
        logits, labels, weight = R.inputs(shape, "u8", 1.0)
        for combo in R.CAP_COMBOS:
            wt, args = R.combo_args(combo, weight)
            take(name, _errs(logits, labels, wt, R.IGNORE, args, R.reference(shape, "u8", 1.0, combo)))
    for pattern in ("no_foreground", "all_foreground"):
        lg, lb, w = R.degenerate_inputs(pattern)
        for combo in R.degenerate_combos(pattern):
            wt, args = R.combo_args(combo, w)
            take("degen", _errs(lg, lb, wt, R.IGNORE, args, R.degenerate_reference(pattern, combo)))
    logits, labels, weight = R.inputs(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    wt, args = R.combo_args(R.IG2_COMBO, weight)
    take("ig2", _errs(logits, labels, wt, R.IG2_IGNORE, args, R.reference(R.IG2_SHAPE, "u8", 1.0, R.IG2_COMBO, R.IG2_IGNORE)))
    return out


def test_recorded_floors_are_the_measured_ones():
    measured = measure_floors()
    assert set(measured) == set(R.FLOOR), set(measured) ^ set(R.FLOOR)
    for key, m in sorted(measured.items()):
        want = max(m, R.FLOOR_MIN)
        print("%-12s recorded %.2e measured %.2e" % (key, R.FLOOR[key], m))
        assert R.FLOOR[key] >= R.FLOOR_MIN, key
        assert 0.5 * want <= R.FLOOR[key] <= 1.25 * want, (key, R.FLOOR[key], m)


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_see_each_mutant(mutant):
    """a wrong formula misses at least one of the three 4 x FLOOR bounds by 10 x or more on the ig2 inputs"""
    logits, labels, weight = R.inputs(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    wt, args = R.combo_args(R.IG2_COMBO, weight)
    ref = R.reference(R.IG2_SHAPE, "u8", 1.0, R.IG2_COMBO, R.IG2_IGNORE)
    bad = R.overlap_ref(logits, labels, wt, R.IG2_IGNORE, *args, mutant=mutant)
    ratio = {k: R.rel_err(bad[k], ref[k]) / (4 * R.FLOOR[R.floor_key(k, "ig2")]) for k in CHECKS}
    print(mutant, {k: "%.1e" % v for k, v in ratio.items()})
    assert max(ratio.values()) >= 10.0, ratio


def test_exports_and_host_side_refusals():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in ("iswm_overlap_loss_fwd", "iswm_overlap_loss_coeffs", "iswm_overlap_loss_bwd"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    fwd = lambda lg=p, lb=p, nb=1, b=1, c=2, hw=4, part=p, sums=p: lib.iswm_overlap_loss_fwd(lg, lb, nb, b, c, hw, None, 255, part,
                                                                                           sums, None)
    assert fwd(lg=None) == 1 and "null" in err()
    assert fwd(sums=None) == 1 and "null" in err()
    assert fwd(c=0) == 1 and "classes" in err()
    assert fwd(c=9) == 1 and "classes" in err()
    assert fwd(nb=4) == 1 and "uint8 or int64" in err()
    assert fwd(hw=0) == 1 and "shape" in err()
    bwd = lambda lg=p, lb=p, nb=1, b=1, c=2, hw=4, coef=p, up=p, grad=p: lib.iswm_overlap_loss_bwd(lg, lb, nb, b, c, hw, None, 255,
                                                                                                 coef, up, grad, None)
    assert bwd(coef=None) == 1 and "null" in err()
    assert bwd(up=None) == 1 and "null" in err()
    assert bwd(grad=None) == 1 and "null" in err()
    assert bwd(c=9) == 1 and "classes" in err()
    assert bwd(c=0) == 1 and "classes" in err()
    assert bwd(nb=2) == 1 and "uint8 or int64" in err()

    def coeffs(sums=p, c=2, lce=1.0, lov=1.0, alpha=0.3, beta=0.7, gamma=1.0, s=1.0, classes=0, loss=p, coef=p):
        return lib.iswm_overlap_loss_coeffs(sums, c, lce, lov, alpha, beta, gamma, s, classes, loss, coef, None)
    assert coeffs(sums=None) == 1 and "null" in err()
    assert coeffs(loss=None) == 1 and coeffs(coef=None) == 1
    assert coeffs(c=0) == 1 and "classes" in err()
    assert coeffs(c=9) == 1 and "classes" in err()
    assert coeffs(s=0.0) == 1 and "smooth" in err()
    assert coeffs(s=-1.0) == 1 and "smooth" in err()
    assert coeffs(s=float("nan")) == 1 and "smooth" in err()
    assert coeffs(alpha=-0.1) == 1 and "alpha" in err()
    assert coeffs(beta=-0.1) == 1 and "beta" in err()
    assert coeffs(gamma=0.0) == 1 and "gamma" in err()
    assert coeffs(gamma=-1.0) == 1 and "gamma" in err()
    assert coeffs(lce=-1.0) == 1 and coeffs(lov=-1.0) == 1
    assert coeffs(classes=2) == 1
    assert coeffs(c=1, classes=0) == 1 and "empty" in err()                  # one class has no foreground class


def test_module_refuses_bad_parameters_and_cpu_tensors():
    from iswm_amd.utils.loss import DiceLoss, TverskyLoss
    for kw in (dict(smooth=0.0), dict(alpha=-1.0), dict(beta=-0.5), dict(gamma=0.0), dict(classes="background"),
               dict(ce_weight=-1.0), dict(overlap_weight=-1.0)):
        with pytest.raises(ValueError):
            TverskyLoss(**kw)
    with pytest.raises(TypeError):
        DiceLoss(alpha=0.3)
    d = DiceLoss(ce_weight=1.0, weight=torch.tensor([1.0, 3.0]))
    assert d.params == (1.0, 1.0, 0.5, 0.5, 1.0, 1.0, "foreground") and torch.equal(d.weight, torch.tensor([1.0, 3.0]))
    assert TverskyLoss().params == (0.0, 1.0, 0.3, 0.7, 1.0, 1.0, "foreground")
    with pytest.raises(ValueError):                                          # no CPU fallback
        TverskyLoss()(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_parser_defaults_refusals_and_criterion_types():
    from iswm_amd import train
    from iswm_amd.utils.loss import CrossEntropyLoss, DiceLoss, TverskyLoss
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    o = parse()
    assert (o.overlap_loss, o.overlap_weight, o.ce_weight, o.tversky_alpha, o.tversky_beta, o.tversky_gamma, o.overlap_smooth,
            o.overlap_classes, o.loss_type) == ("none", 1.0, 1.0, 0.3, 0.7, 0.75, 1.0, "foreground", "IWce_loss")
    for bad in (["--ce_weight", "0"], ["--overlap_loss", "lovasz"], ["--overlap_classes", "background"],
                ["--overlap_loss", "dice", "--overlap_smooth", "0"], ["--overlap_loss", "tversky", "--tversky_alpha", "-1"],
                ["--overlap_loss", "focal_tversky", "--tversky_gamma", "0"], ["--overlap_loss", "dice", "--ce_weight", "-1"],
                ["--loss_type", "dice"]):
        with pytest.raises(SystemExit):
            parse(*bad)
    cw = torch.tensor([1.0, 3.0])
    crit = train.setup_criterion(o, cw)
    assert type(crit) is CrossEntropyLoss and torch.equal(crit.weight, cw)
    assert train.setup_criterion(parse("--loss_type", "ce_loss"), cw).weight is None
    d = train.setup_criterion(parse("--overlap_loss", "dice"), cw)
    assert type(d) is DiceLoss and d.params == (1.0, 1.0, 0.5, 0.5, 1.0, 1.0, "foreground") and torch.equal(d.weight, cw)
    t = train.setup_criterion(parse("--overlap_loss", "tversky", "--loss_type", "ce_loss", "--overlap_classes", "all",
                                    "--tversky_gamma", "0.5"), cw)
    assert type(t) is TverskyLoss and t.params == (1.0, 1.0, 0.3, 0.7, 1.0, 1.0, "all") and t.weight is None
    f = train.setup_criterion(parse("--overlap_loss", "focal_tversky", "--ce_weight", "0", "--overlap_weight", "2",
                                    "--tversky_alpha", "0.4", "--tversky_beta", "0.6", "--overlap_smooth", "0.5"), cw)
    assert type(f) is TverskyLoss and f.params == (0.0, 2.0, 0.4, 0.6, 0.75, 0.5, "foreground")
