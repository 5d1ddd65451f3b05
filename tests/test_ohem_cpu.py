"""No GPU: the restatement of the hard-pixel mining criterion (tests/ohem_ref.py) against float64 stock torch
(F.cross_entropy(reduction='none'), topk, autograd), its degenerate values, the recorded fp32 floors measured again, six wrong
formulas that the checks of tests/test_ohem_gpu.py must see (with the margin found), the host-side refusals of the C entry points,
the module's and the parser's refusals, and setup_criterion unchanged with the option off."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import ohem_ref as R

CHECKS = ("keys", "sums", "loss", "grad")


def stock(logits, labels, weight, ignore_index, thresh, min_kept, upstream=1.0):
    """the definition in float64 stock torch ops: per-pixel CE, topk for the k-th largest, autograd for the gradient"""
    z = logits.double().requires_grad_(True)
    c = z.shape[1]
    y = labels.long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    nll = F.cross_entropy(z, yc, reduction='none')
    k = min(min_kept, int(valid.sum()))
    nu = R.nu0_of(thresh)
    if k > 0:
        nu = min(nu, float(torch.topk(nll.detach()[valid], k).values[-1]))
    kept = valid & (nll.detach() >= nu)
    w = (weight.double() if weight is not None else torch.ones(c, dtype=torch.float64))[yc]
    if int(kept.sum()) == 0:
        return 0.0, torch.zeros_like(z), kept, nu
    loss = (w * nll)[kept].sum() / w[kept].sum()
    (loss * upstream).backward()
    return float(loss), z.grad, kept, nu


@pytest.mark.parametrize("group", ["r2_s1", "r8_s30", "r3_s1", "ig2", "gap"])
def test_restatement_is_stock_torch_in_float64(group):
    worst = 0.0
    for tag, logits, labels, wt, ig, th, k, up in R.group_cases(group):
        ref = R.ohem_ref(logits, labels, wt, ig, th, k, upstream=up)
        loss, grad, kept, nu = stock(logits, labels, wt, ig, th, k, up)
        assert torch.equal(kept, ref["kept"]) and nu == ref["nu"], tag
        assert int(ref["sums"][2]) == int(kept.sum()) >= ref["k"]
        e = max(abs(loss - float(ref["loss"])) / max(abs(loss), 1e-300), R.rel_err(ref["grad"], grad))
        worst = max(worst, e)
        assert e <= 1e-12, (tag, e)
    print(group, "largest difference from float64 stock torch %.1e" % worst)


def test_degenerate_values():
    logits, labels, weight = R.inputs((2, 2, 13, 11), "u8", 1.0)
    nv = int(R.valid_mask(labels, 2).sum())
    none = torch.full_like(labels, R.IGNORE)
    r = R.ohem_ref(logits, none, weight, R.IGNORE, 0.7, 100)                 # V empty
    assert r["k"] == 0 and float(r["loss"]) == 0.0 and not bool(r["grad"].any()) and not bool(r["sums"].any())
    easy = torch.zeros(1, 2, 5, 5)
    easy[:, 0] = 9.0
    r = R.ohem_ref(easy, torch.zeros(1, 5, 5, dtype=torch.uint8), None, R.IGNORE, 0.7, 0)     # K empty: min_kept 0, nothing hard
    assert r["k"] == 0 and r["nu"] == R.nu0_of(0.7) and int(r["kept"].sum()) == 0
    assert float(r["loss"]) == 0.0 and not bool(r["grad"].any())
    r = R.ohem_ref(logits, labels, weight, R.IGNORE, 0.01, nv + 5)           # min_kept > |V|: every valid pixel, no other
    assert r["k"] == nv and torch.equal(r["kept"], r["valid"])
    for k in (0, 7, nv + 5):                                                 # thresh = 1 is the weighted CE whatever min_kept
        r = R.ohem_ref(logits, labels, weight, R.IGNORE, 1.0, k)
        assert r["nu"] == 0.0 and torch.equal(r["kept"], r["valid"])
        y = torch.where(r["valid"], labels.long(), torch.full_like(labels.long(), -100))
        z = logits.double().requires_grad_(True)
        ce = F.cross_entropy(z, y, weight=weight.double(), ignore_index=-100)
        ce.backward()
        assert abs(float(ce) - float(r["loss"])) <= 1e-12 and R.rel_err(r["grad"], z.grad) <= 1e-12
    assert R.nu0_of(1.0) == 0.0 and math.copysign(1.0, R.nu0_of(1.0)) == 1.0


@functools.lru_cache(maxsize=None)
def measure_floors():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                            # the order of an fp32 sum, and with it a floor, depends on the thread count
    try:
        out = {}
        for group in R.GROUPS:
            for tag, logits, labels, wt, ig, th, k, up in R.group_cases(group):
                for check, e in R.floors_of(logits, labels, wt, ig, th, k, up).items():
                    key = R.floor_key(check, group)
                    out[key] = max(out.get(key, 0.0), e)
        return out
    finally:
        torch.set_num_threads(threads)                  # later test modules keep the thread count they would have had


def test_recorded_floors_are_the_measured_ones():
    measured = measure_floors()
    assert set(measured) == set(R.FLOOR), set(measured) ^ set(R.FLOOR)
    for key, m in sorted(measured.items()):
        want = max(m, R.FLOOR_MIN)
        print("%-12s recorded %.2e measured %.2e" % (key, R.FLOOR[key], m))
        assert R.FLOOR[key] >= R.FLOOR_MIN, key
        assert 0.5 * want <= R.FLOOR[key] <= 1.25 * want, (key, R.FLOOR[key], m)


def test_band_of_the_random_inputs_is_nearly_empty():
    """the condition tests/test_ohem_gpu.py puts on the random inputs, checked on fp32 stock torch against float64: outside the
    band the two kept sets agree, and the band holds at most BAND_MAX pixels"""
    most = 0
    for group in R.RANDOM:
        for tag, logits, labels, wt, ig, th, k, up in R.group_cases(group):
            ref = R.ohem_ref(logits, labels, wt, ig, th, k)
            low = R.ohem_ref(logits, labels, wt, ig, th, k, dtype=torch.float32)
            band = R.band_count(ref["nll"], ref["valid"], ref["nu"])
            assert torch.equal(low["kept"] | band, ref["kept"] | band), (group, tag)
            most = max(most, int(band.sum()))
    print("largest band: %d pixels" % most)
    assert most <= R.BAND_MAX


def _mutant_inputs(mutant):
    if mutant == "gt_at_tie":
        logits, labels = R.tie_inputs("four")
        nv = int(R.valid_mask(labels, 2).sum())
        return logits, labels, None, R.IGNORE, 0.05, nv // 3
    if mutant == "ignored_in_k":
        logits, labels, weight = R.inputs(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
        return logits, labels, weight, R.IG2_IGNORE, 0.05, int(R.valid_mask(labels, 3, R.IG2_IGNORE).sum()) // 3
    logits, labels, weight = R.inputs(R.RANDOM["r3_s1"][0], "u8", 1.0)
    nv = int(R.valid_mask(labels, 3).sum())
    return logits, labels, weight, R.IGNORE, (0.05 if mutant == "k_plus_one" else 0.7), nv // 10


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_checks_see_each_mutant(mutant):
    """each wrong formula changes the exact kept count, or misses a 4 x FLOOR bound (the floors of r3_s1: the mutants' shape) by
    10 x or more, or leaves a gradient where it must be exactly 0.  The margin found is printed."""
    logits, labels, wt, ig, th, k = _mutant_inputs(mutant)
    ref = R.ohem_ref(logits, labels, wt, ig, th, k)
    bad = R.ohem_ref(logits, labels, wt, ig, th, k, mutant=mutant)
    dcount = int(bad["sums"][2]) - int(ref["sums"][2])
    ratio = {c: R.rel_err(bad[c], ref[c]) / (4 * R.FLOOR[R.floor_key(c, "r3_s1")]) for c in ("loss", "grad")}
    off = ~ref["kept"]
    leak = float(bad["grad"].permute(0, 2, 3, 1)[off].abs().max()) if bool(off.any()) else 0.0
    print("%-18s kept count off by %+d; loss %.1e x bound, grad %.1e x bound; largest gradient outside K %.1e" %
          (mutant, dcount, ratio["loss"], ratio["grad"], leak))
    if mutant == "gt_at_tie":               # the whole tie group at nu is lost: thousands of pixels
        assert dcount <= -1000
    elif mutant == "k_plus_one":            # distinct values: exactly one pixel more
        assert dcount == 1
    elif mutant == "ignored_in_k":          # a third of the pixels carry the ignored label 2: their losses take ranks, nu rises
        assert bad["nu"] > ref["nu"] and dcount <= -10
    elif mutant == "count_normaliser":
        assert dcount == 0 and min(ratio.values()) >= 1000.0
    elif mutant == "max_of_thresholds":
        assert dcount <= -100 and ratio["loss"] >= 1000.0
    else:
        assert dcount == 0 and leak > 1e-6 and ratio["grad"] >= 1000.0


def test_exports_and_host_side_refusals():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in ("iswm_ohem_keys", "iswm_ohem_hist", "iswm_ohem_scan", "iswm_ohem_sums", "iswm_ohem_loss", "iswm_ohem_bwd",
                 "iswm_ohem_digits", "iswm_ohem_bins"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    assert lib.iswm_ohem_digits() == 3 and lib.iswm_ohem_bins() == 2048
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    keys = lambda lg=p, nb=1, b=1, c=2, hw=4, k=p, nv=p: lib.iswm_ohem_keys(lg, p, nb, b, c, hw, 255, k, p, nv, None)
    assert keys(lg=None) == 1 and "null" in err()
    assert keys(nv=None) == 1 and "null" in err()
    assert keys(c=9) == 1 and "classes" in err()
    assert keys(c=0) == 1 and "classes" in err()
    assert keys(nb=4) == 1 and "uint8 or int64" in err()
    assert keys(hw=0) == 1 and "shape" in err()
    assert lib.iswm_ohem_hist(p, 4, p, 3, p, None) == 1 and "digit" in err()
    assert lib.iswm_ohem_hist(p, 0, p, 0, p, None) == 1
    scan = lambda digit=0, mk=1, nu0=0.5, st=p: lib.iswm_ohem_scan(p, p, digit, mk, nu0, st, p, None)
    assert scan(digit=-1) == 1 and "digit" in err()
    assert scan(mk=-1) == 1 and "min_kept" in err()
    assert scan(nu0=-0.5) == 1 and "thresh" in err()
    assert scan(nu0=float("inf")) == 1 and scan(nu0=float("nan")) == 1
    assert scan(st=None) == 1 and "null" in err()
    sums = lambda nb=1, n=4, c=2, nu=p: lib.iswm_ohem_sums(p, p, nb, n, c, None, nu, p, p, None)
    assert sums(nu=None) == 1 and "null" in err()
    assert sums(n=0) == 1 and sums(c=9) == 1 and sums(nb=2) == 1
    assert lib.iswm_ohem_loss(None, p, None) == 1
    bwd = lambda nb=1, c=2, hw=4, k=p, up=p: lib.iswm_ohem_bwd(p, p, nb, 1, c, hw, None, k, p, p, up, p, None)
    assert bwd(k=None) == 1 and "null" in err()
    assert bwd(up=None) == 1 and "null" in err()
    assert bwd(c=9) == 1 and "classes" in err()
    assert bwd(nb=3) == 1 and bwd(hw=0) == 1


def test_module_refuses_bad_parameters_and_cpu_tensors():
    from iswm_amd.utils.loss import OhemCrossEntropyLoss
    for kw in (dict(thresh=0.0), dict(thresh=1.5), dict(thresh=-0.1), dict(min_kept=-1), dict(min_kept=2.5)):
        with pytest.raises(ValueError):
            OhemCrossEntropyLoss(**kw)
    m = OhemCrossEntropyLoss(thresh=1.0, min_kept=0, weight=torch.tensor([1.0, 3.0]))         # legal: the weighted CE
    assert (m.thresh, m.min_kept, m.ignore_index, m.last_kept, m.last_nu) == (1.0, 0, 255, None, None) and torch.equal(m.weight, torch.tensor([1.0, 3.0]))
    d = OhemCrossEntropyLoss()
    assert (d.thresh, d.min_kept, d.weight, d.group) == (0.7, 100000, None, None)
    with pytest.raises(ValueError):                                          # no CPU fallback
        d(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_parser_defaults_refusals_and_criterion_types():
    from iswm_amd import train
    from iswm_amd.utils.loss import CrossEntropyLoss, DiceLoss, OhemCrossEntropyLoss
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    o = parse()
    assert (o.ohem_thresh, o.ohem_min_kept) == (0.0, 100000)
    for bad in (["--ohem_thresh", "1.5"], ["--ohem_thresh", "-0.1"], ["--ohem_thresh", "0.7", "--ohem_min_kept", "-1"],
                ["--ohem_thresh", "0.7", "--overlap_loss", "dice"], ["--ohem_thresh", "1", "--overlap_loss", "focal_tversky"]):
        with pytest.raises(SystemExit):
            parse(*bad)
    cw = torch.tensor([1.0, 3.0])
    # off: exactly what setup_criterion returned before the option existed, whatever --ohem_min_kept says
    for extra in ([], ["--ohem_min_kept", "7"]):
        crit = train.setup_criterion(parse(*extra), cw)
        assert type(crit) is CrossEntropyLoss and torch.equal(crit.weight, cw) and crit.ignore_index == 255 and crit.group is None
        assert train.setup_criterion(parse("--loss_type", "ce_loss", *extra), cw).weight is None
        assert type(train.setup_criterion(parse("--overlap_loss", "dice", *extra), cw)) is DiceLoss
    m = train.setup_criterion(parse("--ohem_thresh", "0.7"), cw)
    assert type(m) is OhemCrossEntropyLoss and (m.thresh, m.min_kept, m.ignore_index) == (0.7, 100000, 255) and torch.equal(m.weight, cw)
    m = train.setup_criterion(parse("--ohem_thresh", "1", "--ohem_min_kept", "500", "--loss_type", "ce_loss"), cw)
    assert (m.thresh, m.min_kept, m.weight) == (1.0, 500, None)
