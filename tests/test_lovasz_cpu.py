"""No GPU: the restatement of the Lovasz-Softmax criterion (tests/lovasz_ref.py) against float64 autograd of Berman's difference
form (ordering key detached), its degenerate values, the recorded fp32 floors measured again, seven wrong formulas that the
checks of tests/test_lovasz_gpu.py must see (with the margin found), the exports and host-side refusals of the C entry points,
the module's and the parser's refusals, and setup_criterion unchanged with the option off."""
import ctypes
import functools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import lovasz_ref as R


def berman(logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, upstream, order):
    """lovasz_softmax(per_image=True, classes='present' within S) as published: errors sorted by a DETACHED key, the Jaccard
    gradient as the difference J_j - J_{j-1}, in float64 with autograd; + ce_weight x F.cross_entropy.  `order` [B, |S|, HW] is
    the sort's result (the key is detached, so autograd never sees it)."""
    z = logits.double().requires_grad_(True)
    b, c = z.shape[:2]
    y = labels.reshape(b, -1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    p = torch.softmax(z.reshape(b, c, -1), 1)
    first = R.first_class(classes)
    terms = []
    for bi in range(b):
        nv = int(valid[bi].sum())
        for ci in range(first, c):
            fg = ((y[bi] == ci) & valid[bi]).double()
            if fg.sum() == 0:
                continue
            idx = order[bi, ci - first, :nv]
            err = (fg - p[bi, ci]).abs()[idx]
            fgs = fg[idx]
            inter = fgs.sum() - fgs.cumsum(0)
            union = fgs.sum() + (1.0 - fgs).cumsum(0)
            jac = 1.0 - inter / union
            jac = torch.cat([jac[:1], jac[1:] - jac[:-1]])
            terms.append(torch.dot(err, jac))
    loss = torch.zeros((), dtype=torch.float64)
    if terms and lovasz_weight != 0:
        loss = loss + lovasz_weight * torch.stack(terms).mean()
    if ce_weight != 0 and bool(valid.any()):
        yy = torch.where(valid, y, torch.full_like(y, -100)).reshape(labels.shape)
        loss = loss + ce_weight * F.cross_entropy(z, yy, weight=None if weight is None else weight.double(), ignore_index=-100)
    if loss.requires_grad:
        (loss * upstream).backward()
    return float(loss.detach()), (z.grad if z.grad is not None else torch.zeros_like(z)), len(terms)


@pytest.mark.parametrize("group", [g for g in R.SHAPES if g not in R.BIG])
def test_restatement_is_bermans_difference_form_in_float64(group):
    worst = 0.0
    for index, (tag, logits, labels, wt, ig, classes, lce, llv, up) in enumerate(R.group_cases(group)):
        ref = R.group_reference(group, index)
        loss, grad, n = berman(logits, labels, wt, ig, classes, lce, llv, up, ref["perm"])
        assert n == ref["N"], tag
        e = max(abs(loss - float(ref["loss"])) / max(abs(loss), 1e-300), R.rel_err(ref["grad"], grad))
        worst = max(worst, e)
        assert e <= 1e-12, (tag, e)
    print(group, "largest difference from float64 autograd of the difference form %.1e" % worst)


def test_order_is_the_stated_one():
    e = torch.tensor([[0.5, 0.25, 0.5, 0.5, 0.9, 0.25, 0.7]], dtype=torch.float64)
    g = torch.tensor([[False, True, True, False, False, False, True]])
    v = torch.tensor([[True, True, True, True, False, True, True]])
    # 0.9 is invalid: last.  0.7; the 0.5 group with g = 1 (index 2) first, then indices 0, 3; 0.25: g = 1 (1), then 5
    assert R.segment_order(e, g, v).tolist() == [[6, 2, 0, 3, 1, 5, 4]]
    om = R.jaccard_weights(g.gather(1, R.segment_order(e, g, v)), v.gather(1, R.segment_order(e, g, v)), torch.tensor([[3]]),
                           torch.float64)
    assert abs(float(om.sum()) - 1.0) <= 1e-15 and float(om[0, -1]) == 0.0          # the weights telescope to J_last = 1


def test_degenerate_values():
    logits, labels, weight = R.inputs("odd", "u8")
    none = torch.full_like(labels, R.IGNORE)
    r = R.lovasz_ref(logits, none, weight, R.IGNORE, "all", 1.0, 1.0)                        # no valid pixel
    assert float(r["loss"]) == 0.0 and r["N"] == 0 and not bool(r["grad"].any()) and not bool(r["m"].any())
    r = R.lovasz_ref(logits, torch.zeros_like(labels), weight, R.IGNORE, "foreground", 0.0, 1.0)     # no present segment
    assert float(r["loss"]) == 0.0 and r["N"] == 0 and not bool(r["grad"].any())
    one = torch.tensor([[[[0.3]], [[-0.2]]]])                                                   # one pixel: L = e
    r = R.lovasz_ref(one, torch.ones(1, 1, 1, dtype=torch.uint8), None, R.IGNORE, "foreground", 0.0, 1.0)
    p1 = float(torch.softmax(one.double(), 1)[0, 1])
    assert r["N"] == 1 and abs(float(r["loss"]) - (1.0 - p1)) <= 1e-15 and float(r["omega"]) == 1.0
    assert abs(float(r["grad"][0, 1]) + p1 * (1.0 - p1)) <= 1e-15
    same = torch.zeros(1, 2, 5, 7)                                                              # all errors equal: L = e J_last = e
    lab = torch.zeros(1, 5, 7, dtype=torch.uint8)
    lab[0, 2, 3:6] = 1
    r = R.lovasz_ref(same, lab, None, R.IGNORE, "all", 0.0, 1.0)
    assert r["N"] == 2 and abs(float(r["loss"]) - 0.5) <= 1e-15
    assert r["perm"][0, 1, :3].tolist() == [17, 18, 19]                                         # g = 1 first, then pixel index
    lg, lb = R.ig2_inputs()                                                                     # ignore_index inside [0, C)
    r = R.lovasz_ref(lg, lb, None, R.IG2_IGNORE, "all", 1.0, 1.0)
    assert r["N"] == 4 and not bool(r["present"][:, 2].any()) and not bool(r["m"][:, 2].any())
    assert not bool(r["grad"].permute(0, 2, 3, 1)[lb == R.IG2_IGNORE].any())


@functools.lru_cache(maxsize=None)
def measure_floors():
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                            # the order of an fp32 sum, and with it a floor, depends on the thread count
    try:
        out = {}
        for group in R.SHAPES:
            for tag, logits, labels, wt, ig, classes, lce, llv, up in R.group_cases(group):
                for check, e in R.floors_of(logits, labels, wt, ig, classes, lce, llv, up).items():
                    key = R.floor_key(check, group)
                    out[key] = max(out.get(key, 0.0), e)
        return out
    finally:
        torch.set_num_threads(threads)


def test_recorded_floors_are_the_measured_ones():
    measured = measure_floors()
    assert set(measured) == set(R.FLOOR), set(measured) ^ set(R.FLOOR)
    for key, m in sorted(measured.items()):
        want = max(m, R.FLOOR_MIN)
        print("%-12s recorded %.2e measured %.2e" % (key, R.FLOOR[key], m))
        assert R.FLOOR[key] >= R.FLOOR_MIN, key
        assert 0.5 * want <= R.FLOOR[key] <= 1.25 * want, (key, R.FLOOR[key], m)


def _mutant_case(mutant):
    """the inputs on which a mutant shows and the group whose floors bound it"""
    group = {"diff_form": "big", "absent_counted": "img", "batch_order": "img", "invalid_positions": "img"}.get(mutant, "c3")
    logits, labels, weight = R.inputs(group, "u8")
    return group, logits, labels, weight


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_checks_see_each_mutant(mutant):
    """each wrong formula misses at least one 4 x FLOOR bound of its group by 10 x or more; the miss is printed"""
    group, logits, labels, weight = _mutant_case(mutant)
    ref = R.lovasz_ref(logits, labels, weight, R.IGNORE, "foreground", 1.0, 0.8, upstream=R.UPSTREAM)
    keep = None if mutant in ("ascending", "invalid_positions", "batch_order") else ref["perm"]
    bad = R.lovasz_ref(logits, labels, weight, R.IGNORE, "foreground", 1.0, 0.8, upstream=R.UPSTREAM, perm=keep, mutant=mutant)
    ratio = {c: R.rel_err(bad[c], ref[c]) / (4 * R.FLOOR[R.floor_key(c, group)]) for c in ("loss", "grad")}
    if mutant == "batch_order":
        ratio["omega"] = math.inf                       # the segments themselves differ: nothing to compare element by element
    else:
        ratio["omega"] = R.elem_rel_err(bad["omega"], ref["omega"]) / (4 * R.FLOOR[R.floor_key("omega", group)])
    print("%-18s (%s) omega %.1e x bound, loss %.1e x bound, grad %.1e x bound" %
          (mutant, group, ratio["omega"], ratio["loss"], ratio["grad"]))
    if mutant == "diff_form":                           # the cancellation: per-element error of the weights, far above 1
        assert ratio["omega"] * 4 * R.FLOOR["omega.big"] >= 10.0 and ratio["grad"] >= 10.0
    elif mutant == "sign_dropped":                      # the value is untouched; only the gradient moves
        assert ratio["loss"] == 0.0 and ratio["grad"] >= 10.0
    elif mutant == "absent_counted":                    # the weights are untouched; the normaliser moves loss and gradient
        assert ratio["omega"] == 0.0 and min(ratio["loss"], ratio["grad"]) >= 10.0
    else:
        assert min(ratio["loss"], ratio["grad"]) >= 10.0


def test_exports_and_host_side_refusals():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in ("iswm_lovasz_keys", "iswm_lovasz_sort", "iswm_lovasz_weights", "iswm_lovasz_loss", "iswm_lovasz_bwd",
                 "iswm_lovasz_digits", "iswm_lovasz_tile", "iswm_lovasz_workspace"):
        assert name in _lib.EXPORTS and hasattr(lib, name)
    t, d = lib.iswm_lovasz_tile(), lib.iswm_lovasz_digits()
    assert d * 8 == 32 and t >= 256 and t % 64 == 0
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    ws = lib.iswm_lovasz_workspace
    assert ws(1, 1) > 0 and ws(14, 3 * t + 5) >= 4 * 4 * 14 * (3 * t + 5)
    assert ws(1, 0) == 0 and "keys per segment" in err()
    assert ws(1, (1 << 24) + 1) == 0 and "keys per segment" in err()
    assert ws(0, 4) == 0 and "segments" in err()
    assert ws(128, 1 << 24) == 0 and "2^31" in err()
    assert ws(1, 1 << 24) > 0
    keys = lambda lg=p, nb=1, b=1, c=2, hw=4, cl=0, k=p, s=p: lib.iswm_lovasz_keys(lg, p, nb, b, c, hw, None, 255, cl, k, p, p, s, None)
    assert keys(lg=None) == 1 and "null" in err()
    assert keys(s=None) == 1 and "null" in err()
    assert keys(c=9) == 1 and "classes" in err()
    assert keys(c=0) == 1 and "classes" in err()
    assert keys(c=1) == 1 and "foreground" in err()
    assert keys(cl=2) == 1 and "classes" in err()
    assert keys(nb=4) == 1 and "uint8 or int64" in err()
    assert keys(hw=0) == 1 and "shape" in err()
    assert keys(hw=(1 << 24) + 1) == 1 and "keys per segment" in err()
    assert keys(b=200, hw=1 << 24) == 1 and "2^31" in err()
    out2 = (ctypes.c_double * 64)()
    q = ctypes.cast(out2, ctypes.c_void_p)
    assert lib.iswm_lovasz_sort(None, 1, 4, p, 1 << 20, q, q, None) == 1 and "null" in err()
    assert lib.iswm_lovasz_sort(p, 1, 4, None, 1 << 20, q, q, None) == 1 and "null" in err()
    assert lib.iswm_lovasz_sort(p, 1, 4, p, 1 << 20, p, q, None) == 1 and "input" in err()
    assert lib.iswm_lovasz_sort(p, 1, 0, p, 1 << 20, q, q, None) == 1 and "keys per segment" in err()
    assert lib.iswm_lovasz_sort(p, 1, (1 << 24) + 1, p, 1 << 40, q, q, None) == 1 and "keys per segment" in err()
    assert lib.iswm_lovasz_sort(p, 0, 4, p, 1 << 20, q, q, None) == 1 and "segments" in err()
    assert lib.iswm_lovasz_sort(p, 1, 4, p, ws(1, 4) - 1, q, q, None) == 1 and "workspace" in err()
    assert lib.iswm_lovasz_weights(p, p, None, 1, 4, p, 1 << 20, q, q, None) == 1 and "null" in err()
    assert lib.iswm_lovasz_weights(p, p, p, 1, 0, p, 1 << 20, q, q, None) == 1 and "keys per segment" in err()
    assert lib.iswm_lovasz_weights(p, p, p, 1, 4, p, ws(1, 4) - 1, q, q, None) == 1 and "workspace" in err()
    assert lib.iswm_lovasz_loss(None, 1.0, 1.0, p, None) == 1 and "null" in err()
    assert lib.iswm_lovasz_loss(p, -1.0, 1.0, p, None) == 1 and "weights" in err()
    assert lib.iswm_lovasz_loss(p, 1.0, float("inf"), p, None) == 1 and lib.iswm_lovasz_loss(p, float("nan"), 1.0, p, None) == 1
    bwd = lambda nb=1, c=2, hw=4, cl=0, m=p, up=p: lib.iswm_lovasz_bwd(p, p, nb, 1, c, hw, None, 255, cl, m, p, up, p, None)
    assert bwd(m=None) == 1 and "null" in err()
    assert bwd(up=None) == 1 and "null" in err()
    assert bwd(c=9) == 1 and "classes" in err()
    assert bwd(c=1) == 1 and "foreground" in err()
    assert bwd(cl=-1) == 1 and bwd(nb=3) == 1 and bwd(hw=0) == 1 and bwd(hw=(1 << 24) + 1) == 1


def test_module_refuses_bad_parameters_and_cpu_tensors():
    from iswm_amd.utils.loss import LovaszSoftmaxLoss
    for kw in (dict(classes="present"), dict(ce_weight=-1.0), dict(lovasz_weight=-0.5), dict(lovasz_weight=float("inf")),
               dict(lovasz_weight=float("nan")), dict(ce_weight=0.0, lovasz_weight=0.0)):
        with pytest.raises(ValueError):
            LovaszSoftmaxLoss(**kw)
    d = LovaszSoftmaxLoss()
    assert (d.classes, d.ce_weight, d.lovasz_weight, d.weight, d.ignore_index, d.group, d.last_present) == \
        ("foreground", 0.0, 1.0, None, 255, None, None)
    m = LovaszSoftmaxLoss(classes="all", ce_weight=1.0, lovasz_weight=0.5, weight=torch.tensor([1.0, 3.0]))
    assert torch.equal(m.weight, torch.tensor([1.0, 3.0]))
    with pytest.raises(ValueError):                                          # no CPU fallback
        d(torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64))


def test_parser_defaults_refusals_and_criterion_types():
    from iswm_amd import train
    from iswm_amd.utils.loss import CrossEntropyLoss, DiceLoss, LovaszSoftmaxLoss, OhemCrossEntropyLoss
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    assert parse().lovasz_weight == 0.0
    for bad in (["--lovasz_weight", "-1"], ["--lovasz_weight", "inf"], ["--lovasz_weight", "nan"],
                ["--lovasz_weight", "1", "--overlap_loss", "dice"], ["--lovasz_weight", "0.5", "--overlap_loss", "focal_tversky"],
                ["--lovasz_weight", "1", "--ohem_thresh", "0.7"], ["--ce_weight", "0"], ["--overlap_loss", "lovasz"],
                ["--lovasz_weight", "1", "--ce_weight", "-1"]):
        with pytest.raises(SystemExit):
            parse(*bad)
    cw = torch.tensor([1.0, 3.0])
    # off: exactly what setup_criterion returned before the option existed
    crit = train.setup_criterion(parse(), cw)
    assert type(crit) is CrossEntropyLoss and torch.equal(crit.weight, cw) and crit.ignore_index == 255 and crit.group is None
    assert train.setup_criterion(parse("--loss_type", "ce_loss"), cw).weight is None
    assert type(train.setup_criterion(parse("--overlap_loss", "dice"), cw)) is DiceLoss
    assert type(train.setup_criterion(parse("--ohem_thresh", "0.7"), cw)) is OhemCrossEntropyLoss
    m = train.setup_criterion(parse("--lovasz_weight", "1", "--ce_weight", "0"), cw)
    assert type(m) is LovaszSoftmaxLoss and (m.classes, m.ce_weight, m.lovasz_weight, m.ignore_index) == ("foreground", 0.0, 1.0, 255)
    assert torch.equal(m.weight, cw)
    m = train.setup_criterion(parse("--lovasz_weight", "0.5", "--overlap_classes", "all", "--loss_type", "ce_loss"), cw)
    assert (m.classes, m.ce_weight, m.lovasz_weight, m.weight) == ("all", 1.0, 0.5, None)
