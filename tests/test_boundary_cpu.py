"""No GPU: the fourth header's binding, the two restatements of the signed distance map (brute force and scipy) against each
other, the restatement of the boundary criterion (tests/boundary_ref.py) against float64 autograd of the written-out loss, the
degenerate values, the fp32 floors measured again, eight mutants that the checks of tests/test_boundary_gpu.py must see, the new
entry points' host-side refusals, the module's and the parser's refusals, and setup_criterion with the new options off."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import boundary_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BD_NAMES = ("iswm_signed_edt_workspace", "iswm_signed_edt", "iswm_boundary_loss_partials", "iswm_boundary_loss_fwd",
            "iswm_boundary_loss_coeffs", "iswm_boundary_loss_bwd")
KD_NAMES = ("iswm_distill_loss_partials", "iswm_distill_loss_fwd", "iswm_distill_loss_coeffs", "iswm_distill_loss_bwd")
EXT_NAMES = ("iswm_dwconv3x3_pre_fwd", "iswm_dwconv3x3_pre_bwd_workspace", "iswm_dwconv3x3_pre_bwd")


def test_the_fourth_header_binds_into_a_table_of_its_own():
    from iswm_amd import _lib
    assert os.path.samefile(_lib.BD_HEADER, os.path.join(ROOT, "include", "iswm_hip_bd.h"))
    assert _lib.BD_EXPORTS == BD_NAMES and tuple(_lib._BD_SIGS) == BD_NAMES
    assert len(_lib.EXPORTS) == 162 and tuple(_lib._SIGS) == _lib.EXPORTS                 # the other three tables are what they were
    assert _lib.EXT_EXPORTS == EXT_NAMES and tuple(_lib._EXT_SIGS) == EXT_NAMES
    assert _lib.KD_EXPORTS == KD_NAMES and tuple(_lib._KD_SIGS) == KD_NAMES
    assert not set(BD_NAMES) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.KD_EXPORTS))
    with open(_lib.BD_HEADER) as f:
        text = f.read()
    with open(_lib.HEADER) as f:
        base = f.read()
    consts, structs, sigs = _lib.parse_header(text, base=base)
    assert not consts and not structs and tuple(sigs) == BD_NAMES                         # prototypes only
    c = ctypes
    assert sigs["iswm_signed_edt_workspace"] == (c.c_int64, [c.c_int] * 5)
    assert sigs["iswm_signed_edt"] == (c.c_int, [c.c_void_p] + [c.c_int] * 7 + [c.c_void_p, c.c_void_p, c.c_int64, c.c_void_p])
    assert sigs["iswm_boundary_loss_partials"] == (c.c_int64, [c.c_int64])
    assert sigs["iswm_boundary_loss_fwd"] == (c.c_int, [c.c_void_p] * 2 + [c.c_int] * 3 + [c.c_int64, c.c_int, c.c_void_p, c.c_void_p,
                                                                                          c.c_int, c.c_float] + [c.c_void_p] * 3)
    assert sigs["iswm_boundary_loss_coeffs"] == (c.c_int, [c.c_void_p, c.c_int, c.c_double, c.c_double] + [c.c_void_p] * 3)
    assert sigs["iswm_boundary_loss_bwd"] == (c.c_int, [c.c_void_p] * 2 + [c.c_int] * 3 + [c.c_int64, c.c_int, c.c_void_p, c.c_void_p,
                                                                                          c.c_int, c.c_float] + [c.c_void_p] * 4)
    with pytest.raises(ValueError, match="again"):                                        # a name of the main header is refused
        _lib.parse_header(text.replace("iswm_boundary_loss_partials(", "iswm_loss_blocks("), base=base)


def test_every_new_name_is_a_symbol_of_the_built_library_and_refuses_bad_arguments():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in BD_NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BD_SIGS[name][0], list(_lib._BD_SIGS[name][1])), name
    for npix in (1, 1024, 1025, 4 * 515 * 515, 2897 * 2897):
        assert lib.iswm_boundary_loss_partials(npix) == 4 * lib.iswm_loss_blocks(npix)
    ws = lib.iswm_signed_edt_workspace
    assert ws(16, 2, 513, 513, 1) == 16 * 513 * 513 * 4 and ws(2, 3, 5, 7, 0) == 2 * 3 * 5 * 7 * 4 and ws(1, 2, 4096, 4096, 1) == 4 * 4096 ** 2
    assert ws(1, 2, 4097, 4, 1) == -1 and ws(1, 2, 4, 4097, 1) == -1 and ws(1, 1, 4, 4, 1) == -1 and ws(0, 2, 4, 4, 1) == -1
    assert ws(1, 2, 4, 4, 2) == -1
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def edt(lb=p, nb=1, b=1, c=2, h=2, w=2, first=1, sd2=p, work=p, nbytes=16):
        return lib.iswm_signed_edt(lb, nb, b, c, h, w, first, 255, sd2, work, nbytes, None)
    assert edt(lb=None) == 1 and "null" in err()
    assert edt(sd2=None) == 1 and edt(work=None) == 1
    assert edt(w=4097) == 1 and "sides up to 4096" in err()                                # refused on the host: nothing is launched
    assert edt(h=4097) == 1 and "sides up to 4096" in err()
    assert edt(c=1) == 1 and "no class plane" in err()
    assert edt(first=2) == 1 and "first_class" in err()
    assert edt(b=0) == 1 and "shape" in err()
    assert edt(nb=4) == 1 and "uint8 or int64" in err()
    assert edt(nbytes=15) == 1 and "workspace" in err()

    def fwd(z=p, lb=p, nb=1, b=1, c=2, hw=4, first=1, sd2=p, clip=0.0, part=p, sums=p):
        return lib.iswm_boundary_loss_fwd(z, lb, nb, b, c, hw, first, sd2, None, 255, clip, part, sums, None)
    assert fwd(z=None) == 1 and "null" in err()
    assert fwd(sums=None) == 1 and "null" in err()
    assert fwd(sd2=None) == 1 and "distance map pointer null" in err()
    assert fwd(c=0) == 1 and "classes" in err()
    assert fwd(c=9) == 1 and "classes (the boundary loss takes 1 to 8)" in err()
    assert fwd(c=1) == 1 and "no class plane" in err()
    assert fwd(first=3) == 1 and "first_class" in err()
    assert fwd(nb=4) == 1 and "uint8 or int64" in err()
    assert fwd(hw=0) == 1 and "shape" in err()
    assert fwd(b=2, hw=2 ** 36) == 1 and "shape" in err()                                  # N is exact up to 2^36 pixels
    for clip in (-1.0, float("inf"), float("nan")):
        assert fwd(clip=clip) == 1 and "clip" in err()

    def bwd(z=p, lb=p, nb=1, b=1, c=2, hw=4, first=1, sd2=p, clip=0.0, coef=p, up=p, grad=p):
        return lib.iswm_boundary_loss_bwd(z, lb, nb, b, c, hw, first, sd2, None, 255, clip, coef, up, grad, None)
    assert bwd(coef=None) == 1 and "null" in err()
    assert bwd(up=None) == 1 and bwd(grad=None) == 1
    assert bwd(sd2=None) == 1 and "distance map pointer null" in err()
    assert bwd(c=9) == 1 and "classes" in err()
    assert bwd(nb=2) == 1 and "uint8 or int64" in err()
    assert bwd(clip=-0.5) == 1 and "clip" in err()

    def coeffs(sums=p, nsel=1, lce=1.0, lbd=1.0, out=p, coef=p):
        return lib.iswm_boundary_loss_coeffs(sums, nsel, lce, lbd, out, coef, None)
    assert coeffs(sums=None) == 1 and "null" in err()
    assert coeffs(out=None) == 1 and coeffs(coef=None) == 1
    assert coeffs(nsel=0) == 1 and coeffs(nsel=9) == 1 and "selected classes" in err()
    assert coeffs(lce=-1.0) == 1 and coeffs(lbd=-1.0) == 1 and coeffs(lbd=float("inf")) == 1 and "weights" in err()


SMALL_MAPS = [n for n, (b, c, h, w, _) in R.MAP_SHAPES.items() if h * w <= R.BRUTE_MAX]


@pytest.mark.parametrize("shape", SMALL_MAPS)
def test_brute_force_equals_scipy(shape):
    """every small plane, every pattern, both label widths, both class selections, ignore_index 255 and ignore_index inside the
    class range"""
    b, c, h, w, _ = R.MAP_SHAPES[shape]
    seen_invalid = False
    for pat, kind, classes, ig in itertools.product(R.map_runs(shape), ("u8", "i64"), R.CLASSES, (R.IGNORE, c - 1)):
        labels = R.map_labels(shape, pat, kind, ig)
        a = R.signed_edt_ref(labels, c, classes, ig, how="brute")
        s = R.signed_edt_ref(labels, c, classes, ig, how="scipy")
        assert a.dtype == torch.int32 and a.shape == (b, len(R.selected(c, classes)), h, w)
        assert torch.equal(a, s), (shape, pat, kind, classes, ig)
        invalid = ~R.valid_mask(labels, c, ig)
        seen_invalid |= bool(invalid.any())
        assert not bool(a.permute(0, 2, 3, 1)[invalid].any()), "an invalid pixel has a distance"
    assert seen_invalid or h * w < 4


def test_the_map_on_cases_worked_out_by_hand():
    y = torch.zeros(1, 3, 5, dtype=torch.int64)
    y[0, 1, 1] = 1
    want = torch.tensor([[2, 1, 2, 5, 10], [1, -1, 1, 4, 9], [2, 1, 2, 5, 10]], dtype=torch.int32)
    assert torch.equal(R.signed_edt_ref(y, 2)[0, 0], want)
    both = R.signed_edt_ref(y, 2, "all")
    assert torch.equal(both[0, 1], want) and torch.equal(both[0, 0], -want)               # with two classes the planes mirror
    y[0, 1, 0] = 255                                                                      # an ignored pixel is in neither set
    want[1, 0] = 0
    assert torch.equal(R.signed_edt_ref(y, 2)[0, 0], want)
    y[0, 0, 1] = y[0, 2, 1] = y[0, 1, 2] = 255                                            # ... and no contour: the nearest background
    got = R.signed_edt_ref(y, 2)[0, 0]                                                    # pixel of (1, 1) is a diagonal one
    assert int(got[1, 1]) == -2 and int(got[0, 1]) == 0 and int(got[1, 3]) == 4
    for fill in (0, 1, 255):                                                              # F or G empty: the whole plane is 0
        assert not bool(R.signed_edt_ref(torch.full((2, 4, 4), fill, dtype=torch.uint8), 2).any())
    band = R.label_case("img", "u8")[:1]
    phi = R.phi_of(R.signed_edt_ref(band, 2), 0.0)
    assert float(phi.max()) > 30 and float(phi.min()) <= 0.0 and bool((phi == 0).any())   # structure: |phi| from 0 to above 30


def plain_autograd(logits, labels, sd2, weight, ignore_index, lce, lbd, clip, classes):
    """the loss written the way a user would with torch ops, float64, differentiated by autograd"""
    z = logits.double().requires_grad_(True)
    c = z.shape[1]
    y = labels.long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    d = sd2.double()
    dist = torch.where(d > 0, d.abs().sqrt(), torch.where(d < 0, 1.0 - d.abs().sqrt(), torch.zeros_like(d)))
    if clip > 0:
        dist = dist.clamp(-clip, clip)
    ks = R.selected(c, classes)
    p = F.softmax(z, 1)[:, ks]
    n = int(valid.sum())
    loss = lbd * (p * dist * valid[:, None]).sum() / (n * len(ks)) if n else (z * 0).sum()
    if lce != 0:
        target = torch.where(valid, y, torch.full_like(y, -100))
        loss = loss + lce * F.cross_entropy(z, target, weight=None if weight is None else weight.double(), ignore_index=-100)
    loss.backward()
    return loss.detach(), z.grad


def _close(ref, loss, grad):
    return abs(float(ref["loss"]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))) and \
        float((ref["grad"] - grad).abs().max()) <= 1e-12 * max(1.0, float(grad.abs().max()))


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_restatement_equals_float64_autograd(case):
    shape, kind, scale = case
    logits, labels, weight, sd2, classes = R.case(shape, kind, R.SCALES[scale])
    for combo in R.COMBOS:
        wt, lce, lbd, clip = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], combo)
        loss, grad = plain_autograd(logits, labels, sd2, wt, R.IGNORE, lce, lbd, clip, classes)
        assert _close(ref, loss, grad), R.combo_id(combo)
        assert abs(float(ref["ce"] + ref["bd"]) - float(ref["loss"])) == 0.0
        assert int(ref["sums"][3]) == int(R.valid_mask(labels, logits.shape[1]).sum())
        invalid = ~R.valid_mask(labels, logits.shape[1])
        assert not bool(ref["grad"].permute(0, 2, 3, 1)[invalid].any())


def test_restatement_equals_autograd_on_the_other_inputs():
    """the ignore_index inside the class range, the degenerate label patterns and the data-parallel batch"""
    logits, labels, weight, sd2, classes = R.case(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE, R.IG2_PATTERNS)
    assert int((labels == 2).sum()) > 20 and sd2.shape[1] == 2 and not bool(sd2[:, 1].any())   # class 2 is ignored: its plane is 0
    for combo in R.IG2_COMBOS:
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, combo, R.IG2_IGNORE, R.IG2_PATTERNS)
        loss, grad = plain_autograd(logits, labels, sd2, weight, R.IG2_IGNORE, combo[1], combo[2], combo[3], classes)
        assert _close(ref, loss, grad)
        assert int(ref["sums"][3]) == int(((labels != 2) & (labels < 3)).sum())           # none of the pixels labelled 2 in N


@pytest.mark.parametrize("pattern", R.DEGENERATE)
def test_degenerate_values(pattern):
    """all ignored: N = 0, everything is exactly 0 (CE left out: lce = 0).  No foreground / all foreground: the map is 0 over the
    whole plane, the boundary term and its gradient are exactly 0 and what is left is the CE."""
    logits, labels, weight, sd2, classes = R.degenerate_case(pattern)
    assert not bool(sd2.any())
    for combo in R.degenerate_combos(pattern):
        wt, lce, lbd, clip = R.combo_args(combo, weight)
        ref = R.degenerate_reference(pattern, combo)
        loss, grad = plain_autograd(logits, labels, sd2, wt, R.IGNORE, lce, lbd, clip, classes)
        assert _close(ref, loss, grad)
        assert float(ref["bd"]) == 0.0 and float(ref["sums"][2]) == 0.0
        if pattern == "all_ignored":
            assert lce == 0 and float(ref["loss"]) == 0.0 and not bool(ref["grad"].any()) and not bool(ref["sums"].any())
        elif lce == 0:
            assert float(ref["loss"]) == 0.0 and not bool(ref["grad"].any())              # lambda_ce = 0: nothing is left
        else:
            only_ce = R.boundary_ref(logits, labels, sd2, wt, R.IGNORE, lce, 0.0, clip, classes)
            assert torch.equal(only_ce["loss"], ref["loss"]) and torch.equal(only_ce["grad"], ref["grad"])
            assert float(ref["sums"][3]) == labels.numel()
    s, lb, w, m = R.ddp_inputs()
    ref = R.ddp_reference()
    loss, grad = plain_autograd(s, lb, m, w, R.IGNORE, R.DDP_COMBO[1], R.DDP_COMBO[2], R.DDP_COMBO[3], "foreground")
    assert _close(ref, loss, grad) and not bool(ref["grad"][:2].any())


def _errs(logits, labels, sd2, wt, ignore_index, lce, lbd, clip, classes, ref):
    low = R.boundary_ref(logits, labels, sd2, wt, ignore_index, lce, lbd, clip, classes, dtype=torch.float32)
    return R.errors(low["sums"], low["loss"], low["grad"], ref)


@functools.lru_cache(maxsize=None)
def measure_floors():
    """{key: largest fp32-vs-float64 error of the group's cases} -- the figures FLOOR records (before the 2^-24 minimum); on one
    thread (the order of torch's fp32 sums), and the thread count is put back for the tests that run after this file"""
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        return _measure_floors()
    finally:
        torch.set_num_threads(threads)


def _measure_floors():
    out = {}

    def take(group, errs):
        for k, e in errs.items():
            key = R.floor_key(k, group)
            out[key] = max(out.get(key, 0.0), e)
    for shape, kind, scale in R.INPUT_CASES:
        logits, labels, weight, sd2, classes = R.case(shape, kind, R.SCALES[scale])
        for combo in R.COMBOS:
            wt, lce, lbd, clip = R.combo_args(combo, weight)
            take(R.group(shape, scale), _errs(logits, labels, sd2, wt, R.IGNORE, lce, lbd, clip, classes,
                                              R.reference(shape, kind, R.SCALES[scale], combo)))
    for name in R.BIG:
        logits, labels, weight, sd2, classes = R.case(name, "u8", 1.0)
        wt, lce, lbd, clip = R.combo_args(R.BIG_COMBO, weight)
        take(name, _errs(logits, labels, sd2, wt, R.IGNORE, lce, lbd, clip, classes, R.reference(name, "u8", 1.0, R.BIG_COMBO)))
    for pattern in ("no_foreground", "all_foreground"):
        logits, labels, weight, sd2, classes = R.degenerate_case(pattern)
        for combo in R.degenerate_combos(pattern):
            wt, lce, lbd, clip = R.combo_args(combo, weight)
            take("degen", _errs(logits, labels, sd2, wt, R.IGNORE, lce, lbd, clip, classes, R.degenerate_reference(pattern, combo)))
    logits, labels, weight, sd2, classes = R.case(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE, R.IG2_PATTERNS)
    for combo in R.IG2_COMBOS:
        take("ig2", _errs(logits, labels, sd2, weight, R.IG2_IGNORE, combo[1], combo[2], combo[3], classes,
                          R.reference(R.IG2_SHAPE, "u8", 1.0, combo, R.IG2_IGNORE, R.IG2_PATTERNS)))
    s, lb, w, m = R.ddp_inputs()
    take("ddp", _errs(s, lb, m, w, R.IGNORE, R.DDP_COMBO[1], R.DDP_COMBO[2], R.DDP_COMBO[3], "foreground", R.ddp_reference()))
    return out


def test_recorded_floors_are_the_measured_ones():
    measured = measure_floors()
    assert set(measured) == set(R.FLOOR), set(measured) ^ set(R.FLOOR)
    for key, m in sorted(measured.items()):
        want = max(m, R.FLOOR_MIN)
        print("%-18s recorded %.2e measured %.2e" % (key, R.FLOOR[key], m))
        assert R.FLOOR[key] >= R.FLOOR_MIN, key
        assert 0.5 * want <= R.FLOOR[key] <= 1.25 * want, (key, R.FLOOR[key], m)


MAP_MUTANT_CASE = {"cityblock": ("bands", "foreground"), "column_only": ("bands", "foreground"),
                   "invalid_as_background": ("one_bg", "foreground")}


@pytest.mark.parametrize("mutant", R.MAP_MUTANTS)
def test_integer_equality_sees_each_map_mutant(mutant):
    """a wrong map differs from the exact one in at least one pixel of an image of the ig2 labels (three classes, ignore_index 2)"""
    _, labels, _, sd2, classes = R.case(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE, R.IG2_PATTERNS)
    pat, classes = MAP_MUTANT_CASE[mutant]
    image = R.IG2_PATTERNS.index(pat)
    bad = R.signed_edt_ref(labels, 3, classes, R.IG2_IGNORE, how="brute", mutant=mutant)
    differ = int((bad[image] != sd2[image]).sum())
    print(mutant, "differs in", differ, "pixels of image", image)
    assert differ >= 1


@pytest.mark.parametrize("mutant", R.FORMULA_MUTANTS)
def test_bounds_see_each_formula_mutant(mutant):
    """a wrong formula misses at least one of the 4 x FLOOR bounds of tests/test_boundary_gpu.py by 3 x or more on the ig2 inputs
    (three classes, ignore_index 2, class weights, lce 1, lbd 2); the clamp mutant is the definition itself without a clamp and is
    judged at clip 8, the others at both"""
    logits, labels, weight, sd2, classes = R.case(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE, R.IG2_PATTERNS)
    for combo in R.IG2_COMBOS:
        _, lce, lbd, clip = combo
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, combo, R.IG2_IGNORE, R.IG2_PATTERNS)
        bad = R.boundary_ref(logits, labels, sd2, weight, R.IG2_IGNORE, lce, lbd, clip, classes, mutant=mutant)
        if mutant == "clamp_before_minus_one" and clip == 0:
            assert torch.equal(bad["loss"], ref["loss"]) and torch.equal(bad["grad"], ref["grad"])
            continue
        ratio = {k: e / (4 * R.FLOOR[R.floor_key(k, "ig2")]) for k, e in R.errors(bad["sums"], bad["loss"], bad["grad"], ref).items()}
        print(mutant, "clip", clip, {k: "%.1e" % v for k, v in ratio.items()})
        assert max(ratio.values()) >= 3.0, ratio


def test_module_refuses_bad_parameters_and_bad_tensors():
    from iswm_amd import ops
    from iswm_amd.utils.loss import BoundaryLoss
    for kw in (dict(classes="background"), dict(ce_weight=-1.0), dict(boundary_weight=-0.5), dict(ce_weight=0.0, boundary_weight=0.0),
               dict(boundary_weight=float("inf")), dict(boundary_weight=float("nan")), dict(clip=-1.0), dict(clip=float("inf")),
               dict(clip=float("nan"))):
        with pytest.raises(ValueError):
            BoundaryLoss(**kw)
    d = BoundaryLoss(classes="all", ce_weight=0, clip=8, weight=torch.tensor([1.0, 3.0]))
    assert (d.classes, d.ce_weight, d.boundary_weight, d.clip, d.ignore_index, d.group) == ("all", 0.0, 1.0, 8.0, 255, None)
    assert torch.equal(d.weight, torch.tensor([1.0, 3.0])) and d.last_terms is None and d.last_valid is None
    z, y = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        BoundaryLoss()(z, y)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.signed_edt(y, 2)
    with pytest.raises(ValueError, match="foreground"):
        ops.signed_edt(y, 2, classes="some")


def test_parser_defaults_and_refusals():
    from iswm_amd import train
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    o = parse()
    assert (o.boundary_weight, o.boundary_clip, o.boundary_ramp_itrs) == (0.0, 0.0, 0)
    o = parse("--boundary_weight", "0.01", "--boundary_clip", "8", "--boundary_ramp_itrs", "100")
    assert (o.boundary_weight, o.boundary_clip, o.boundary_ramp_itrs) == (0.01, 8.0, 100)
    o = parse("--boundary_weight", "1", "--ce_weight", "0")                                 # the boundary term alone is a loss
    assert (o.boundary_weight, o.ce_weight) == (1.0, 0.0)
    bw = ["--boundary_weight", "0.5"]
    for bad in (bw + ["--overlap_loss", "dice"], bw + ["--lovasz_weight", "1"], bw + ["--ohem_thresh", "0.7"],
                bw + ["--distill_ckpt", "t.pth", "--distill_model", "deeplabv3plus_resnet101"], bw + ["--test_only"],
                ["--ce_weight", "0"], ["--ce_weight", "0", "--boundary_weight", "0"],
                ["--boundary_weight", "-1"], ["--boundary_weight", "inf"], ["--boundary_weight", "nan"],
                bw + ["--boundary_clip", "-1"], bw + ["--boundary_clip", "inf"], bw + ["--boundary_clip", "nan"],
                bw + ["--boundary_ramp_itrs", "-1"], bw + ["--boundary_ramp_itrs", "1.5"],
                ["--boundary_clip", "8"], ["--boundary_ramp_itrs", "10"]):                   # no --boundary_weight
        with pytest.raises(SystemExit):
            parse(*bad)


def test_the_ramp_is_a_function_of_the_iteration():
    """linear from 0 to W over the first N iterations, W after them; taken from the current iteration, so a resumed run continues"""
    import argparse
    from iswm_amd import train
    o = argparse.Namespace(boundary_weight=0.5, boundary_ramp_itrs=4)
    assert [train.boundary_factor(o, i) for i in (1, 2, 3, 4, 5, 400)] == [0.125, 0.25, 0.375, 0.5, 0.5, 0.5]
    assert train.boundary_factor(argparse.Namespace(boundary_weight=0.5, boundary_ramp_itrs=0), 1) == 0.5
    assert train.boundary_factor(argparse.Namespace(), 7) == 0.0


def _describe(crit):
    return (type(crit).__name__, getattr(crit, "params", None), getattr(crit, "ignore_index", None),
            None if getattr(crit, "weight", None) is None else crit.weight.tolist(), getattr(crit, "group", None),
            tuple(getattr(crit, n, None) for n in ("thresh", "min_kept", "classes", "ce_weight", "lovasz_weight", "reduction",
                                                   "temperature", "distill_weight")))


def test_setup_criterion_is_unchanged_with_the_new_options_off():
    """every existing criterion option combination: an options object WITHOUT the boundary_* attributes (as older callers build
    it) and the parser's own defaults give the same criterion, of the type and with the parameters it had"""
    import argparse
    from iswm_amd import train
    from iswm_amd.utils.loss import (BoundaryLoss, CrossEntropyLoss, DiceLoss, DistillationLoss, LovaszSoftmaxLoss,
                                     OhemCrossEntropyLoss, TverskyLoss)
    cw = torch.tensor([1.0, 3.0])
    parse = lambda a: train.get_argparser().parse_args(list(a))
    want = {(): CrossEntropyLoss, ("--overlap_loss", "dice"): DiceLoss, ("--overlap_loss", "tversky"): TverskyLoss,
            ("--overlap_loss", "focal_tversky"): TverskyLoss, ("--lovasz_weight", "0.5"): LovaszSoftmaxLoss,
            ("--ohem_thresh", "0.7"): OhemCrossEntropyLoss,
            ("--distill_ckpt", "t.pth", "--distill_model", "deeplabv3plus_resnet50"): DistillationLoss}
    for (extra, kind), loss_type, ce in itertools.product(want.items(), ("ce_loss", "IWce_loss"), ("1", "0.5")):
        o = parse(extra + ("--loss_type", loss_type, "--ce_weight", ce))
        assert o.boundary_weight == 0
        old = argparse.Namespace(**{k: v for k, v in vars(o).items() if not k.startswith("boundary_")})
        a, b = train.setup_criterion(o, cw), train.setup_criterion(old, cw)
        assert type(a) is kind and type(b) is kind and _describe(a) == _describe(b), extra
        assert (a.weight is None) == (loss_type == "ce_loss")
    d = train.setup_criterion(parse(["--boundary_weight", "0.5", "--boundary_clip", "8", "--ce_weight", "0.25"]), cw)
    assert type(d) is BoundaryLoss and (d.classes, d.ce_weight, d.boundary_weight, d.clip) == ("foreground", 0.25, 0.5, 8.0)
    assert torch.equal(d.weight, cw) and d.group is None
    assert train.setup_criterion(parse(["--boundary_weight", "1", "--loss_type", "ce_loss"]), cw).weight is None
