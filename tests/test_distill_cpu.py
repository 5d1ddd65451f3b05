"""No GPU: the third header's binding, the restatement of the distillation criterion (tests/distill_ref.py) against float64
autograd of the written-out loss, the fp32 floors measured again, seven mutants that the bounds of tests/test_distill_gpu.py must
see, the new entry points' host-side refusals, the module's and the parser's refusals, and setup_criterion with the new options
off."""
import ctypes
import functools
import itertools
import os

import pytest
import torch
import torch.nn.functional as F

from tests import distill_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_NAMES = ("iswm_distill_loss_partials", "iswm_distill_loss_fwd", "iswm_distill_loss_coeffs", "iswm_distill_loss_bwd")
EXT_NAMES = ("iswm_dwconv3x3_pre_fwd", "iswm_dwconv3x3_pre_bwd_workspace", "iswm_dwconv3x3_pre_bwd")


def test_the_third_header_binds_into_a_table_of_its_own():
    from iswm_amd import _lib
    assert os.path.samefile(_lib.KD_HEADER, os.path.join(ROOT, "include", "iswm_hip_kd.h"))
    assert _lib.KD_EXPORTS == KD_NAMES and tuple(_lib._KD_SIGS) == KD_NAMES
    assert len(_lib.EXPORTS) == 162 and tuple(_lib._SIGS) == _lib.EXPORTS                 # the other two tables are what they were
    assert _lib.EXT_EXPORTS == EXT_NAMES and tuple(_lib._EXT_SIGS) == EXT_NAMES
    assert not set(KD_NAMES) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS))
    with open(_lib.KD_HEADER) as f:
        text = f.read()
    with open(_lib.HEADER) as f:
        base = f.read()
    consts, structs, sigs = _lib.parse_header(text, base=base)
    assert not consts and not structs and tuple(sigs) == KD_NAMES                         # prototypes only
    c = ctypes
    assert sigs["iswm_distill_loss_partials"] == (c.c_int64, [c.c_int64])
    assert sigs["iswm_distill_loss_fwd"] == (c.c_int, [c.c_void_p] * 3 + [c.c_int] * 3 + [c.c_int64, c.c_void_p, c.c_int, c.c_float,
                                                                                     c.c_void_p, c.c_void_p, c.c_void_p])
    assert sigs["iswm_distill_loss_coeffs"] == (c.c_int, [c.c_void_p] + [c.c_double] * 3 + [c.c_void_p] * 3)
    assert sigs["iswm_distill_loss_bwd"] == (c.c_int, [c.c_void_p] * 3 + [c.c_int] * 3 + [c.c_int64, c.c_void_p, c.c_int, c.c_float] +
                                             [c.c_void_p] * 4)
    with pytest.raises(ValueError, match="again"):                                        # a name of the main header is refused
        _lib.parse_header(text.replace("iswm_distill_loss_partials(", "iswm_loss_blocks("), base=base)


def test_every_new_name_is_a_symbol_of_the_built_library_and_refuses_bad_arguments():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in KD_NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib._KD_SIGS[name][0], list(_lib._KD_SIGS[name][1])), name
    blocks = lib.iswm_loss_blocks
    for npix in (1, 1024, 1025, 4 * 515 * 515, 2897 * 2897):
        assert lib.iswm_distill_loss_partials(npix) == 5 * blocks(npix)
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def fwd(s=p, t=p, lb=p, nb=1, b=1, c=2, hw=4, inv=0.5, part=p, sums=p):
        return lib.iswm_distill_loss_fwd(s, t, lb, nb, b, c, hw, None, 255, inv, part, sums, None)
    assert fwd(s=None) == 1 and "null" in err()
    assert fwd(sums=None) == 1 and "null" in err()
    assert fwd(t=None) == 1 and "teacher pointer null" in err()
    assert fwd(c=0) == 1 and "classes" in err()
    assert fwd(c=9) == 1 and "classes (the distillation loss takes 1 to 8)" in err()
    assert fwd(nb=4) == 1 and "uint8 or int64" in err()
    assert fwd(hw=0) == 1 and "shape" in err()
    assert fwd(b=2, hw=2 ** 36) == 1 and "shape" in err()                                  # the counts are exact up to 2^36 pixels
    for inv in (0.0, -1.0, float("inf"), float("nan")):
        assert fwd(inv=inv) == 1 and "temperature" in err()

    def bwd(s=p, t=p, lb=p, nb=1, b=1, c=2, hw=4, inv=0.5, coef=p, up=p, grad=p):
        return lib.iswm_distill_loss_bwd(s, t, lb, nb, b, c, hw, None, 255, inv, coef, up, grad, None)
    assert bwd(coef=None) == 1 and "null" in err()
    assert bwd(up=None) == 1 and "null" in err()
    assert bwd(grad=None) == 1 and "null" in err()
    assert bwd(t=None) == 1 and "teacher pointer null" in err()
    assert bwd(c=9) == 1 and "classes" in err()
    assert bwd(nb=2) == 1 and "uint8 or int64" in err()
    assert bwd(inv=0.0) == 1 and "temperature" in err()

    def coeffs(sums=p, lce=1.0, lkd=1.0, tau=2.0, out=p, coef=p):
        return lib.iswm_distill_loss_coeffs(sums, lce, lkd, tau, out, coef, None)
    assert coeffs(sums=None) == 1 and "null" in err()
    assert coeffs(out=None) == 1 and coeffs(coef=None) == 1
    for tau in (0.0, -2.0, float("inf"), float("nan")):
        assert coeffs(tau=tau) == 1 and "temperature" in err()
    assert coeffs(lce=-1.0) == 1 and coeffs(lkd=-1.0) == 1 and coeffs(lkd=float("inf")) == 1 and "weights" in err()


def plain_autograd(student, teacher, labels, weight, ignore_index, tau, lce, lkd):
    """the loss written the way a user would with torch ops, float64, differentiated by autograd"""
    z = student.double().requires_grad_(True)
    t = teacher.double()
    c = z.shape[1]
    y = labels.long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    logp, logq = F.log_softmax(z / tau, 1), F.log_softmax(t / tau, 1)
    kl = (logq.exp() * (logq - logp)).sum(1)
    n = int(valid.sum())
    loss = lkd * tau * tau * (kl * valid).sum() / n if n else (z * 0).sum()
    if lce != 0:
        target = torch.where(valid, y, torch.full_like(y, -100))
        loss = loss + lce * F.cross_entropy(z, target, weight=None if weight is None else weight.double(), ignore_index=-100)
    loss.backward()
    return loss.detach(), z.grad


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_restatement_equals_float64_autograd(case):
    shape, kind, scale = case
    student, teacher, labels, weight = R.pair(shape, kind, R.SCALES[scale])
    for temp, combo in itertools.product(R.TEMPS, R.COMBOS):
        wt, lce, lkd = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], temp, combo)
        loss, grad = plain_autograd(student, teacher, labels, wt, R.IGNORE, R.TEMPS[temp], lce, lkd)
        what = "%s %s" % (temp, R.combo_id(combo))
        assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))), what
        assert float((ref["grad"] - grad).abs().max()) <= 1e-12, what
        assert abs(float(ref["ce"] + ref["kd"]) - float(ref["loss"])) == 0.0
        assert int(ref["sums"][3]) == int(R.valid_mask(labels, student.shape[1]).sum()) and 0 <= int(ref["sums"][4]) <= int(ref["sums"][3])


def test_restatement_equals_autograd_on_the_other_inputs():
    """the ignore_index inside the class range, the degenerate label patterns, teacher == student and the data-parallel batch"""
    student, teacher, labels, weight = R.pair(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    assert int((labels == 2).sum()) > 20
    for temp in R.IG2_TEMPS:
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, temp, R.IG2_COMBO, R.IG2_IGNORE)
        loss, grad = plain_autograd(student, teacher, labels, weight, R.IG2_IGNORE, R.TEMPS[temp], 1.0, 2.0)
        assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 and float((ref["grad"] - grad).abs().max()) <= 1e-12
        assert int(ref["sums"][3]) == int(((labels != 2) & (labels < 3)).sum())           # none of the pixels labelled 2 in N
    for pattern in R.DEGENERATE:
        s, t, lb, w = R.degenerate_inputs(pattern)
        for combo in R.degenerate_combos(pattern):
            wt, lce, lkd = R.combo_args(combo, w)
            ref = R.degenerate_reference(pattern, combo)
            loss, grad = plain_autograd(s, t, lb, wt, R.IGNORE, R.TEMPS[R.DEGEN_TEMP], lce, lkd)
            assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 and float((ref["grad"] - grad).abs().max()) <= 1e-12
            if pattern == "all_ignored":
                assert float(ref["loss"]) == 0.0 and not bool(ref["grad"].any()) and not bool(ref["sums"].any())
    for temp in R.SAME_TEMPS:
        ref = R.same_reference(temp)
        assert float(ref["sums"][2]) == 0.0 and float(ref["kd"]) == 0.0 and float(ref["sums"][3]) == float(ref["sums"][4])
    s, t, lb, w = R.ddp_inputs()
    ref = R.ddp_reference()
    loss, grad = plain_autograd(s, t, lb, w, R.IGNORE, R.DDP_TEMP, R.DDP_COMBO[1], R.DDP_COMBO[2])
    assert abs(float(ref["loss"]) - float(loss)) <= 1e-12 and float((ref["grad"] - grad).abs().max()) <= 1e-12


def _errs(student, teacher, labels, wt, ignore_index, tau, lce, lkd, ref):
    low = R.distill_ref(student, teacher, labels, wt, ignore_index, tau, lce, lkd, dtype=torch.float32)
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
        student, teacher, labels, weight = R.pair(shape, kind, R.SCALES[scale])
        for temp, combo in itertools.product(R.TEMPS, R.COMBOS):
            wt, lce, lkd = R.combo_args(combo, weight)
            take(R.group(shape, scale), _errs(student, teacher, labels, wt, R.IGNORE, R.TEMPS[temp], lce, lkd,
                                              R.reference(shape, kind, R.SCALES[scale], temp, combo)))
    for name, shape in R.BIG.items():
        student, teacher, labels, weight = R.pair(shape, "u8", 1.0)
        wt, lce, lkd = R.combo_args(R.BIG_COMBO, weight)
        take(name, _errs(student, teacher, labels, wt, R.IGNORE, R.TEMPS[R.BIG_TEMP], lce, lkd,
                         R.reference(shape, "u8", 1.0, R.BIG_TEMP, R.BIG_COMBO)))
    for pattern in ("no_foreground", "all_foreground"):
        s, t, lb, w = R.degenerate_inputs(pattern)
        for combo in R.degenerate_combos(pattern):
            wt, lce, lkd = R.combo_args(combo, w)
            take("degen", _errs(s, t, lb, wt, R.IGNORE, R.TEMPS[R.DEGEN_TEMP], lce, lkd, R.degenerate_reference(pattern, combo)))
    student, teacher, labels, weight = R.pair(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    for temp in R.IG2_TEMPS:
        take("ig2", _errs(student, teacher, labels, weight, R.IG2_IGNORE, R.TEMPS[temp], 1.0, 2.0,
                          R.reference(R.IG2_SHAPE, "u8", 1.0, temp, R.IG2_COMBO, R.IG2_IGNORE)))
    student, _, labels, weight = R.pair(R.SAME_CASE[0], R.SAME_CASE[1], R.SCALES[R.SAME_CASE[2]])
    for temp in R.SAME_TEMPS:
        take("same", _errs(student, student, labels, weight, R.IGNORE, R.TEMPS[temp], 1.0, 2.0, R.same_reference(temp)))
    s, t, lb, w = R.ddp_inputs()
    take("ddp", _errs(s, t, lb, w, R.IGNORE, R.DDP_TEMP, R.DDP_COMBO[1], R.DDP_COMBO[2], R.ddp_reference()))
    return out


def test_recorded_floors_are_the_measured_ones():
    measured = measure_floors()
    assert set(measured) == set(R.FLOOR), set(measured) ^ set(R.FLOOR)
    for key, m in sorted(measured.items()):
        want = max(m, R.FLOOR_MIN)
        print("%-18s recorded %.2e measured %.2e" % (key, R.FLOOR[key], m))
        assert R.FLOOR[key] >= R.FLOOR_MIN, key
        assert 0.5 * want <= R.FLOOR[key] <= 1.25 * want, (key, R.FLOOR[key], m)


def test_the_single_pixel_runs_at_scale_one_only():
    """p1 runs at logit scale 1 only and has floor groups of its own (tests/distill_ref.py says why)"""
    assert ("p1", "u8", "s1") in R.INPUT_CASES and not [c for c in R.INPUT_CASES if c[0] == "p1" and c[2] != "s1"]
    assert all(R.floor_key(k, R.group("p1", "s1")) in R.FLOOR for k in R.CHECKS)
    assert not [k for k in R.FLOOR if k.endswith(".p1_s30")]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_bounds_see_each_mutant(mutant):
    """a wrong formula misses at least one of the bounds of tests/test_distill_gpu.py by 3 x or more on the ig2 inputs (three
    classes, ignore_index 2, class weights, lce 1, lkd 2) at tau = 2 AND at tau = 3: a float check by 3 x its 4 x FLOOR bound,
    an exact count (N, A) by 3 pixels or more.  At tau = 1 tau_not_squared and grad_tau_squared are the definition itself
    (tau = tau^2 = 1) and teacher_unscaled is too (t / 1 = t): the three are shown to be the same function there, which is why
    the mutants are not judged at that temperature."""
    student, teacher, labels, weight = R.pair(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    for temp in R.IG2_TEMPS:
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, temp, R.IG2_COMBO, R.IG2_IGNORE)
        bad = R.distill_ref(student, teacher, labels, weight, R.IG2_IGNORE, R.TEMPS[temp], 1.0, 2.0, mutant=mutant)
        ratio = {k: e / (4 * R.FLOOR[R.floor_key(k, "ig2")]) for k, e in R.errors(bad["sums"], bad["loss"], bad["grad"], ref).items()}
        counts = {k: abs(int(bad["sums"][i]) - int(ref["sums"][i])) for k, i in (("N", 3), ("A", 4))}
        print(mutant, temp, {k: "%.1e" % v for k, v in ratio.items()}, counts)
        assert max(ratio.values()) >= 3.0 or max(counts.values()) >= 3, (ratio, counts)
    if mutant in ("tau_not_squared", "grad_tau_squared", "teacher_unscaled"):
        ref = R.distill_ref(student, teacher, labels, weight, R.IG2_IGNORE, 1.0, 1.0, 2.0)
        bad = R.distill_ref(student, teacher, labels, weight, R.IG2_IGNORE, 1.0, 1.0, 2.0, mutant=mutant)
        assert torch.equal(bad["sums"], ref["sums"]) and torch.equal(bad["loss"], ref["loss"]) and torch.equal(bad["grad"], ref["grad"])


def test_module_refuses_bad_parameters_and_bad_tensors():
    from iswm_amd.utils.loss import DistillationLoss
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
               dict(ce_weight=-1.0), dict(distill_weight=-0.5), dict(ce_weight=0.0, distill_weight=0.0),
               dict(distill_weight=float("inf"))):
        with pytest.raises(ValueError):
            DistillationLoss(**kw)
    d = DistillationLoss(temperature=2, ce_weight=0, weight=torch.tensor([1.0, 3.0]))
    assert (d.temperature, d.ce_weight, d.distill_weight, d.ignore_index) == (2.0, 0.0, 1.0, 255)
    assert torch.equal(d.weight, torch.tensor([1.0, 3.0])) and d.last_terms is None and d.last_agreement is None
    z, y = torch.zeros(1, 2, 4, 4), torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        DistillationLoss()(z, y, z.clone())
    with pytest.raises(ValueError, match="detached"):
        DistillationLoss()(z, y, z.clone().requires_grad_(True))
    with pytest.raises(ValueError, match=r"\(1, 2, 4, 5\).*\(1, 2, 4, 4\)"):                 # both shapes are named
        DistillationLoss()(z, y, torch.zeros(1, 2, 4, 5))
    with pytest.raises(TypeError):
        DistillationLoss()(z, y)


DISTILL = ["--distill_ckpt", "t.pth", "--distill_model", "deeplabv3plus_resnet101"]


def test_parser_defaults_and_refusals():
    from iswm_amd import train
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    o = parse()
    assert (o.distill_ckpt, o.distill_model, o.distill_output_stride, o.distill_use_ema, o.distill_weight,
            o.distill_temperature) == (None, None, 16, False, 1.0, 1.0)
    o = parse(*DISTILL)
    assert (o.distill_ckpt, o.distill_model, o.distill_output_stride, o.distill_use_ema, o.distill_weight,
            o.distill_temperature) == ("t.pth", "deeplabv3plus_resnet101", 16, False, 1.0, 1.0)
    o = parse(*DISTILL, "--distill_output_stride", "8", "--distill_use_ema", "--distill_weight", "0.5", "--distill_temperature", "3",
              "--ce_weight", "0")
    assert (o.distill_output_stride, o.distill_use_ema, o.distill_weight, o.distill_temperature, o.ce_weight) == (8, True, 0.5, 3.0, 0.0)
    for bad in (["--distill_model", "deeplabv3plus_resnet101"], ["--distill_output_stride", "8"], ["--distill_use_ema"],
                ["--distill_weight", "1"], ["--distill_temperature", "2"],                      # no --distill_ckpt
                ["--distill_ckpt", "t.pth"],                                                    # no --distill_model
                DISTILL[:3] + ["resnet101"], DISTILL + ["--distill_output_stride", "32"],
                DISTILL + ["--overlap_loss", "dice"], DISTILL + ["--lovasz_weight", "1"], DISTILL + ["--ohem_thresh", "0.7"],
                DISTILL + ["--test_only"],
                DISTILL + ["--distill_weight", "0"], DISTILL + ["--distill_weight", "-1"], DISTILL + ["--distill_weight", "inf"],
                DISTILL + ["--distill_weight", "nan"],
                DISTILL + ["--distill_temperature", "0"], DISTILL + ["--distill_temperature", "-2"],
                DISTILL + ["--distill_temperature", "inf"], DISTILL + ["--distill_temperature", "nan"],
                ["--ce_weight", "0"]):                                                          # still no loss term without a teacher
        with pytest.raises(SystemExit):
            parse(*bad)


def test_teacher_checkpoint_is_refused_before_the_data_set_is_touched(tmp_path, monkeypatch):
    from iswm_amd import train

    def no_dataset(opts):
        raise AssertionError("the data set was touched")
    monkeypatch.setattr(train, "get_dataset", no_dataset)
    with pytest.raises(FileNotFoundError, match="distill_ckpt"):
        train.main(["--distill_ckpt", str(tmp_path / "absent.pth"), "--distill_model", "deeplabv3plus_resnet50"])
    int8 = str(tmp_path / "int8.pth")
    from iswm_amd import quant
    torch.save({"format": quant.FORMAT, "arch": {}, "convs": {}, "act": {}, "stem": {}}, int8)
    with pytest.raises(ValueError, match="INT8"):
        train.main(["--distill_ckpt", int8, "--distill_model", "deeplabv3plus_resnet50"])
    ckdir = tmp_path / "ck"
    ckdir.mkdir()
    own = str(ckdir / "best_teacher.pth")
    torch.save({"model_state": {}}, own)
    with pytest.raises(ValueError, match="checkpoints_dir"):            # the run would delete its own teacher
        train.main(["--distill_ckpt", own, "--distill_model", "deeplabv3plus_resnet50", "--checkpoints_dir", str(ckdir)])


def _describe(crit):
    return (type(crit).__name__, getattr(crit, "params", None), getattr(crit, "ignore_index", None),
            None if getattr(crit, "weight", None) is None else crit.weight.tolist(), getattr(crit, "group", None),
            tuple(getattr(crit, n, None) for n in ("thresh", "min_kept", "classes", "ce_weight", "lovasz_weight", "reduction")))


def test_setup_criterion_is_unchanged_with_the_new_options_off():
    """every existing criterion option combination: an options object WITHOUT the distill_* attributes (as older callers build
    it) and the parser's own defaults give the same criterion, of the type and with the parameters it had"""
    import argparse
    from iswm_amd import train
    from iswm_amd.utils.loss import (CrossEntropyLoss, DiceLoss, DistillationLoss, LovaszSoftmaxLoss, OhemCrossEntropyLoss,
                                     TverskyLoss)
    cw = torch.tensor([1.0, 3.0])
    parse = lambda a: train.get_argparser().parse_args(list(a))
    want = {(): CrossEntropyLoss, ("--overlap_loss", "dice"): DiceLoss, ("--overlap_loss", "tversky"): TverskyLoss,
            ("--overlap_loss", "focal_tversky"): TverskyLoss, ("--lovasz_weight", "0.5"): LovaszSoftmaxLoss,
            ("--ohem_thresh", "0.7"): OhemCrossEntropyLoss}
    for (extra, kind), loss_type, ce in itertools.product(want.items(), ("ce_loss", "IWce_loss"), ("1", "0.5")):
        o = parse(extra + ("--loss_type", loss_type, "--ce_weight", ce))
        assert o.distill_ckpt is None
        old = argparse.Namespace(**{k: v for k, v in vars(o).items() if not k.startswith("distill_")})
        a, b = train.setup_criterion(o, cw), train.setup_criterion(old, cw)
        assert type(a) is kind and _describe(a) == _describe(b), extra
        assert (a.weight is None) == (loss_type == "ce_loss")
    d = train.setup_criterion(parse(DISTILL + ["--distill_temperature", "2", "--distill_weight", "0.5", "--ce_weight", "0.25"]), cw)
    assert type(d) is DistillationLoss and (d.temperature, d.ce_weight, d.distill_weight) == (2.0, 0.25, 0.5)
    assert torch.equal(d.weight, cw) and d.group is None
    assert train.setup_criterion(parse(DISTILL + ["--loss_type", "ce_loss"]), cw).weight is None
