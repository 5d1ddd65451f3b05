"""No GPU: the fifth header's binding, the new entry points' host-side refusals, the two restatements of the contour against each
other and against the signed map of tests/boundary_ref.py, the two restatements of the distances, hand-worked planes, the rank
rule, the degenerate values, eight mutants that the integer equalities of tests/test_boundary_metrics_gpu.py must see, the 20-pixel
condition on the shared cases, the parser's refusals, and validate / validate_sequence with the new switch off and on."""
import argparse
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from tests import boundary_metrics_ref as R
from tests import boundary_ref as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BM_NAMES = ("iswm_boundary_metrics_workspace", "iswm_boundary_metrics")
BD_NAMES = ("iswm_signed_edt_workspace", "iswm_signed_edt", "iswm_boundary_loss_partials", "iswm_boundary_loss_fwd",
            "iswm_boundary_loss_coeffs", "iswm_boundary_loss_bwd")
KD_NAMES = ("iswm_distill_loss_partials", "iswm_distill_loss_fwd", "iswm_distill_loss_coeffs", "iswm_distill_loss_bwd")
EXT_NAMES = ("iswm_dwconv3x3_pre_fwd", "iswm_dwconv3x3_pre_bwd_workspace", "iswm_dwconv3x3_pre_bwd")
SMALL = [n for n, cs in R.CASES.items() if cs["shape"][2] * cs["shape"][3] <= E.BRUTE_MAX]


def test_the_fifth_header_binds_into_a_table_of_its_own():
    from iswm_amd import _lib
    assert os.path.samefile(_lib.BM_HEADER, os.path.join(ROOT, "include", "iswm_hip_bm.h"))
    assert _lib.BM_EXPORTS == BM_NAMES and tuple(_lib._BM_SIGS) == BM_NAMES
    assert len(_lib.EXPORTS) == 162 and tuple(_lib._SIGS) == _lib.EXPORTS                 # the other four tables are what they were
    assert _lib.EXT_EXPORTS == EXT_NAMES and tuple(_lib._EXT_SIGS) == EXT_NAMES
    assert _lib.KD_EXPORTS == KD_NAMES and tuple(_lib._KD_SIGS) == KD_NAMES
    assert _lib.BD_EXPORTS == BD_NAMES and tuple(_lib._BD_SIGS) == BD_NAMES
    assert not set(BM_NAMES) & (set(_lib.EXPORTS) | set(_lib.EXT_EXPORTS) | set(_lib.KD_EXPORTS) | set(_lib.BD_EXPORTS))
    with open(_lib.BM_HEADER) as f:
        text = f.read()
    with open(_lib.HEADER) as f:
        base = f.read()
    consts, structs, sigs = _lib.parse_header(text, base=base)
    assert not consts and not structs and tuple(sigs) == BM_NAMES                         # prototypes only
    c = ctypes
    assert sigs["iswm_boundary_metrics_workspace"] == (c.c_int64, [c.c_int] * 5)
    assert sigs["iswm_boundary_metrics"] == (c.c_int, [c.c_void_p, c.c_int, c.c_void_p] + [c.c_int] * 9 + [c.c_void_p] * 3 +
                                             [c.c_int64, c.c_void_p])
    with pytest.raises(ValueError, match="again"):                                        # a name of the main header is refused
        _lib.parse_header(text.replace("iswm_boundary_metrics_workspace(", "iswm_loss_blocks("), base=base)
    with open(os.path.join(ROOT, "iswm_amd", "_lib.py")) as f:                            # ... and one of an earlier extension header
        src = f.read()
    assert "set(_BM_SIGS) & (set(_EXT_SIGS) | set(_KD_SIGS) | set(_BD_SIGS))" in src


def test_every_new_name_is_a_symbol_of_the_built_library_and_refuses_bad_arguments():
    from iswm_amd import _lib
    from iswm_amd.build import build
    build(verbose=False)
    lib = _lib.load()
    for name in BM_NAMES:
        fn = getattr(lib, name)
        assert (fn.restype, list(fn.argtypes)) == (_lib._BM_SIGS[name][0], list(_lib._BM_SIGS[name][1])), name
    ws = lib.iswm_boundary_metrics_workspace
    assert ws(16, 2, 513, 513, 1) == 16 * 513 * 513 * 4 and ws(2, 3, 5, 7, 0) == 2 * 3 * 5 * 7 * 4
    assert ws(1, 2, 4096, 4096, 1) == 4 * 4096 ** 2 and ws(1, 2, 1, 1, 1) == 4           # at most 16 B per pixel and class plane
    for b, c, h, w, first in ((16, 2, 513, 513, 1), (2, 3, 5, 7, 0), (1, 2, 1, 1, 1), (3, 9, 1, 4096, 0)):
        assert 0 < ws(b, c, h, w, first) <= 16 * b * (c - first) * h * w
    assert ws(1, 2, 4097, 4, 1) == -1 and ws(1, 2, 4, 4097, 1) == -1 and ws(1, 1, 4, 4, 1) == -1 and ws(0, 2, 4, 4, 1) == -1
    assert ws(1, 2, 0, 4, 1) == -1 and ws(1, 2, 4, 0, 1) == -1 and ws(1, 2, 4, 4, 2) == -1
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)

    def bm(pr=p, pb=1, lb=p, nb=1, b=1, c=2, h=2, w=2, first=1, tol=2, pc=95, stats=p, dsum=p, work=p, nbytes=16):
        return lib.iswm_boundary_metrics(pr, pb, lb, nb, b, c, h, w, first, 255, tol, pc, stats, dsum, work, nbytes, None)
    for kw in (dict(pr=None), dict(lb=None), dict(stats=None), dict(dsum=None), dict(work=None)):
        assert bm(**kw) == 1 and "null" in err(), kw
    assert bm(w=4097) == 1 and "sides up to 4096" in err()                                # refused on the host: nothing is launched
    assert bm(h=4097) == 1 and "sides up to 4096" in err()
    assert bm(c=1) == 1 and "no class plane" in err()
    assert bm(first=2) == 1 and "first_class" in err()
    for kw in (dict(b=0), dict(h=0), dict(w=0), dict(b=-1), dict(h=-3), dict(w=-1)):
        assert bm(**kw) == 1 and "shape" in err(), kw
    assert bm(pb=4) == 1 and "predictions must be uint8 or int64" in err()
    assert bm(nb=2) == 1 and "labels must be uint8 or int64" in err()
    for pc in (0, 101, -5):
        assert bm(pc=pc) == 1 and "percent" in err()
    for tol in (-1, 4097):
        assert bm(tol=tol) == 1 and "tolerance" in err()
    assert bm(nbytes=15) == 1 and "workspace" in err()


def test_the_op_and_the_metrics_object_refuse_bad_tensors():
    from iswm_amd import ops
    from iswm_amd.metrics import BoundaryMetrics
    y = torch.zeros(1, 4, 4, dtype=torch.int64)
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.boundary_metrics(y, y, 2)
    with pytest.raises(ValueError, match="foreground"):
        ops.boundary_metrics(y, y, 2, classes="some")
    m = BoundaryMetrics(2, device="cpu")
    assert (m.n_classes, m.classes, m.ignore_index, m.tolerance, m.percent) == (2, "foreground", 255, 2, 95)
    with pytest.raises(ValueError, match="no CPU fallback"):
        m.update(y, y)
    empty = m.get_results()                                                               # nothing seen: M = 0
    assert set(empty) == set(R.KEYS) and empty["Boundary F1"] == 0.0 and math.isnan(empty["ASSD"]) and math.isnan(empty["HD95"])
    assert all(type(v) is float for v in empty.values())


def _sd2_minus_one(mask, valid):
    """{sd2 == -1} of tests/boundary_ref.py's brute-force signed map of the mask: a two-class label image whose class 1 is the mask"""
    lab = np.where(valid, np.where(mask, 1, 0), E.IGNORE).astype(np.int64)
    return (E.signed_edt_ref(torch.from_numpy(lab)[None], 2, "foreground", E.IGNORE, how="brute")[0, 0] == -1).numpy()


@pytest.mark.parametrize("name", SMALL)
def test_contour_restatements_agree_and_equal_the_signed_map(name):
    """S(A) by the written-out rule == by erosion == {sd2 == -1} of boundary_ref's brute-force map, for both masks of every plane"""
    cs = R.CASES[name]
    pred, lab = R.build(name)
    c, seen = cs["shape"][1], 0
    for n in range(lab.shape[0]):
        for cls in R.selected(c, cs["classes"]):
            g, p, valid = R.masks(lab[n].astype(np.int64), pred[n].astype(np.int64), c, cls, cs["ignore_index"])
            for a in (g, p):
                rule = R.contour_rule(a, valid)
                assert np.array_equal(rule, R.contour_erosion(a, valid)), (name, n, cls)
                assert np.array_equal(rule, _sd2_minus_one(a, valid)), (name, n, cls)
                assert not (rule & ~a).any() and not (rule & ~valid).any()
                seen += int(rule.sum())
    assert seen > 0 or cs["degenerate"]


@pytest.mark.parametrize("name", SMALL)
def test_distance_restatements_agree(name):
    cs = R.CASES[name]
    pred, lab = R.build(name)
    for tol, pc in ((2, 95), (0, 50)):
        a = R.reference(pred, lab, cs["shape"][1], cs["classes"], cs["ignore_index"], tol, pc, how="brute", contour="rule")
        b = R.reference(pred, lab, cs["shape"][1], cs["classes"], cs["ignore_index"], tol, pc, how="scipy", contour="erosion")
        assert np.array_equal(a[0], b[0]), name
        assert np.array_equal(a[1], b[1]), name                                           # the same integers under fsum: the same bits


def test_every_case_meets_the_condition_on_its_inputs():
    """nP >= 20 and nG >= 20 on every plane of every case that is not labelled degenerate, by the restatement alone (build()
    asserts it; here it is counted again, and the labelled cases are shown to need the label)"""
    for name, cs in R.CASES.items():
        pred, lab = R.build(name)
        counts = R.contour_counts(pred, lab, cs["shape"][1], cs["classes"], cs["ignore_index"])
        first = R.selected(cs["shape"][1], cs["classes"])[0]
        low = [(n, cls) for n, cls, a, b in counts if min(a, b) < R.MIN_CONTOUR]
        if cs["degenerate"]:
            assert low, name
        else:
            assert all(cls - first in cs["degenerate_planes"] for _, cls in low), (name, low)
    far = R.expected("4096x4096")[0]
    assert int(far[0, 0, 0, 2]) > 1 << 24 and int(far[0, 0, 1, 3]) > 1 << 24             # the select's top bit
    assert int(R.expected("2x4096")[0][0, 0, 0, 2]) > 4000 ** 2
    assert len(set(R.d2_brute(*_contours("all_equal")).tolist())) == 1                    # a segment whose d2 are all equal
    spread = R.expected("33x300")[0]
    assert int(spread[..., 2].max()) > 20 ** 2 and int(spread[..., 3].min()) >= 0         # distances from 0 to tens of pixels


def _contours(name, n=0, cls=1):
    cs = R.CASES[name]
    pred, lab = R.build(name)
    g, p, valid = R.masks(lab[n].astype(np.int64), pred[n].astype(np.int64), cs["shape"][1], cls, cs["ignore_index"])
    return R.contour_rule(p, valid), R.contour_rule(g, valid)


def _one(pred, lab, c=2, **kw):
    stats, dsum = R.reference(np.asarray(pred)[None], np.asarray(lab)[None], c, **kw)
    return stats[0, 0].tolist(), dsum[0, 0].tolist()


def test_planes_worked_out_by_hand():
    z = np.zeros((5, 9), np.int64)
    lab, pred = z.copy(), z.copy()
    lab[1, 1], pred[4, 5] = 1, 1                                                          # two single pixels: 3 down, 4 across
    stats, dsum = _one(pred, lab, tolerance=5)
    assert stats == [[1, 1, 25, 25], [1, 1, 25, 25]] and dsum == [5.0, 5.0]
    assert _one(pred, lab, tolerance=4)[0] == [[1, 0, 25, 25], [1, 0, 25, 25]]
    for k in (1, 2, 6):                                                                   # two parallel lines k apart
        lab, pred = np.zeros((12, 30), np.int64), np.zeros((12, 30), np.int64)
        lab[2, :], pred[2 + k, :] = 1, 1
        stats, dsum = _one(pred, lab, tolerance=2)
        assert stats == [[30, 30 if k <= 2 else 0, k * k, k * k]] * 2 and dsum == [30.0 * k, 30.0 * k]
    lab = R.rect_labels(13, 31)                                                           # a mask against itself
    stats, dsum = _one(lab, lab)
    n = stats[0][0]
    assert n == 2 * 27 + 2 * 10 - 4 and stats == [[n, n, 0, 0]] * 2 and dsum == [0.0, 0.0]
    res = R.aggregate([R.reference(lab[None], lab[None], 2)])
    assert (res["Boundary F1"], res["Boundary Precision"], res["Boundary Recall"]) == (1.0, 1.0, 1.0)
    assert (res["ASSD"], res["HD"], res["HD95"], res["Boundary Pairs"]) == (0.0, 0.0, 0.0, 1.0)
    lab, pred = z.copy(), z.copy()                                                        # a pixel on both contours:
    lab[2, 2:5], pred[2, 4:7] = 1, 1                                                      # G = x 2..4, P = x 4..6 of row 2
    stats, dsum = _one(pred, lab, tolerance=1)
    assert stats == [[3, 2, 4, 4], [3, 2, 4, 4]] and dsum == [3.0, 3.0]                   # distances 0, 1, 2 each way
    lab[0, 0] = 255                                                                       # validity is the label's alone:
    pred[0, 0] = 1                                                                        # a prediction on an ignored pixel is no P
    assert _one(pred, lab, tolerance=1)[0] == stats
    pred[4, 8] = 7                                                                        # a predicted value outside [0, C): in no mask,
    assert _one(pred, lab, tolerance=1)[0] == stats                                       # and far from every contour
    lab2 = np.ones((4, 6), np.int64)                                                      # a mask over every valid pixel has no contour,
    lab2[0, :] = 255                                                                      # the ignored row and the image edge make none
    assert _one(lab2, lab2)[0] == [[0, 0, -1, -1]] * 2


def test_the_rank_rule():
    want = {1: 1, 19: 19, 20: 19, 21: 20, 100: 95, 101: 96}
    for n, r in want.items():
        assert R.rank_of(n, 95) == r == math.ceil(95 * n / 100), n
        d2 = np.arange(n, 0, -1, dtype=np.int64) ** 2                                     # distinct, not sorted
        stats, _ = R.direction_stats(d2, n, 2, 95)
        assert stats == [n, min(n, 2), n * n, r * r]
        assert R.direction_stats(d2, n, 2, 100)[0][3] == n * n == stats[2]                # percent 100 is the maximum
        assert R.direction_stats(d2, n, 2, 1)[0][3] == (1 if n <= 100 else 4)             # percent 1: rank 1 up to n = 100, then 2
    ties = np.array([0] * 10 + [4] * 9 + [9], np.int64)                                   # rank 19 of 20 falls on the last 4
    assert R.direction_stats(ties, 20, 2, 95)[0] == [20, 19, 9, 4]
    assert R.direction_stats(ties, 20, 2, 50)[0][3] == 0 and R.direction_stats(ties, 20, 2, 51)[0][3] == 4
    assert R.direction_stats(np.full(7, 25, np.int64), 7, 2, 95) == ([7, 0, 25, 25], 35.0)


@pytest.mark.parametrize("name", ["no_pred", "no_label", "neither", "all_ignored", "all_foreground"])
def test_degenerate_values(name):
    stats, dsum = R.expected(name)
    (sp, sg), (dp, dg) = stats[0, 0].tolist(), dsum[0, 0].tolist()
    n_p, n_g = {"no_pred": (0, 70), "no_label": (70, 0)}.get(name, (0, 0))
    assert sp == [n_p, 0, -1, -1] and sg == [n_g, 0, -1, -1] and dp == 0.0 and dg == 0.0
    res = R.aggregate([(stats, dsum)])
    assert res["Boundary Pairs"] == 0.0 and all(math.isnan(res[k]) for k in ("ASSD", "HD", "HD95"))    # M = 0 -> nan
    assert (res["Boundary Precision"], res["Boundary Recall"], res["Boundary F1"]) == (0.0, 0.0, 0.0)
    assert (res["Boundary Missed"], res["Boundary Spurious"]) == (float(name == "no_pred"), float(name == "no_label"))
    assert set(res) == set(R.KEYS)


def test_aggregation_follows_the_definition():
    """two matched pairs, one missed and one spurious, with numbers small enough to check by hand"""
    stats = np.array([[[[4, 2, 9, 9], [2, 1, 16, 4]]], [[[10, 10, 1, 1], [10, 5, 4, 4]]],
                      [[[0, 0, -1, -1], [5, 0, -1, -1]]], [[[3, 0, -1, -1], [0, 0, -1, -1]]]], np.int64)
    dsum = np.array([[[6.0, 3.0]], [[5.0, 15.0]], [[0.0, 0.0]], [[0.0, 0.0]]])
    res = R.aggregate([(stats[:2], dsum[:2]), (stats[2:], dsum[2:])])
    p, r = 12 / 17, 6 / 17
    assert res["Boundary Precision"] == p and res["Boundary Recall"] == r and res["Boundary F1"] == 2 * p * r / (p + r)
    assert res["ASSD"] == (9.0 / 6 + 20.0 / 20) / 2 and res["HD"] == (4.0 + 2.0) / 2 and res["HD95"] == (3.0 + 2.0) / 2
    assert (res["Boundary Pairs"], res["Boundary Missed"], res["Boundary Spurious"]) == (2.0, 1.0, 1.0)


# each mutant, the case it is judged on, and the class selection's first plane
MUTANT_CASE = {"eight_neighbours": "b3c3_fg", "edge_is_contour": "7x40", "invalid_is_outside": "ig_inside", "cityblock": "33x300",
               "column_only": "33x300", "directions_swapped": "33x300", "rank_floor": "all_ranks", "strict_tolerance": "all_equal"}


@pytest.mark.parametrize("mutant", R.CONTOUR_MUTANTS + R.DISTANCE_MUTANTS + R.STAT_MUTANTS)
def test_integer_equality_sees_each_mutant(mutant):
    """a wrong contour, distance or statistic changes at least one INTEGER statistic of the stated case"""
    name = MUTANT_CASE[mutant]
    if name == "all_ranks":                                     # floor(percent n / 100) is the rule's rank only where 100 divides it
        d2 = np.arange(1, 22, dtype=np.int64)
        assert R.direction_stats(d2, 21, 2, 95)[0][3] == 20 and R.direction_stats(d2, 21, 2, 95, mutant)[0][3] == 19
        stats = R.reference(*R.build("33x300"), 2, "foreground", R.IGNORE, 2, 95, how="brute", mutant=mutant)[0]
        differ = int((stats != R.expected("33x300")[0]).sum())
    else:
        cs = R.CASES[name]
        tol = 5 if name == "all_equal" else 2                   # the lines are 5 apart: d2 == tolerance^2 exactly
        pred, lab = R.build(name)
        stats = R.reference(pred, lab, cs["shape"][1], cs["classes"], cs["ignore_index"], tol, 95, how="brute", mutant=mutant)[0]
        differ = int((stats != R.expected(name, tol, 95)[0]).sum())
    print(mutant, "changes", differ, "integer statistics of", name)
    assert differ >= 1


def test_parser_defaults_and_refusals():
    from iswm_amd import train
    parse = lambda *a: train.get_argparser().parse_args(list(a))
    o = parse()
    assert (o.val_boundary_metrics, o.boundary_tolerance, o.boundary_percentile) == (False, None, None)
    o = parse("--val_boundary_metrics")
    assert (o.val_boundary_metrics, o.boundary_tolerance, o.boundary_percentile) == (True, 2, 95)
    o = parse("--val_boundary_metrics", "--boundary_tolerance", "0", "--boundary_percentile", "100", "--test_only")
    assert (o.boundary_tolerance, o.boundary_percentile, o.test_only) == (0, 100, True)
    o = parse("--val_boundary_metrics", "--boundary_weight", "0.5", "--val_metrics", "sequence")        # goes with any criterion
    assert o.val_boundary_metrics and o.boundary_weight == 0.5
    vb = ["--val_boundary_metrics"]
    for bad in (["--boundary_tolerance", "2"], ["--boundary_percentile", "95"], ["--boundary_tolerance", "0"],    # without the flag
                vb + ["--boundary_tolerance", "-1"], vb + ["--boundary_tolerance", "4097"], vb + ["--boundary_tolerance", "1.5"],
                vb + ["--boundary_percentile", "0"], vb + ["--boundary_percentile", "101"], vb + ["--boundary_percentile", "-5"],
                vb + ["--boundary_percentile", "95.5"]):
        with pytest.raises(SystemExit):
            parse(*bad)


class _Model(torch.nn.Module):
    def forward(self, x):
        return torch.stack([-x[:, 0], x[:, 0]], 1)


class _Stream(object):
    """stands in for StreamMetrics where there is no GPU: counts its calls, returns fixed scores"""
    calls = []

    def __init__(self, n_classes, **kw):
        self.kw = kw

    def update_logits(self, labels, logits):
        _Stream.calls.append(("logits", tuple(labels.shape)))

    def update(self, labels, preds, sequence_data=True):
        _Stream.calls.append(("window", tuple(labels.shape)))

    def get_results(self):
        return {"MIoU": 0.5, "Foreground IoU": 0.25, "Foreground F1": 0.4}


class _Boundary(object):
    made, frames = [], []

    def __init__(self, n_classes, **kw):
        _Boundary.made.append((n_classes, kw))

    def update_logits(self, labels, logits):
        _Boundary.frames.append(("logits", labels.shape[0]))

    def update(self, labels, preds):
        _Boundary.frames.append(("masks", labels.shape[0]))

    def get_results(self):
        return {k: 1.0 for k in R.KEYS}


class _Loader(list):
    pass


def test_validation_is_unchanged_with_the_switch_off_and_merges_the_keys_with_it_on(monkeypatch):
    from iswm_amd import metrics, ops, train
    monkeypatch.setattr(metrics, "StreamMetrics", _Stream)
    monkeypatch.setattr(metrics, "BoundaryMetrics", _Boundary)
    monkeypatch.setattr(ops, "argmax_nchw", lambda z: z.max(1)[1])
    loader = _Loader([(torch.randn(2, 3, 8, 8), torch.zeros(2, 8, 8, dtype=torch.uint8)) for _ in range(3)])
    loader.dataset = argparse.Namespace(images=["f%d" % i for i in range(6)])
    old = argparse.Namespace(num_classes=2, sequence_length=3)                              # built before the switch existed
    off = argparse.Namespace(num_classes=2, sequence_length=3, val_boundary_metrics=False, boundary_tolerance=None,
                             boundary_percentile=None)
    today = {"MIoU": 0.5, "Foreground IoU": 0.25, "Foreground F1": 0.4}
    for opts in (old, off):
        for fn in (train.validate, train.validate_sequence):
            _Boundary.made.clear(), _Boundary.frames.clear()
            assert fn(_Model(), loader, "cpu", opts) == today                               # exactly today's keys
            assert not _Boundary.made and not _Boundary.frames
    on = argparse.Namespace(num_classes=2, sequence_length=3, val_boundary_metrics=True, boundary_tolerance=3, boundary_percentile=90)
    bare = argparse.Namespace(num_classes=2, sequence_length=3, val_boundary_metrics=True)  # the two values left out: 2 and 95
    for opts, (tol, pc) in ((on, (3, 90)), (bare, (2, 95))):
        for fn, kind in ((train.validate, "logits"), (train.validate_sequence, "masks")):
            _Boundary.made.clear(), _Boundary.frames.clear(), _Stream.calls.clear()
            score = fn(_Model(), loader, "cpu", opts)
            assert set(score) == set(today) | set(R.KEYS) and all(score[k] == v for k, v in today.items())
            assert _Boundary.made == [(2, dict(classes="foreground", ignore_index=255, tolerance=tol, percent=pc, device="cpu"))]
            assert _Boundary.frames == [(kind, 2)] * 3                                      # every frame once, not once per window
            if kind == "masks":
                assert _Stream.calls == [("window", (3, 8, 8))] * 4
    for key in R.KEYS:                                                                      # model selection never looks at them
        assert key not in train.METRIC_WEIGHTS and key not in train.initialize_best_score()
    full = dict(today, **{"Temporal Consistency": 0.5, "Region Continuity": 0.5, "Front Tracking Error": 2.0})
    better = dict(full, **{k: 1.0 for k in R.KEYS})
    assert train.is_best_score(better, dict(full)) is False and train.update_best_score(better) == train.update_best_score(full)
    assert train.logged_weighted_score(better) == train.logged_weighted_score(full)
