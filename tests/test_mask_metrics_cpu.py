"""Sequence-validation metrics, CPU side: hand-worked cases pin the restatement (tests/mask_metrics_ref.py) to cv2's
semantics and the reference's formulas, and the new C-ABI entry points validate their arguments without a GPU."""
import ctypes

import numpy as np
import pytest

from tests import mask_metrics_ref as R


def frame(h, w, *blocks):
    m = np.zeros((h, w), dtype=np.uint8)
    for y0, y1, x0, x1 in blocks:
        m[y0:y1, x0:x1] = 1
    return m


def test_morphology_border_is_neutral():
    full = np.ones((5, 6), dtype=np.uint8)
    assert np.array_equal(R.erode(full), full)                 # outside pixels never erode
    assert np.array_equal(R.open3(full), full) and np.array_equal(R.close3(full), full)
    corner = frame(5, 6, (0, 1, 0, 1))
    assert np.array_equal(R.dilate(corner), frame(5, 6, (0, 2, 0, 2)))     # and never dilate
    assert R.open3(corner).sum() == 0                          # a lone pixel does not survive the opening
    # repair: 3 x dilate then 2 x erode == one 7x7 dilation then one 5x5 erosion
    rng = np.random.default_rng(0)
    m = (rng.random((23, 17)) < 0.05).astype(np.uint8)
    assert np.array_equal(R.repair_small_gaps(m), R.erode(R.dilate(m, 3), 2))
    assert np.array_equal(R.erode(R.erode(m)), R.erode(m, 2))


def test_diagonal_pixels_are_one_component():
    m = np.eye(6, dtype=np.uint8)[:, ::-1].copy()
    lab, n, areas = R.components(m)
    assert n == 1 and areas.tolist() == [6]
    canon, root_area = R.canonical_labels(m)
    assert set(canon[m > 0].tolist()) == {5} and root_area.ravel()[5] == 6     # root = first pixel in raster order
    two = np.zeros((4, 4), dtype=np.uint8)
    two[0, 0] = two[0, 2] = 1
    assert R.components(two)[1] == 2                                   # no 4- or 8-neighbour: two components


def test_area_threshold_is_a_thousandth_of_the_frame():
    # 100 x 100: valid from 10 pixels.  A 3x3 block (9 px) survives the opening but is too small.
    assert R.preprocess_mask(frame(100, 100, (10, 13, 10, 13))).sum() == 0
    p = R.preprocess_mask(frame(100, 100, (10, 13, 10, 14)))
    assert p.dtype == np.uint8 and p.sum() == 12
    # inclusive: a 12 px block is valid in a 12000 px frame (threshold 12.0) and not in a 13000 px one
    assert R.preprocess_mask(frame(120, 100, (0, 3, 0, 4))).sum() == 12
    assert R.preprocess_mask(frame(130, 100, (0, 3, 0, 4))).sum() == 0


def test_multi_region_weight_removes_fronts_and_stability():
    m = frame(100, 100, (10, 20, 10, 20), (50, 60, 50, 58))
    p = R.preprocess_mask(m)
    assert p.dtype == np.float64 and abs(p.max() - 0.8) < 1e-15 and p.sum() == pytest.approx(0.8 * 100)
    assert R.find_front_positions(m) == []                    # values are 0.8, never == 1
    assert R.calculate_stability(m, m) == 0.0 and R.calculate_motion(m, m) == 0.0
    three = frame(100, 100, (0, 10, 0, 10), (30, 40, 30, 40), (60, 70, 60, 70), (85, 95, 85, 95))
    assert abs(R.preprocess_mask(three).max() - 0.4) < 1e-15  # max(0.4, 1 - 0.2 * 3)
    ties = frame(100, 100, (50, 60, 0, 10), (0, 10, 50, 60))
    assert R.preprocess_mask(ties)[0, 50] > 0 and R.preprocess_mask(ties)[55, 5] == 0    # first pixel in raster order


def test_single_region_fronts_and_motion():
    a = frame(40, 50, (5, 15, 20, 30))
    b = frame(40, 50, (5, 15, 22, 32))
    fa = R.find_front_positions(a)
    assert [f[0] for f in fa] == list(range(5, 15)) and all(f[1] == 20 for f in fa)
    # stability: window int(0.1 * 50) = 5, front moved by 2 -> 1 / (1 + 2/5) per row
    assert R.calculate_stability(b, a) == pytest.approx(1.0 / 1.4, abs=1e-15)
    assert R.calculate_motion(b, a) == pytest.approx(1.0 / (1.0 + 2.0 / 4.0), abs=1e-15)


def test_front_error_special_cases():
    f = R.FrontTrackingMetrics()
    f.max_distance_threshold = 5.0
    empty, a = np.zeros((40, 50), np.uint8), frame(40, 50, (5, 15, 20, 30))
    assert f.calculate_error(empty, a) == 10.0                 # missed: 2 tau
    assert f.calculate_error(a, empty) == 7.5                  # false alarm: 1.5 tau
    assert f.calculate_error(empty, empty) == 0.0
    assert f.calculate_error(a, frame(40, 50, (5, 15, 40, 50))) == 10.0    # every point beyond tau: 2 tau
    assert f.calculate_error(a, a) == 0.0
    # one column apart: every min_dist = 1, weights 1/(1+1e-6) -> error 1; full coverage
    assert f.calculate_error(frame(40, 50, (5, 15, 21, 30)), a) == pytest.approx(1.0, abs=1e-12)
    # half the gt rows have no prediction within tau: coverage penalty (1 - 10/20) * tau * 0.5
    gt = frame(40, 50, (5, 25, 20, 30))
    e = f.calculate_error(a, gt)
    assert e > 1.25 - 1e-12
    m = R.FrontTrackingMetrics()
    assert m.get_mean_error() == float("inf")
    m.update(a, empty)
    assert m.max_distance_threshold == 5.0 and m.get_mean_error() == 7.5
    m.reset()
    assert m.max_distance_threshold == 5.0 and m.get_mean_error() == 10.0


def test_fragmentation_and_region_score():
    assert R.fragmentation([]) == 0.0 and R.fragmentation([80]) == 1.0
    assert R.fragmentation([50, 100, 50]) == pytest.approx(0.5 - 0.5 * (0.25 / 3 + 0.25 * 2 / 3), abs=1e-15)
    assert R.fragmentation([60, 60, 60, 60]) == pytest.approx(0.25 - 0.5 * 0.25 * (1 + 2 + 3) / 4, abs=1e-15)
    assert R.region_metrics(np.zeros((30, 30), np.uint8), frame(30, 30, (0, 5, 0, 5))) is None
    assert R.region_metrics(frame(30, 30, (0, 5, 0, 5)), np.zeros((30, 30), np.uint8)) is None
    # a 10x10 block: the repair grows it by 1 on each side that is not the border; one region -> frag 1
    p = frame(40, 40, (10, 20, 10, 20))
    assert R.region_metrics(p, p) == pytest.approx(0.7 + 0.3 * 100 / 144, abs=1e-15)
    # gaps of up to 4 pixels close
    split = frame(40, 40, (10, 20, 10, 15), (10, 20, 19, 24))
    assert R.components(R.repair_small_gaps(split))[1] == 1


def _seq(kinds, h=32, w=40):
    """frames with (k = 1) a wave block or (k = 0) nothing"""
    return np.stack([frame(h, w, (4, 20, 10 + t, 20 + t)) if k else np.zeros((h, w), np.uint8)
                     for t, k in enumerate(kinds)])


def test_temporal_branches():
    L = 4
    t = R.TemporalMetrics(sequence_length=L)
    gt, pred = _seq([0, 0, 0, 0]), _seq([0, 1, 0, 0])
    for i in range(L):
        t.update(pred[:i + 1], gt[:i + 1])
    assert t.temporal_scores == [0.75]                         # no wave: 1 - 1/4 wrong frames
    t = R.TemporalMetrics(sequence_length=L)
    gt = pred = _seq([1, 1, 1, 1])
    for i in range(L):
        t.update(pred[:i + 1], gt[:i + 1])
    s = t.get_detailed_statistics()
    assert s["score_count"] == 1 and s["mean_transition"] == 0.0 and 0.0 < t.temporal_scores[0] < 1.0
    assert s["mean_stability"] == pytest.approx(1.0 / (1.0 + 1.0 / 4.0), abs=1e-15)      # front moves 1 px, ws = 4
    t = R.TemporalMetrics(sequence_length=L)
    gt, pred = _seq([0, 0, 1, 1]), _seq([0, 1, 1, 1])
    for i in range(L):
        t.update(pred[:i + 1], gt[:i + 1])
    s = t.get_detailed_statistics()
    assert s["mean_transition"] == pytest.approx(1.0 / 2.0)    # one transition each, one frame apart
    assert t.temporal_scores[0] == pytest.approx(0.6 * 0.5 + 0.4 * s["mean_wave_segment"])
    assert len(t.transition_scores) == 1 and len(t.stability_scores) == 0


def test_stream_best_score_is_running_max():
    m = R.StreamMetrics(2, sequence_length=3)
    gt, pred = _seq([1, 1, 0, 1, 1]), _seq([1, 0, 0, 1, 1])
    bests = []
    for i in range(3):
        m.update(gt[i:i + 3], pred[i:i + 3])
        bests.append(m.best)
    assert bests == sorted(bests) and m.get_results()["Best Score"] >= bests[-1]
    assert R.is_best_score({"MIoU": 0.5, "Foreground IoU": 0.5, "Foreground F1": 0.5, "Temporal Consistency": 0.5,
                            "Region Continuity": 0.5, "Front Tracking Error": 1.0},
                           {"MIoU": -np.inf, "Foreground IoU": -np.inf, "Foreground F1": -np.inf,
                            "Temporal Consistency": -np.inf, "Region Continuity": -np.inf,
                            "Front Tracking Error": np.inf})


def test_c_abi_argument_checks_of_the_mask_metrics():
    from iswm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.iswm_mask_morph(None, 0, 1, 4, 4, 1, 1, p, None) == 1 and "null" in err()
    assert lib.iswm_mask_morph(p, 0, 1, 0, 4, 1, 1, p, None) == 1 and "size" in err()
    assert lib.iswm_mask_morph(p, 2, 1, 4, 4, 1, 1, p, None) == 1 and "dtype" in err()
    assert lib.iswm_ccl(p, 1, 4, 4, None, p, None) == 1 and "null" in err()
    assert lib.iswm_ccl(p, 1, 4, 4096, p, p, None) == 1 and "size" in err()
    assert lib.iswm_mask_preprocess_workspace(1, 0, 4) == 0 and lib.iswm_mask_preprocess_workspace(2, 9, 7) > 0
    assert lib.iswm_mask_preprocess(p, 0, 1, 4, 4, p, p, p, None, 0, None) == 1 and "null" in err()
    assert lib.iswm_mask_preprocess(p, 5, 1, 4, 4, p, p, p, p, 1 << 20, None) == 1 and "dtype" in err()
    assert lib.iswm_mask_preprocess(p, 0, 1, 4, 4, p, p, p, p, 8, None) == 1 and "workspace" in err()
    assert lib.iswm_mask_fronts(p, None, 0, 4, 4, p, p, None) == 1 and "size" in err()
    assert lib.iswm_mask_fronts(None, None, 1, 4, 4, p, p, None) == 1 and "null" in err()
    assert lib.iswm_front_error(p, p, 1, 4, ctypes.c_double(0.0), p, None) == 1 and "size" in err()
    assert lib.iswm_front_error(p, None, 1, 4, ctypes.c_double(1.0), p, None) == 1 and "null" in err()
    assert lib.iswm_mask_pair_scores(p, p, p, None, p, 1, 4, 4, p, p, None) == 1 and "null" in err()
    assert lib.iswm_mask_pair_scores(p, p, p, p, p, 1, -1, 4, p, p, None) == 1 and "size" in err()
    assert lib.iswm_region_workspace(0, 4, 4) == 0
    assert lib.iswm_region_score(p, 0, p, 3, 1, 4, 4, p, p, p, 1 << 20, None) == 1 and "dtype" in err()
    assert lib.iswm_region_score(p, 0, p, 0, 1, 4, 4, p, None, p, 1 << 20, None) == 1 and "null" in err()
    assert lib.iswm_region_score(p, 0, p, 0, 1, 4, 4, p, p, p, 8, None) == 1 and "workspace" in err()
