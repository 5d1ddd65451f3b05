"""The contour-distance kernels of csrc/boundary_metrics.hip, the metrics object and the trainer switch against
tests/boundary_metrics_ref.py.

The four integer statistics (n, within, max2, q2) are compared by equality, no tolerance: the trivial planes, widths around the row
block's 256 threads, heights around the column batch of 8, three images and three classes with both class selections, rows and
columns longer than any chunk, the two contours at opposite ends of a 4096-long plane and at opposite corners of a 4096 x 4096
plane (d2 > 2^24: the top bit of the select), every label pattern, the four label / prediction width pairs, ignore_index inside
the class range, a predicted value outside it, three tolerances and four percentiles, a segment of equal distances and the
degenerate planes; 4097 wide is refused without a launch.

dsum: within 1e-12 relative of math.fsum over the same integers on the cases with n <= 4096 per segment (n 2^-53 < 5e-13 keeps the
reference's own reordering inside the bound), and within (n + 1) 2^-52 relative on 16 x 513 x 513 band labels: the kernel adds n
correctly-rounded roots with fewer than n roundings of at most 2^-53 of the running sum each, and the fsum reference adds one.

With ISWM_TEST_REPORT=<file> every dsum check appends its bound and measured error to that file."""
import math
import os

import numpy as np
import pytest
import torch

from tests import boundary_metrics_ref as R

pytestmark = pytest.mark.gpu
TIGHT = 1e-12


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def emit(line):
    print(line)
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write(line + "\n")


def run(name, tolerance=2, percent=95):
    from iswm_amd import ops
    cs = R.CASES[name]
    pred, lab = R.build(name)
    return ops.boundary_metrics(torch.from_numpy(pred).to(dev()), torch.from_numpy(lab).to(dev()), cs["shape"][1], cs["classes"],
                                cs["ignore_index"], tolerance, percent)


def dsum_error(got, want):
    """the largest relative error over the segments (absolute where the reference is 0: the kernel must give 0 there)"""
    got, want = got.cpu().numpy().reshape(-1), np.asarray(want).reshape(-1)
    return max((abs(g - w) / w if w > 0 else abs(g)) for g, w in zip(got.tolist(), want.tolist()))


@pytest.mark.parametrize("name", list(R.CASES))
def test_statistics_equal_the_definition(name):
    cs = R.CASES[name]
    b, c, h, w = cs["shape"]
    stats, dsum = run(name)
    want_stats, want_dsum = R.expected(name)
    assert stats.dtype == torch.int64 and tuple(stats.shape) == want_stats.shape and stats.is_cuda
    assert dsum.dtype == torch.float64 and tuple(dsum.shape) == want_dsum.shape and dsum.is_cuda
    got = stats.cpu().numpy()
    print(name, "n", want_stats[..., 0].reshape(-1).tolist(), "max2", want_stats[..., 2].reshape(-1).tolist())
    assert np.array_equal(got, want_stats), "%s: got %s want %s" % (name, got.tolist(), want_stats.tolist())
    assert int(want_stats[..., 0].max()) <= 4096
    err = dsum_error(dsum, want_dsum)
    emit("dsum %-16s %d x %d x %d x %d  n <= %4d  bound %.1e  measured %.2e" % (name, b, c, h, w, int(want_stats[..., 0].max()), TIGHT, err))
    assert err <= TIGHT
    if cs["degenerate"] and name in ("no_pred", "no_label", "neither", "all_ignored", "all_foreground"):
        assert not bool(dsum.any()) and got[..., 1:].reshape(-1, 3).tolist() == [[0, -1, -1]] * (2 * b * (c - 1))


@pytest.mark.parametrize("name", ["33x300", "b3c3_all", "all_equal", "2x4096", "pat_blobs", "ig_inside"])
def test_tolerances_and_percentiles(name):
    for tol in R.TOLERANCES:
        for pc in R.PERCENTS:
            stats, dsum = run(name, tol, pc)
            want_stats, want_dsum = R.expected(name, tol, pc)
            got = stats.cpu().numpy()
            assert np.array_equal(got, want_stats), "%s tolerance %d percent %d: got %s want %s" % (name, tol, pc, got.tolist(),
                                                                                                   want_stats.tolist())
            assert dsum_error(dsum, want_dsum) <= TIGHT
            if pc == 100:
                assert np.array_equal(got[..., 3], got[..., 2])                            # percent 100 is the maximum


def test_the_sum_of_distances_at_the_training_shape():
    """16 x 513 x 513, band labels, the prediction shifted by 3 pixels: integers by equality, dsum within (n + 1) 2^-52"""
    from iswm_amd import ops
    pred, lab, want_stats, want_dsum = R.big_case()
    stats, dsum = ops.boundary_metrics(torch.from_numpy(pred).to(dev()), torch.from_numpy(lab).to(dev()), 2, "foreground", R.IGNORE,
                                       R.BIG["tolerance"], R.BIG["percent"])
    assert np.array_equal(stats.cpu().numpy(), want_stats)
    got = dsum.cpu().numpy()
    worst = 0.0
    for i in np.ndindex(want_dsum.shape):
        n, w = int(want_stats[i][0]), float(want_dsum[i])
        assert n >= R.MIN_CONTOUR and w > 0
        bound, err = (n + 1) * 2.0 ** -52, abs(float(got[i]) - w) / w
        worst = max(worst, err)
        assert err <= bound, (i, n, err, bound)
    emit("dsum big              16 x 2 x 513 x 513  n = %d .. %d  bound (n + 1) 2^-52 >= %.1e  measured %.2e" %
         (int(want_stats[..., 0].min()), int(want_stats[..., 0].max()), (int(want_stats[..., 0].min()) + 1) * 2.0 ** -52, worst))


def test_two_calls_give_identical_bits():
    for name in ("33x300", "b3c3_all", "pat_checker"):
        a, b = run(name), run(name)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64)), name
    from iswm_amd import ops
    pred, lab, _, _ = R.big_case()
    p, y = torch.from_numpy(pred).to(dev()), torch.from_numpy(lab).to(dev())
    a, b = ops.boundary_metrics(p, y, 2), ops.boundary_metrics(p, y, 2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int64), b[1].view(torch.int64))


def test_refusals():
    from iswm_amd import ops
    d = dev()
    for shape in ((1, 1, 4097), (1, 4097, 1)):
        y = torch.zeros(shape, dtype=torch.uint8, device=d)
        with pytest.raises(ValueError, match="sides up to 4096"):
            ops.boundary_metrics(y, y, 2)
    y = torch.zeros((1, 4, 4), dtype=torch.uint8, device=d)
    for bad in (dict(pred=y.float()), dict(pred=y[:, :2]), dict(pred=y.cpu()), dict(num_classes=1), dict(tolerance=-1),
                dict(tolerance=1.5), dict(percent=0), dict(percent=101), dict(classes="background")):
        kw = dict(dict(pred=y, labels=y, num_classes=2), **bad)
        with pytest.raises(ValueError):
            ops.boundary_metrics(**kw)
    with pytest.raises(ValueError, match="empty"):
        ops.boundary_metrics(y[:0], y[:0], 2)


MIXED = ("33x300", "b3c3_fg", "same", "no_pred", "no_label", "u8_i64", "all_equal", "7x40")


def test_metrics_object_over_a_run_of_mixed_sizes():
    """every key equals the restatement's aggregation over batches of different H x W and different label widths; update()
    issues no synchronisation; reset() empties the log"""
    from iswm_amd.metrics import BoundaryMetrics
    d = dev()
    fed = [tuple(torch.from_numpy(a).to(d) for a in R.build(name)) for name in MIXED]
    m = BoundaryMetrics(3, classes="foreground", tolerance=2, percent=95, device=d)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for pred, lab in fed:
            m.update(lab, pred)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = m.get_results()
    want = R.aggregate([R.reference(*R.build(name), 3, "foreground", R.IGNORE, 2, 95) for name in MIXED])
    assert set(got) == set(want) == set(R.KEYS) and all(type(v) is float for v in got.values())
    assert want["Boundary Pairs"] >= 8 and want["Boundary Missed"] >= 1 and want["Boundary Spurious"] >= 1
    for k in ("Boundary Pairs", "Boundary Missed", "Boundary Spurious"):
        assert got[k] == want[k], (k, got[k], want[k])
    for k in ("Boundary Precision", "Boundary Recall", "Boundary F1", "ASSD", "HD", "HD95"):
        assert abs(got[k] - want[k]) <= 1e-12 * abs(want[k]), (k, got[k], want[k])
    assert 0 < got["Boundary F1"] < 1 and got["HD"] >= got["HD95"] > 0 and got["ASSD"] > 0
    m.reset()
    empty = m.get_results()
    assert empty["Boundary Pairs"] == 0.0 and math.isnan(empty["ASSD"]) and empty["Boundary F1"] == 0.0
    # update_logits is the argmax, then update
    pred, lab = fed[0]
    logits = torch.stack([(pred != 1).float(), (pred == 1).float() * 2], 1)
    a, b = BoundaryMetrics(2, device=d), BoundaryMetrics(2, device=d)
    a.update_logits(lab, logits)
    b.update(lab, (pred == 1).to(torch.int64))
    assert a.get_results() == b.get_results() and a.get_results()["Boundary Pairs"] == 2.0


@pytest.mark.parametrize("mode", ["confusion", "sequence"])
def test_trainer_reports_the_metrics_of_the_masks_it_saw(mode, tmp_path, capsys, monkeypatch):
    """--test_only --val_boundary_metrics on the synthetic data set: the printed score has today's keys and the new ones, and the
    new ones equal a BoundaryMetrics fed the same masks one image at a time; sequence mode feeds each frame once"""
    from iswm_amd import metrics, train
    seen, plain = [], metrics.BoundaryMetrics

    class Recording(plain):
        """records what the trainer feeds.  An untrained model predicts one class everywhere, which has no contour, so the
        recorded prediction is the model's own argmax with the labels' foreground, moved by (2, 3), laid over it"""

        def update(self, label_trues, label_preds):
            moved = torch.roll(label_trues.to(torch.int64), (2, 3), (-2, -1)).clamp(max=1)
            label_preds = torch.maximum(label_preds.to(torch.int64), moved)
            seen.append((label_trues.clone(), label_preds.clone()))
            return super().update(label_trues, label_preds)
    monkeypatch.setattr(metrics, "BoundaryMetrics", Recording)
    base = ["--model", "deeplabv3plus_mobilenet", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
            "--val_batch_size", "4", "--checkpoints_dir", str(tmp_path / "ck"), "--num_workers", "0", "--test_only",
            "--val_metrics", mode, "--sequence_length", "3"]

    def scored(*flags):
        train.main(base + list(flags))
        lines = [l for l in capsys.readouterr().out.splitlines() if l.startswith("{")]
        assert len(lines) == 1, lines
        return eval(lines[0], {"nan": float("nan"), "inf": float("inf")})
    off = scored()
    assert not seen and not set(off) & set(R.KEYS)
    on = scored("--val_boundary_metrics", "--boundary_tolerance", "3", "--boundary_percentile", "90")
    assert set(on) == set(off) | set(R.KEYS) and on["Boundary Pairs"] >= 1 and 0 < on["HD95"] <= on["HD"]
    same = lambda a, b: a == b or (a != a and b != b)
    assert all(same(on[k], off[k]) for k in off)                                          # the keys of today: the same values
    frames = sum(g.shape[0] for g, _ in seen)
    assert seen and frames == sum(p.shape[0] for _, p in seen)
    again = plain(2, tolerance=3, percent=90, device=dev())
    for g, p in seen:
        for i in range(g.shape[0]):
            again.update(g[i:i + 1], p[i:i + 1])
    want = again.get_results()
    assert all(same(on[k], want[k]) for k in R.KEYS), (on, want)
    ref = R.aggregate([R.reference(p.cpu().numpy(), g.cpu().numpy(), 2, "foreground", 255, 3, 90) for g, p in seen])
    for k in R.KEYS:
        assert same(on[k], ref[k]) or abs(on[k] - ref[k]) <= 1e-12 * abs(ref[k]), (k, on[k], ref[k])
    if mode == "sequence":                                                                # each frame once, not once per window
        off_frames = frames
        seen.clear()
        scored("--val_boundary_metrics", "--sequence_length", "2")
        assert sum(g.shape[0] for g, _ in seen) == off_frames
