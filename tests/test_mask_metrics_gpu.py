"""Sequence-validation metrics on the GPU (iswm_amd/csrc/mask_metrics.hip, iswm_amd/metrics) against the CPU
restatement tests/mask_metrics_ref.py: integer stages bit-exact, fp64 scores within 1e-12 relative, StreamMetrics
end to end, and the --val_metrics sequence training loop."""
import glob
import os

import numpy as np
import pytest
import torch

from tests import mask_metrics_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (7, 5), (65, 65), (129, 97), (513, 513)]
DENSITIES = [0.0, 0.02, 0.15, 0.5, 0.9, 1.0]


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def blobs(h, w, density, seed, cell=None):
    """blob masks: a coarse random field, nearest-upsampled, thresholded at `density`, plus pixel noise"""
    rng = np.random.default_rng(seed)
    cell = cell or max(1, min(h, w) // 8)
    coarse = rng.random(((h + cell - 1) // cell, (w + cell - 1) // cell))
    m = np.kron(coarse, np.ones((cell, cell)))[:h, :w] < density
    flip = rng.random((h, w)) < 0.02 * density * (1 - density)
    return (m ^ flip).astype(np.uint8)


def rel_close(a, b, tol=1e-12):
    return abs(float(a) - float(b)) <= tol * max(1.0, abs(float(b)))


def check_integer_stages(masks):
    from iswm_amd import ops
    t = torch.as_tensor(masks).to(dev())
    labels, areas = ops.ccl(t)
    pre, weight, area = ops.mask_preprocess(t)
    fronts, stats = ops.mask_fronts(pre, weight)
    rep = ops.mask_morph(ops.mask_morph(t, 3, True), 2, False)
    labels, areas, pre, weight, area = (x.cpu().numpy() for x in (labels, areas, pre, weight, area))
    fronts, stats, rep = fronts.cpu().numpy(), stats.cpu().numpy(), rep.cpu().numpy()
    for k, m in enumerate(masks):
        cl, ca = R.canonical_labels(m)
        assert np.array_equal(labels[k], cl), "ccl labels, frame %d" % k
        assert np.array_equal(areas[k], ca), "ccl areas, frame %d" % k
        ref = R.preprocess_mask(m)
        assert np.array_equal(pre[k], (ref > 0).astype(np.uint8)), "preprocess mask, frame %d" % k
        assert weight[k] == (ref.max() if ref.any() else 0.0), "preprocess weight, frame %d" % k
        assert area[k] == (ref > 0).sum()
        want = np.full(m.shape[0], -1)
        for y in range(m.shape[0]):
            cols = np.flatnonzero(ref[y] == 1)
            if len(cols):
                want[y] = cols[0]
        assert np.array_equal(fronts[k], want), "fronts, frame %d" % k
        ys = np.flatnonzero(want >= 0)
        assert stats[k].tolist() == [len(ys), int(ys.sum()), int(want[ys].sum())]
        assert np.array_equal(rep[k], R.repair_small_gaps(m)), "repair, frame %d" % k


@pytest.mark.parametrize("h,w", SIZES)
def test_integer_stages_bit_exact_on_blobs(h, w):
    masks = np.stack([blobs(h, w, d, 1000 * h + 10 * w + i) for i, d in enumerate(DENSITIES)])
    check_integer_stages(masks)


def spiral(n):
    m = np.zeros((n, n), np.uint8)
    y0, x0, y1, x1 = 0, 0, n - 1, n - 1
    while y0 <= y1 and x0 <= x1:
        m[y0, x0:x1 + 1] = 1
        m[y0:y1 + 1, x1] = 1
        if y1 > y0 + 1:
            m[y1, x0:x1 + 1] = 1
        if x1 > x0 + 2:
            m[y0 + 2:y1 + 1, x0] = 1
        y0, x0, y1, x1 = y0 + 2, x0 + 2, y1 - 2, x1 - 2
    return m


def snake(h, w):
    m = np.zeros((h, w), np.uint8)
    for y in range(0, h, 2):
        m[y, :] = 1
        if y + 1 < h:
            m[y + 1, w - 1 if (y // 2) % 2 == 0 else 0] = 1
    return m


def test_ccl_adversarial_masks():
    from iswm_amd import ops
    n = 129
    cb = (np.add.outer(np.arange(n), np.arange(n)) % 2 == 0).astype(np.uint8)        # diagonal-only: one component
    tie = np.zeros((n, n), np.uint8)
    tie[70:90, 5:25] = 1
    tie[3:23, 100:120] = 1                                      # equal areas: the one whose first pixel comes first
    for m in (spiral(n), snake(n, n), snake(97, 300), cb, np.ones((n, n), np.uint8), np.zeros((n, n), np.uint8), tie):
        check_integer_stages(m[None])
    lab, _ = ops.ccl(torch.as_tensor(cb[None]).to(dev()))
    assert int((lab.cpu() == 0).sum()) == int(cb.sum())
    pre, weight, _ = ops.mask_preprocess(torch.as_tensor(tie[None]).to(dev()))
    assert pre.cpu()[0, 3, 100] == 1 and pre.cpu()[0, 70, 5] == 0 and float(weight.cpu()[0]) == 0.8


def test_scores_against_restatement():
    from iswm_amd import ops
    for (h, w) in SIZES[1:]:
        pr = np.stack([blobs(h, w, d, 7 * h + i, cell=max(1, min(h, w) // 3)) for i, d in enumerate(DENSITIES)])
        gt = np.stack([blobs(h, w, d, 9 * h + i, cell=max(1, min(h, w) // 3)) for i, d in enumerate(DENSITIES)])
        gt[2] = pr[2]
        gt[3, :, 1:] = pr[3, :, :-1]                            # one column apart
        P, G = torch.as_tensor(pr).to(dev()), torch.as_tensor(gt).to(dev())
        # second preprocess, as every consumer of the reference sees it
        pv, pw, _ = ops.mask_preprocess(ops.mask_preprocess(P)[0])
        gv, gw, _ = ops.mask_preprocess(ops.mask_preprocess(G)[0])
        pf, ps = ops.mask_fronts(pv, pw)
        gf, gs = ops.mask_fronts(gv, gw)
        tau = w * 0.1
        err = ops.front_error(pf, gf, tau).cpu().numpy()
        stab, mot = ops.mask_pair_scores(pf, ps, gv, gw, gs)
        stab, mot = stab.cpu().numpy(), mot.cpu().numpy()
        reg, valid = (x.cpu().numpy() for x in ops.region_score(P, G))
        ft = R.FrontTrackingMetrics()
        ft.max_distance_threshold = tau
        for k in range(len(pr)):
            assert rel_close(err[k], ft.calculate_error(pr[k], gt[k])), ("front error", h, w, k)
            p1, g1 = R.preprocess_mask(pr[k]), R.preprocess_mask(gt[k])
            assert rel_close(stab[k], R.calculate_stability(p1, g1)), ("stability", h, w, k)
            assert rel_close(mot[k], R.calculate_motion(p1, g1)), ("motion", h, w, k)
            r = R.region_metrics(pr[k], gt[k])
            assert valid[k] == (r is not None), ("region valid", h, w, k)
            if r is not None:
                assert rel_close(reg[k], r), ("region", h, w, k)


def wave_sequence(n, h, w, kinds, seed, shift=0):
    """a front moving right one column per frame where kinds[t] = 1, empty frames elsewhere"""
    rng = np.random.default_rng(seed)
    out = np.zeros((n, h, w), np.uint8)
    for t in range(n):
        if kinds[t]:
            x0 = 8 + 2 * t + shift
            out[t, 5:h - 5, x0:x0 + w // 3] = 1
            out[t, rng.integers(0, h), rng.integers(0, w)] = 1
    return out


def reference_run(gt, pr, L):
    ref = R.StreamMetrics(2, sequence_length=L)
    for i in range(len(gt) - L + 1):
        ref.update(gt[i:i + L], pr[i:i + L])
    return ref.get_results()


def test_stream_metrics_end_to_end():
    from iswm_amd.metrics import StreamMetrics
    n, h, w, L = 20, 65, 80, 7
    gk = [0] * 7 + [1] * 7 + [1, 0, 1, 1, 0, 1]                # no-wave, all-wave and mixed windows
    pk = [0, 1, 0, 0, 0, 0, 0] + [1] * 6 + [0] + [1, 1, 0, 1, 0, 1]
    gt = wave_sequence(n, h, w, gk, 1)
    pr = wave_sequence(n, h, w, pk, 2, shift=1)
    pr[9, 30:40, 60:70] = 1                                     # a second region: weight 0.8, no fronts
    want = reference_run(gt, pr, L)
    m = StreamMetrics(2, sequence_length=L)
    G, P = torch.as_tensor(gt).to(dev()), torch.as_tensor(pr).to(dev()).to(torch.int64)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for i in range(n - L + 1):
            m.update(G[i:i + L], P[i:i + L], sequence_data=True)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    got = m.get_results()
    assert set(got) == set(want)
    for k in want:
        assert rel_close(got[k], want[k]), (k, got[k], want[k])
    assert got["Best Score"] > 0 and 0 < got["Transition Accuracy"] < 1
    # the confusion-matrix keys are those of update_logits over the same last frames
    last = torch.as_tensor(pr[L - 1:]).to(dev())
    logits = torch.stack([1.0 - last.float(), last.float()], 1)
    m2 = StreamMetrics(2)
    m2.update_logits(G[L - 1:], logits)
    r2 = m2.get_results()
    for k in ("MIoU", "Foreground IoU", "Foreground F1", "Precision", "Recall"):
        assert got[k] == r2[k], k
    # the evaluators' own interfaces
    t = m.temporal_evaluator.get_detailed_statistics()
    updates = n - L + 1                                         # one stored frame per update; a score from the L-th
    assert t["score_count"] == updates - L + 1 and rel_close(t["mean_score"], want["Temporal Consistency"])
    st = m.region_evaluator.get_statistics()
    assert st["total_cases"] == updates and rel_close(st["valid_ratio"], want["Region Valid Ratio"])
    best = m.best_score["weighted_score"]
    m.reset()
    assert m.get_results()["Best Score"] == best and m.front_tracking_evaluator.max_distance_threshold == w * 0.1


def test_train_sequence_validation(tmp_path, capsys):
    from iswm_amd import network, ops, train
    ck = str(tmp_path / "ck")
    args = ["--model", "deeplabv3plus_resnet50", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
            "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "2", "--val_interval", "2",
            "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0", "--total_itrs", "2",
            "--val_metrics", "sequence", "--sequence_length", "4"]
    train.main(args)
    out = capsys.readouterr().out
    assert "Validation @2" in out
    for key in ("Temporal Consistency", "Front Tracking Error", "Region Continuity", "Transition Accuracy",
                "Stability Score", "Motion Consistency", "Wave Segment Score", "Region Valid Ratio", "Best Score"):
        assert key in out, key
    files = glob.glob(os.path.join(ck, "best_*.pth"))
    assert len(files) == 1
    ckpt = torch.load(files[0], map_location="cpu", weights_only=True)
    # the same masks again from the saved weights, scored by the restatement
    opts = train.get_argparser().parse_args(args)
    opts.num_classes = 2
    model = network.modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    model.load_state_dict(ckpt["model_state"])
    model = model.to(dev()).eval()
    _, val = train.get_dataset(opts)
    preds, gts = [], []
    with torch.no_grad():                                       # the validation loader's batches, as in training
        for img, lab in torch.utils.data.DataLoader(val, batch_size=4, shuffle=False, num_workers=0):
            preds.append(ops.argmax_nchw(model(img.to(dev(), dtype=torch.float32))).cpu().numpy())
            gts.append(lab.numpy())
    order = sorted(range(len(val)), key=lambda i: val.images[i])
    want = reference_run(np.concatenate(gts)[order], np.concatenate(preds)[order], 4)
    assert rel_close(ckpt["weighted_score"], train.logged_weighted_score(want))
    assert ckpt["best_score"]["Foreground IoU"] == pytest.approx(want["Foreground IoU"], abs=1e-12)
