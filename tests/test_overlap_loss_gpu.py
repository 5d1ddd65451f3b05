"""The two-pass overlap-loss kernels of csrc/loss.hip (soft Dice / Tversky / focal-Tversky next to the weighted CE) against the
float64 restatement of tests/overlap_loss_ref.py: sums, loss and gradient within 4 x FLOOR (the rule of
tests/test_streaming_kernels_gpu.py; gradient error = max |difference| / max |float64 gradient|), exactly zero gradients at
invalid pixels, the CE sums bit for bit as iswm_loss_fwd forms them, identical bits from two calls, a saturated probe whose sums
are integer counts (one dropped or doubled pixel fails it at any size), the autograd module, and the trainer with the new options.

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import glob
import os

import pytest
import torch

from tests import overlap_loss_ref as R

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def emit(line):
    print(line)
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write(line + "\n")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def run(logits, labels, wt, ignore_index, args, upstream=1.0):
    """the three ops calls -> (sums float64, loss fp32 [1], grad), all on the device"""
    from iswm_amd import ops
    d = dev()
    lg, lb, w = logits.to(d), labels.to(d), None if wt is None else wt.to(d)
    sums = ops.overlap_loss_fwd(lg, lb, w, ignore_index)
    loss, coef = ops.overlap_loss_coeffs(sums, logits.shape[1], *args)
    grad = ops.overlap_loss_bwd(lg, lb, w, ignore_index, coef, torch.tensor([upstream], dtype=torch.float32, device=d))
    return sums, loss, grad


def check3(group, got, ref, what, worst, ignore_index=R.IGNORE, labels=None):
    sums, loss, grad = got
    for key, a, e in (("sums", sums, ref["sums"]), ("loss", loss.reshape(()), ref["loss"]), ("grad", grad, ref["grad"])):
        k = R.floor_key(key, group)
        floor = R.FLOOR[k]
        err = R.rel_err(a.cpu(), e)
        line = "%-16s floor %.1e  bound %.1e  measured %.2e  %s" % (k, floor, 4 * floor, err, what)
        if err >= worst.get(k, (-1.0, ""))[0]:
            worst[k] = (err, line)
        assert err <= 4 * floor, line
    invalid = ~R.valid_mask(labels, grad.shape[1], ignore_index)
    at_invalid = grad.cpu().permute(0, 2, 3, 1)[invalid]
    assert torch.equal(at_invalid, torch.zeros_like(at_invalid)), "gradient of an ignored / out-of-range label is not exactly 0"
    return int(invalid.sum())


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_sums_loss_gradient(case):
    """every COMBOS entry (class weights x CE factor x parameter set x class set) on one input; per combination also: the CE
    sums are ops.loss_fwd's bits, and a second call gives the same bits"""
    from iswm_amd import ops
    shape, kind, scale = case
    logits, labels, weight = R.inputs(shape, kind, R.SCALES[scale])
    worst, d = {}, dev()
    ce_sums = {}
    for wt_on in (False, True):
        w = weight.to(d) if wt_on else None
        ce_sums[wt_on] = ops.loss_fwd(logits.to(d), labels.to(d), w, R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1].clone()
    for combo in R.COMBOS:
        wt, args = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], combo)
        got = run(logits, labels, wt, R.IGNORE, args)
        n_invalid = check3(R.group(shape, scale), got, ref, R.combo_id(combo), worst, labels=labels)
        assert n_invalid >= (4 if labels.numel() >= 8 else 0)
        assert torch.equal(bits(got[0][:2].float()), bits(ce_sums[combo[0]])), "CE sums differ from iswm_loss_fwd's"
        again = run(logits, labels, wt, R.IGNORE, args)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), "two calls differ"
    for k in sorted(worst):
        emit(worst[k][1] + "  (largest of %d combinations)" % len(R.COMBOS))


@pytest.mark.parametrize("name", list(R.BIG))
def test_many_blocks(name):
    """cap: 1 x 2897 x 2897 = 8 392 609 pixels > 8192 blocks x 256 threads x 4: a second trip through the grid-stride loop, ragged.
    fin: 1037 blocks: the finalize kernel adds one 16-deep batch of partials in every lane, then a tail in 13 lanes."""
    from iswm_amd import _lib, ops
    shape = R.BIG[name]
    logits, labels, weight = R.inputs(shape, "u8", 1.0)
    npix, d = labels.numel(), dev()
    blocks = _lib.load().iswm_loss_blocks(npix)
    if name == "cap":
        assert blocks == 8192 and 8192 * 1024 < npix < 2 * 8192 * 1024 and npix % 1024 != 0
    else:
        assert 16 * 64 < blocks < 17 * 64
    worst = {}
    for combo in R.CAP_COMBOS:
        wt, args = R.combo_args(combo, weight)
        ref = R.reference(shape, "u8", 1.0, combo)
        got = run(logits, labels, wt, R.IGNORE, args)
        check3(name, got, ref, R.combo_id(combo), worst, labels=labels)
        ce = ops.loss_fwd(logits.to(d), labels.to(d), None if wt is None else wt.to(d), R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1]
        assert torch.equal(bits(got[0][:2].float()), bits(ce))
    for k in sorted(worst):
        emit(worst[k][1])


@pytest.mark.parametrize("pattern", R.DEGENERATE)
@pytest.mark.parametrize("kind", ["u8", "i64"])
def test_degenerate_label_patterns(pattern, kind):
    logits, labels, weight = R.degenerate_inputs(pattern, kind)
    worst = {}
    for combo in R.degenerate_combos(pattern):
        wt, args = R.combo_args(combo, weight)
        ref = R.degenerate_reference(pattern, combo, kind)
        sums, loss, grad = run(logits, labels, wt, R.IGNORE, args)
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(grad).all()), R.combo_id(combo)
        if pattern == "all_ignored":
            assert float(loss) == 0.0 and not bool(grad.any()) and not bool(sums.any()), R.combo_id(combo)
        else:
            check3("degen", (sums, loss, grad), ref, R.combo_id(combo), worst, labels=labels)
    for k in sorted(worst):
        emit(worst[k][1] + "  (%s)" % pattern)


def test_ignore_index_inside_the_class_range():
    """three classes with ignore_index 2: pixels labelled 2 are no part of I, P or G and get a zero gradient (the inputs the
    mutants of test_overlap_loss_cpu.py are shown on)"""
    logits, labels, weight = R.inputs(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    wt, args = R.combo_args(R.IG2_COMBO, weight)
    ref = R.reference(R.IG2_SHAPE, "u8", 1.0, R.IG2_COMBO, R.IG2_IGNORE)
    worst = {}
    got = run(logits, labels, wt, R.IG2_IGNORE, args)
    assert check3("ig2", got, ref, R.combo_id(R.IG2_COMBO), worst, R.IG2_IGNORE, labels) > 20
    for k in sorted(worst):
        emit(worst[k][1])


SATURATED = [(sh, kind) for sh in R.SHAPES for kind in ("u8", "i64")] + [(sh, "u8") for sh in R.BIG]


@pytest.mark.parametrize("shape,kind", SATURATED, ids=["%s_%s" % c for c in SATURATED])
def test_saturated_probe_counts_every_pixel_once(shape, kind):
    """logits +-40 by a hard mask: every probability is 0 or 1 to within 1e-34, so I_c, P_c and G_c are the integer true-positive,
    predicted and labelled counts of the valid pixels (< 2^24: exact in every fp32 partial) -- to 1e-6 absolute"""
    from iswm_amd import ops
    logits, labels, counts = R.saturated_inputs(shape, kind)
    assert float(counts.max()) < 2 ** 24
    d = dev()
    sums = ops.overlap_loss_fwd(logits.to(d), labels.to(d), None, R.IGNORE).cpu()
    err = float((sums[2:] - counts).abs().max())
    emit("saturated %-8s %-3s  largest count %d  max |sums - counts| %.1e" % (shape, kind, int(counts.max()), err))
    assert err <= 1e-6
    assert float(sums[1]) == float(counts[2 * logits.shape[1]:].sum())               # sum w without weights: the valid pixels


@pytest.mark.parametrize("name", ["dice", "focal"])
def test_module_end_to_end(name):
    """TverskyLoss / DiceLoss through autograd: the ops calls' loss and gradient, bit for bit; an upstream factor scales it"""
    from iswm_amd.utils.loss import DiceLoss, TverskyLoss
    logits, labels, weight = R.inputs("img", "u8", 1.0)
    d = dev()
    if name == "dice":
        crit = DiceLoss(ce_weight=1.0, overlap_weight=2.0, weight=weight).to(d)
        args = (1.0, 2.0, 0.5, 0.5, 1.0, 1.0, "foreground")
    else:
        crit = TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75, classes="all", weight=weight).to(d)
        args = (0.0, 1.0, 0.3, 0.7, 0.75, 1.0, "all")
    z = logits.to(d).requires_grad_(True)
    loss = crit(z, labels.to(d))
    loss.backward()
    _, want_loss, want_grad = run(logits, labels, weight, R.IGNORE, args)
    assert loss.shape == () and torch.equal(bits(loss.detach().reshape(1)), bits(want_loss)) and torch.equal(bits(z.grad), bits(want_grad))
    z2 = logits.to(d).requires_grad_(True)
    (crit(z2, labels.to(d).long()) * 0.37).backward()                          # int64 labels, upstream 0.37
    _, _, scaled = run(logits, labels.long(), weight, R.IGNORE, args, upstream=0.37)
    assert torch.equal(bits(z2.grad), bits(scaled))
    ref = R.overlap_ref(logits, labels, weight, R.IGNORE, *args)
    err = R.rel_err(z2.grad.cpu(), ref["grad"] * float(torch.tensor(0.37, dtype=torch.float32)))
    emit("module %-5s upstream 0.37: gradient rel err %.2e (bound %.1e)" % (name, err, 4 * R.FLOOR["grad.img_s1"]))
    assert err <= 4 * R.FLOOR["grad.img_s1"]


def test_more_than_eight_classes_is_refused():
    from iswm_amd.utils.loss import DiceLoss
    d = dev()
    with pytest.raises(ValueError, match="at most 8 classes"):
        DiceLoss()(torch.zeros(1, 9, 4, 4, device=d), torch.zeros(1, 4, 4, dtype=torch.int64, device=d))


@pytest.mark.parametrize("extra", [["--overlap_loss", "dice"], ["--overlap_loss", "focal_tversky", "--ce_weight", "0"]],
                         ids=["dice", "focal_tversky_only"])
def test_train_main_with_an_overlap_loss(tmp_path, capsys, extra):
    """the small synthetic configuration of tests/test_train_entry.py with the new criterion: the iterations run, the printed
    losses are finite and a checkpoint is written"""
    import math
    import re
    from iswm_amd import train
    dev()
    ck = str(tmp_path / "ck")
    train.main(["--model", "deeplabv3plus_resnet50", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
                "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "2", "--val_interval", "2",
                "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0", "--total_itrs", "4"] + extra)
    out = capsys.readouterr().out
    assert "Itrs 4/4" in out and "Validation @2" in out
    losses = [float(v) for v in re.findall(r"Loss[=: ]+([-+0-9.eE]+|nan|inf)", out)]
    assert len(losses) >= 2 and all(math.isfinite(v) and v > 0 for v in losses), out[-2000:]
    assert len(glob.glob(os.path.join(ck, "best_*.pth"))) == 1
