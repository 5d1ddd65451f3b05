"""The two-pass distillation kernels of csrc/distill.hip (weighted CE + tau^2 KL(teacher || student)) against the float64
restatement of tests/distill_ref.py: the three float sums each by its own scale, loss and gradient within 4 x FLOOR (gradient
error = max |difference| / max |float64 gradient|), N and A exactly, exactly zero gradients at invalid pixels, the CE sums bit for
bit as iswm_loss_fwd forms them, identical bits from two calls, a teacher equal to the student (sum KL == 0.0 and a distillation
gradient of exactly 0), a saturated probe whose agreement count is an integer known beforehand (one dropped or doubled pixel fails
it at any size), the autograd module, and the trainer with a frozen teacher.

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import glob
import itertools
import math
import os
import re

import pytest
import torch

from tests import distill_ref as R

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


def run(student, teacher, labels, wt, ignore_index, tau, lce, lkd, upstream=1.0):
    """the three ops calls -> (sums float64 [5], out fp32 [3] = {loss, CE term, KD term}, grad), all on the device"""
    from iswm_amd import ops
    d = dev()
    s, t, lb, w = student.to(d), teacher.to(d), labels.to(d), None if wt is None else wt.to(d)
    sums = ops.distill_loss_fwd(s, t, lb, w, ignore_index, tau)
    out, coef = ops.distill_loss_coeffs(sums, lce, lkd, tau)
    grad = ops.distill_loss_bwd(s, t, lb, w, ignore_index, tau, coef, torch.tensor([upstream], dtype=torch.float32, device=d))
    return sums, out, grad


def check(group, got, ref, what, worst, labels, ignore_index=R.IGNORE):
    """every float check of R.CHECKS within 4 x FLOOR, N and A exactly, zero gradients at invalid pixels -> invalid pixels"""
    sums, out, grad = got
    for key, err in R.errors(sums, out[0].cpu(), grad.cpu(), ref).items():
        k = R.floor_key(key, group)
        floor = R.FLOOR[k]
        line = "%-16s floor %.1e  bound %.1e  measured %.2e  %s" % (k, floor, 4 * floor, err, what)
        if err >= worst.get(k, (-1.0, ""))[0]:
            worst[k] = (err, line)
        assert err <= 4 * floor, line
    assert sums[3:].cpu().tolist() == ref["sums"][3:].tolist(), "N, A = %s, expected %s (%s)" % (sums[3:].tolist(), ref["sums"][3:].tolist(), what)
    terms = out.cpu().double()
    assert abs(float(terms[1] + terms[2]) - float(terms[0])) <= 2.0 ** -23 * abs(float(terms[0])), "terms do not add up: %s" % what
    invalid = ~R.valid_mask(labels, grad.shape[1], ignore_index)
    at_invalid = grad.cpu().permute(0, 2, 3, 1)[invalid]
    assert torch.equal(at_invalid, torch.zeros_like(at_invalid)), "gradient of an ignored / out-of-range label is not exactly 0"
    return int(invalid.sum())


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_sums_loss_gradient(case):
    """every temperature x COMBOS entry on one input; per combination also: the CE sums are ops.loss_fwd's bits, and a second call
    gives the same bits"""
    from iswm_amd import ops
    shape, kind, scale = case
    student, teacher, labels, weight = R.pair(shape, kind, R.SCALES[scale])
    worst, d = {}, dev()
    ce_sums = {}
    for wt_on in (False, True):
        w = weight.to(d) if wt_on else None
        ce_sums[wt_on] = ops.loss_fwd(student.to(d), labels.to(d), w, R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1].clone()
    for temp, combo in itertools.product(R.TEMPS, R.COMBOS):
        wt, lce, lkd = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], temp, combo)
        what = "%s %s" % (temp, R.combo_id(combo))
        got = run(student, teacher, labels, wt, R.IGNORE, R.TEMPS[temp], lce, lkd)
        n_invalid = check(R.group(shape, scale), got, ref, what, worst, labels)
        assert n_invalid >= (4 if labels.numel() >= 8 else 0)
        assert torch.equal(bits(got[0][:2].float()), bits(ce_sums[combo[0]])), "CE sums differ from iswm_loss_fwd's (%s)" % what
        again = run(student, teacher, labels, wt, R.IGNORE, R.TEMPS[temp], lce, lkd)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), "two calls differ (%s)" % what
    for k in sorted(worst):
        emit(worst[k][1] + "  (largest of %d combinations)" % (len(R.TEMPS) * len(R.COMBOS)))


@pytest.mark.parametrize("name", list(R.BIG))
def test_many_blocks(name):
    """cap: 1 x 2897 x 2897 = 8 392 609 pixels > 8192 blocks x 256 threads x 4: a second trip through the grid-stride loop, ragged,
    with two logit tensors.  fin: 1037 blocks: the finalize kernel adds one 16-deep batch of partials in every lane, then a tail
    in 13 lanes."""
    from iswm_amd import _lib, ops
    shape = R.BIG[name]
    student, teacher, labels, weight = R.pair(shape, "u8", 1.0)
    npix, d = labels.numel(), dev()
    blocks = _lib.load().iswm_loss_blocks(npix)
    assert _lib.load().iswm_distill_loss_partials(npix) == 5 * blocks
    if name == "cap":
        assert blocks == 8192 and 8192 * 1024 < npix < 2 * 8192 * 1024 and npix % 1024 != 0
    else:
        assert 16 * 64 < blocks < 17 * 64
    worst = {}
    wt, lce, lkd = R.combo_args(R.BIG_COMBO, weight)
    ref = R.reference(shape, "u8", 1.0, R.BIG_TEMP, R.BIG_COMBO)
    got = run(student, teacher, labels, wt, R.IGNORE, R.TEMPS[R.BIG_TEMP], lce, lkd)
    check(name, got, ref, R.combo_id(R.BIG_COMBO), worst, labels)
    ce = ops.loss_fwd(student.to(d), labels.to(d), wt.to(d), R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1]
    assert torch.equal(bits(got[0][:2].float()), bits(ce))
    for k in sorted(worst):
        emit(worst[k][1])


@pytest.mark.parametrize("temp", R.SAME_TEMPS)
def test_teacher_equal_to_the_student(temp):
    """the same bits in both tensors: sum KL == 0.0 and A == N; with lce = 0 the gradient is exactly 0 everywhere, with lce = 1 it
    is the CE's (within 4 x FLOOR of the float64 gradient)"""
    student, _, labels, weight = R.pair(R.SAME_CASE[0], R.SAME_CASE[1], R.SCALES[R.SAME_CASE[2]])
    tau = R.TEMPS[temp]
    sums, out, grad = run(student, student.clone(), labels, weight, R.IGNORE, tau, 0.0, 1.0)
    assert float(sums[2]) == 0.0 and float(sums[3]) == float(sums[4]) > 0
    assert float(out[0]) == 0.0 and float(out[2]) == 0.0
    assert torch.equal(grad.cpu(), torch.zeros_like(student)), "distillation gradient of teacher == student is not exactly 0"
    worst = {}
    got = run(student, student.clone(), labels, weight, R.IGNORE, tau, 1.0, 2.0)
    assert float(got[0][2]) == 0.0 and float(got[1][2]) == 0.0
    check("same", got, R.same_reference(temp), temp, worst, labels)
    for k in sorted(worst):
        emit(worst[k][1])


SATURATED = [(sh, kind) for sh in R.SHAPES for kind in ("u8", "i64")] + [(sh, "u8") for sh in R.BIG]


@pytest.mark.parametrize("shape,kind", SATURATED, ids=["%s_%s" % c for c in SATURATED])
def test_saturated_probe_counts_every_pixel_once(shape, kind):
    """student and teacher logits +-40 by two different hard masks: A is the integer count of valid pixels where the masks
    coincide and N the valid count, exactly, at every size"""
    from iswm_amd import ops
    student, teacher, labels, n, a = R.saturated_pair(shape, kind)
    d = dev()
    sums = ops.distill_loss_fwd(student.to(d), teacher.to(d), labels.to(d), None, R.IGNORE, 2.0).cpu()
    emit("saturated %-8s %-3s  N %d  A %d  got N %.1f  A %.1f" % (shape, kind, n, a, float(sums[3]), float(sums[4])))
    assert sums[3:].tolist() == [float(n), float(a)]
    assert float(sums[1]) == float(n)                                    # sum w without weights: the valid pixels
    assert n == 0 or 0 < a < n or labels.numel() == 1


@pytest.mark.parametrize("pattern", R.DEGENERATE)
@pytest.mark.parametrize("kind", ["u8", "i64"])
def test_degenerate_label_patterns(pattern, kind):
    student, teacher, labels, weight = R.degenerate_inputs(pattern, kind)
    worst = {}
    for combo in R.degenerate_combos(pattern):
        wt, lce, lkd = R.combo_args(combo, weight)
        ref = R.degenerate_reference(pattern, combo, kind)
        sums, out, grad = run(student, teacher, labels, wt, R.IGNORE, R.TEMPS[R.DEGEN_TEMP], lce, lkd)
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all()), R.combo_id(combo)
        if pattern == "all_ignored":
            assert float(out[0]) == 0.0 and not bool(grad.any()) and not bool(sums.any()), R.combo_id(combo)
        else:
            check("degen", (sums, out, grad), ref, R.combo_id(combo), worst, labels)
    for k in sorted(worst):
        emit(worst[k][1] + "  (%s)" % pattern)


def test_ignore_index_inside_the_class_range():
    """three classes with ignore_index 2: pixels labelled 2 are no part of N, A or sum KL and get a zero gradient (the inputs the
    mutants of test_distill_cpu.py are shown on)"""
    student, teacher, labels, weight = R.pair(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE)
    worst = {}
    for temp in R.IG2_TEMPS:
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, temp, R.IG2_COMBO, R.IG2_IGNORE)
        got = run(student, teacher, labels, weight, R.IG2_IGNORE, R.TEMPS[temp], R.IG2_COMBO[1], R.IG2_COMBO[2])
        assert check("ig2", got, ref, temp, worst, labels, R.IG2_IGNORE) > 20
    for k in sorted(worst):
        emit(worst[k][1])


def test_equal_maxima_take_the_lowest_class():
    """all-zero student and teacher logits: every class is a maximum, both argmax are class 0 -> A == N, and sum KL == 0"""
    from iswm_amd import ops
    d = dev()
    for c in (2, 3, 8):
        z = torch.zeros(2, c, 5, 7, device=d)
        y = torch.zeros(2, 5, 7, dtype=torch.uint8, device=d)
        y[0, 0, :3] = R.IGNORE
        sums = ops.distill_loss_fwd(z, z.clone(), y, None, R.IGNORE, 2.0).cpu()
        assert sums[2:].tolist() == [0.0, 67.0, 67.0], (c, sums.tolist())
    # a tie in ONE tensor only: the student's maxima are classes 0 and 1 (-> 0), the teacher prefers class 1: no agreement
    s = torch.zeros(1, 2, 2, 2, device=d)
    t = torch.zeros(1, 2, 2, 2, device=d)
    t[:, 1] = 1.0
    sums = ops.distill_loss_fwd(s, t, torch.zeros(1, 2, 2, dtype=torch.int64, device=d), None, R.IGNORE, 1.0).cpu()
    assert sums[3:].tolist() == [4.0, 0.0]


def test_module_end_to_end():
    """DistillationLoss through autograd: the ops calls' loss and gradient, bit for bit; an upstream factor scales it; a second
    backward through the same call is refused; last_terms and last_agreement"""
    from iswm_amd.network._hip import CONSUMED
    from iswm_amd.utils.loss import DistillationLoss
    student, teacher, labels, weight = R.pair("img", "u8", 1.0)
    d, tau = dev(), 2.0
    crit = DistillationLoss(temperature=tau, ce_weight=1.0, distill_weight=2.0, weight=weight).to(d)
    z = student.to(d).requires_grad_(True)
    loss = crit(z, labels.to(d), teacher.to(d))
    terms, (agree, nvalid) = crit.last_terms, crit.last_agreement
    loss.backward(retain_graph=True)
    sums, want, want_grad = run(student, teacher, labels, weight, R.IGNORE, tau, 1.0, 2.0)
    assert loss.shape == () and torch.equal(bits(loss.detach().reshape(1)), bits(want[:1])) and torch.equal(bits(z.grad), bits(want_grad))
    with pytest.raises(RuntimeError, match=re.escape(CONSUMED)):
        loss.backward()
    ref = R.reference("img", "u8", 1.0, "t2", (True, 1.0, 2.0))
    assert torch.equal(bits(terms), bits(want[1:]))
    assert abs(float(terms.double().sum()) - float(loss.detach())) <= 2.0 ** -23 * abs(float(loss.detach()))       # one fp32 rounding
    assert (float(nvalid), float(agree)) == (float(ref["sums"][3]), float(ref["sums"][4])) and agree.dim() == 0
    z2 = student.to(d).requires_grad_(True)
    (crit(z2, labels.to(d).long(), teacher.to(d)) * 0.37).backward()          # int64 labels, upstream 0.37
    _, _, scaled = run(student, teacher, labels.long(), weight, R.IGNORE, tau, 1.0, 2.0, upstream=0.37)
    assert torch.equal(bits(z2.grad), bits(scaled))
    err = R.rel_err(z2.grad.cpu(), ref["grad"] * float(torch.tensor(0.37, dtype=torch.float32)))
    emit("module upstream 0.37: gradient rel err %.2e (bound %.1e)" % (err, 4 * R.FLOOR["grad.img_s1"]))
    assert err <= 4 * R.FLOOR["grad.img_s1"]


def test_more_than_eight_classes_and_another_shape_are_refused():
    from iswm_amd import ops
    from iswm_amd.utils.loss import DistillationLoss
    d = dev()
    y = torch.zeros(1, 4, 4, dtype=torch.int64, device=d)
    with pytest.raises(ValueError, match="at most 8 classes"):
        DistillationLoss()(torch.zeros(1, 9, 4, 4, device=d), y, torch.zeros(1, 9, 4, 4, device=d))
    z = torch.zeros(1, 2, 4, 4, device=d)
    for bad in (torch.zeros(1, 2, 4, 5, device=d), torch.zeros(1, 3, 4, 4, device=d), torch.zeros(2, 2, 4, 4, device=d)):
        with pytest.raises(ValueError, match="shape"):                  # before any launch: the ops calls check it themselves
            ops.distill_loss_fwd(z, bad, y, None, 255, 1.0)
        with pytest.raises(ValueError, match="shape"):
            ops.distill_loss_bwd(z, bad, y, None, 255, 1.0, torch.zeros(2, device=d), torch.ones(1, device=d))
        with pytest.raises(ValueError, match="shape"):
            DistillationLoss()(z, y, bad)
    with pytest.raises(ValueError, match="teacher"):
        ops.distill_loss_fwd(z, z.double(), y, None, 255, 1.0)
    with pytest.raises(ValueError, match="teacher"):
        ops.distill_loss_fwd(z, z.cpu(), y, None, 255, 1.0)


COMMON = ["--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16", "--optimizer", "sgd", "--loss_type", "IWce_loss",
          "--print_interval", "2", "--val_interval", "2", "--val_batch_size", "4", "--num_workers", "0"]


@pytest.mark.parametrize("ema", [False, True], ids=["live", "ema"])
def test_train_main_with_a_teacher(tmp_path, capsys, ema):
    """the small synthetic configuration of tests/test_train_entry.py: a ResNet-50 teacher trained for 2 iterations, then a
    MobileNetV2 student trained for 4 against its checkpoint (ema: against the checkpoint's EMA weights)"""
    from iswm_amd import network, train
    dev()
    tdir, sdir = str(tmp_path / "teacher"), str(tmp_path / "student")
    train.main(["--model", "deeplabv3plus_resnet50", "--checkpoints_dir", tdir, "--total_itrs", "2"] + COMMON +
               (["--ema_decay", "0.9"] if ema else []))
    (teacher_ck,) = glob.glob(os.path.join(tdir, "best_*.pth"))
    with open(teacher_ck, "rb") as f:
        before = f.read()
    capsys.readouterr()
    train.main(["--model", "deeplabv3plus_mobilenet", "--checkpoints_dir", sdir, "--total_itrs", "4", "--distill_ckpt", teacher_ck,
                "--distill_model", "deeplabv3plus_resnet50", "--distill_temperature", "2"] + COMMON +
               (["--distill_use_ema"] if ema else []))
    out = capsys.readouterr().out
    assert "Itrs 4/4" in out and "Validation @2" in out and "Validation @4" in out and "Teacher deeplabv3plus_resnet50" in out
    losses = [float(v) for v in re.findall(r"Loss[=: ]+([-+0-9.eE]+|nan|inf)", out)]
    kds = [float(v) for v in re.findall(r"kd=([-+0-9.eE]+|nan|inf)", out)]
    agrees = [float(v) for v in re.findall(r"agree=([-+0-9.eE]+|nan|inf)%", out)]
    assert len(losses) >= 2 and all(math.isfinite(v) and v > 0 for v in losses), out[-2000:]
    assert len(kds) == 2 and all(math.isfinite(v) and v > 0 for v in kds), out[-2000:]
    assert len(agrees) == 2 and all(0.0 <= v <= 100.0 for v in agrees), out[-2000:]
    (student_ck,) = glob.glob(os.path.join(sdir, "best_*.pth"))
    saved = train.load_checkpoint(student_ck)
    fresh = network.modeling.deeplabv3plus_mobilenet(num_classes=2, output_stride=16, pretrained_backbone=False)
    assert set(saved["model_state"]) == set(fresh.state_dict())          # the student's keys, no teacher key
    assert "deeplabv3plus_mobilenet" in os.path.basename(student_ck) and saved["model_config"]["model_name"] == "deeplabv3plus_mobilenet"
    with open(teacher_ck, "rb") as f:
        assert f.read() == before, "the teacher checkpoint changed"
