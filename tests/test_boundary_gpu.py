"""The signed distance map and the two-pass boundary criterion of csrc/boundary.hip against tests/boundary_ref.py.

The map is compared by integer equality, no tolerance: the trivial planes, widths around the row block's 256 threads, three
images and three classes (leaks across planes), rows and columns longer than any chunk, every label pattern, both label widths,
both class selections, ignore_index outside and inside the class range; 4097 wide is refused without a launch.

The criterion: the three float sums each by its own scale, loss and gradient within 4 x FLOOR (gradient error = max |difference|
/ max |float64 gradient|; the boundary sum relative to sum |p phi|), N exactly, exactly zero gradients at invalid pixels, the CE
sums bit for bit as iswm_loss_fwd forms them, identical bits from two calls, the autograd module, and the trainer with the ramp.

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import itertools
import math
import os
import re

import pytest
import torch

from tests import boundary_ref as R

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


@pytest.mark.parametrize("shape", list(R.MAP_SHAPES))
def test_map_equals_the_definition(shape):
    from iswm_amd import ops
    b, c, h, w, _ = R.MAP_SHAPES[shape]
    d, runs = dev(), 0
    for pat, kind, classes, ig in itertools.product(R.map_runs(shape), ("u8", "i64"), R.CLASSES, (R.IGNORE, c - 1)):
        labels = R.map_labels(shape, pat, kind, ig)
        want = R.signed_edt_ref(labels, c, classes, ig)
        got = ops.signed_edt(labels.to(d), c, classes, ig)
        assert got.dtype == torch.int32 and got.shape == want.shape
        wrong = int((got.cpu() != want).sum())
        assert wrong == 0, "%s %s %s %s ignore %d: %d of %d pixels differ" % (shape, pat, kind, classes, ig, wrong, want.numel())
        runs += 1
    emit("map %-8s %d x %d x %d x %d: %d label tensors, every pixel equal" % (shape, b, c, h, w, runs))


@pytest.mark.parametrize("h,w", [(2, 4096), (4096, 2)])
def test_map_at_the_largest_side(h, w):
    """one foreground pixel in a corner of a 4096-long plane: the farthest distance is 4095^2 (+1), the row pass holds 32 KiB"""
    from iswm_amd import ops
    labels = torch.zeros(1, h, w, dtype=torch.uint8)
    labels[0, 0, 0] = 1
    got = ops.signed_edt(labels.to(dev()), 2).cpu()
    assert torch.equal(got, R.signed_edt_ref(labels, 2, how="scipy"))
    assert int(got.max()) == 4095 ** 2 + 1 and int(got[0, 0, 0, 0]) == -1


def test_a_side_above_4096_is_refused_without_a_launch():
    from iswm_amd import ops
    d = dev()
    for shape in ((1, 2, 4097), (1, 4097, 2)):
        with pytest.raises(ValueError, match="sides up to 4096"):
            ops.signed_edt(torch.zeros(shape, dtype=torch.uint8, device=d), 2)
    with pytest.raises(ValueError, match="no class plane"):
        ops.signed_edt(torch.zeros(1, 4, 4, dtype=torch.uint8, device=d), 1)
    with pytest.raises(ValueError, match="labels"):
        ops.signed_edt(torch.zeros(1, 4, 4, dtype=torch.int32, device=d), 2)
    torch.cuda.synchronize()


def run(logits, labels, wt, ignore_index, lce, lbd, clip, classes, sd2=None, upstream=1.0):
    """the map (unless given) and the three ops calls -> (sums float64 [4], out fp32 [3] = {loss, CE term, boundary term}, grad,
    map), all on the device"""
    from iswm_amd import ops
    d = dev()
    z, lb, w = logits.to(d), labels.to(d), None if wt is None else wt.to(d)
    m = ops.signed_edt(lb, z.shape[1], classes, ignore_index) if sd2 is None else sd2.to(d)
    sums = ops.boundary_loss_fwd(z, lb, m, w, ignore_index, classes, clip)
    out, coef = ops.boundary_loss_coeffs(sums, m.shape[1], lce, lbd)
    grad = ops.boundary_loss_bwd(z, lb, m, w, ignore_index, coef, torch.tensor([upstream], dtype=torch.float32, device=d), classes, clip)
    return sums, out, grad, m


def check(group, got, ref, what, worst, labels, ignore_index=R.IGNORE):
    """every float check of R.CHECKS within 4 x FLOOR, N exactly, zero gradients at invalid pixels -> invalid pixels"""
    sums, out, grad = got[:3]
    for key, err in R.errors(sums, out[0].cpu(), grad.cpu(), ref).items():
        k = R.floor_key(key, group)
        floor = R.FLOOR[k]
        line = "%-16s floor %.1e  bound %.1e  measured %.2e  %s" % (k, floor, 4 * floor, err, what)
        if err >= worst.get(k, (-1.0, ""))[0]:
            worst[k] = (err, line)
        assert err <= 4 * floor, line
    assert float(sums[3]) == float(ref["sums"][3]), "N = %s, expected %s (%s)" % (float(sums[3]), float(ref["sums"][3]), what)
    terms = out.cpu().double()
    assert abs(float(terms[1] + terms[2]) - float(terms[0])) <= 2.0 ** -22 * max(abs(float(terms[1])), abs(float(terms[2]))), \
        "terms do not add up: %s" % what
    invalid = ~R.valid_mask(labels, grad.shape[1], ignore_index)
    at_invalid = grad.cpu().permute(0, 2, 3, 1)[invalid]
    assert torch.equal(at_invalid, torch.zeros_like(at_invalid)), "gradient of an ignored / out-of-range label is not exactly 0"
    return int(invalid.sum())


@pytest.mark.parametrize("case", R.INPUT_CASES, ids=R.INPUT_IDS)
def test_sums_loss_gradient(case):
    """every COMBOS entry on one input, the map built on the device; per combination also: the CE sums are ops.loss_fwd's bits,
    and a second call gives the same bits"""
    from iswm_amd import ops
    shape, kind, scale = case
    logits, labels, weight, sd2, classes = R.case(shape, kind, R.SCALES[scale])
    worst, d = {}, dev()
    ce_sums = {}
    for wt_on in (False, True):
        w = weight.to(d) if wt_on else None
        ce_sums[wt_on] = ops.loss_fwd(logits.to(d), labels.to(d), w, R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1].clone()
    for combo in R.COMBOS:
        wt, lce, lbd, clip = R.combo_args(combo, weight)
        ref = R.reference(shape, kind, R.SCALES[scale], combo)
        what = R.combo_id(combo)
        got = run(logits, labels, wt, R.IGNORE, lce, lbd, clip, classes)
        assert torch.equal(got[3].cpu(), sd2), "the map differs from the definition"
        n_invalid = check(R.group(shape, scale), got, ref, what, worst, labels)
        assert n_invalid >= (4 if labels.numel() >= 8 else 0)
        assert torch.equal(bits(got[0][:2].float()), bits(ce_sums[combo[0]])), "CE sums differ from iswm_loss_fwd's (%s)" % what
        again = run(logits, labels, wt, R.IGNORE, lce, lbd, clip, classes)
        assert all(torch.equal(bits(a), bits(b)) for a, b in zip(got, again)), "two calls differ (%s)" % what
    for k in sorted(worst):
        emit(worst[k][1] + "  (largest of %d combinations)" % len(R.COMBOS))


@pytest.mark.parametrize("name", list(R.BIG))
def test_many_blocks(name):
    """cap: 1 x 2897 x 2897 = 8 392 609 pixels > 8192 blocks x 256 threads x 4: a second trip through the grid-stride loop, ragged.
    fin: 1037 blocks: the finalize kernel adds one 16-deep batch of partials in every lane, then a tail in 13 lanes.  The map is
    scipy's; on fin the device's map is held against it as well."""
    from iswm_amd import _lib, ops
    logits, labels, weight, sd2, classes = R.case(name, "u8", 1.0)
    npix, d = labels.numel(), dev()
    blocks = _lib.load().iswm_loss_blocks(npix)
    assert _lib.load().iswm_boundary_loss_partials(npix) == 4 * blocks
    if name == "cap":
        assert blocks == 8192 and 8192 * 1024 < npix < 2 * 8192 * 1024 and npix % 1024 != 0
    else:
        assert 16 * 64 < blocks < 17 * 64
        assert torch.equal(ops.signed_edt(labels.to(d), 2).cpu(), sd2)
    worst = {}
    wt, lce, lbd, clip = R.combo_args(R.BIG_COMBO, weight)
    ref = R.reference(name, "u8", 1.0, R.BIG_COMBO)
    got = run(logits, labels, wt, R.IGNORE, lce, lbd, clip, classes, sd2=sd2)
    check(name, got, ref, R.combo_id(R.BIG_COMBO), worst, labels)
    ce = ops.loss_fwd(logits.to(d), labels.to(d), wt.to(d), R.IGNORE, 1.0, 0.0, ops.MODE_WCE)[1]
    assert torch.equal(bits(got[0][:2].float()), bits(ce))
    for k in sorted(worst):
        emit(worst[k][1])


@pytest.mark.parametrize("pattern", R.DEGENERATE)
@pytest.mark.parametrize("kind", ["u8", "i64"])
def test_degenerate_label_patterns(pattern, kind):
    logits, labels, weight, sd2, classes = R.degenerate_case(pattern, kind)
    worst = {}
    for combo in R.degenerate_combos(pattern):
        wt, lce, lbd, clip = R.combo_args(combo, weight)
        ref = R.degenerate_reference(pattern, combo, kind)
        sums, out, grad, m = run(logits, labels, wt, R.IGNORE, lce, lbd, clip, classes)
        assert not bool(m.any()), "a plane without foreground or without background has a distance"
        assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(grad).all()), R.combo_id(combo)
        assert float(sums[2]) == 0.0 and float(out[2]) == 0.0
        if pattern == "all_ignored":
            assert float(out[0]) == 0.0 and not bool(grad.any()) and not bool(sums.any()), R.combo_id(combo)
        else:
            check("degen", (sums, out, grad), ref, R.combo_id(combo), worst, labels)
            if lce == 0:
                assert float(out[0]) == 0.0 and not bool(grad.any())
    for k in sorted(worst):
        emit(worst[k][1] + "  (%s)" % pattern)


def test_ignore_index_inside_the_class_range():
    """three classes with ignore_index 2: pixels labelled 2 are in neither set of the map, no part of N or of the boundary sum and
    get a zero gradient; the plane of class 2 is 0 (the inputs the mutants of test_boundary_cpu.py are shown on)"""
    logits, labels, weight, sd2, classes = R.case(R.IG2_SHAPE, "u8", 1.0, R.IG2_IGNORE, R.IG2_PATTERNS)
    worst = {}
    for combo in R.IG2_COMBOS:
        ref = R.reference(R.IG2_SHAPE, "u8", 1.0, combo, R.IG2_IGNORE, R.IG2_PATTERNS)
        got = run(logits, labels, weight, R.IG2_IGNORE, combo[1], combo[2], combo[3], classes)
        assert torch.equal(got[3].cpu(), sd2) and not bool(got[3][:, 1].any())
        assert check("ig2", got, ref, R.combo_id(combo), worst, labels, R.IG2_IGNORE) > 20
    for k in sorted(worst):
        emit(worst[k][1])


def test_module_end_to_end():
    """BoundaryLoss through autograd: the ops calls' loss and gradient, bit for bit, and the restatement's within 4 x FLOOR; an
    upstream factor scales it; boundary_weight set between calls is the next call's factor; a second backward through the same
    call is refused; last_terms and last_valid"""
    from iswm_amd.network._hip import CONSUMED
    from iswm_amd.utils.loss import BoundaryLoss
    logits, labels, weight, sd2, classes = R.case("img", "u8", 1.0)
    d = dev()
    crit = BoundaryLoss(ce_weight=1.0, boundary_weight=5.0, clip=8.0, weight=weight).to(d)
    crit.boundary_weight = 2.0                                          # as the trainer's ramp sets it
    z = logits.to(d).requires_grad_(True)
    loss = crit(z, labels.to(d))
    terms, nvalid = crit.last_terms, crit.last_valid
    loss.backward(retain_graph=True)
    combo = (True, 1.0, 2.0, 8.0)
    sums, want, want_grad, _ = run(logits, labels, weight, R.IGNORE, 1.0, 2.0, 8.0, classes)
    assert loss.shape == () and torch.equal(bits(loss.detach().reshape(1)), bits(want[:1])) and torch.equal(bits(z.grad), bits(want_grad))
    with pytest.raises(RuntimeError, match=re.escape(CONSUMED)):
        loss.backward()
    ref = R.reference("img", "u8", 1.0, combo)
    worst = {}
    check("img_s1", (sums, want, z.grad), ref, "module", worst, labels)
    assert torch.equal(bits(terms), bits(want[1:]))
    assert float(nvalid) == float(ref["sums"][3]) and nvalid.dim() == 0
    z2 = logits.to(d).requires_grad_(True)
    (crit(z2, labels.to(d).long()) * 0.37).backward()                   # int64 labels, upstream 0.37
    scaled = run(logits, labels.long(), weight, R.IGNORE, 1.0, 2.0, 8.0, classes, upstream=0.37)[2]
    assert torch.equal(bits(z2.grad), bits(scaled))
    err = R.rel_err(z2.grad.cpu(), ref["grad"] * float(torch.tensor(0.37, dtype=torch.float32)))
    emit("module upstream 0.37: gradient rel err %.2e (bound %.1e)" % (err, 4 * R.FLOOR["grad.img_s1"]))
    assert err <= 4 * R.FLOOR["grad.img_s1"]
    crit.boundary_weight = float("nan")
    with pytest.raises(ValueError, match="boundary_weight"):
        crit(z2.detach(), labels.to(d))


def test_more_than_eight_classes_and_another_map_shape_are_refused():
    from iswm_amd import ops
    from iswm_amd.utils.loss import BoundaryLoss
    d = dev()
    y = torch.zeros(1, 4, 4, dtype=torch.int64, device=d)
    with pytest.raises(ValueError, match="at most 8 classes"):
        BoundaryLoss()(torch.zeros(1, 9, 4, 4, device=d), y)
    z = torch.zeros(1, 2, 4, 4, device=d)
    m = ops.signed_edt(y, 2)
    for bad in (torch.zeros(1, 2, 4, 4, dtype=torch.int32, device=d), torch.zeros(1, 1, 4, 5, dtype=torch.int32, device=d),
                torch.zeros(2, 1, 4, 4, dtype=torch.int32, device=d)):
        with pytest.raises(ValueError, match="shape"):                  # before any launch
            ops.boundary_loss_fwd(z, y, bad, None, 255)
        with pytest.raises(ValueError, match="shape"):
            ops.boundary_loss_bwd(z, y, bad, None, 255, torch.zeros(2, device=d), torch.ones(1, device=d))
    assert ops.boundary_loss_fwd(z, y, torch.zeros(1, 2, 4, 4, dtype=torch.int32, device=d), None, 255, "all").shape == (4,)
    with pytest.raises(ValueError, match="int32"):
        ops.boundary_loss_fwd(z, y, m.float(), None, 255)
    with pytest.raises(ValueError, match="int32"):
        ops.boundary_loss_fwd(z, y, m.cpu(), None, 255)
    for clip in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="clip"):
            ops.boundary_loss_fwd(z, y, m, None, 255, "foreground", clip)
    torch.cuda.synchronize()


COMMON = ["--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16", "--optimizer", "sgd", "--loss_type", "IWce_loss",
          "--print_interval", "1", "--val_interval", "4", "--val_batch_size", "4", "--num_workers", "0"]


def test_train_main_with_the_boundary_term(tmp_path, capsys):
    """the small synthetic configuration of tests/test_train_entry.py on a MobileNetV2 DeepLab for 4 iterations with
    --boundary_weight 0.01 ramped over 2: finite losses, bd= in every printed line, and the factor 0.005, 0.01, 0.01, 0.01"""
    from iswm_amd import train
    dev()
    train.main(["--model", "deeplabv3plus_mobilenet", "--checkpoints_dir", str(tmp_path / "ck"), "--total_itrs", "4",
                "--boundary_weight", "0.01", "--boundary_ramp_itrs", "2", "--boundary_clip", "20"] + COMMON)
    out = capsys.readouterr().out
    assert "Itrs 4/4" in out and "Validation @4" in out and "Boundary term: CE x 1 + BD x 0.01" in out
    losses = [float(v) for v in re.findall(r"Loss[=: ]+([-+0-9.eE]+|nan|inf)", out)]
    bds = [float(v) for v in re.findall(r", bd=([-+0-9.eE]+|nan|inf)", out)]
    factors = [float(v) for v in re.findall(r"lbd=([-+0-9.eE]+|nan|inf)", out)]
    assert len(losses) >= 4 and all(math.isfinite(v) for v in losses), out[-2000:]
    assert len(bds) == 4 and all(math.isfinite(v) for v in bds) and any(v != 0.0 for v in bds), out[-2000:]
    assert factors == [0.005, 0.01, 0.01, 0.01], out[-2000:]
