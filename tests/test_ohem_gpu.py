"""The hard-pixel mining kernels of csrc/loss.hip against the float64 restatement of tests/ohem_ref.py, stage by stage so that no
check leans on another:

  keys    every valid key within 4 x FLOOR of the float64 nll, -1 at every invalid pixel, |V| exact, no negative-zero key
  select  nu equal, bit for bit, to the order statistic of the kernel's OWN keys as numpy.sort gives it, for every rank and
          threshold, on tie-heavy inputs, on keys spanning every digit, with one and with no valid pixel; |K| = count(keys >= nu)
  sums    the kept mask taken from the pinned keys and nu agrees with nll64 >= nu outside the band of tests/ohem_ref.py; loss,
          sums and gradient then match float64 ON THAT MASK within 4 x FLOOR; the gradient is exactly 0 off it; with thresh = 1
          the first two sums are ops.loss_fwd's mode-0 bits
  shapes  the edge shapes with both label widths; then the module through autograd and the trainer with the new options.

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import glob
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import ohem_ref as R

pytestmark = pytest.mark.gpu
CHECKS = ("keys", "sums", "loss", "grad")


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


def f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def expected_nu_bits(keys, k, thresh):
    """min(bits(nu_0), the min(k, |V|)-th largest valid key) by numpy.sort -- non-negative floats order as their int32 bits"""
    v = np.sort(keys[keys >= 0])
    kk = min(k, v.size)
    nu0 = int(np.float32(R.nu0_of(thresh)).view(np.int32))
    return nu0 if kk == 0 else min(nu0, int(v[v.size - kk]))


def select_and_count(keys, nvalid, labels, k, thresh):
    """-> (bits of nu, |K| from the sums pass, sums) for keys already on the device"""
    from iswm_amd import ops
    nu = ops.ohem_select(keys, nvalid, k, thresh)
    sums = ops.ohem_sums(keys, labels, None, nu)
    return int(bits(nu)[0]), sums, nu


def check_select(name, keys, nvalid, labels):
    """every rank x threshold on one set of device keys"""
    kn = keys.cpu().numpy().reshape(-1)
    nv = int((kn >= 0).sum())
    assert int(nvalid.cpu()[0]) == nv
    ranks = sorted({max(r, 0) for r in (0, 1, 2, nv // 3, nv - 1, nv, nv + 5)})
    small = 0.999 if nv == 0 else min(0.999, math.exp(-0.5 * float(np.sort(kn[kn >= 0])[0:1].view(np.float32)[0])))
    n = 0
    for thresh in (1.0, 0.7, small):            # `small`: nu_0 at or below half the smallest key: nu_0 decides at every rank
        for k in ranks:
            want = expected_nu_bits(kn, k, thresh)
            got, sums, nu = select_and_count(keys, nvalid, labels, k, thresh)
            assert got == want, "%s: k %d thresh %g: nu bits %#x, numpy.sort says %#x" % (name, k, thresh, got, want)
            kept = int(((kn >= 0) & (kn >= want)).sum())
            assert float(sums.cpu()[2]) == kept >= min(k, nv), (name, k, thresh)
            again, sums2, _ = select_and_count(keys, nvalid, labels, k, thresh)
            assert again == got and torch.equal(bits(sums), bits(sums2)), "two calls differ"
            n += 1
    emit("select %-10s |V| %-7d %d rank x threshold cases: nu = numpy.sort's order statistic bit for bit, |K| = count(keys >= nu)"
         % (name, nv, n))


@pytest.mark.parametrize("pattern", ["four", "same", "one", "none"])
def test_select_exact_on_ties(pattern):
    from iswm_amd import ops
    logits, labels = R.tie_inputs(pattern)
    d = dev()
    lb = labels.to(d)
    keys, nvalid = ops.ohem_keys(logits.to(d), lb, R.IGNORE)
    kn = keys.cpu().numpy().reshape(-1)
    distinct = np.unique(kn[kn >= 0]).size
    assert distinct <= 16 and (pattern != "same" or distinct == 1)
    if pattern == "four":                       # every rank from |V| / 3 on falls inside a tie group of thousands
        assert np.bincount(np.unique(kn[kn >= 0], return_inverse=True)[1]).min() >= 1000
    check_select(pattern, keys, nvalid, lb)


def test_select_exact_on_keys_spanning_every_digit():
    """the kernel's keys of logit gaps from -80 to 69 (fp32 rounds the nll to 0 once the lead passes 17), then keys made by hand
    from 1e-30 to 80 with zeros, denormals, +inf and tie runs: every bit of the three digits takes both values"""
    from iswm_amd import ops
    d = dev()
    logits, labels = R.span_inputs()
    lb = labels.to(d)
    keys, nvalid = ops.ohem_keys(logits.to(d), lb, R.IGNORE)
    kf = keys.cpu().view(torch.float32)[keys.cpu() >= 0]
    assert float(kf.max()) > 75 and float(kf[kf > 0].min()) < 1e-6 and int((kf == 0).sum()) > 100
    check_select("gaps", keys, nvalid, lb)
    hand = R.span_keys()
    spread = np.bitwise_or.reduce(hand.numpy()[hand.numpy() >= 0]) & ~np.bitwise_and.reduce(hand.numpy()[hand.numpy() >= 0])
    assert spread == 0x7FFFFFFF                 # all 31 bits vary
    hk = hand.to(d)
    nv = torch.tensor([int((hand >= 0).sum())], dtype=torch.int64, device=d)
    check_select("by hand", hk, nv, torch.zeros(hand.shape, dtype=torch.uint8, device=d))


def test_keys_have_no_negative_zero():
    """the true class wins by 40 or more: -log_softmax is -0.0 there, whose bit pattern would sort above every other key"""
    from iswm_amd import ops
    d = dev()
    g = R.gen(58)
    labels = torch.randint(0, 2, (2, 33, 37), generator=g)
    lead = 40.0 + 40.0 * torch.rand(2, 33, 37, generator=g)
    for scale, kind in ((1.0, torch.uint8), (0.1, torch.int64)):               # leads of 40-80 (|m| >= 8) and, scaled, of 4-8 (|m| < 8)
        logits = torch.zeros(2, 2, 33, 37).scatter_(1, labels[:, None], (lead * scale)[:, None])
        if scale == 1.0:
            logits = logits - 20.0
        keys, nvalid = ops.ohem_keys(logits.to(d), labels.to(kind).to(d), R.IGNORE)
        kn = keys.cpu().numpy()
        assert int(nvalid.cpu()[0]) == kn.size and (kn >= 0).all(), "a key has its sign bit set"
        if scale == 1.0:
            assert (kn == 0).all()
    emit("keys: no negative zero among %d saturated pixels" % kn.size)


def run_case(group, case, worst, band_max):
    """one case of tests/ohem_ref.group_cases through the six stages, each checked on its own (module docstring)"""
    from iswm_amd import ops
    tag, logits, labels, wt, ig, th, k, up = case
    d = dev()
    lg, lb, w = logits.to(d), labels.to(d), None if wt is None else wt.to(d)
    keys, nvalid = ops.ohem_keys(lg, lb, ig)
    nu = ops.ohem_select(keys, nvalid, k, th)
    sums = ops.ohem_sums(keys, lb, w, nu)
    out = ops.ohem_loss(sums)
    grad = ops.ohem_bwd(lg, lb, w, keys, nu, out, torch.tensor([up], dtype=torch.float32, device=d))
    terms = R.pixel_terms(logits, labels, ig)
    valid, nll64 = terms[2].reshape(labels.shape), terms[3].reshape(labels.shape)
    kc = keys.cpu()
    got = {}
    # keys
    assert torch.equal(kc >= 0, valid) and bool((kc[~valid] == R.SENTINEL).all()) and int(nvalid.cpu()[0]) == int(valid.sum())
    kf = kc.view(torch.float32)
    got["keys"] = R.rel_err(kf[valid], nll64[valid])
    # select
    nub = int(bits(nu)[0])
    assert nub == expected_nu_bits(kc.numpy().reshape(-1), k, th), "%s %s: nu is not the order statistic of the keys" % (group, tag)
    nuf = float(nu.cpu()[0])
    # the kept set, pinned by the kernel's keys and nu
    mask = valid & (kc >= nub)
    assert torch.equal(mask, valid & (kf >= nuf))
    sc = sums.cpu()
    assert float(sc[2]) == int(mask.sum()) >= min(k, int(valid.sum()))
    band = R.band_count(nll64, valid, nuf)
    assert torch.equal(mask | band, (valid & (nll64 >= nuf)) | band), "%s %s: kept set differs outside the band" % (group, tag)
    nband = int(band.sum())
    assert band_max is None or nband <= band_max, "%s %s: %d pixels in the band" % (group, tag, nband)
    # sums, loss, gradient on that mask
    ref = R.ohem_ref(logits, labels, wt, ig, th, k, upstream=f32(up), kept=mask, terms=terms)
    got["sums"] = R.rel_err(sc[:2], ref["sums"][:2])
    got["loss"] = R.rel_err(out.cpu()[0], ref["loss"])
    got["grad"] = R.rel_err(grad.cpu(), ref["grad"])
    gc = grad.cpu().permute(0, 2, 3, 1)
    assert not bool(gc[~mask].any()), "gradient outside the kept set is not exactly 0"
    assert int(mask.sum()) == 0 or bool(gc[mask].any())
    for check in CHECKS:
        key = R.floor_key(check, group)
        floor = R.FLOOR[key]
        line = "%-12s floor %.1e  bound %.1e  measured %.2e  %s (|K| %d of %d valid, %d in the band)" % (
            key, floor, 4 * floor, got[check], tag, int(mask.sum()), int(valid.sum()), nband)
        if got[check] >= worst.get(key, (-1.0, ""))[0]:
            worst[key] = (got[check], line)
        assert got[check] <= 4 * floor, line
    # thresh = 1: the weighted CE's own sums, bit for bit
    nu1 = ops.ohem_select(keys, nvalid, k, 1.0)
    s1 = ops.ohem_sums(keys, lb, w, nu1)
    ce = ops.loss_fwd(lg, lb, w, ig, 1.0, 0.0, ops.MODE_WCE)[1]
    assert int(bits(nu1)[0]) == 0 and torch.equal(bits(s1[:2].float()), bits(ce)), "%s %s: sums at thresh 1 differ from loss_fwd's" % (group, tag)
    assert float(s1.cpu()[2]) == int(valid.sum())
    return mask


def run_group(group, kind, band_max=R.BAND_MAX):
    worst, n = {}, 0
    for case in R.group_cases(group):
        if kind is None or case[0].startswith(kind + "_"):
            run_case(group, case, worst, band_max)
            n += 1
    assert n > 0
    for key in sorted(worst):
        emit(worst[key][1] + "  (largest of %d cases%s)" % (n, "" if kind is None else ", " + kind))


@pytest.mark.parametrize("name,kind", R.RANDOM_CASES, ids=["%s_%s" % c for c in R.RANDOM_CASES])
def test_random_inputs(name, kind):
    """k in {1, |V| / 10, |V| / 3} x thresh in {0.7, 1} x with and without class weights; at most BAND_MAX pixels in the band"""
    run_group(name, kind)


@pytest.mark.parametrize("name,kind", R.SHAPE_CASES, ids=["%s_%s" % c for c in R.SHAPE_CASES])
def test_edge_shapes(name, kind):
    """one pixel, ragged blocks, image boundaries inside a thread's pixels, 3 and 8 classes, 1037 blocks, the grid-stride loop's
    second trip.  fin and cap hold millions of pixels: their band necessarily holds more than BAND_MAX (pixels x band width x
    density of the nll at nu), so only the agreement outside it is asked of them."""
    from iswm_amd import _lib
    npix = R.SHAPES[name][0] * R.SHAPES[name][2] * R.SHAPES[name][3]
    blocks = _lib.load().iswm_loss_blocks(npix)
    if name == "cap":
        assert blocks == 8192 and 8192 * 1024 < npix < 2 * 8192 * 1024 and npix % 1024 != 0
    if name == "fin":
        assert 16 * 64 < blocks < 17 * 64
    if name == "odd":
        assert npix % 4 and npix % 256 and npix % 1024 and blocks == 2
    run_group(name, kind, None if name in R.BIG else R.BAND_MAX)


@pytest.mark.parametrize("kind", ["u8", "i64"])
def test_ignore_index_inside_the_class_range(kind):
    """three classes with ignore_index 2: the pixels labelled 2 carry the sentinel, take no rank and get a zero gradient"""
    run_group("ig2", kind)
    _, labels, _ = R.inputs(R.IG2_SHAPE, kind, 1.0, R.IG2_IGNORE)
    assert int((labels == 2).sum()) > 50


@pytest.mark.parametrize("case", R.GAP_CASES, ids=["%s_%s_%s_%s" % (c[0], c[1], "w" if c[2] else "now", c[3]) for c in R.GAP_CASES])
def test_gap_inputs_keep_exactly_the_hard_population(case):
    """hard pixels with nll in [1, 3], easy ones below 0.1, k = the number of hard ones: the kept set is the hard population in any
    arithmetic, whether nu_0 (inside the gap) or the k-th largest loss decides; upstream 0.37"""
    idx = R.GAP_CASES.index(case)
    full = R.group_cases("gap")[idx]
    ref = R.group_reference("gap", idx)
    worst = {}
    mask = run_case("gap", full, worst, R.BAND_MAX)
    assert torch.equal(mask, ref["kept"]) and int(mask.sum()) == full[6] > 100
    for key in sorted(worst):
        emit(worst[key][1])


def test_nothing_valid_and_nothing_kept():
    from iswm_amd import ops
    d = dev()
    logits, labels, weight = R.inputs((2, 2, 13, 11), "u8", 1.0)
    up = torch.ones(1, device=d)
    for what, lb, k in (("no valid pixel", torch.full_like(labels, R.IGNORE), 100), ("nothing kept", torch.zeros_like(labels), 0)):
        lg = logits.to(d) if what == "no valid pixel" else torch.tensor([9.0, 0.0], device=d).view(1, 2, 1, 1).expand(2, 2, 13, 11).contiguous()
        keys, nvalid = ops.ohem_keys(lg, lb.to(d), R.IGNORE)
        nu = ops.ohem_select(keys, nvalid, k, 0.7)
        sums = ops.ohem_sums(keys, lb.to(d), weight.to(d), nu)
        out = ops.ohem_loss(sums)
        grad = ops.ohem_bwd(lg, lb.to(d), weight.to(d), keys, nu, out, up)
        assert int(bits(nu)[0]) == int(np.float32(R.nu0_of(0.7)).view(np.int32)), what
        assert not bool(sums.any()) and not bool(out.any()) and not bool(grad.any()), what
        assert bool(torch.isfinite(grad).all())
    emit("degenerate: no valid pixel and an empty kept set give loss 0 and a zero gradient")


def test_module_end_to_end():
    """OhemCrossEntropyLoss through autograd: the ops calls' loss and gradient bit for bit, last_kept, an upstream factor, int64
    labels; thresh = 1 is CrossEntropyLoss's loss to the fp32 floor"""
    from iswm_amd import ops
    from iswm_amd.utils.loss import CrossEntropyLoss, OhemCrossEntropyLoss
    logits, labels, weight = R.inputs(R.SHAPES["img"], "u8", 1.0)
    d = dev()
    nv = int(R.valid_mask(labels, 2).sum())
    crit = OhemCrossEntropyLoss(thresh=0.7, min_kept=500, weight=weight).to(d)
    z = logits.to(d).requires_grad_(True)
    loss = crit(z, labels.to(d))
    (loss * 0.37).backward()
    lg, lb, w = logits.to(d), labels.to(d), weight.to(d)
    keys, nvalid = ops.ohem_keys(lg, lb, R.IGNORE)
    nu = ops.ohem_select(keys, nvalid, 500, 0.7)
    sums = ops.ohem_sums(keys, lb, w, nu)
    out = ops.ohem_loss(sums)
    want = ops.ohem_bwd(lg, lb, w, keys, nu, out, torch.tensor([0.37], device=d))
    assert loss.shape == () and torch.equal(bits(loss.detach().reshape(1)), bits(out[:1])) and torch.equal(bits(z.grad), bits(want))
    assert crit.last_kept.shape == () and crit.last_kept.is_cuda and float(crit.last_kept) == float(sums[2]) >= min(500, nv)
    assert crit.last_nu.shape == () and crit.last_nu.is_cuda and torch.equal(bits(crit.last_nu.reshape(1)), bits(nu))
    z2 = logits.to(d).requires_grad_(True)
    crit(z2, labels.to(d).long()).backward()
    k64, _ = ops.ohem_keys(lg, lb.long(), R.IGNORE)
    assert torch.equal(k64, keys)
    assert torch.equal(bits(z2.grad), bits(ops.ohem_bwd(lg, lb.long(), w, keys, nu, out, torch.ones(1, device=d))))
    z3, z4 = logits.to(d).requires_grad_(True), logits.to(d).requires_grad_(True)
    a = OhemCrossEntropyLoss(thresh=1.0, min_kept=7, weight=weight).to(d)(z3, labels.to(d))
    b = CrossEntropyLoss(weight=weight).to(d)(z4, labels.to(d))
    a.backward()
    b.backward()
    e = (R.rel_err(a.cpu(), b.detach().cpu()), R.rel_err(z3.grad.cpu(), z4.grad.cpu()))
    emit("module: thresh 1 against CrossEntropyLoss: loss rel err %.1e, gradient %.1e (bound %.1e)" % (e[0], e[1], 4 * R.FLOOR["grad.img"]))
    assert e[0] <= 4 * R.FLOOR["loss.img"] and e[1] <= 4 * R.FLOOR["grad.img"]


def test_more_than_eight_classes_is_refused():
    from iswm_amd.utils.loss import OhemCrossEntropyLoss
    d = dev()
    with pytest.raises(ValueError, match="at most 8 classes"):
        OhemCrossEntropyLoss()(torch.zeros(1, 9, 4, 4, device=d), torch.zeros(1, 4, 4, dtype=torch.int64, device=d))


def test_train_main_with_hard_pixel_mining(tmp_path, capsys):
    """the small synthetic configuration of tests/test_train_entry.py with --ohem_thresh 0.7 --ohem_min_kept 500: three
    iterations run, the printed losses are finite and every printed kept count is at least min(500, pixels of the batch)"""
    from iswm_amd import train
    dev()
    ck = str(tmp_path / "ck")
    common = ["--model", "deeplabv3plus_resnet50", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
              "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "1", "--val_interval", "3",
              "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0", "--total_itrs", "3"]
    train.main(common + ["--ohem_thresh", "0.7", "--ohem_min_kept", "500"])
    out = capsys.readouterr().out
    assert "Itrs 3/3" in out and "Validation @3" in out
    losses = [float(v) for v in re.findall(r"Loss[=: ]+([-+0-9.eE]+|nan|inf)", out)]
    kept = [int(v) for v in re.findall(r"kept=(\d+) \(", out)]
    assert len(losses) == 3 and all(math.isfinite(v) and v > 0 for v in losses), out[-2000:]
    assert len(kept) == 3 and all(500 <= v <= 4 * 65 * 65 for v in kept), kept
    assert len(glob.glob(os.path.join(ck, "best_*.pth"))) == 1
    for bad in (["--ohem_thresh", "0.7", "--overlap_loss", "dice"], ["--ohem_thresh", "2"]):
        with pytest.raises(SystemExit):
            train.main(common + bad)
