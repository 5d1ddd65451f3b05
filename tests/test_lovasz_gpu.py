"""The Lovasz-Softmax kernels of csrc/lovasz.hip against the float64 restatement of tests/lovasz_ref.py, stage by stage so that
no check leans on another:

  keys     the decoded e within 4 x FLOOR (absolute: e <= 1) of the float64 error; g, validity, the per-image counts and G_bc
           exact; the CE sums iswm_loss_fwd's mode-0 bits
  sort     sorted keys and perm equal, bit for bit, to numpy's stable descending argsort of the kernel's OWN keys: hand-made keys
           spanning every digit, tie groups of thousands, all keys identical, one valid pixel, none; lengths around the tile
           size, above 256 tiles and one 2897 x 2897 image; 1, 3 and 14 segments
  order    along the kernel's perm the float64 errors never increase by more than the fp32 rounding band of e: two errors of at
           most 4 x FLOOR["e"] each, 8 x FLOOR["e"]
  weights  with the kernel's own sorted keys, omega_j (read back through m at perm[j]) within 4 x FLOOR per element (relative)
           of the float64 closed form; m exactly 0 at invalid pixels and in absent segments
  loss     against float64 on the restatement's own order (the loss is 1-Lipschitz in max |de|: the order need not be pinned)
  grad     against float64 evaluated WITH the kernel's perm -- one order, no circular check; exactly 0 at invalid pixels
  module   LovaszSoftmaxLoss through autograd: both label widths, C = 2, 3, 8, class weights on and off, l_ce in {0, 1}, both
           class sets, upstream != 1, two calls giving the same bits; then the trainer with the new option.

With ISWM_TEST_REPORT=<file> every check appends its floor, bound and measured error to that file."""
import os

import numpy as np
import pytest
import torch

from tests import lovasz_ref as R

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


def bound(name, check, group, err):
    floor = R.FLOOR[R.floor_key(check, group)]
    emit("%-34s %-6s floor %.1e bound %.1e measured %.2e" % (name, check, floor, 4 * floor, err))
    assert err <= 4 * floor, (name, check, err, 4 * floor)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def u32(t):
    """an int32 device tensor of uint32 values -> int64 numpy"""
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def decode(keys):
    """uint32 keys (int64 numpy) -> (e float32, g bool, valid bool)"""
    valid = keys != 0
    k = np.where(valid, keys - 1, 0)
    return (k >> 1).astype(np.uint32).view(np.float32), (k & 1).astype(bool) & valid, valid


def to_dev(logits, labels, weight):
    d = dev()
    return logits.to(d), labels.to(d), None if weight is None else weight.to(d)


def check_sort(name, keys64):
    """keys64: int64 [nseg, P] of uint32 values; the kernel's result against numpy's stable descending argsort"""
    from iswm_amd import ops
    k = torch.from_numpy((keys64 & 0xFFFFFFFF).astype(np.uint32).view(np.int32)).to(dev()).contiguous()
    got_s, got_p = ops.lovasz_sort(k)
    again_s, again_p = ops.lovasz_sort(k)
    want_s, want_p = R.sort_reference(keys64)
    gs, gp = u32(got_s), u32(got_p)
    assert np.array_equal(gs, want_s), name
    assert np.array_equal(gp, want_p), name
    assert torch.equal(got_s, again_s) and torch.equal(got_p, again_p), name
    emit("%-34s sort   %d x %d keys equal to numpy's stable descending argsort, twice" % (name, keys64.shape[0], keys64.shape[1]))


def sort_lengths():
    from iswm_amd import _lib
    t = _lib.load().iswm_lovasz_tile()
    return t, [1, 2, t - 1, t, t + 1, 3 * t + 5]


@pytest.mark.parametrize("nseg", [1, 3, 14])
def test_sort_hand_made_keys_at_the_tile_edges(nseg):
    from iswm_amd import _lib
    assert _lib.load().iswm_lovasz_digits() * 8 == 32
    t, lengths = sort_lengths()
    for p in lengths:
        keys = np.stack([R.span_keys(p, seed=57 + 3 * s + p % 11).numpy() for s in range(nseg)])
        check_sort("span_P%d_nseg%d" % (p, nseg), keys)


def test_sort_above_256_tiles_and_one_large_image():
    t, _ = sort_lengths()
    check_sort("span_257_tiles", np.stack([R.span_keys(256 * t + 77, seed=91 + s).numpy() for s in range(2)]))
    check_sort("span_2897x2897", R.span_keys(2897 * 2897, seed=93).numpy()[None])


@pytest.mark.parametrize("pattern", ["four", "same", "one", "none"])
def test_sort_of_the_kernels_own_keys_on_tie_inputs(pattern):
    from iswm_amd import ops
    logits, labels = R.tie_inputs(pattern)
    lg, lb, _ = to_dev(logits, labels, None)
    for classes in R.CLASSES:
        keys, counts, _ = ops.lovasz_keys(lg, lb, None, R.IGNORE, classes)
        kn = u32(keys)
        nv = int(R.valid_mask(labels, 2).reshape(2, -1).sum(1).max())
        assert int(counts[:, 0].max()) == nv
        if pattern in ("four", "same") and classes == "foreground":
            _, cnt = np.unique(kn[0], return_counts=True)
            assert cnt.max() >= 1000                            # tie groups of thousands
        check_sort("tie_%s_%s" % (pattern, classes), kn)


CASES = [(g, i) for g in R.SHAPES for i in range(len(R.group_cases(g)))]


@pytest.mark.parametrize("group,index", CASES, ids=["%s-%s" % (g, R.group_cases(g)[i][0]) for g, i in CASES])
def test_stages_against_float64(group, index):
    from iswm_amd import ops
    tag, logits, labels, wt, ig, classes, lce, llv, up = R.group_cases(group)[index]
    name = "%s_%s" % (group, tag)
    ref = R.group_reference(group, index)
    lg, lb, w = to_dev(logits, labels, wt)
    b, c = logits.shape[:2]
    ns = c - R.first_class(classes)

    # keys
    keys, counts, sums = ops.lovasz_keys(lg, lb, w, ig, classes)
    e, g, valid = decode(u32(keys).reshape(b, ns, -1))
    v = ref["valid"][:, None, :].expand_as(ref["e"]).contiguous().numpy()
    assert np.array_equal(valid, v) and np.array_equal(g, ref["g"].numpy() & v), name
    bound(name, "e", group, R.abs_err(torch.from_numpy(e)[torch.from_numpy(v)], ref["e"][torch.from_numpy(v)]))
    cn = counts.cpu().reshape(b, ns, 2)
    assert torch.equal(cn[..., 0].long(), ref["valid"].sum(1)[:, None].expand(b, ns)), name
    assert torch.equal(cn[..., 1].long(), ref["G"]), name
    _, fsums, _ = ops.loss_fwd(lg, lb, w, ig, 1.0, 0.0, ops.MODE_WCE)
    assert torch.equal(bits(sums[:2].float()), bits(fsums)), name

    # sort of the kernel's own keys, then the order against float64
    skeys, perm = ops.lovasz_sort(keys)
    want_s, want_p = R.sort_reference(u32(keys))
    assert np.array_equal(u32(skeys), want_s) and np.array_equal(u32(perm), want_p), name
    pl = torch.from_numpy(u32(perm)).reshape(b, ns, -1)
    e64 = ref["e"].gather(-1, pl)
    nv = ref["valid"].sum(1)
    band = 8 * R.FLOOR[R.floor_key("e", group)]
    rise = 0.0
    for bi in range(b):
        if int(nv[bi]) > 1:
            d = e64[bi, :, 1:int(nv[bi])] - e64[bi, :, :int(nv[bi]) - 1]
            rise = max(rise, float(d.max()))
        assert bool(ref["valid"][bi][pl[bi, :, :int(nv[bi])]].all()), name      # the valid pixels take the first |V_b| positions
    emit("%-34s order  band %.1e largest rise of the float64 error along the kernel's perm %.2e" % (name, band, rise))
    assert rise <= band, (name, rise)

    # weights, with the kernel's own order
    m, sums = ops.lovasz_weights(skeys, perm, counts, sums)
    pin = R.lovasz_ref(logits, labels, wt, ig, classes, lce, llv, upstream=up, perm=pl)
    mk = m.cpu().reshape(b, ns, -1)
    bound(name, "omega", group, R.elem_rel_err(mk.gather(-1, pl), pin["omega"]))
    assert not bool(mk[~torch.from_numpy(v)].any()) and not bool(mk[~pin["present"]].any()), name
    assert int(sums[3].item()) == ref["N"] == pin["N"], name

    # loss on the restatement's own order; gradient with the kernel's
    out = ops.lovasz_loss(sums, lce, llv)
    bound(name, "loss", group, R.rel_err(out[0], ref["loss"]))
    upt = torch.tensor([up], dtype=torch.float32, device=dev())
    grad = ops.lovasz_bwd(lg, lb, w, ig, classes, m, out, upt).cpu()
    bound(name, "grad", group, R.rel_err(grad, pin["grad"]))
    assert not bool(grad.permute(0, 2, 3, 1)[~ref["valid"].reshape(labels.shape)].any()), name


@pytest.mark.parametrize("group", [g for g in R.SHAPES if g not in R.BIG])
def test_module_through_autograd(group):
    from iswm_amd.utils.loss import LovaszSoftmaxLoss
    for index, (tag, logits, labels, wt, ig, classes, lce, llv, up) in enumerate(R.group_cases(group)):
        name = "module_%s_%s" % (group, tag)
        crit = LovaszSoftmaxLoss(classes=classes, ce_weight=lce, lovasz_weight=llv, weight=wt, ignore_index=ig).to(dev())
        runs = []
        for _ in range(2):
            z = logits.to(dev()).requires_grad_(True)
            loss = crit(z, labels.to(dev()))
            (loss * up).backward()
            runs.append((loss.detach(), z.grad, int(crit.last_present)))
        assert torch.equal(bits(runs[0][0]), bits(runs[1][0])) and torch.equal(bits(runs[0][1]), bits(runs[1][1])), name
        ref = R.group_reference(group, index)
        assert runs[0][2] == ref["N"], name
        bound(name, "loss", group, R.rel_err(runs[0][0], ref["loss"]))
        # the gradient against float64 on the order the kernels chose: take it from the stages
        from iswm_amd import ops
        keys, _, _ = ops.lovasz_keys(logits.to(dev()), labels.to(dev()), None, ig, classes)
        perm = torch.from_numpy(u32(ops.lovasz_sort(keys)[1])).reshape(logits.shape[0], -1, keys.shape[1])
        pin = R.lovasz_ref(logits, labels, wt, ig, classes, lce, llv, upstream=up, perm=perm)
        bound(name, "grad", group, R.rel_err(runs[0][1].cpu(), pin["grad"]))


def test_degenerate_batches_on_the_device():
    """no valid pixel and no present segment: loss 0, gradient exactly 0, N = 0; an ignore_index inside [0, C)"""
    from iswm_amd.utils.loss import LovaszSoftmaxLoss
    logits, labels, _ = R.inputs("odd", "u8")
    for lab in (torch.full_like(labels, R.IGNORE), torch.zeros_like(labels)):
        z = logits.to(dev()).requires_grad_(True)
        crit = LovaszSoftmaxLoss()
        loss = crit(z, lab.to(dev()))
        loss.backward()
        assert float(loss.detach()) == 0.0 and not bool(z.grad.any()) and int(crit.last_present) == 0
    lg, lb = R.ig2_inputs()
    ref = R.lovasz_ref(lg, lb, None, R.IG2_IGNORE, "all", 1.0, 1.0)
    z = lg.to(dev()).requires_grad_(True)
    crit = LovaszSoftmaxLoss(classes="all", ce_weight=1.0, ignore_index=R.IG2_IGNORE)
    loss = crit(z, lb.to(dev()))
    loss.backward()
    assert int(crit.last_present) == ref["N"] == 4                      # class 2 is the ignored label: never present
    assert R.rel_err(loss, ref["loss"]) <= 4 * R.FLOOR["loss.c3"]
    assert not bool(z.grad.cpu().permute(0, 2, 3, 1)[lb == R.IG2_IGNORE].any())


def test_more_than_eight_classes_is_refused():
    from iswm_amd.utils.loss import LovaszSoftmaxLoss
    d = dev()
    with pytest.raises(ValueError, match="at most 8 classes"):
        LovaszSoftmaxLoss()(torch.zeros(1, 9, 4, 4, device=d), torch.zeros(1, 4, 4, dtype=torch.int64, device=d))


def test_train_main_with_the_lovasz_term(tmp_path, capsys):
    """the small synthetic configuration of tests/test_train_entry.py with --lovasz_weight 1 --ce_weight 1: three iterations
    run, the printed losses are finite and every printed N lies between 0 and the batch's image count (one foreground class)"""
    import glob
    import math
    import re
    from iswm_amd import train
    dev()
    ck = str(tmp_path / "ck")
    common = ["--model", "deeplabv3plus_resnet50", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
              "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "1", "--val_interval", "3",
              "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0", "--total_itrs", "3"]
    train.main(common + ["--lovasz_weight", "1", "--ce_weight", "1"])
    out = capsys.readouterr().out
    assert "Itrs 3/3" in out and "Validation @3" in out
    losses = [float(v) for v in re.findall(r"Loss[=: ]+([-+0-9.eE]+|nan|inf)", out)]
    present = [int(v) for v in re.findall(r"present=(\d+)", out)]
    assert len(losses) == 3 and all(math.isfinite(v) and v > 0 for v in losses), out[-2000:]
    assert len(present) == 3 and all(0 <= v <= 4 for v in present) and max(present) >= 1, present
    assert len(glob.glob(os.path.join(ck, "best_*.pth"))) == 1
    for bad in (["--lovasz_weight", "1", "--overlap_loss", "dice"], ["--lovasz_weight", "-1"]):
        with pytest.raises(SystemExit):
            train.main(common + bad)
