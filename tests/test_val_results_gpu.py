"""The validation image panels on the GPU (iswm_amd/csrc/val_panels.hip, ops.val_panels, iswm_amd/val_results.py)
against the CPU restatement tests/val_results_ref.py: every byte panel exact, the class map equal to the unfused
argmax the metrics score, the confidence within predict_maps's pinned bounds, and one training run end to end."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import val_results_ref as R

pytestmark = pytest.mark.gpu

N = 3                                   # H * W odd for every shape below: image boundaries fall inside 16-pixel chunks
SHAPES = [((1, 1), (1, 1)), ((9, 9), (33, 33)), ((17, 23), (65, 93))]
CLASSES = [(2, 8), (3, 8), (5, 8), (16, 16), (17, 20)]          # (C, pitch): G = 1, 1, 2, 4 register groups and two passes


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda")


def _logits(n, h, w, c, ld, seed):
    """low-res NHWC logits with saturated pixels (+-30) and exact ties between class 0, class 1 and the last class
    (the generator of test_predict_gpu)"""
    g = torch.Generator().manual_seed(seed)
    yl = torch.randn((n, h, w, ld), generator=g) * 3.0
    sat = torch.rand((n, h, w), generator=g) < 0.1
    yl[..., 0][sat] = 30.0
    yl[..., 1][sat] = -30.0
    flip = torch.rand((n, h, w), generator=g) < 0.05
    yl[..., 0][flip] = -30.0
    yl[..., 1][flip] = 30.0
    tie = torch.rand((n, h, w), generator=g) < 0.1
    yl[..., c - 1][tie] = yl[..., 0][tie]
    yl[..., 1][tie] = yl[..., 0][tie]
    return yl


_CASES = {}


def _case(c, ld, lo_hi):
    """inputs, the kernel's outputs and the references of one case, computed once and shared by the tests below"""
    key = (c, ld, lo_hi)
    if key in _CASES:
        return _CASES[key]
    from iswm_amd import ops
    (hl, wl), (H, W) = lo_hi
    d = dev()
    seed = hl * 31 + c * 7
    rng = np.random.default_rng(seed)
    yl = _logits(N, hl, wl, c, ld, seed).to(d)
    img = rng.integers(0, 256, (N, H, W, 3), dtype=np.uint8)
    img[0, 0, 0] = (0, 255, 128)
    x = ops.predict_normalize(torch.from_numpy(img).to(d), R.MEAN, R.STD)
    # what no uint8 image produces: checked against the clamp rule only
    planted = [((0, 0, H - 1, W - 1), float("nan"), 0), ((1, 1, H // 2, W // 2), 1e9, 255), ((2, 2, 0, W - 1), -1e9, 0),
               ((1, 0, H - 1, 0), float("inf"), 255), ((2, 1, H // 3, 0), -2.2, 0)]
    for idx, v, _ in planted:
        x[idx] = v
    lab = rng.choice(np.array([0, 255] + list(range(1, c)), dtype=np.uint8), size=(N, H, W),
                     p=[0.5, 0.1] + [0.4 / (c - 1)] * (c - 1))
    lab.reshape(-1)[:3] = (0, 1, 255)                                   # all three kinds present, also at 1 x 1
    lab8 = torch.from_numpy(lab).to(d)
    m = ops.val_panels(x, yl, lab8, c, R.MEAN, R.STD, want_prob=True)
    lg = ops.bilinear_to_nchw_fwd(yl, c, H, W)                          # the unfused path's own logits: model(x)
    pred_ref = ops.argmax_nchw(lg).cpu().numpy()
    out = dict(c=c, H=H, W=W, x=x, yl=yl, lab=lab, lab8=lab8, m=m, planted=planted, pred_ref=pred_ref,
               lg64=lg.cpu().double().numpy(), pal=R.palette(c),
               original_ref=np.stack([R.denormalize_u8(xx) for xx in x.cpu()]))
    _CASES[key] = out
    return out


ALL = [(c, ld, s) for c, ld in CLASSES for s in SHAPES]


@pytest.mark.parametrize("c,ld,lo_hi", ALL)
def test_byte_panels_equal_the_restatement(c, ld, lo_hi):
    k = _case(c, ld, lo_hi)
    m = k["m"]
    original = m.original.cpu().numpy()
    assert np.array_equal(original, k["original_ref"])
    for (n, ch, y, xx), _, want in k["planted"]:
        assert original[n, y, xx, ch] == want, "clamp rule"
    pred = m.pred.cpu().numpy()
    assert pred.dtype == np.uint8 and np.array_equal(pred, k["pred_ref"]), "not the mask the metrics score"
    pal = k["pal"]
    assert np.array_equal(m.target_rgb.cpu().numpy(), pal[k["lab"]])
    assert np.array_equal(m.pred_rgb.cpu().numpy(), pal[k["pred_ref"]])
    assert np.array_equal(m.overlay.cpu().numpy(), R.overlay(k["original_ref"], pal[k["pred_ref"]]))
    err = R.error_map(k["lab"], k["pred_ref"])
    assert np.array_equal(m.error.cpu().numpy(), err)
    if k["H"] > 1:
        seen = {tuple(v) for v in err.reshape(-1, 3).tolist()}
        assert {R.GREY, R.BLACK, R.WHITE, R.RED, R.BLUE} <= seen and ((R.MAGENTA in seen) == (c > 2))
    if c == 2:
        assert np.array_equal(m.target_rgb.cpu().numpy()[0], R.decode_target(k["lab"][0], 2))


@pytest.mark.parametrize("c,ld", [(4, 4), (8, 8), (16, 16), (19, 20)])
def test_class_map_carries_the_unfused_kernels_roundings(c, ld):
    """every class with the SAME low-resolution logits: the up-sampled logits of two classes then differ only where the
    unfused kernel rounds their float4 lanes differently, so argmax is a per-pixel fingerprint of those roundings.
    The fused class map must be that fingerprint byte for byte -- the sampled logits are model(x)'s bits, not merely
    close -- and p_max can never exceed 1 (the maximal class contributes expf(0) = 1 to the sum)."""
    from iswm_amd import ops
    (hl, wl), (H, W) = SHAPES[2]
    d = dev()
    g = torch.Generator().manual_seed(c)
    yl = (torch.randn((N, hl, wl, 1), generator=g) * 9.0).expand(N, hl, wl, ld).contiguous().to(d)
    lg = ops.bilinear_to_nchw_fwd(yl, c, H, W)
    want = ops.argmax_nchw(lg).cpu().numpy()
    x = torch.zeros((N, 3, H, W), device=d)
    lab = torch.zeros((N, H, W), dtype=torch.uint8, device=d)
    m = ops.val_panels(x, yl, lab, c, R.MEAN, R.STD, want=("pred",), want_prob=True)
    pred = m.pred.cpu().numpy()
    lanes = np.bincount(want.reshape(-1) % 4, minlength=4)
    print("same-logit classes C=%d: argmax by lane %s, %d pixels differ" % (c, lanes.tolist(), int((pred != want).sum())))
    assert (lanes > 0).sum() >= 2, "the unfused kernel rounds every lane alike: this case shows nothing"
    assert np.array_equal(pred, want)
    assert float(m.prob.max()) <= 1.0


@pytest.mark.parametrize("c,ld,lo_hi", ALL)
def test_int64_labels_give_the_same_panels(c, ld, lo_hi):
    from iswm_amd import ops
    k = _case(c, ld, lo_hi)
    m64 = ops.val_panels(k["x"], k["yl"], k["lab8"].long(), c, R.MEAN, R.STD, want=("target_rgb", "error"))
    assert torch.equal(m64.target_rgb, k["m"].target_rgb) and torch.equal(m64.error, k["m"].error)
    assert m64.original is None and m64.pred is None and m64.prob is None
    assert m64.packed.numel() == ops.val_panels_layout(N, k["H"], k["W"], ("target_rgb", "error"))["end"]


@pytest.mark.parametrize("c,ld,lo_hi", ALL)
def test_confidence_against_restatement(c, ld, lo_hi):
    """the bounds test_predict_maps_against_restatement holds the same arithmetic to"""
    k = _case(c, ld, lo_hi)
    m = k["m"]
    prob = m.prob.cpu().numpy()
    conf = m.conf.cpu().numpy()
    npix = prob.size
    assert prob.dtype == np.float32 and np.array_equal(conf, R.conf_u8(prob)), "conf is not the truncation of the kernel's own p"
    p64 = R.max_prob(k["lg64"])
    dmax = float(np.abs(prob.astype(np.float64) - p64).max())
    conf_r = R.conf_u8(p64)
    edge = R.near_boundary(p64, 2e-6)
    bad = conf != conf_r
    absorbed = bad & (prob == 1.0)          # fp32's 1 + e = 1 once e < 2^-24, where the rounded fp64 p is 1 - 2^-24
    print("val_panels C=%d %s->%dx%d: max |p - p64| %.2e, %d boundary pixels, %d conf differ (%d of them p = 1 in fp32)"
          % (c, lo_hi[0], k["H"], k["W"], dmax, int(edge.sum()), int(bad.sum()), int(absorbed.sum())))
    assert dmax <= 1e-6
    assert not (bad & ~edge).any(), "mismatch away from a truncation boundary"
    assert (bad & ~absorbed).sum() <= (2e-4 if c <= 3 else 1e-3) * npix + 2
    assert prob.min() >= 1.0 / c - 1e-6 and prob.max() <= 1.0


@pytest.mark.parametrize("c,ld,lo_hi", [(2, 8, SHAPES[2]), (5, 8, SHAPES[1]), (17, 20, SHAPES[2])])
def test_two_calls_give_identical_bytes(c, ld, lo_hi):
    from iswm_amd import ops
    k = _case(c, ld, lo_hi)
    again = ops.val_panels(k["x"], k["yl"], k["lab8"], c, R.MEAN, R.STD, want_prob=True)
    for name, a, b in zip(ops.VAL_PANELS, again[:7], k["m"][:7]):           # (the padding between panels is never written)
        assert torch.equal(a, b), name
    assert torch.equal(again.prob.view(torch.int32), k["m"].prob.view(torch.int32))


@pytest.mark.parametrize("c,ld", [(3, 8), (17, 20)])
def test_a_single_output_writes_only_itself(c, ld):
    """every output alone, through the C ABI, into a sentinel-filled copy of the packed buffer: its bytes are the full
    call's, every other byte keeps the sentinel"""
    from iswm_amd import _lib, ops
    k = _case(c, ld, SHAPES[2])
    H, W, m = k["H"], k["W"], k["m"]
    lay = ops.val_panels_layout(N, H, W)
    m3, s3 = ops.denorm_constants(R.MEAN, R.STD)
    m3, s3 = (ctypes.c_float * 3)(*m3.tolist()), (ctypes.c_float * 3)(*s3.tolist())
    pal = torch.from_numpy(ops.val_palette(c)).to(dev())
    _, hl, wl, _ = k["yl"].shape
    order = ("original", "pred", "conf", "prob", "target_rgb", "pred_rgb", "overlay", "error")       # the C argument order
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for name in order:
        packed = torch.full_like(m.packed, 0xA5)
        prob = torch.full_like(m.prob, -7.0)
        outs = [None] * 8
        if name == "prob":
            outs[3] = ptr(prob)
        else:
            size = N * H * W * (1 if name in ("pred", "conf") else 3)
            outs[order.index(name)] = ctypes.c_void_p(packed.data_ptr() + lay[name])
        _lib.call("iswm_val_panels", ptr(k["x"]), ptr(k["yl"]), ptr(k["lab8"]), 0, N, hl, wl, ld, c, H, W, m3, s3, ptr(pal),
                  *(outs + [stream]))
        if name == "prob":
            assert torch.equal(prob, m.prob) and bool((packed == 0xA5).all())
        else:
            lo = lay[name]
            assert torch.equal(packed[lo:lo + size], m.packed[lo:lo + size]), name
            assert bool((packed[:lo] == 0xA5).all()) and bool((packed[lo + size:] == 0xA5).all()), name
            assert bool((prob == -7.0).all())


def test_argument_checks():
    from iswm_amd import ops
    k = _case(2, 8, SHAPES[1])
    x, yl, lab = k["x"], k["yl"], k["lab8"]
    with pytest.raises(ValueError, match="want"):
        ops.val_panels(x, yl, lab, 2, R.MEAN, R.STD, want=("nope",))
    with pytest.raises(ValueError, match="do not hold"):
        ops.val_panels(x, yl, lab, 9, R.MEAN, R.STD)
    with pytest.raises(ValueError, match="labels"):
        ops.val_panels(x, yl, lab[:, :-1], 2, R.MEAN, R.STD)
    with pytest.raises(TypeError, match="uint8 or int64"):
        ops.val_panels(x, yl, lab.int(), 2, R.MEAN, R.STD)
    with pytest.raises(ValueError, match="CUDA"):
        ops.val_panels(x.cpu(), yl, lab, 2, R.MEAN, R.STD)
    with pytest.raises(ValueError, match="batch of"):
        ops.val_panels(x, yl[:2], lab, 2, R.MEAN, R.STD)


def test_train_saves_the_best_models_validation_images(tmp_path, capsys):
    """the run of test_train_validate_checkpoint_resume with --save_val_results --save_confidence_map: one directory
    per best checkpoint, six files per validation batch, _pred.png the palette of argmax(model(x)) of the saved
    checkpoint on frame 0 of batch 0, _original.png the restatement of that frame; --test_only writes its own
    directory; without the flag nothing is written"""
    from iswm_amd import ops, train
    from iswm_amd import val_results as V
    from iswm_amd.network import modeling
    d = dev()
    ck, vr = str(tmp_path / "ck"), str(tmp_path / "vr")
    base = ["--model", "deeplabv3plus_resnet50", "--crop_size", "65", "--batch_size", "4", "--synthetic_len", "16",
            "--optimizer", "sgd", "--loss_type", "IWce_loss", "--print_interval", "2", "--val_interval", "2",
            "--val_batch_size", "4", "--checkpoints_dir", ck, "--num_workers", "0"]
    train.main(base + ["--total_itrs", "4", "--save_val_results", "--save_confidence_map", "--val_results_dir", vr])
    out = capsys.readouterr().out
    nbest = sum(1 for line in out.splitlines() if line.startswith("saved "))
    dirs = sorted(os.listdir(vr))
    assert nbest >= 1 and len(dirs) == nbest and all(x.startswith("best_model_iter_") for x in dirs)
    assert out.count("Saved 2 validation images of the best model") == nbest
    names = sorted("%04d_%s.png" % (i, kind) for i in range(2) for kind in V.panel_kinds(True))        # 8 val tiles, batch 4
    for x in dirs:
        assert sorted(os.listdir(os.path.join(vr, x))) == names and len(names) == 12

    files = glob.glob(os.path.join(ck, "best_*.pth"))
    assert len(files) == 1
    ckpt = torch.load(files[0], map_location="cpu", weights_only=True)
    best_dir = os.path.join(vr, V.results_dirname(ckpt["cur_itrs"], ckpt["weighted_score"]))
    assert os.path.isdir(best_dir)
    model = modeling.deeplabv3plus_resnet50(num_classes=2, output_stride=16)
    model.load_state_dict(ckpt["model_state"], strict=True)
    model = model.to(d).eval()
    val = train.SyntheticBinarySegmentation(split='val', size=65, length=8, seed=1)
    xb = torch.stack([val[i][0] for i in range(4)]).to(d)
    with torch.no_grad():
        pred = ops.argmax_nchw(model(xb))[0].cpu().numpy()
    for kind, mode in (("original", "RGB"), ("target", "RGB"), ("pred", "RGB"), ("overlay", "RGB"), ("error", "RGB"),
                       ("confidence", "L")):
        im = Image.open(os.path.join(best_dir, "0000_%s.png" % kind))
        assert im.mode == mode and im.size == (65, 65), kind
    png = lambda kind: np.asarray(Image.open(os.path.join(best_dir, "0000_%s.png" % kind)))
    assert np.array_equal(png("pred"), R.palette(2)[pred])
    assert np.array_equal(png("original"), R.denormalize_u8(val[0][0]))
    assert np.array_equal(png("target"), R.decode_target(val[0][1].numpy(), 2))
    assert np.array_equal(png("overlay"), R.overlay(png("original"), png("pred")))
    assert np.array_equal(png("error"), R.error_map(val[0][1].numpy(), pred))

    # --test_only on that checkpoint: one more directory, named after the checkpoint's iteration, no confidence map
    train.main(base + ["--test_only", "--ckpt", files[0], "--save_val_results", "--val_results_dir", vr])
    capsys.readouterr()
    extra = [x for x in sorted(os.listdir(vr)) if x not in dirs]
    assert len(extra) == 1 and extra[0].startswith("test_only_iter_%d_score_" % ckpt["cur_itrs"])
    assert sorted(os.listdir(os.path.join(vr, extra[0]))) == [n for n in names if "confidence" not in n]
    assert np.array_equal(np.asarray(Image.open(os.path.join(vr, extra[0], "0000_pred.png"))), png("pred"))

    # the same run without the flag writes no directory
    off = str(tmp_path / "off")
    train.main(base + ["--total_itrs", "2", "--checkpoints_dir", str(tmp_path / "ck2"), "--val_results_dir", off])
    assert "Saved" not in capsys.readouterr().out and not os.path.exists(off)


def test_resident_loader_and_sequence_branch_save_images(tmp_path, capsys):
    """--dataset binary: the validation batches come from the device tile store, whose groups follow the tiles' sizes
    (3 + 2 + 4 tiles of 65x65 / 41x57 / 65x65 at batch 4: three frames saved, each at its own size); then the
    --val_metrics sequence branch, which names the directory after its own weighted score"""
    from iswm_amd import train
    from iswm_amd import val_results as V
    from iswm_amd.datasets import BinarySegmentation
    from tests.test_dataset_gpu import TRAIN_SIZES, VAL_SIZES, _args, _blob_split
    dev()
    root, vr = str(tmp_path / "data"), str(tmp_path / "vr")
    _blob_split(root, "train", TRAIN_SIZES, 1)
    _blob_split(root, "val", VAL_SIZES, 2)
    train.main(_args(root, str(tmp_path / "ck"), ["--total_itrs", "2", "--save_val_results", "--val_results_dir", vr]))
    out = capsys.readouterr().out
    dirs = os.listdir(vr)
    assert len(dirs) == 1 and dirs[0].startswith("best_model_iter_2_score_") and "Saved 3 validation images" in out
    d = os.path.join(vr, dirs[0])
    assert sorted(os.listdir(d)) == sorted("%04d_%s.png" % (i, k) for i in range(3) for k in V.panel_kinds(False))
    val = BinarySegmentation(root, "val")
    m, s = torch.tensor(R.MEAN)[:, None, None], torch.tensor(R.STD)[:, None, None]
    for frame, tile in ((0, 0), (1, 3), (2, 5)):                      # frame 0 of the groups (0, 3), (3, 2), (5, 4)
        img, mask = val[tile]
        h, w = VAL_SIZES[tile]
        png = lambda kind: np.asarray(Image.open(os.path.join(d, "%04d_%s.png" % (frame, kind))))
        assert png("pred").shape == (h, w, 3)
        x = torch.from_numpy(np.ascontiguousarray(img)).permute(2, 0, 1).float().div(255).sub(m).div(s)
        assert np.array_equal(png("original"), R.denormalize_u8(x))
        gt = (np.asarray(mask) > 0).astype(np.uint8)
        assert np.array_equal(png("target"), R.decode_target(gt, 2))
        pred = (png("pred")[..., 0] == 255).astype(np.uint8)
        assert np.array_equal(png("error"), R.error_map(gt, pred))
        assert np.array_equal(png("overlay"), R.overlay(png("original"), png("pred")))

    root2, vr2 = str(tmp_path / "seq"), str(tmp_path / "vr2")
    _blob_split(root2, "train", TRAIN_SIZES, 1)
    _blob_split(root2, "val", [(65, 65)] * 5, 2)
    train.main(_args(root2, str(tmp_path / "ck2"), ["--total_itrs", "2", "--val_metrics", "sequence", "--sequence_length", "3",
                                                    "--save_val_results", "--save_confidence_map", "--val_results_dir", vr2]))
    out = capsys.readouterr().out
    ckpt = torch.load(glob.glob(os.path.join(str(tmp_path / "ck2"), "best_*.pth"))[0], map_location="cpu", weights_only=True)
    assert os.listdir(vr2) == [V.results_dirname(2, ckpt["weighted_score"])] and "Saved 2 validation images" in out
    assert sorted(os.listdir(os.path.join(vr2, os.listdir(vr2)[0]))) == \
        sorted("%04d_%s.png" % (i, k) for i in range(2) for k in V.panel_kinds(True))
