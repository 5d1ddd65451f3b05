"""Inference entry point on the CPU: the restatement's decision edges, the band bounds the kernel receives, the
reference's command line, and the folder walk with a stub predictor (iswm_amd/predict.py)."""
import os

import numpy as np
import pytest
import torch
from PIL import Image

from tests import predict_ref as R

f32 = np.float32


def test_threshold_and_truncation_edges():
    # torch compares a float32 tensor with a Python float in float32: 0.2f is not > 0.2
    assert not bool(torch.tensor([0.2], dtype=torch.float32) > 0.2)
    up = np.nextafter(f32(0.2), f32(1))
    p = np.array([f32(0.2), up, f32(0.6), f32(0.5), f32(1.0), f32(0.0)], dtype=np.float32)
    pred, conf = R.predict_mask(p, 0.2)
    assert pred.tolist() == [0, 255, 255, 255, 255, 0]
    # 0.2f * 255 == 51 exactly, one ulp above stays 51 (51.000004), 0.6f * 255 == 153 exactly, 127.5 truncates
    assert conf.tolist() == [51, 51, 153, 127, 255, 0]
    mn, mx, s, n_low, n_pred = R.prob_stats(p, 0.2)
    assert (mn, mx, n_low, n_pred) == (0.0, 1.0, 1, 4)
    # the compare is done in fp32 for the threshold too: p = 0.5 against 0.5 is background
    assert R.predict_mask(np.array([0.5], np.float32), 0.5)[0].tolist() == [0]
    assert R.has_internal_wave(np.array([[255, 0], [0, 0]], np.uint8), 0.2) == (0.25, True)
    assert R.has_internal_wave(np.array([[255, 0], [0, 0]], np.uint8), 0.25) == (0.25, False)


PROBS = sorted({0.0, 1.0, 0.2, 0.7, 0.5, 51 / 255, 52 / 255, 178 / 255, 179 / 255, 0.2 + 1e-12, 0.2 - 1e-12,
                0.7 + 1e-12, 0.7 - 1e-12, 1 / 255, 254 / 255, -0.1, 1.1, 0.33, 0.999})


@pytest.mark.parametrize("min_prob", PROBS)
def test_band_bounds_exhaustive(min_prob):
    from iswm_amd import ops
    k = np.arange(256, dtype=np.uint8)
    for max_prob in PROBS:
        lo, hi = ops.band_bounds(min_prob, max_prob)
        want = R.binarize_confidence_map(k, min_prob, max_prob)
        got = np.where((k.astype(int) >= lo) & (k.astype(int) <= hi), 255, 0).astype(np.uint8)
        assert np.array_equal(got, want), (min_prob, max_prob, lo, hi)
        if min_prob > max_prob:
            assert not got.any()
    assert ops.band_bounds(0.2, 0.7) == (51, 178)     # 0.2 == 51/255 in fp64 is included
    assert ops.band_bounds(0.7, 0.2) == (1, 0)


REFERENCE_FLAGS = {
    "input": None, "dataset": "binary", "model": "deeplabv3plus_resnet50", "ckpt": None, "gpu_id": "0",
    "save_val_results_to": None, "output_stride": 16, "save_confidence": False, "save_binary": False,
    "binary_threshold": 200, "pred_threshold": 0.5, "internal_wave_area_threshold": 0.01,
    "synthetic_broken_prob": 0.8, "synthetic_broken_ratio": 0.05, "enable_wave_processing": False,
    "min_broken_prob": 0.2, "max_broken_prob": 0.7,
}


def test_argparser_keeps_reference_flags():
    from iswm_amd.predict import get_argparser
    opts = vars(get_argparser().parse_args(["--input", "in", "--save_val_results_to", "out"]))
    for name, default in REFERENCE_FLAGS.items():
        assert name in opts, name
        if name not in ("input", "save_val_results_to"):
            assert opts[name] == default, (name, opts[name], default)
    assert opts["batch_size"] == 1 and opts["workers"] == 4
    parsed = vars(get_argparser().parse_args([
        "--input", "a", "--save_val_results_to", "b", "--ckpt", "c.pth", "--gpu_id", "1", "--output_stride", "8",
        "--save_confidence", "--save_binary", "--binary_threshold", "100", "--pred_threshold", "0.3",
        "--internal_wave_area_threshold", "0.02", "--synthetic_broken_prob", "0.5", "--synthetic_broken_ratio", "0.1",
        "--min_broken_prob", "0.1", "--max_broken_prob", "0.9", "--model", "deeplabv3plus_resnet101"]))
    assert parsed["pred_threshold"] == 0.3 and parsed["max_broken_prob"] == 0.9 and parsed["output_stride"] == 8
    with pytest.raises(SystemExit):          # required, unlike the reference's default None
        get_argparser().parse_args(["--input", "in"])


def test_wave_processing_is_refused(capsys):
    from iswm_amd.predict import main
    with pytest.raises(SystemExit) as e:
        main(["--input", "in", "--save_val_results_to", "out", "--enable_wave_processing"])
    assert e.value.code == 2
    assert "--enable_wave_processing is not supported" in capsys.readouterr().err


def _write(path, h, w, seed):
    rng = np.random.default_rng(seed)
    Image.fromarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)).save(path)


def _tree(root):
    inp = os.path.join(root, "in")
    os.makedirs(os.path.join(inp, "a"))
    os.makedirs(os.path.join(inp, "b"))
    os.makedirs(os.path.join(inp, "b", "nested.png"))          # a directory with an image name: not a file
    _write(os.path.join(inp, "top.png"), 8, 8, 0)              # directly inside --input: ignored
    _write(os.path.join(inp, "a", "m.jpeg"), 8, 8, 1)
    _write(os.path.join(inp, "a", "q.tif"), 10, 6, 2)
    _write(os.path.join(inp, "a", "x.png"), 8, 8, 3)
    _write(os.path.join(inp, "a", "y.PNG"), 8, 8, 4)
    _write(os.path.join(inp, "a", "z.jpg"), 8, 8, 5)
    with open(os.path.join(inp, "a", "bad.png"), "wb") as f:
        f.write(b"not an image")
    with open(os.path.join(inp, "a", "notes.txt"), "w") as f:
        f.write("skip me")
    _write(os.path.join(inp, "b", "c.png"), 5, 7, 6)
    _write(os.path.join(inp, "b", "d.png"), 5, 7, 7)
    _write(os.path.join(inp, "b", "e.bmp"), 5, 7, 8)           # extension outside the reference's list
    return inp


class StubPredictor:
    """pred / conf / band = the three colour channels; records the batches it was given"""

    def __init__(self):
        self.batches = []

    def __call__(self, batch):
        self.batches.append(batch.shape)
        b = batch.copy()

        def wait():
            return {"pred": b[..., 0], "conf": b[..., 1], "band": b[..., 2], "stats": np.zeros((len(b), 5))}
        return wait


@pytest.mark.parametrize("batch_size", [1, 2, 3])
def test_folder_walk_with_stub(tmp_path, batch_size):
    from iswm_amd.predict import decode_image, process_images
    inp = _tree(str(tmp_path))
    out = os.path.join(str(tmp_path), "out")
    lines = []
    stub = StubPredictor()
    n = process_images(inp, out, stub, save_confidence=True, save_binary=True, pred_threshold=0.5,
                       batch_size=batch_size, workers=2, log=lines.append, progress=False)
    assert n == 7
    assert sorted(os.listdir(out)) == ["a", "b"]
    want = {"a": ["m", "q", "x", "y", "z"], "b": ["c", "d"]}
    for sub, names in want.items():
        files = sorted(os.listdir(os.path.join(out, sub)))
        assert files == sorted("%s_%s.png" % (b, k) for b in names for k in ("predict", "confidence", "binary_mask"))
        for f in os.listdir(os.path.join(inp, sub)):
            base, ext = os.path.splitext(f)
            if base not in names:
                continue
            src = decode_image(os.path.join(inp, sub, f))
            for k, kind in enumerate(("predict", "confidence", "binary_mask")):
                im = Image.open(os.path.join(out, sub, "%s_%s.png" % (base, kind)))
                assert im.mode == "L"
                assert np.array_equal(np.asarray(im), src[..., k]), (sub, f, kind)
    assert any("bad.png" in line for line in lines)
    # batches group consecutive same-size frames of one folder: a = [m, (bad), q, x, y, z], b = [c, d]
    sizes = [(s[0], s[1], s[2]) for s in stub.batches]
    expect = {1: [(1, 8, 8), (1, 10, 6), (1, 8, 8), (1, 8, 8), (1, 8, 8), (1, 5, 7), (1, 5, 7)],
              2: [(1, 8, 8), (1, 10, 6), (2, 8, 8), (1, 8, 8), (2, 5, 7)],
              3: [(1, 8, 8), (1, 10, 6), (3, 8, 8), (2, 5, 7)]}[batch_size]
    assert sizes == expect


def test_folder_walk_only_requested_maps(tmp_path):
    from iswm_amd.predict import process_images
    inp = _tree(str(tmp_path))
    out = os.path.join(str(tmp_path), "out")
    process_images(inp, out, StubPredictor(), save_confidence=False, save_binary=False, log=lambda s: None,
                   progress=False)
    assert sorted(os.listdir(os.path.join(out, "b"))) == ["c_predict.png", "d_predict.png"]


def test_predictor_failure_skips_its_batch(tmp_path):
    from iswm_amd.predict import process_images
    inp = _tree(str(tmp_path))
    out = os.path.join(str(tmp_path), "out")
    inner = StubPredictor()

    def flaky(batch):
        if batch.shape[1:3] == (10, 6):
            raise RuntimeError("boom")
        return inner(batch)
    lines = []
    n = process_images(inp, out, flaky, save_confidence=False, save_binary=False, log=lines.append, progress=False)
    assert n == 6
    assert any("q.tif" in line and "boom" in line for line in lines)
    assert "q_predict.png" not in os.listdir(os.path.join(out, "a"))


def test_pipeline_crosses_folders(tmp_path):
    """the next folder's first batch is enqueued before the previous folder's last batch is waited for"""
    from iswm_amd.predict import process_images
    inp = _tree(str(tmp_path))
    events = []

    def pred(batch):
        k = len([e for e in events if e[0] == "enqueue"])
        events.append(("enqueue", k, batch.shape))
        b = batch.copy()

        def wait():
            events.append(("wait", k))
            return {"pred": b[..., 0], "conf": b[..., 1], "band": b[..., 2], "stats": np.zeros((len(b), 5))}
        return wait
    lines = []
    process_images(inp, os.path.join(str(tmp_path), "out"), pred, save_confidence=False, save_binary=False,
                   batch_size=3, log=lines.append, progress=False)
    # a: [m], [q], [x, y, z]; b: [c, d]
    assert [e[1:] for e in events if e[0] == "enqueue"] == [(0, (1, 8, 8, 3)), (1, (1, 10, 6, 3)),
                                                              (2, (3, 8, 8, 3)), (3, (2, 5, 7, 3))]
    assert events.index(("enqueue", 3, (2, 5, 7, 3))) < events.index(("wait", 2))
    assert [e for e in events if e[0] == "wait"] == [("wait", k) for k in range(4)]
    assert lines.index("Finished folder a") < lines.index("Finished folder b")
