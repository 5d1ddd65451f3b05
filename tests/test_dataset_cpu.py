"""--dataset binary without a device: the image / mask folder data set (iswm_amd/datasets.py), the command line that
selects it, and the host-side validation of the tile-store entry points (csrc/dataset.hip)."""
import ctypes
import os

import numpy as np
import pytest


def _write(path, arr):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(arr).save(path)


def _make_split(root, split, names, sizes, seed=0, skip_masks=(), mask_size=None):
    """names: image file names; masks are <base>_mask<ext> of the same extension.  Returns {name: (img, mask)}."""
    rng = np.random.default_rng(seed)
    out = {}
    for k, (name, (h, w)) in enumerate(zip(names, sizes)):
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        mask = (rng.random((h, w)) < 0.3).astype(np.uint8) * rng.integers(1, 256, (h, w), dtype=np.uint8)
        base, ext = os.path.splitext(name)
        _write(os.path.join(root, split, "imgs", name), img)
        if name not in skip_masks:
            m = mask if mask_size is None or name not in mask_size else np.zeros(mask_size[name], np.uint8)
            _write(os.path.join(root, split, "masks", base + "_mask" + ext), m)
        out[name] = (img, mask)
    return out


def test_pairing_order_extensions_and_raw_items(tmp_path):
    from iswm_amd.datasets import BinarySegmentation
    names = ["b_002.PNG", "a_010.png", "c_001.Jpg", "a_002.jpeg", "d_000.JPEG"]
    sizes = [(40, 56), (97, 129), (41, 57), (40, 56), (64, 48)]
    want = _make_split(str(tmp_path), "train", names, sizes)
    open(os.path.join(str(tmp_path), "train", "imgs", "notes.txt"), "w").write("not an image")
    _write(os.path.join(str(tmp_path), "train", "imgs", "e.bmp"), np.zeros((8, 8, 3), np.uint8))
    ds = BinarySegmentation(str(tmp_path), split="train")
    assert ds.images == sorted(names) and len(ds) == 5
    assert ds.masks == [os.path.splitext(n)[0] + "_mask" + os.path.splitext(n)[1] for n in sorted(names)]
    for i, n in enumerate(ds.images):
        img, mask = ds[i]
        assert img.dtype == np.uint8 and mask.dtype == np.uint8
        assert img.shape == want[n][0].shape and mask.shape == want[n][1].shape
        if n.lower().endswith(".png"):                                   # lossless: the bytes come back, the mask NOT binarised
            assert np.array_equal(img, want[n][0]) and np.array_equal(mask, want[n][1])
            assert mask.max() > 1
    assert np.array_equal(ds.decode_target(np.array([[0, 1], [1, 0]], np.uint8)), np.array([[0, 255], [255, 0]], np.uint8))
    assert ds.decode_target(np.ones((2, 2), np.uint8)).dtype == np.uint8


def test_missing_masks_are_all_named(tmp_path):
    from iswm_amd.datasets import BinarySegmentation
    names = ["f0.png", "f1.png", "f2.jpg", "f3.png"]
    _make_split(str(tmp_path), "val", names, [(40, 56)] * 4, skip_masks=("f1.png", "f2.jpg"))
    with pytest.raises(FileNotFoundError) as e:
        BinarySegmentation(str(tmp_path), split="val")
    msg = str(e.value)
    assert "f1_mask.png" in msg and "f2_mask.jpg" in msg and "f0_mask.png" not in msg and "f3_mask.png" not in msg


def test_mask_size_mismatches_are_all_named(tmp_path):
    from iswm_amd.datasets import BinarySegmentation
    names = ["f0.png", "f1.png", "f2.png"]
    _make_split(str(tmp_path), "train", names, [(40, 56)] * 3, mask_size={"f0.png": (40, 55), "f2.png": (41, 56)})
    with pytest.raises(ValueError) as e:
        BinarySegmentation(str(tmp_path), split="train")
    msg = str(e.value)
    assert "f0.png" in msg and "f2.png" in msg and "f1.png" not in msg and "40x55" in msg


def test_missing_layout_is_a_clear_error(tmp_path):
    from iswm_amd.datasets import BinarySegmentation
    with pytest.raises(FileNotFoundError) as e:
        BinarySegmentation(str(tmp_path), split="train")
    assert "imgs" in str(e.value)


def test_dataset_binary_is_accepted_and_constructed(tmp_path):
    from iswm_amd import train
    from iswm_amd.datasets import BinarySegmentation
    _make_split(str(tmp_path), "train", ["t%d.png" % i for i in range(3)], [(40, 56)] * 3)
    _make_split(str(tmp_path), "val", ["v%d.png" % i for i in range(2)], [(41, 57)] * 2)
    opts = train.get_argparser().parse_args(["--dataset", "binary", "--data_root", str(tmp_path)])
    assert opts.dataset == "binary"
    tr, va = train.get_dataset(opts)
    assert isinstance(tr, BinarySegmentation) and isinstance(va, BinarySegmentation)
    assert (len(tr), len(va)) == (3, 2) and va.images == ["v0.png", "v1.png"] and tr.sizes == [(40, 56)] * 3


def test_epoch_batches_partition_the_order():
    from iswm_amd import train
    n, B = 37, 4
    one = train.epoch_batches(n, B, seed=3, epoch=1)
    assert len(one) == n // B and all(len(b) == B for b in one)
    flat = [i for b in one for i in b]
    assert len(set(flat)) == len(flat) and set(flat) <= set(range(n))
    assert one == train.epoch_batches(n, B, seed=3, epoch=1)                      # a function of (seed, epoch) alone
    assert one != train.epoch_batches(n, B, seed=3, epoch=2) and one != train.epoch_batches(n, B, seed=4, epoch=1)
    for world in (2, 3):
        parts = [train.epoch_batches(n, B, 3, 1, r, world) for r in range(world)]
        assert len(set(len(p) for p in parts)) == 1                               # every rank steps equally often
        got = [i for p in parts for b in p for i in b]
        assert len(got) == len(set(got)) == n // (B * world) * B * world
        assert parts[1][0] == one[1]                                              # rank r takes batches r, r + world, ...


def test_tile_store_entry_points_are_exported_and_validate_on_the_host():
    from iswm_amd import _lib
    lib = _lib.load()
    err = lambda: lib.iswm_last_error().decode()
    names = ("iswm_label_prepare_workspace", "iswm_label_prepare", "iswm_label_count_workspace", "iswm_label_count",
             "iswm_aug_tables_workspace", "iswm_aug_tables", "iswm_gather_normalize")
    for n in names:
        assert n in _lib.EXPORTS and hasattr(lib, n), n
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    f3 = (ctypes.c_float * 3)(0.5, 0.5, 0.5)
    # workspace queries: pure host arithmetic, 0 for an empty problem
    assert lib.iswm_label_prepare_workspace(0) == 0 and lib.iswm_label_prepare_workspace(16) == 8
    assert lib.iswm_label_prepare_workspace(1 << 30) == 2048 * 8                  # capped grid: one int64 per workgroup
    assert lib.iswm_label_count_workspace(0) == 0 and lib.iswm_label_count_workspace(100) == 16
    assert lib.iswm_aug_tables_workspace(None, 4) == 0
    from iswm_amd.utils.ext_transforms import _AUG_DTYPE, _ksize, _nearest_table, _resample_tables
    rec = np.zeros(2, dtype=_AUG_DTYPE)
    total = 0
    for b, (sh, sw, rh, rw) in enumerate([(40, 56, 20, 28), (97, 129, 150, 200)]):
        ksh, ksv = _ksize(sw, rw), _ksize(sh, rh)
        assert (ksh, ksv) == (_resample_tables(sw, rw)[2], _resample_tables(sh, rh)[2])
        rec[b] = (0, 0, sh, sw, rh, rw, 0, 0, 0, 0, total, ksh, ksv, 0)
        total += sum(t.size for t in (_nearest_table(sw, rw), _nearest_table(sh, rh), _resample_tables(sw, rw)[0],
                                      _resample_tables(sw, rw)[1], _resample_tables(sh, rh)[0], _resample_tables(sh, rh)[1]))
    assert _AUG_DTYPE.itemsize == 64
    assert lib.iswm_aug_tables_workspace(rec.ctypes.data_as(ctypes.c_void_p), 2) == total * 4
    rec["rs_w"][1] = 0
    assert lib.iswm_aug_tables_workspace(rec.ctypes.data_as(ctypes.c_void_p), 2) == 0        # a bad record
    # null pointers / bad sizes: status 1 and a message, nothing launched
    assert lib.iswm_label_prepare(None, 16, None, None, 0, None) == 1 and "null" in err()
    assert lib.iswm_label_prepare(p, 24, p, p, 64, None) == 1 and "16" in err()
    assert lib.iswm_label_prepare(p, 32, p, p, 0, None) == 1 and "workspace" in err()
    assert lib.iswm_label_count(None, 16, 255, None, None, 0, None) == 1 and "null" in err()
    assert lib.iswm_label_count(p, 0, 255, p, p, 64, None) == 1
    assert lib.iswm_label_count(p, 16, 300, p, p, 64, None) == 1 and "ignore_index" in err()
    assert lib.iswm_label_count(p, 16, 255, p, p, 0, None) == 1 and "workspace" in err()
    assert lib.iswm_aug_tables(None, 1, 8, None, 64, None) == 1 and "null" in err()
    assert lib.iswm_aug_tables(p, 0, 8, p, 64, None) == 1
    assert lib.iswm_aug_tables(p, 1, 0, p, 64, None) == 1
    assert lib.iswm_aug_tables(p, 1, 8, p, 0, None) == 1 and "table" in err()
    assert lib.iswm_gather_normalize(None, None, None, 1, 8, 8, None, None, None, None, None) == 1 and "null" in err()
    assert lib.iswm_gather_normalize(p, p, p, 0, 8, 8, f3, f3, p, p, None) == 1 and "size" in err()
    assert lib.iswm_gather_normalize(p, p, p, 1, 8, 0, f3, f3, p, p, None) == 1


def test_resident_class_weights_need_device_labels():
    import torch
    from iswm_amd.utils.loss import calculate_class_weights_resident
    with pytest.raises(ValueError):
        calculate_class_weights_resident([(None, torch.zeros(2, 4, 4, dtype=torch.uint8))])
    with pytest.raises(ValueError):
        calculate_class_weights_resident([])
