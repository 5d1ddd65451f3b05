"""Rotation, vertical flip and colour jitter on the GPU (csrc/augment.hip): iswm_aug_rotate and
iswm_augment_batch_ex through ExtCompose.batch / batch_resident, bit for bit against tests/augment_ext_ref.py, which
tests/test_augment_ext_cpu.py pins to Pillow.  Every comparison is torch.equal."""
import ctypes
import itertools
import math
import random
import time

import numpy as np
import pytest
import torch

from oracle import augment as oaug
from tests import augment_ext_ref as R
from tests.test_dataset_cpu import _make_split

pytestmark = pytest.mark.gpu
MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
CROP = (65, 65)
SOURCES = [(40, 40), (60, 90), (33, 200)]                   # with crop 65 the first and the last are always padded
B, C, S, H = R.BRIGHTNESS, R.CONTRAST, R.SATURATION, R.HUE


def dev():
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    return torch.device("cuda:0")


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _compose(rotate=None, vflip=False, jitter=None, crop=CROP, depth=4):
    from iswm_amd.utils import ext_transforms as et
    chain = [et.ExtRandomRotation(rotate)] if rotate is not None else []
    chain += [et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(size=crop, pad_if_needed=True), et.ExtRandomHorizontalFlip()]
    if vflip:
        chain.append(et.ExtRandomVerticalFlip())
    if jitter is not None:
        chain.append(et.ExtColorJitter(*jitter))
    return et.ExtCompose(chain + [et.ExtToTensor(), et.ExtNormalize(MEAN, STD)], ring_depth=depth)


def _tiles(sizes, seed):
    rng = np.random.default_rng(seed)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    lbls = [(rng.random((h, w)) < 0.3).astype(np.uint8) for h, w in sizes]
    return imgs, lbls


def _geometry(sizes, crop, seed):
    random.seed(seed)
    return [oaug.draw_params(h, w, crop) for h, w in sizes]


def _check(comp, imgs, lbls, params, crop=CROP):
    d = dev()
    out, out_lbl = comp.batch([torch.from_numpy(a).to(d) for a in imgs], [torch.from_numpy(a).to(d) for a in lbls],
                              params=params)
    out, out_lbl = out.cpu(), out_lbl.cpu()
    assert out.shape == (len(imgs), 3) + tuple(crop) and out_lbl.dtype == torch.uint8
    for b in range(len(imgs)):
        t, lab = R.chain(imgs[b], lbls[b], params[b], crop, MEAN, STD)
        assert torch.equal(out_lbl[b], lab), "label %d, params %r" % (b, params[b])
        assert torch.equal(out[b], t), "image %d, params %r: %d values differ" % (b, params[b], int((out[b] != t).sum()))
    return out, out_lbl


# ---- 1. the rotation pass alone ------------------------------------------------------------------------------------
def test_aug_rotate_alone_equals_the_restatement():
    from iswm_amd import _lib
    from iswm_amd.utils import ext_transforms as et
    d = dev()
    sizes = [(1, 1), (2, 3), (7, 5), (37, 53), (64, 64), (64, 64), (97, 129), (129, 97), (17, 300)]   # (h, w); 300 wide
    angles = [180, -33.3, 0, 44.999, 90, 33.3, 359.99, 270, -150.0]
    imgs, lbls = _tiles(sizes, 21)
    imgs = [np.maximum(a, 1) for a in imgs]                                # no zero: the fill is told from the source
    lbls = [a + 1 for a in lbls]
    rec = np.zeros(len(sizes), dtype=et._AUG_DTYPE)
    ext = np.zeros(len(sizes), dtype=et._AUG_EXTRA_DTYPE)
    io = lo = ro = rl = 0
    places = []
    for b, ((h, w), angle) in enumerate(zip(sizes, angles)):
        rec[b] = (io, lo, h, w, h, w, 0, 0, 0, 0, 0, 3, 3, 0)
        rotated, _ = et._fill_extra(ext[b], (h, w, 0, 0, 0, 0, angle, 0, (), (None,) * 4), h, w, ro, rl)
        assert rotated == (angle != 0)
        ext[b]["rot_img_off"], ext[b]["rot_lbl_off"] = ro, rl              # a place for every sample, used or not
        places.append((ro, rl))
        io, lo = io + h * w * 3, lo + h * w                                # sources packed without alignment
        ro, rl = ro + et._align16(h * w * 3), rl + et._align16(h * w)
    img_buf = torch.from_numpy(np.concatenate([a.reshape(-1) for a in imgs])).to(d)
    lbl_buf = torch.from_numpy(np.concatenate([a.reshape(-1) for a in lbls])).to(d)
    rec_dev, ext_dev = torch.from_numpy(rec.view(np.uint8)).to(d), torch.from_numpy(ext.view(np.uint8)).to(d)
    rimg = torch.full((ro + 64,), 7, dtype=torch.uint8, device=d)
    rlbl = torch.full((rl + 64,), 7, dtype=torch.uint8, device=d)
    _lib.call("iswm_aug_rotate", img_buf.data_ptr(), lbl_buf.data_ptr(), rec_dev.data_ptr(), ext_dev.data_ptr(),
              len(sizes), max(h * w for h, w in sizes),
              rimg.data_ptr(), ro, rlbl.data_ptr(), rl, _stream())
    gi, gl = rimg.cpu().numpy(), rlbl.cpu().numpy()
    want_i, want_l = np.full(ro + 64, 7, np.uint8), np.full(rl + 64, 7, np.uint8)      # untouched: gaps, mode "none", the tail
    for b, ((h, w), angle) in enumerate(zip(sizes, angles)):
        if angle == 0:
            continue
        po, pl = places[b]
        want_i[po:po + h * w * 3] = R.rotate_nearest(imgs[b], angle).reshape(-1)
        want_l[pl:pl + h * w] = R.rotate_nearest(lbls[b], angle).reshape(-1)
    assert np.array_equal(gi, want_i), "rotated images: %d bytes differ" % int((gi != want_i).sum())
    assert np.array_equal(gl, want_l), "rotated labels: %d bytes differ" % int((gl != want_l).sum())
    # a copy that would end past its arena is left unwritten
    rimg.fill_(7)
    rlbl.fill_(7)
    _lib.call("iswm_aug_rotate", img_buf.data_ptr(), lbl_buf.data_ptr(), rec_dev.data_ptr(), ext_dev.data_ptr(),
              len(sizes), max(h * w for h, w in sizes),
              rimg.data_ptr(), places[-1][0] + 17 * 300 * 3 - 1, rlbl.data_ptr(), rl, _stream())
    po, pl = places[-1]
    assert bool((rimg[po:] == 7).all()) and bool((rlbl[pl:] == 7).all()) and bool((rimg[:po] != 7).any())


# ---- 2. the whole chain ----------------------------------------------------------------------------------------------
def test_each_transform_alone_and_all_together():
    imgs, lbls = _tiles(SOURCES, 3)
    geo = _geometry(SOURCES, CROP, 11)
    assert sum(p[2] > 0 for p in geo) >= 2                                 # at least two padded samples
    none = (None,) * 4
    f = (0.7, 1.3, 0.4, 0.2)
    angles = (33.3, -71.0, 180)
    cases = {
        "rotation": (_compose(rotate=90), [g + (a, 0, (), none) for g, a in zip(geo, angles)]),
        "vflip": (_compose(vflip=True), [g + (None, v, (), none) for g, v in zip(geo, (1, 1, 0))]),
        "brightness": (_compose(jitter=(0.5, 0, 0, 0)), [g + (None, 0, (B,), (x, None, None, None)) for g, x in zip(geo, (0.6, 1.4, 1.9))]),
        "contrast": (_compose(jitter=(0, 0.5, 0, 0)), [g + (None, 0, (C,), (None, x, None, None)) for g, x in zip(geo, (0.6, 1.4, 1.9))]),
        "saturation": (_compose(jitter=(0, 0, 0.5, 0)), [g + (None, 0, (S,), (None, None, x, None)) for g, x in zip(geo, (0.6, 1.4, 1.9))]),
        "hue": (_compose(jitter=(0, 0, 0, 0.5)), [g + (None, 0, (H,), (None, None, None, x)) for g, x in zip(geo, (-0.5, 0.1, 0.37))]),
        "all": (_compose(rotate=90, vflip=True, jitter=(0.5, 0.5, 0.5, 0.5)),
                [g + (a, v, o, f) for g, a, v, o in zip(geo, angles, (1, 0, 1), ((S, C, H, B), (H, B, C, S), (C, S, B, H)))]),
    }
    for name, (comp, params) in cases.items():
        assert comp.extended, name
        _check(comp, imgs, lbls, params)


def test_all_op_orders_and_exact_factors():
    orders = list(itertools.permutations((B, C, S, H)))
    assert len(orders) == 24
    sizes = [SOURCES[k % 3] for k in range(24)]
    imgs, lbls = _tiles(sizes, 4)
    geo = _geometry(sizes, CROP, 12)
    rng = random.Random(8)
    params = [g + (None, k & 1, o, (rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(0.2, 1.8), rng.uniform(-0.5, 0.5)))
              for k, (g, o) in enumerate(zip(geo, orders))]
    comp = _compose(vflip=True, jitter=(0.8, 0.8, 0.8, 0.5))
    _check(comp, imgs, lbls, params)
    # a factor of exactly 0 (the degenerate image) and of exactly 1 (the image), for each blend; hue 0
    exact = [geo[0] + (None, 0, (B, C, S), (0.0, 1.0, 1.0, None)), geo[1] + (None, 0, (C, B, S), (1.0, 0.0, 1.0, None)),
             geo[2] + (None, 1, (S, B, C, H), (1.0, 1.0, 0.0, 0.0)), geo[3] + (None, 0, (C, S), (None, 0.0, 0.0, None))]
    out, _ = _check(comp, imgs[:4], lbls[:4], exact)
    assert len(torch.unique(out[1])) == 3                                  # contrast 0: one grey level per channel


def test_contrast_mean_depends_on_the_ops_before_it():
    imgs, lbls = _tiles(SOURCES, 5)
    geo = _geometry(SOURCES, CROP, 13)
    f = (1.7, 0.5, 0.3, None)
    comp = _compose(jitter=(0.8, 0.8, 0.8, 0))
    first, _ = _check(comp, imgs, lbls, [g + (None, 0, (B, C), f) for g in geo])       # brightness, then contrast
    after, _ = _check(comp, imgs, lbls, [g + (None, 0, (C, B), f) for g in geo])
    assert not torch.equal(first, after)
    _check(comp, imgs, lbls, [g + (None, 0, (S, B, C), f) for g in geo])


def test_full_size_sample_sums_grey_over_many_workgroups():
    crop = (513, 513)
    imgs, lbls = _tiles([(513, 513)], 6)
    geo = _geometry([(513, 513)], crop, 14)
    comp = _compose(rotate=30, vflip=True, jitter=(0.5, 0.5, 0.5, 0.2), crop=crop)
    _check(comp, imgs, lbls, [geo[0] + (17.0, 1, (B, C, H, S), (1.2, 0.6, 1.4, -0.2))], crop=crop)


# ---- 3. the two host paths --------------------------------------------------------------------------------------------
STORE_SIZES = [(40, 56), (97, 129), (41, 57), (64, 48), (65, 65), (56, 40)]


def _store(tmp_path):
    from iswm_amd.datasets import BinarySegmentation, DeviceTileStore
    _make_split(str(tmp_path), "train", ["t%03d.png" % i for i in range(len(STORE_SIZES))], STORE_SIZES, seed=2)
    return DeviceTileStore(BinarySegmentation(str(tmp_path), "train"), dev(), workers=2)


def test_batch_resident_equals_batch(tmp_path):
    store = _store(tmp_path)
    comp = _compose(rotate=45, vflip=True, jitter=(0.4, 0.4, 0.4, 0.1))
    idx = [1, 0, 4, 3, 5, 2]
    geo = _geometry([STORE_SIZES[i] for i in idx], CROP, 15)
    none = (None,) * 4
    params = [geo[0] + (12.5, 1, (H, C, B, S), (0.8, 1.2, 0.9, 0.05)), geo[1] + (None, 0, (), none), geo[2] + (90.0, 1, (C,), (None, 0.7, None, None)),
              geo[3], geo[4] + (0.0, 0, (B,), (1.3, None, None, None)), geo[5] + (-45.0, 0, (S, H), (None, None, 1.4, -0.1))]
    want, want_l = comp.batch(*store.tiles(idx), params=params)
    got, got_l = comp.batch_resident(store, idx, params=params)
    assert torch.equal(got, want) and torch.equal(got_l, want_l)
    imgs, lbls = store.tiles(idx)
    for b in (0, 2, 5):                                                    # and both are the restatement's
        t, lab = R.chain(imgs[b].cpu().numpy(), lbls[b].cpu().numpy(), params[b], CROP, MEAN, STD)
        assert torch.equal(got[b].cpu(), t) and torch.equal(got_l[b].cpu(), lab)
    for seed in (5, 6):                                                    # the random path: the same draws in the same order
        random.seed(seed)
        want, want_l = comp.batch(*store.tiles(idx))
        after = random.random()
        random.seed(seed)
        got, got_l = comp.batch_resident(store, idx)
        assert random.random() == after
        assert torch.equal(got, want) and torch.equal(got_l, want_l)


def test_neutral_extras_give_the_plain_kernels_bits(monkeypatch):
    from iswm_amd.utils import ext_transforms as et
    names, real_call = [], et.call
    monkeypatch.setattr(et, "call", lambda name, *a: (names.append(name), real_call(name, *a))[1])
    imgs, lbls = _tiles(SOURCES + [(100, 70)], 7)
    geo = _geometry(SOURCES + [(100, 70)], CROP, 16)
    d = dev()
    timgs, tlbls = [torch.from_numpy(a).to(d) for a in imgs], [torch.from_numpy(a).to(d) for a in lbls]
    plain = _compose()
    assert not plain.extended
    want, want_l = plain.batch(timgs, tlbls, params=geo)
    assert names == ["iswm_augment_batch"]                                 # the untouched pipeline: the one call it always made
    ext = _compose(rotate=10, vflip=True, jitter=(0.4, 0.4, 0.4, 0.1))
    got, got_l = ext.batch(timgs, tlbls, params=geo)                       # 6-tuples: no rotation, no flip, no op
    assert names == ["iswm_augment_batch", "iswm_augment_batch_ex"]        # nothing rotates: no iswm_aug_rotate either
    assert torch.equal(got, want) and torch.equal(got_l, want_l)
    neutral = [g + (None, 0, (), (None,) * 4) for g in geo]
    got, got_l = ext.batch(timgs, tlbls, params=neutral)
    assert torch.equal(got, want) and torch.equal(got_l, want_l)
    with pytest.raises(ValueError, match="extended parameters"):
        plain.batch(timgs, tlbls, params=neutral)


def test_random_path_equals_the_restatement_on_the_same_draws():
    imgs, lbls = _tiles(SOURCES, 9)
    d = dev()
    comp = _compose(rotate=25, vflip=True, jitter=(0.4, 0.3, 0.5, 0.2))
    random.seed(31)
    out, out_lbl = comp.batch([torch.from_numpy(a).to(d) for a in imgs], [torch.from_numpy(a).to(d) for a in lbls])
    random.seed(31)
    params = [comp.draw(h, w) for h, w in SOURCES]                         # test_augment_ext_cpu pins draw() to the replay
    assert all(len(p) == 10 and p[6] is not None and len(p[8]) == 4 for p in params)
    for b in range(3):
        t, lab = R.chain(imgs[b], lbls[b], params[b], CROP, MEAN, STD)
        assert torch.equal(out[b].cpu(), t) and torch.equal(out_lbl[b].cpu(), lab)


# ---- 4. no host stall --------------------------------------------------------------------------------------------------
def test_batch_resident_with_all_transforms_returns_while_the_device_is_busy(tmp_path):
    """tests/test_dataset_gpu.py's event method: device work is queued in front of `ring_depth` calls; they must return
    while that work's end event is still pending.  A condition, not a timing."""
    depth = 4
    store = _store(tmp_path)
    comp = _compose(rotate=30, vflip=True, jitter=(0.4, 0.4, 0.4, 0.1), depth=depth)
    idx = [1, 0, 4, 3, 5, 2, 1, 4]
    d = dev()
    x = torch.randn(4096, 4096, device=d)
    y = torch.empty_like(x)

    def busy(n):
        for _ in range(n):
            torch.mm(x, x, out=y)

    def run(n_busy):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        busy(n_busy)
        b.record()
        t0 = time.perf_counter()
        outs = [comp.batch_resident(store, idx) for _ in range(depth)]
        early = not b.query()
        host_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return early, a.elapsed_time(b), host_ms, outs

    busy(3)
    for _ in range(2):                                            # warm-up: allocator blocks, pinned ring, code objects
        run(1)
    _, ms1, host_ms, _ = run(4)
    n_busy = max(8, int(math.ceil(8 * max(host_ms, 0.5) / (ms1 / 4))))     # queued work ~8x the host time of the calls
    random.seed(3)
    early, busy_ms, host_ms, outs = run(n_busy)
    print("batch_resident (all transforms) x%d: host %.3f ms, queued device work %.3f ms (%d matmuls), returned early: %s"
          % (depth, host_ms, busy_ms, n_busy, early))
    assert busy_ms > 3 * host_ms, "the queued work (%.3f ms) is not several times the host time (%.3f ms)" % (busy_ms, host_ms)
    assert early, "batch_resident waited for the device (%.3f ms of queued work, %.3f ms on the host)" % (busy_ms, host_ms)
    random.seed(3)
    for got, got_l in outs:                                       # and what it enqueued behind the busy device is right
        want, want_l = comp.batch(*store.tiles(idx))
        assert torch.equal(got, want) and torch.equal(got_l, want_l)
