"""Input-path timing on one GPU: the resident tile store against the parent path.

    python tools/input_time.py [--out profiles/input_time.txt] [--kernels-only]

Tiles are generated into a temporary directory (PNG, blob masks), so the files are decoded as a user's would be.

1. per batch of 16, crop 513 from 513^2 tiles and crop 200 from 200^2 tiles: host time per call (perf_counter around
   the call, device idle at its start) and device-event window of ExtCompose.batch (the parent path: torch.cat of the
   tiles, numpy tables, two blocking uploads) and of ExtCompose.batch_resident, alternated in one process, warm-up
   excluded, median and range; plus iswm_gather_normalize of 16 tiles; plus batch_resident with rotation only, colour
   jitter without and with contrast, and rotation + vertical flip + jitter;
2. training images/s of deeplabv3plus_resnet101 os16, 16 x 513^2: (a) one fixed resident batch (what bench.py times),
   (b) batch_resident from the store, (b') the same with rotation + vertical flip + jitter, (c) the parent's --device_augment loop on the same tiles (DataLoader of uint8
   tiles, 2 workers started before the timed window, .to(device), ExtCompose.batch), alternated, three rounds each;
3. one-off cost: decode + upload of 2000 tiles of 200^2 with 4 threads, arena size.

--kernels-only runs a short part 1 alone, for
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/input_time.py --kernels-only
"""
import argparse
import os
import random
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from iswm_amd.datasets import BinarySegmentation, DeviceTileStore  # noqa: E402
from iswm_amd.utils import ext_transforms as et  # noqa: E402

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]


def make_tiles(root, split, n, size, seed):
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:size, 0:size]
    for sub in ("imgs", "masks"):
        os.makedirs(os.path.join(root, split, sub), exist_ok=True)
    for k in range(n):
        mask = np.zeros((size, size), np.uint8)
        for _ in range(4):
            cy, cx, r = rng.integers(0, size), rng.integers(0, size), rng.integers(size // 16, size // 5)
            mask[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = 255
        base = rng.integers(0, 256, (size // 8 + 2, size // 8 + 2, 3), dtype=np.uint8)
        img = np.asarray(Image.fromarray(base).resize((size, size), Image.BILINEAR))
        Image.fromarray(img).save(os.path.join(root, split, "imgs", "f%05d.png" % k))
        Image.fromarray(mask).save(os.path.join(root, split, "masks", "f%05d_mask.png" % k))


def compose(crop, rotate=None, vflip=False, jitter=None):
    chain = [et.ExtRandomRotation(rotate)] if rotate is not None else []
    chain += [et.ExtRandomScale((0.5, 2.0)), et.ExtRandomCrop(size=(crop, crop), pad_if_needed=True),
              et.ExtRandomHorizontalFlip()]
    if vflip:
        chain.append(et.ExtRandomVerticalFlip())
    if jitter is not None:
        chain.append(et.ExtColorJitter(*jitter))
    return et.ExtCompose(chain + [et.ExtToTensor(), et.ExtNormalize(MEAN, STD)])


# the arms of DESIGN.md section 15: batch_resident with the transforms the plain pipeline lacks
EXT_ARMS = (("rotation only", dict(rotate=30)),
            ("jitter without contrast", dict(jitter=(0.4, 0, 0.4, 0.1))),
            ("jitter with contrast", dict(jitter=(0.4, 0.4, 0.4, 0.1))),
            ("all on", dict(rotate=30, vflip=True, jitter=(0.4, 0.4, 0.4, 0.1))))


def one_call(fn):
    """(host ms, device-event ms) of one call that starts on an idle device"""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t0 = time.perf_counter()
    fn()
    host = (time.perf_counter() - t0) * 1e3
    b.record()
    b.synchronize()
    return host, a.elapsed_time(b)


def spread(v):
    return "%8.3f (%.3f - %.3f)" % (statistics.median(v), min(v), max(v))


class HostTiles(torch.utils.data.Dataset):
    """the decoded tiles in host memory, as the parent's --device_augment DataLoader hands them over"""

    def __init__(self, ds, repeat):
        self.pairs = [ds[i] for i in range(len(ds))]
        self.repeat = repeat                 # one epoch covers the whole timed window: the workers start once

    def __len__(self):
        return len(self.pairs) * self.repeat

    def __getitem__(self, i):
        img, mask = self.pairs[i % len(self.pairs)]
        return torch.from_numpy(img), torch.from_numpy((mask > 0).astype(np.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    dev = torch.device("cuda")
    say("input_time: %s, batch 16" % torch.cuda.get_device_name())
    reps = 5 if args.kernels_only else 24
    with tempfile.TemporaryDirectory() as tmp:
        stores = {}
        say("1. per batch of 16: host ms per call | device-event window ms; median (min - max) of %d alternated calls" % reps)
        for size in (513, 200):
            root = os.path.join(tmp, "d%d" % size)
            make_tiles(root, "train", 64, size, size)
            ds = BinarySegmentation(root, "train")
            store = stores[size] = (ds, DeviceTileStore(ds, dev, workers=4))
            store = store[1]
            comp = compose(size)
            random.seed(1)
            idx = list(range(16))
            parent = lambda: comp.batch(*store.tiles(idx))
            resident = lambda: comp.batch_resident(store, idx)
            gather = lambda: store.gather(0, 16, MEAN, STD)
            arms = [("parent", parent), ("resident", resident), ("gather", gather)]
            labels = [("parent", "ExtCompose.batch (parent path)"), ("resident", "batch_resident"),
                      ("gather", "gather_normalize (validation)")]
            for arm, kw in EXT_ARMS:
                arms.append((arm, lambda c=compose(size, **kw): c.batch_resident(store, idx)))
                labels.append((arm, "batch_resident, " + arm))
            for _ in range(4):
                for _name, fn in arms:
                    fn()
            res = {name: [] for name, _ in arms}
            for _ in range(reps):
                for name, fn in arms:
                    res[name].append(one_call(fn))
            for name, label in labels:
                say("   %d^2 crop %d  %-30s host %s | device %s" % (size, size, label, spread([r[0] for r in res[name]]),
                                                                 spread([r[1] for r in res[name]])))
        if args.kernels_only:
            return

        # 2. training images/s
        from iswm_amd.network import modeling
        from iswm_amd.optim import FusedSGD
        from iswm_amd.utils.loss import CrossEntropyLoss
        torch.manual_seed(0)
        model = modeling.deeplabv3plus_resnet101(num_classes=2, output_stride=16).to(dev).train()
        opt = FusedSGD(model.parameters(), momentum=0.9, weight_decay=1e-4, nesterov=True)
        crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]), ignore_index=255).to(dev)
        ds, store = stores[513]
        comp = compose(513)
        B, steps, warm = 16, 12, 3

        def train_steps(batches):
            n, t0 = 0, None
            for images, labels in batches:
                if n == warm:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                loss = crit(model(images), labels)
                opt.zero_grad()
                loss.backward()
                opt.step()
                n += 1
                if n == warm + steps:
                    break
            torch.cuda.synchronize()
            return B * steps / (time.perf_counter() - t0)

        fixed = comp.batch_resident(store, list(range(B)))
        order = [[(s * B + k) % len(store) for k in range(B)] for s in range(warm + steps)]

        def loop_fixed():
            return train_steps(fixed for _ in range(warm + steps))

        def loop_resident():
            return train_steps(comp.batch_resident(store, idx) for idx in order)

        host = HostTiles(ds, repeat=8)

        def loop_parent():
            loader = torch.utils.data.DataLoader(host, batch_size=B, shuffle=True, num_workers=2, drop_last=True)

            def gen():
                while True:
                    for images, labels in loader:
                        yield comp.batch(list(images.to(dev, non_blocking=True)), list(labels.to(dev, non_blocking=True)))
            return train_steps(gen())

        comp_all = compose(513, **dict(EXT_ARMS)["all on"])

        def loop_resident_all():
            return train_steps(comp_all.batch_resident(store, idx) for idx in order)

        say("2. training images/s, deeplabv3plus_resnet101 os16, 16 x 513^2, %d steps after %d warm-up, alternated:" % (steps, warm))
        loop_fixed()
        rates = {"fixed": [], "resident": [], "resident_all": [], "parent": []}
        for _ in range(3):
            rates["fixed"].append(loop_fixed())
            rates["resident"].append(loop_resident())
            rates["resident_all"].append(loop_resident_all())
            rates["parent"].append(loop_parent())
        for name, label in (("fixed", "one fixed resident batch (no input path)"), ("resident", "resident store + batch_resident"),
                            ("resident_all", "resident store + batch_resident, rotation + vflip + jitter"),
                            ("parent", "parent --device_augment loop (DataLoader, 2 workers + batch)")):
            say("   %-62s %s" % (label, "  ".join("%6.1f" % r for r in rates[name])))
        del model, opt

        # 3. one-off cost
        root = os.path.join(tmp, "big")
        t0 = time.perf_counter()
        make_tiles(root, "train", 2000, 200, 9)
        t_gen = time.perf_counter() - t0
        ds = BinarySegmentation(root, "train")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        big = DeviceTileStore(ds, dev, workers=4)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        say("3. 2000 tiles of 200^2 (generated in %.1f s): decode + pack + upload + label_prepare with 4 threads %.2f s, "
            "arenas %.1f MB, pixel counts %r" % (t_gen, dt, big.nbytes / 1e6, big.pixel_counts))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
