"""Real image / mask folders, decoded once and kept on the GPU.

``BinarySegmentation`` stands where the reference's ``datasets.BinarySegmentation`` (train.py:14,371-380) would:
that class is not in the reference tree, so this one is written from the file convention the reference uses where
it does read tiles (evaluate_quantization.py:36-80, tensorrt_tools/predict_trt.py:50,178-179) and that this
package's ``evaluate_quantization`` already follows -- ``imgs/<base><ext>`` paired with ``masks/<base>_mask<ext>``,
the mask read as mode ``L``, every non-zero pixel class 1 -- one level up: ``<root>/{train,val}/{imgs,masks}``.

``DeviceTileStore`` decodes a whole split once, packs it into two uint8 arenas in device memory and binarises the
masks there (csrc/dataset.hip).  ``ExtCompose.batch_resident`` augments straight out of the arenas; ``batches``
yields normalised validation batches.  Layout and exactness: DESIGN.md section 11.
"""
import ctypes
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from ._lib import call

IMAGE_EXTENSIONS = ('.png', '.jpg', '.jpeg')
ALIGN = 16                      # every tile starts at a multiple of 16 bytes in its arena
MAX_DECODE_WORKERS = 16
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _float3(v):
    return (ctypes.c_float * 3)(*[float(np.float32(x)) for x in v])


class BinarySegmentation(object):
    """``<root>/<split>/imgs/<base><ext>`` with ``<root>/<split>/masks/<base>_mask<ext>`` (.png / .jpg / .jpeg, any
    letter case), sorted by file name.  ``__getitem__`` returns the RAW pair -- uint8 [H,W,3] RGB and uint8 [H,W]
    mode-L mask, not yet binarised (DeviceTileStore does that on the device); ``transform`` is kept for the
    reference's constructor shape and applied to the pair when given.

    A missing mask is an error that lists every missing file.  The reference's evaluation class substitutes a blank
    mask with a warning; in training that would silently teach "no wave" for the frame, so it is refused here.  A
    mask whose size differs from its image's is an error too (found when the headers are read, at construction)."""

    def __init__(self, root, split='train', transform=None):
        self.root, self.split, self.transform = root, split, transform
        self.img_dir = os.path.join(root, split, 'imgs')
        self.mask_dir = os.path.join(root, split, 'masks')
        if not os.path.isdir(self.img_dir):
            raise FileNotFoundError("no image folder %s (expected <data_root>/{train,val}/{imgs,masks})" % self.img_dir)
        self.images = sorted(f for f in os.listdir(self.img_dir) if f.lower().endswith(IMAGE_EXTENSIONS))
        if not self.images:
            raise FileNotFoundError("no .png / .jpg / .jpeg files in %s" % self.img_dir)
        self.masks = []
        for f in self.images:
            base, ext = os.path.splitext(f)
            self.masks.append(base + '_mask' + ext)
        missing = [m for m in self.masks if not os.path.isfile(os.path.join(self.mask_dir, m))]
        if missing:
            raise FileNotFoundError("%d of %d masks are missing in %s: %s" %
                                    (len(missing), len(self.masks), self.mask_dir, ", ".join(missing)))
        from PIL import Image
        self.sizes, wrong = [], []
        for f, m in zip(self.images, self.masks):
            with Image.open(os.path.join(self.img_dir, f)) as im, Image.open(os.path.join(self.mask_dir, m)) as mk:
                if im.size != mk.size:
                    wrong.append("%s %dx%d vs %s %dx%d" % (f, im.size[1], im.size[0], m, mk.size[1], mk.size[0]))
                self.sizes.append((im.size[1], im.size[0]))                 # (h, w)
        if wrong:
            raise ValueError("%d masks differ in size (HxW) from their images: %s" % (len(wrong), "; ".join(wrong)))

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        from PIL import Image
        with Image.open(os.path.join(self.img_dir, self.images[i])) as im:
            img = np.array(im.convert('RGB'), dtype=np.uint8)
        with Image.open(os.path.join(self.mask_dir, self.masks[i])) as mk:
            mask = np.array(mk.convert('L'), dtype=np.uint8)
        if self.transform is not None:
            return self.transform(img, mask)
        return img, mask

    @staticmethod
    def decode_target(mask):
        return (np.asarray(mask) * 255).astype(np.uint8)


def _align(n):
    return (n + ALIGN - 1) // ALIGN * ALIGN


class _ValBatches(object):
    """iterable of (float32 [B,3,H,W], uint8 [B,H,W]) device batches over a store in name order; `.dataset.images`
    is what train.validate_sequence sorts by"""

    def __init__(self, store, batch_size, mean, std):
        self.dataset = store
        self.store, self.batch_size = store, max(1, int(batch_size))
        self.mean, self.std = _float3(mean), _float3(std)

    def groups(self):
        """runs of consecutive tiles of one size, at most batch_size long: [(first, count)]"""
        out, meta, i = [], self.store.meta, 0
        while i < len(meta):
            n = 1
            while n < self.batch_size and i + n < len(meta) and meta[i + n][2:] == meta[i][2:]:
                n += 1
            out.append((i, n))
            i += n
        return out

    def __len__(self):
        return len(self.groups())

    def __iter__(self):
        for first, n in self.groups():
            yield self.store.gather(first, n, self.mean, self.std)


class DeviceTileStore(object):
    """Every (image, mask) pair of `dataset` decoded once (thread pool; PIL releases the GIL while it decodes) and
    kept in device memory: one uint8 arena of HWC RGB images, one of HW masks, each uploaded with a single copy from
    pinned memory; tile i lives at `meta[i] = (img_off, lbl_off, h, w)`, offsets multiples of 16, tiles may differ in
    size.  The masks are binarised in place on the device (iswm_label_prepare); `pixel_counts` = (n(0), n(1)) over
    the real pixels.  `max_share` is the share of the device's FREE memory the two arenas may take."""

    def __init__(self, dataset, device, workers=4, max_share=0.5):
        self.device = torch.device(device)
        if self.device.type != 'cuda':
            raise ValueError("DeviceTileStore keeps the tiles on a GPU (got device %s)" % (device,))
        self.images = list(dataset.images)
        self.decode_target = dataset.decode_target
        n = len(dataset)
        workers = max(1, min(int(workers), MAX_DECODE_WORKERS, n))
        with ThreadPoolExecutor(max_workers=workers) as ex:
            pairs = list(ex.map(dataset.__getitem__, range(n)))
        self.meta, img_off, lbl_off = [], 0, 0
        for i, (img, mask) in enumerate(pairs):
            if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3 or mask.dtype != np.uint8 or \
                    mask.shape != img.shape[:2]:
                raise ValueError("tile %d (%s): expected uint8 [H,W,3] and uint8 [H,W], got %s %s and %s %s" %
                                 (i, self.images[i], img.shape, img.dtype, mask.shape, mask.dtype))
            h, w = int(img.shape[0]), int(img.shape[1])
            self.meta.append((img_off, lbl_off, h, w))
            img_off, lbl_off = img_off + _align(h * w * 3), lbl_off + _align(h * w)
        self.nbytes = img_off + lbl_off
        free, _total = torch.cuda.mem_get_info(self.device)
        if self.nbytes > max_share * free:
            raise MemoryError("the data set needs %d bytes on the device; %.0f %% of the %d bytes free there is %d "
                              "(streaming from the host is not built)" %
                              (self.nbytes, 100.0 * max_share, free, int(max_share * free)))
        himg = torch.zeros(img_off, dtype=torch.uint8).pin_memory()
        hlbl = torch.zeros(lbl_off, dtype=torch.uint8).pin_memory()           # alignment padding stays 0
        nimg, nlbl = himg.numpy(), hlbl.numpy()
        for (io, lo, h, w), (img, mask) in zip(self.meta, pairs):
            nimg[io:io + h * w * 3] = img.reshape(-1)
            nlbl[lo:lo + h * w] = mask.reshape(-1)
        del pairs
        with torch.cuda.device(self.device):
            self.img_arena = himg.to(self.device, non_blocking=True)
            self.lbl_arena = hlbl.to(self.device, non_blocking=True)
            off = torch.tensor([[m[0], m[1]] for m in self.meta], dtype=torch.int64).pin_memory()
            self.offsets = off.to(self.device, non_blocking=True)                # [n, 2], read by iswm_gather_normalize
            lib = _lib.load()
            counts = torch.zeros(2, dtype=torch.int64, device=self.device)
            ws_bytes = lib.iswm_label_prepare_workspace(lbl_off)
            ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=self.device)
            call("iswm_label_prepare", self.lbl_arena.data_ptr(), lbl_off, counts.data_ptr(), ws.data_ptr(), ws_bytes,
                 _stream())
            n0, n1 = (int(v) for v in counts.cpu())                                # one read-back; also ends the uploads
        padding = lbl_off - sum(h * w for _, _, h, w in self.meta)
        self.pixel_counts = (n0 - padding, n1)

    def __len__(self):
        return len(self.meta)

    @property
    def uniform_size(self):
        return len(set(m[2:] for m in self.meta)) == 1

    def tiles(self, indices):
        """(uint8 [h,w,3] image views, uint8 [h,w] label views) of the arenas"""
        imgs, lbls = [], []
        for i in indices:
            io, lo, h, w = self.meta[int(i)]
            imgs.append(self.img_arena[io:io + h * w * 3].view(h, w, 3))
            lbls.append(self.lbl_arena[lo:lo + h * w].view(h, w))
        return imgs, lbls

    def gather(self, first, count, mean, std, offsets=None):
        """`count` consecutive equal-sized tiles from `first` on (or the tiles whose (img_off, lbl_off) rows are the
        int64 device tensor `offsets`, all of tile `first`'s size) -> (float32 [count,3,h,w], uint8 [count,h,w])"""
        _, _, h, w = self.meta[first]
        if offsets is None:
            if any(m[2:] != (h, w) for m in self.meta[first:first + count]) or first + count > len(self.meta):
                raise ValueError("tiles %d..%d are not all %dx%d" % (first, first + count - 1, h, w))
            offsets = self.offsets[first:first + count]
        mean = mean if isinstance(mean, ctypes.Array) else _float3(mean)
        std = std if isinstance(std, ctypes.Array) else _float3(std)
        with torch.cuda.device(self.device):
            out = torch.empty((count, 3, h, w), dtype=torch.float32, device=self.device)
            lbl = torch.empty((count, h, w), dtype=torch.uint8, device=self.device)
            call("iswm_gather_normalize", self.img_arena.data_ptr(), self.lbl_arena.data_ptr(), offsets.data_ptr(), count,
                 h, w, mean, std, out.data_ptr(), lbl.data_ptr(), _stream())
        return out, lbl

    def batches(self, batch_size, mean=IMAGENET_MEAN, std=IMAGENET_STD):
        """validation loader: name order, consecutive tiles of equal size batched up to batch_size"""
        return _ValBatches(self, batch_size, mean, std)
