"""Training entry point -- runnable counterpart of the reference's train.py for the accelerated path.

Same command-line flags (get_argparser, train.py:272-351), same step sequence (train.py:1029-1055),
same optimizer / scheduler / criterion construction (train.py:421-459), same checkpoint dictionary
(train.py:567-582, atomic .tmp + os.replace) and resume logic (train.py:972-1016).  Differences, all
forced by the reference not being runnable as shipped:

  * data: ``--dataset synthetic`` (default) generates seeded tiles with the reference's
    ``(image float32 [3,H,W], label uint8 [H,W])`` tuple contract, ``.images`` list and
    ``decode_target``; ``--dataset binary`` reads ``<data_root>/{train,val}/{imgs,masks}`` (datasets.py: the
    reference's ``BinarySegmentation`` is not in its tree, the file convention is), decodes both splits once into
    device memory and augments / validates from there;
  * ``--model`` is honoured (the reference always builds resnet50, train.py:412-419);
  * ``--loss_type`` defaults to IWce_loss (the reference's default 'cross_entropy' is not in its own
    choices and yields ``None``);
  * ``--lr`` still only feeds the scheduler's eta_min and the optimizers run at torch's default lr,
    exactly as the reference does (train.py:421-452) -- reproduced on purpose, see SURVEY F5(e);
  * multi-GPU is one process per GPU (``torchrun --nproc-per-node N -m iswm_amd.train ...``) with RCCL
    gradient all-reduce instead of nn.DataParallel (train.py:970);
  * MLflow logging is used when the package is importable, skipped otherwise; the loss is read back
    every ``--print_interval`` steps instead of every step (train.py:1051 syncs each iteration);
  * ``--save_val_results`` defaults to False (the reference: True, train.py:297).  With it, every new best
    checkpoint -- and a ``--test_only`` run, into ``test_only_iter_<itr>_score_<weighted>`` -- writes the validation
    images of val_results.save_validation_results under ``--val_results_dir``; ``--save_confidence_map`` adds the
    confidence map.  Without the flag nothing is written there;
  * ``--clip_grad_norm`` and ``--ema_decay`` (both off by default) run inside the fused optimizer step (DESIGN.md
    section 18).  With EMA on, validation, best-model selection and the validation images use the EMA weights, the
    checkpoint gains ``"ema_state"`` (``"model_state"`` stays the live weights) and ``--test_only --use_ema`` scores it;
  * ``--ohem_thresh P`` (off by default) averages the CE over the hard pixels only: those predicted below P and at least
    ``--ohem_min_kept`` per process, selected on the device;
  * ``--lovasz_weight W`` (off by default) adds W x the per-image Lovasz-Softmax term to ``--ce_weight`` x the CE, on a
    segmented radix sort on the device;
  * ``--distill_ckpt PATH --distill_model NAME`` (off by default) trains against a frozen teacher: the checkpoint is loaded
    strictly into NAME, runs in eval mode without gradients on every augmented batch, and the criterion becomes
    ``--ce_weight`` x the CE plus ``--distill_weight`` x T^2 x KL(teacher || student) at ``--distill_temperature`` T (DESIGN.md
    section 22).  The teacher never enters the optimizer, the gradient all-reduce or the checkpoint;
  * ``--boundary_weight W`` (off by default) adds W x the boundary loss (Kervadec et al. 2019) to ``--ce_weight`` x the CE: the
    mean of probability x signed Euclidean distance to the ground-truth contour, on a distance map built on the device from
    every augmented batch's labels; ``--boundary_clip D`` clamps the distance, ``--boundary_ramp_itrs N`` raises the factor
    linearly from 0 over the first N iterations.
"""
import argparse
import contextlib
import math
import os
import random
import time
from datetime import datetime

import numpy as np
import torch
import torch.distributed as dist
from torch.utils import data

from . import network, ops
from .optim import FusedAdam, FusedAdamW, FusedSGD, ema_model_state
from .parallel import DistributedDataParallelHIP
from .utils.loss import (BoundaryLoss, CrossEntropyLoss, DiceLoss, DistillationLoss, LovaszSoftmaxLoss, OhemCrossEntropyLoss,
                         TverskyLoss, calculate_class_weights, calculate_class_weights_resident)
from .val_results import save_validation_results


class _ArgParser(argparse.ArgumentParser):
    """refuses, at parse time, the combinations of the criterion options that no criterion can be built from"""

    def parse_known_args(self, args=None, namespace=None):
        opts, rest = super().parse_known_args(args, namespace)
        if not (math.isfinite(opts.lovasz_weight) and opts.lovasz_weight >= 0):
            self.error("--lovasz_weight must be finite and not negative (0 = off)")
        if not (math.isfinite(opts.boundary_weight) and opts.boundary_weight >= 0):
            self.error("--boundary_weight must be finite and not negative (0 = off)")
        if opts.overlap_loss == 'none' and opts.lovasz_weight == 0 and opts.ce_weight == 0 and opts.distill_ckpt is None and \
                opts.boundary_weight == 0:
            self.error("--ce_weight 0 with --overlap_loss none leaves no loss term")
        if opts.lovasz_weight > 0 and opts.overlap_loss != 'none':
            self.error("--lovasz_weight with --overlap_loss %s: one region term at a time" % opts.overlap_loss)
        if opts.lovasz_weight > 0 and opts.ohem_thresh > 0:
            self.error("--lovasz_weight with --ohem_thresh: hard-pixel mining inside the combined criterion is not supported")
        if opts.ce_weight < 0 or opts.overlap_weight < 0:
            self.error("--ce_weight and --overlap_weight must not be negative")
        if not opts.overlap_smooth > 0:
            self.error("--overlap_smooth must be positive")
        if opts.tversky_alpha < 0 or opts.tversky_beta < 0 or not opts.tversky_gamma > 0:
            self.error("--tversky_alpha and --tversky_beta must not be negative, --tversky_gamma must be positive")
        if not (math.isfinite(opts.clip_grad_norm) and opts.clip_grad_norm >= 0):
            self.error("--clip_grad_norm must be a finite norm >= 0 (0 = off)")
        if not 0 <= opts.ema_decay < 1:
            self.error("--ema_decay must lie in [0, 1) (0 = off)")
        if not 0 <= opts.ohem_thresh <= 1:
            self.error("--ohem_thresh must lie in [0, 1] (0 = off, 1 = every valid pixel)")
        if opts.ohem_min_kept < 0:
            self.error("--ohem_min_kept must not be negative")
        if opts.ohem_thresh > 0 and opts.overlap_loss != 'none':
            self.error("--ohem_thresh with --overlap_loss %s: hard-pixel mining inside the combined criterion is not "
                       "supported" % opts.overlap_loss)
        if opts.use_ema and not (opts.test_only and opts.ckpt):
            self.error("--use_ema evaluates the EMA weights of a checkpoint: it needs --test_only and --ckpt")
        self._check_distill(opts)
        self._check_boundary(opts)
        self._check_boundary_metrics(opts)
        return opts, rest

    def _check_boundary_metrics(self, opts):
        """--boundary_tolerance and --boundary_percentile: given only with --val_boundary_metrics; left out, they take 2 and 95"""
        given = [flag for flag, value in (("--boundary_tolerance", opts.boundary_tolerance),
                                          ("--boundary_percentile", opts.boundary_percentile)) if value is not None]
        if not opts.val_boundary_metrics:
            if given:
                self.error("%s without --val_boundary_metrics: there is no boundary metric" % ", ".join(given))
            return
        if opts.boundary_tolerance is None:
            opts.boundary_tolerance = 2
        if opts.boundary_percentile is None:
            opts.boundary_percentile = 95
        if not 0 <= opts.boundary_tolerance <= ops.EDT_MAX_SIDE:
            self.error("--boundary_tolerance must lie in [0, %d] pixels" % ops.EDT_MAX_SIDE)
        if not 1 <= opts.boundary_percentile <= 100:
            self.error("--boundary_percentile must lie in [1, 100]")

    def _check_boundary(self, opts):
        """the --boundary_* options: the term goes with the plain weighted CE of a training run only, and the clamp and the
        ramp are given only with it"""
        if not (math.isfinite(opts.boundary_clip) and opts.boundary_clip >= 0):
            self.error("--boundary_clip must be a finite distance >= 0 (0 = no clamp)")
        if opts.boundary_ramp_itrs < 0:
            self.error("--boundary_ramp_itrs must not be negative")
        if opts.boundary_weight == 0:
            given = [flag for flag, on in (("--boundary_clip", opts.boundary_clip > 0),
                                           ("--boundary_ramp_itrs", opts.boundary_ramp_itrs > 0)) if on]
            if given:
                self.error("%s without --boundary_weight: there is no boundary term" % ", ".join(given))
            return
        for flag, on in (("--overlap_loss %s" % opts.overlap_loss, opts.overlap_loss != 'none'),
                         ("--lovasz_weight", opts.lovasz_weight > 0), ("--ohem_thresh", opts.ohem_thresh > 0),
                         ("--distill_ckpt", opts.distill_ckpt is not None), ("--test_only", opts.test_only)):
            if on:
                self.error("--boundary_weight with %s: the boundary term goes with the plain CE term of a training run only" % flag)

    def _check_distill(self, opts):
        """the --distill_* options: given only with --distill_ckpt, and with no criterion or mode that has no teacher; the
        options left out then take their defaults"""
        given = [flag for flag, value in (("--distill_model", opts.distill_model),
                                          ("--distill_output_stride", opts.distill_output_stride),
                                          ("--distill_use_ema", opts.distill_use_ema or None),
                                          ("--distill_weight", opts.distill_weight),
                                          ("--distill_temperature", opts.distill_temperature)) if value is not None]
        if opts.distill_ckpt is None:
            if given:
                self.error("%s without --distill_ckpt: there is no teacher" % ", ".join(given))
        else:
            if opts.distill_model is None:
                self.error("--distill_ckpt needs --distill_model: the architecture the checkpoint is loaded into")
            for flag, on in (("--overlap_loss %s" % opts.overlap_loss, opts.overlap_loss != 'none'),
                             ("--lovasz_weight", opts.lovasz_weight > 0), ("--ohem_thresh", opts.ohem_thresh > 0),
                             ("--test_only", opts.test_only)):
                if on:
                    self.error("--distill_ckpt with %s: distillation goes with the plain CE term of a training run only" % flag)
        for name, default in (("distill_output_stride", 16), ("distill_weight", 1.0), ("distill_temperature", 1.0)):
            if getattr(opts, name) is None:
                setattr(opts, name, default)
        if not (math.isfinite(opts.distill_weight) and opts.distill_weight > 0):
            self.error("--distill_weight must be positive and finite")
        if not (math.isfinite(opts.distill_temperature) and opts.distill_temperature > 0):
            self.error("--distill_temperature must be positive and finite")


def get_argparser():
    parser = _ArgParser()
    parser.add_argument("--data_root", type=str, default='./datasets/data', help="path to Dataset")
    parser.add_argument("--dataset", type=str, default='synthetic', choices=['synthetic', 'binary'])
    parser.add_argument("--num_classes", type=int, default=None)
    available_models = sorted(name for name in network.modeling.__dict__ if name.islower() and
                              not (name.startswith("__") or name.startswith('_')) and
                              callable(network.modeling.__dict__[name]))
    parser.add_argument("--model", type=str, default='deeplabv3plus_resnet50', choices=available_models)
    parser.add_argument("--separable_conv", action='store_true', default=False)
    parser.add_argument("--output_stride", type=int, default=16, choices=[8, 16])
    parser.add_argument("--optimizer", type=str, default='adamw', choices=['sgd', 'adam', 'adamw'])
    parser.add_argument("--test_only", action='store_true', default=False)
    parser.add_argument("--save_val_results", action='store_true', default=False)
    parser.add_argument("--total_itrs", type=int, default=int(30e3))
    parser.add_argument("--lr", type=float, default=0.01)
    parser.add_argument("--step_size", type=int, default=10000)
    parser.add_argument("--crop_val", action='store_true', default=False)
    parser.add_argument("--batch_size", type=int, default=64, help="per-process batch size")
    parser.add_argument("--val_batch_size", type=int, default=4)
    parser.add_argument("--crop_size", type=int, default=513)
    parser.add_argument("--ckpt", default=None, type=str)
    parser.add_argument("--continue_training", action='store_true', default=False)
    parser.add_argument("--loss_type", type=str, default='IWce_loss', choices=['ce_loss', 'IWce_loss'])
    parser.add_argument("--gpu_id", type=str, default='0')
    parser.add_argument("--weight_decay", type=float, default=1e-4)
    parser.add_argument("--random_seed", type=int, default=1)
    parser.add_argument("--print_interval", type=int, default=10)
    parser.add_argument("--val_interval", type=int, default=500)
    parser.add_argument("--checkpoints_dir", type=str, default='checkpoints')
    parser.add_argument("--val_results_dir", type=str, default='val_results')
    parser.add_argument("--metrics_plots_dir", type=str, default='metrics_plots')
    parser.add_argument("--save_confidence_map", action='store_true', default=False)
    parser.add_argument("--sequence_length", type=int, default=7)
    parser.add_argument('--save_feature_maps', action='store_true', default=False)
    parser.add_argument('--feature_maps_dir', type=str)
    parser.add_argument("--training_stage", type=str, default='spatial',
                        choices=['spatial', 'temporal_p1', 'temporal_p2', 'temporal_p3', 'temporal_p4'])
    # additions
    parser.add_argument("--synthetic_len", type=int, default=256, help="tiles in the synthetic train split")
    parser.add_argument("--num_workers", type=int, default=2,
                        help="DataLoader worker processes of the train loader (the reference hard-codes 4, train.py:950); "
                             "with --dataset binary: the threads that decode the files once (1 to 16)")
    parser.add_argument("--device_augment", action='store_true', default=False,
                        help="run the reference's train_transform (random scale / crop / flip / normalise, "
                             "train.py:355-362) as one HIP kernel per batch on uint8 tiles")
    parser.add_argument("--aug_rotate", type=float, default=0.0, metavar="DEG",
                        help="device augmentation: ExtRandomRotation(DEG) (nearest, about the tile centre) before the random "
                             "scale; 0 = off.  Needs --device_augment or --dataset binary")
    parser.add_argument("--aug_vflip", action='store_true', default=False,
                        help="device augmentation: ExtRandomVerticalFlip() after the horizontal flip")
    parser.add_argument("--aug_color_jitter", type=str, default=None, metavar="B,C,S,H",
                        help="device augmentation: ExtColorJitter(brightness, contrast, saturation, hue) after the flips; "
                             "four non-negative numbers, H <= 0.5")
    parser.add_argument("--pretrained_backbone", action='store_true', default=False)
    parser.add_argument("--val_metrics", type=str, default='confusion', choices=['confusion', 'sequence'],
                        help="confusion: every validation frame counted into the confusion matrix, best checkpoint on "
                             "0.5*FG-IoU + 0.5*FG-F1; sequence: the reference's validate_and_save (train.py:620-745) -- "
                             "sliding windows of --sequence_length frames ordered by file name, the temporal / front / "
                             "region evaluators, best checkpoint by is_best_score")
    parser.add_argument("--overlap_loss", type=str, default='none', choices=['none', 'dice', 'tversky', 'focal_tversky'],
                        help="add a region-overlap term to the criterion: soft Dice, Tversky(alpha, beta) or focal-Tversky "
                             "(Tversky raised to --tversky_gamma); --loss_type still selects the CE term's class weights")
    parser.add_argument("--overlap_weight", type=float, default=1.0, help="factor of the overlap term")
    parser.add_argument("--ce_weight", type=float, default=1.0, help="factor of the CE term; 0 = overlap term only")
    parser.add_argument("--tversky_alpha", type=float, default=0.3, help="false-positive weight (tversky, focal_tversky)")
    parser.add_argument("--tversky_beta", type=float, default=0.7, help="false-negative weight (tversky, focal_tversky)")
    parser.add_argument("--tversky_gamma", type=float, default=0.75, help="exponent of focal_tversky")
    parser.add_argument("--overlap_smooth", type=float, default=1.0, help="smoothing constant of the overlap term (> 0)")
    parser.add_argument("--overlap_classes", type=str, default='foreground', choices=['foreground', 'all'],
                        help="classes the overlap term averages over: every class but 0, or all")
    parser.add_argument("--lovasz_weight", type=float, default=0.0, metavar="W",
                        help="add W x the per-image Lovasz-Softmax term (the Jaccard loss's convex extension, sorted on the "
                             "device) to --ce_weight x the CE; --overlap_classes selects its classes; 0 = off")
    parser.add_argument("--ohem_thresh", type=float, default=0.0, metavar="P",
                        help="online hard-example mining: average the CE over the pixels whose true-class probability is at "
                             "most P, and over at least the --ohem_min_kept hardest ones; --loss_type still selects the class "
                             "weights; 0 = off, 1 = every valid pixel")
    parser.add_argument("--ohem_min_kept", type=int, default=100000, metavar="N",
                        help="pixels per process that hard-example mining always keeps (the N x world-size hardest of the "
                             "global batch)")
    parser.add_argument("--clip_grad_norm", type=float, default=0.0, metavar="NORM",
                        help="clip the global L2 norm of the gradients to NORM inside the fused optimizer step "
                             "(torch.nn.utils.clip_grad_norm_'s factor; the stored gradients stay unclipped); 0 = off")
    parser.add_argument("--ema_decay", type=float, default=0.0, metavar="DECAY",
                        help="keep an exponential moving average of the weights inside the optimizer step and validate, select "
                             "and save the best checkpoint on it (BatchNorm statistics stay the live ones); 0 = off")
    parser.add_argument("--ema_no_warmup", action='store_true', default=False,
                        help="use DECAY from the first update instead of min(DECAY, (1 + t) / (10 + t))")
    parser.add_argument("--use_ema", action='store_true', default=False,
                        help="with --test_only --ckpt: evaluate the checkpoint's EMA weights")
    parser.add_argument("--distill_ckpt", type=str, default=None, metavar="PATH",
                        help="train against a frozen teacher: a checkpoint of this trainer, loaded strictly into "
                             "--distill_model; the criterion is --ce_weight x CE + --distill_weight x T^2 x KL(teacher || "
                             "student) at --distill_temperature T; --loss_type still selects the CE term's class weights")
    parser.add_argument("--distill_model", type=str, default=None, choices=available_models,
                        help="the teacher's architecture")
    parser.add_argument("--distill_output_stride", type=int, default=None, choices=[8, 16],
                        help="the teacher's output stride (default 16)")
    parser.add_argument("--distill_use_ema", action='store_true', default=False,
                        help="load the teacher checkpoint's EMA weights")
    parser.add_argument("--distill_weight", type=float, default=None, metavar="W",
                        help="factor of the distillation term (default 1.0)")
    parser.add_argument("--distill_temperature", type=float, default=None, metavar="T",
                        help="temperature both logit tensors are divided by (default 1.0)")
    parser.add_argument("--boundary_weight", type=float, default=0.0, metavar="W",
                        help="add W x the boundary loss (probability x signed Euclidean distance to the ground-truth contour, "
                             "on a distance map built on the device every step) to --ce_weight x CE; 0 = off")
    parser.add_argument("--boundary_clip", type=float, default=0.0, metavar="D",
                        help="clamp the signed distance of the boundary term at D pixels (0 = no clamp)")
    parser.add_argument("--boundary_ramp_itrs", type=int, default=0, metavar="N",
                        help="raise the boundary term's factor linearly from 0 to --boundary_weight over the first N "
                             "iterations (0 = the full factor from the first one)")
    parser.add_argument("--val_boundary_metrics", action='store_true', default=False,
                        help="validation also reports boundary precision / recall / F1 at --boundary_tolerance, ASSD, HD and "
                             "HD95 between predicted and labelled contours of the foreground classes (exact distances on the "
                             "device); model selection does not look at them")
    parser.add_argument("--boundary_tolerance", type=int, default=None, metavar="PX",
                        help="with --val_boundary_metrics: a contour pixel counts as matched within PX pixels (default 2)")
    parser.add_argument("--boundary_percentile", type=int, default=None, metavar="Q",
                        help="with --val_boundary_metrics: the nearest-rank percentile of the HD95 key, 1 to 100 (default 95)")
    return parser


class SyntheticBinarySegmentation(data.Dataset):
    """Stand-in for the absent ``datasets.BinarySegmentation`` (train.py:14,371-380): ImageNet-normalised
    float32 [3,H,W] images, uint8 [H,W] labels in {0,1} with ~10 % foreground blobs, ``.images`` names."""

    def __init__(self, root=None, split='train', transform=None, size=513, length=256, seed=0, raw=False):
        self.size, self.length, self.seed = size, length, seed + (0 if split == 'train' else 10_000)
        self.raw = raw      # uint8 [H,W,3] source tiles for the device augmentation pipeline (--device_augment)
        self.images = ["synthetic_%s_%06d.png" % (split, i) for i in range(length)]

    def __len__(self):
        return self.length

    def __getitem__(self, i):
        g = torch.Generator().manual_seed(self.seed + i)
        s = self.size
        img = torch.randn(3, s, s, generator=g)
        coarse = torch.rand(1, 1, (s + 31) // 32, (s + 31) // 32, generator=g)
        lab = (torch.nn.functional.interpolate(coarse, size=(s, s), mode='nearest')[0, 0] < 0.10).to(torch.uint8)
        if self.raw:
            img = (img.permute(1, 2, 0) * 58.0 + 116.0).clamp(0, 255).to(torch.uint8)     # what a decoded PNG tile holds
        return img, lab

    @staticmethod
    def decode_target(mask):
        return (np.asarray(mask) * 255).astype(np.uint8)


def get_dataset(opts):
    if opts.dataset == 'binary':
        from .datasets import BinarySegmentation
        return (BinarySegmentation(opts.data_root, split='train'), BinarySegmentation(opts.data_root, split='val'))
    return (SyntheticBinarySegmentation(split='train', size=opts.crop_size, length=opts.synthetic_len,
                                        seed=opts.random_seed, raw=opts.device_augment),
            SyntheticBinarySegmentation(split='val', size=opts.crop_size, length=max(8, opts.val_batch_size * 2),
                                        seed=opts.random_seed))


def epoch_batches(n, batch_size, seed, epoch, rank=0, world=1):
    """tile indices of one epoch's batches for one rank over a resident store of n tiles: the order is
    torch.randperm(n) from a generator seeded with (seed, epoch) -- identical on every rank --, the last partial
    batch is dropped and rank r takes the batches r, r + world, ... (every rank the same number of them)"""
    g = torch.Generator()
    g.manual_seed((int(seed) * 1000003 + int(epoch)) % (2 ** 63))
    order = torch.randperm(n, generator=g).tolist()
    nb = n // batch_size // world * world
    return [order[b * batch_size:(b + 1) * batch_size] for b in range(rank, nb, world)]


def load_checkpoint(path):
    """torch.load that executes nothing from the file; the reference's checkpoints (train.py:567-582) carry numpy
    scalars inside val_score / best_score, which the weights-only unpickler admits once their types are allow-listed"""
    _npcore = getattr(np, "_core", None) or getattr(np, "core", None)
    allow = [_npcore.multiarray.scalar if _npcore is not None else None, np.dtype, np.float64, np.float32, np.int64]
    try:
        from numpy import dtypes as _npd
        allow += [getattr(_npd, n) for n in ("Float64DType", "Float32DType", "Int64DType") if hasattr(_npd, n)]
    except ImportError:
        pass
    allow = [a for a in allow if a is not None]
    try:
        with torch.serialization.safe_globals(allow):
            return torch.load(path, map_location='cpu', weights_only=True)
    except Exception as e:                      # still refused: keep the tensors, drop the score dictionaries
        raise RuntimeError("checkpoint %s cannot be read with the weights-only loader: %s" % (path, e))


def scalar_score(v, weighted=None):
    """best_score as this loop keeps it (one float).  The reference stores a dictionary of per-metric bests
    (update_best_score, train.py:799-811) next to the checkpoint's own `weighted_score` (train.py:567-582): a resumed
    run compares against that weighted score."""
    if isinstance(v, dict):
        if weighted is not None:
            return float(weighted)
        if "Foreground IoU" in v and "Foreground F1" in v:
            return 0.5 * float(v["Foreground IoU"]) + 0.5 * float(v["Foreground F1"])
        return -1.0
    return float(v)


def setup_model(opts):
    ctor = network.modeling.__dict__[opts.model]
    return ctor(num_classes=opts.num_classes, output_stride=opts.output_stride,
                pretrained_backbone=opts.pretrained_backbone)


def read_teacher_checkpoint(opts):
    """the contents of --distill_ckpt (None without the option), read before anything else is set up: a missing file is a
    FileNotFoundError, an INT8 checkpoint is refused (it holds quantized convolutions, not a state dict to train against)"""
    path = getattr(opts, "distill_ckpt", None)
    if path is None:
        return None
    if not os.path.isfile(path):
        raise FileNotFoundError("--distill_ckpt: no checkpoint at %r" % (path,))
    name = os.path.basename(path)
    if name.startswith('best_') and name.endswith('.pth') and os.path.isdir(opts.checkpoints_dir) and \
            os.path.samefile(os.path.dirname(os.path.abspath(path)), opts.checkpoints_dir):
        raise ValueError("--distill_ckpt %s lies in --checkpoints_dir, where the run replaces every best_*.pth: it would "
                         "delete its own teacher; pick another --checkpoints_dir" % path)
    from . import quant
    q, ck = quant.read_checkpoint(path)
    if q is not None:
        raise ValueError("--distill_ckpt %s is an INT8 checkpoint: a teacher is an FP32 checkpoint of this trainer (an INT8 "
                         "teacher is not supported)" % path)
    return ck


def setup_teacher(opts, device, ck=None):
    """the frozen teacher of --distill_ckpt: --distill_model built as setup_model builds the student, the checkpoint (its EMA
    weights with --distill_use_ema) loaded strictly, eval mode, no parameter requires grad.  It is no part of the optimizer,
    the data-parallel wrapper or the checkpoint.  `ck`: the file's contents when the caller has read it already."""
    from .predict import load_model
    if ck is None:
        ck = read_teacher_checkpoint(opts)
    ctor = network.modeling.__dict__[opts.distill_model]
    teacher = ctor(num_classes=opts.num_classes, output_stride=opts.distill_output_stride, pretrained_backbone=False)
    load_model(teacher, opts.distill_ckpt, ck=ck, use_ema=opts.distill_use_ema)
    teacher.to(device).eval().requires_grad_(False)
    return teacher


def setup_optimizer(model, opts):
    """train.py:421-444 -- note: no lr argument, torch defaults apply"""
    params = model.parameters()
    if opts.optimizer == 'sgd':
        return FusedSGD(params, momentum=0.9, weight_decay=opts.weight_decay, nesterov=True)
    if opts.optimizer == 'adam':
        return FusedAdam(params, weight_decay=opts.weight_decay)
    if opts.optimizer == 'adamw':
        return FusedAdamW(params, weight_decay=opts.weight_decay)
    raise ValueError('Unsupported optimizer: %s' % opts.optimizer)


def setup_scheduler(optimizer, opts):
    """train.py:446-452"""
    return torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=opts.total_itrs, eta_min=opts.lr * 0.01)


def setup_criterion(opts, class_weights, group=None):
    """train.py:454-459; with --overlap_loss the same CE (times --ce_weight) plus a Dice / Tversky / focal-Tversky term; with
    --ohem_thresh the same CE over the hard pixels only"""
    weight = None if opts.loss_type == 'ce_loss' else class_weights
    if getattr(opts, 'distill_ckpt', None) is not None:
        return DistillationLoss(temperature=opts.distill_temperature, ce_weight=opts.ce_weight,
                                distill_weight=opts.distill_weight, weight=weight, ignore_index=255, group=group)
    if getattr(opts, 'boundary_weight', 0.0) > 0:
        return BoundaryLoss(classes='foreground', ce_weight=opts.ce_weight, boundary_weight=opts.boundary_weight,
                            clip=getattr(opts, 'boundary_clip', 0.0), weight=weight, ignore_index=255, group=group)
    kind = getattr(opts, 'overlap_loss', 'none')
    if kind != 'none':
        common = dict(smooth=opts.overlap_smooth, classes=opts.overlap_classes, ce_weight=opts.ce_weight,
                      overlap_weight=opts.overlap_weight, weight=weight, ignore_index=255, group=group)
        if kind == 'dice':
            return DiceLoss(**common)
        return TverskyLoss(alpha=opts.tversky_alpha, beta=opts.tversky_beta,
                           gamma=opts.tversky_gamma if kind == 'focal_tversky' else 1.0, **common)
    if getattr(opts, 'lovasz_weight', 0.0) > 0:
        return LovaszSoftmaxLoss(classes=opts.overlap_classes, ce_weight=opts.ce_weight, lovasz_weight=opts.lovasz_weight,
                                 weight=weight, ignore_index=255, group=group)
    if getattr(opts, 'ohem_thresh', 0.0) > 0:
        world = dist.get_world_size(group) if group is not None else 1      # --ohem_min_kept is per process, like --batch_size
        return OhemCrossEntropyLoss(thresh=opts.ohem_thresh, min_kept=opts.ohem_min_kept * world, weight=weight,
                                    ignore_index=255, group=group)
    if opts.loss_type == 'ce_loss':
        return CrossEntropyLoss(ignore_index=255, reduction='mean', group=group)
    return CrossEntropyLoss(weight=class_weights, ignore_index=255, reduction='mean', group=group)


def boundary_factor(opts, itr):
    """the boundary term's factor at iteration `itr` (counted from 1): --boundary_weight, raised linearly from 0 over the first
    --boundary_ramp_itrs iterations.  A function of the iteration alone, so a resumed run continues the ramp."""
    weight, ramp = getattr(opts, 'boundary_weight', 0.0), getattr(opts, 'boundary_ramp_itrs', 0)
    return weight * min(1.0, itr / ramp) if ramp > 0 else weight


def validate(model, loader, device, opts):
    """train.py:620-666,686-694: eval-mode logits -> ``logits.max(1)[1]`` masks -> StreamMetrics scores.  The
    argmax and the confusion matrix run in one kernel on the device (metrics.StreamMetrics.update_logits); no mask
    is copied to the host."""
    from .metrics import StreamMetrics
    model.eval()
    metrics = StreamMetrics(opts.num_classes, device=device)
    boundary = boundary_metrics_of(opts, device)
    with torch.no_grad():
        for images, labels in loader:
            logits = model(images.to(device, dtype=torch.float32))
            labels = labels.to(device)
            metrics.update_logits(labels, logits)
            if boundary is not None:                            # one more argmax per batch, only with the flag on
                boundary.update_logits(labels, logits)
    model.train()
    score = {k: float(v) for k, v in metrics.get_results().items()}
    if boundary is not None:
        score.update(boundary.get_results())
    return score


def boundary_metrics_of(opts, device):
    """the BoundaryMetrics of --val_boundary_metrics (the criterion's ignore_index 255 and foreground classes), or None with the
    flag off; options objects built without the flag are taken as off"""
    if not getattr(opts, 'val_boundary_metrics', False):
        return None
    from .metrics import BoundaryMetrics
    tolerance, percent = getattr(opts, 'boundary_tolerance', None), getattr(opts, 'boundary_percentile', None)
    return BoundaryMetrics(opts.num_classes, classes='foreground', ignore_index=255, tolerance=2 if tolerance is None else tolerance,
                           percent=95 if percent is None else percent, device=device)


METRIC_WEIGHTS = {"MIoU": 0.05, "Foreground IoU": 0.25, "Foreground F1": 0.25, "Front Tracking Error": 0.25,
                  "Temporal Consistency": 0.10, "Region Continuity": 0.10}         # get_metric_weights, train.py:842-850


def validate_sequence(model, loader, device, opts):
    """the metric half of train.py:620-694: eval-mode argmax masks (kept on the device), ordered by
    ``loader.dataset.images``, fed to StreamMetrics as sliding windows of ``--sequence_length`` frames; with fewer
    frames than that nothing is counted"""
    from .metrics import StreamMetrics
    model.eval()
    preds, gts = [], []
    with torch.no_grad():
        for images, labels in loader:
            preds.append(ops.argmax_nchw(model(images.to(device, dtype=torch.float32))))
            gts.append(labels.to(device))
    model.train()
    metrics = StreamMetrics(opts.num_classes, sequence_length=opts.sequence_length, device=device)
    boundary = boundary_metrics_of(opts, device)
    if boundary is not None:                                    # every frame once, not once per window; one call per batch
        for p, g in zip(preds, gts):
            boundary.update(g, p)
    L = opts.sequence_length
    if preds:
        preds, gts = torch.cat(preds), torch.cat(gts)
        names = loader.dataset.images
        order = sorted(range(preds.shape[0]), key=lambda i: names[i])        # stable, as list.sort in the reference
        idx = torch.tensor(order, dtype=torch.int64).to(device)
        preds, gts = preds.index_select(0, idx), gts.index_select(0, idx)
        for i in range(preds.shape[0] - L + 1):
            metrics.update(gts[i:i + L], preds[i:i + L], sequence_data=True)
    score = {k: float(v) for k, v in metrics.get_results().items()}
    if boundary is not None:
        score.update(boundary.get_results())
    return score


def initialize_best_score():
    """train.py:747-758"""
    inf = float('inf')
    return {'MIoU': -inf, 'Foreground IoU': -inf, 'Foreground F1': -inf, 'Temporal Consistency': -inf,
            'Front Tracking Error': inf, 'Region Continuity': -inf, 'Precision': -inf, 'Recall': -inf}


def is_best_score(current, best, weights=METRIC_WEIGHTS):
    """train.py:760-797 (without the prints)"""
    if best is None:
        return True
    current_total = best_total = 0
    for metric in ('MIoU', 'Foreground IoU', 'Foreground F1', 'Temporal Consistency', 'Region Continuity'):
        if metric in weights and weights[metric] > 0:
            v = float(current[metric])
            if not np.isnan(v):
                current_total += weights[metric] * v
                best_total += weights[metric] * float(best.get(metric, 0.0))
    if 'Front Tracking Error' in current:
        w = abs(weights.get('Front Tracking Error', 0.03))
        current_total += w * max(0, 1 - float(current['Front Tracking Error']) / 10.0)
        best_total += w * max(0, 1 - float(best.get('Front Tracking Error', 10.0)) / 10.0)
    return current_total > best_total


def update_best_score(val_score):
    """train.py:799-840 (without the prints)"""
    best = {}
    for metric in ('MIoU', 'Foreground IoU', 'Foreground F1', 'Region Continuity'):
        v = val_score.get(metric)
        best[metric] = float(v) if v is not None and not np.isnan(v) else 0.0
    if 'Front Tracking Error' in val_score:
        e = float(val_score['Front Tracking Error'])
        best['Front Tracking Error'] = e if not np.isnan(e) else 10.0
    if 'Temporal Consistency' in val_score:
        v = val_score['Temporal Consistency']
        best['Temporal Consistency'] = float(v) if v is not None and not np.isnan(v) else 0.0
    for metric in ('Precision', 'Recall'):
        if metric in val_score and not np.isnan(val_score[metric]):
            best[metric] = float(val_score[metric])
    return best


def logged_weighted_score(val_score, weights=METRIC_WEIGHTS):
    """MetricsLogger.get_weighted_score (train.py:128-167) over the values validate_and_save logs (:686-694): FG-IoU,
    FG-F1 and region continuity, the front error as max(0, 1 - e/10), temporal consistency"""
    score = 0.0
    for metric in ('Foreground IoU', 'Foreground F1', 'Region Continuity'):
        v = float(val_score.get(metric, 0))
        if not np.isnan(v):
            score += weights[metric] * v
    score += abs(weights['Front Tracking Error']) * max(0, 1 - float(val_score.get('Front Tracking Error', 0)) / 10.0)
    v = float(val_score.get('Temporal Consistency', 0))
    if not np.isnan(v):
        score += weights['Temporal Consistency'] * v
    return score


def save_best_model(model, optimizer, scheduler, opts, val_score, weighted_score, cur_itrs, best_score):
    """train.py:525-609 -- same payload keys, atomic replace, older best_*.pth removed"""
    os.makedirs(opts.checkpoints_dir, exist_ok=True)
    for old in os.listdir(opts.checkpoints_dir):
        if old.startswith('best_') and old.endswith('.pth'):
            os.remove(os.path.join(opts.checkpoints_dir, old))
    path = os.path.join(opts.checkpoints_dir, 'best_%s_%s_os%d_weighted%.3f.pth' %
                        (opts.model, opts.dataset, opts.output_stride, weighted_score))
    to_save = model.module if hasattr(model, 'module') else model
    ckpt = {"model_state": to_save.state_dict(), "optimizer_state": optimizer.state_dict(),
            "scheduler_state": scheduler.state_dict(), "val_score": val_score, "weighted_score": weighted_score,
            "cur_itrs": cur_itrs, "best_score": best_score, "save_time": datetime.now().strftime('%Y%m%d_%H%M%S'),
            "model_config": {"model_name": opts.model, "dataset": opts.dataset,
                             "output_stride": opts.output_stride, "num_classes": opts.num_classes}}
    if getattr(optimizer, "ema_enabled", False):            # called OUTSIDE ema_weights(): model_state is the live weights
        ckpt["ema_state"] = optimizer.ema_state_dict(to_save)
    torch.save(ckpt, path + '.tmp')
    os.replace(path + '.tmp', path)
    return path


def main(argv=None):
    opts = get_argparser().parse_args(argv)
    opts.num_classes = 2                                   # train.py:853
    opts._teacher_ck = read_teacher_checkpoint(opts)       # refused here, before the data set is touched
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", opts.gpu_id.split(',')[0]))
    if not torch.cuda.is_available():
        raise SystemExit("iswm_amd.train needs an MI355X (no CPU fallback)")
    torch.cuda.set_device(local)
    device = torch.device('cuda', local)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=device)
    # model initialisation is seeded identically on every rank (and broadcast anyway); the augmentation draws
    # (Python `random`) and the dropout masks (torch's initial seed feeds the Philox counter) must differ per rank
    torch.manual_seed(opts.random_seed)
    np.random.seed(opts.random_seed)
    random.seed(opts.random_seed)

    check_augment_flags(opts)
    train_dst, val_dst = get_dataset(opts)
    if opts.dataset == 'binary':
        return _main_resident(opts, train_dst, val_dst, device, rank, world)
    return _main_loader(opts, train_dst, val_dst, device, rank, world)


def _augment_flags(opts):
    """(--aug_rotate, --aug_vflip, --aug_color_jitter); off for an options object built without them"""
    return getattr(opts, "aug_rotate", 0.0), getattr(opts, "aug_vflip", False), getattr(opts, "aug_color_jitter", None)


def check_augment_flags(opts):
    """--aug_rotate / --aug_vflip / --aug_color_jitter live in the device pipeline only"""
    rotate, vflip, jitter = _augment_flags(opts)
    if (rotate or vflip or jitter) and not opts.device_augment and opts.dataset != 'binary':
        raise ValueError("--aug_rotate, --aug_vflip and --aug_color_jitter act in the device input pipeline: add "
                         "--device_augment (or train with --dataset binary); the DataLoader path has no such transforms")


def _color_jitter_arg(text):
    try:
        v = [float(x) for x in text.split(",")]
    except ValueError:
        v = []
    if len(v) != 4 or any(not x >= 0 for x in v) or v[3] > 0.5:
        raise ValueError("--aug_color_jitter wants B,C,S,H: four non-negative numbers, H <= 0.5 (got %r)" % (text,))
    return v


def _train_transform(opts, et):
    """the reference's train_transform (train.py:355-362), plus what --aug_rotate, --aug_vflip and --aug_color_jitter add"""
    rotate, vflip, jitter = _augment_flags(opts)
    if rotate < 0:
        raise ValueError("--aug_rotate wants a non-negative angle in degrees (got %r)" % (rotate,))
    chain = [et.ExtRandomRotation(rotate)] if rotate else []
    chain += [
        et.ExtRandomScale((0.5, 2.0)),
        et.ExtRandomCrop(size=(opts.crop_size, opts.crop_size), pad_if_needed=True),
        et.ExtRandomHorizontalFlip(),
    ]
    if vflip:
        chain.append(et.ExtRandomVerticalFlip())
    if jitter:
        chain.append(et.ExtColorJitter(*_color_jitter_arg(jitter)))
    chain += [
        et.ExtToTensor(),
        et.ExtNormalize(mean=[0.485, 0.456, 0.406], std=[0.229, 0.224, 0.225]),
    ]
    return et.ExtCompose(chain)


def _main_resident(opts, train_dst, val_dst, device, rank, world):
    """--dataset binary: both splits live on the device (datasets.DeviceTileStore); a training batch is
    ExtCompose.batch_resident over the epoch's index order, a validation batch is iswm_gather_normalize"""
    from .datasets import DeviceTileStore
    from .utils import ext_transforms as et
    workers = max(1, min(16, opts.num_workers))
    if rank == 0:
        print("Dataset binary: device pipeline (tiles decoded once by %d threads, resident on %s; augmentation and "
              "validation batches are built there)" % (workers, device))
    val_store = DeviceTileStore(val_dst, device, workers=workers)
    if opts.val_metrics == 'sequence' and not val_store.uniform_size:
        raise ValueError("--val_metrics sequence needs validation tiles of ONE size (its windows stack consecutive "
                         "frames); %s holds tiles of mixed sizes: %s" %
                         (val_dst.img_dir, sorted(set(m[2:] for m in val_store.meta))))
    val_loader = val_store.batches(opts.val_batch_size)
    if opts.test_only:                        # nothing of the train split is needed to score a checkpoint
        return _run(opts, device, rank, world, None, 0, val_loader, torch.ones(2))
    train_store = DeviceTileStore(train_dst, device, workers=workers)
    per_rank = len(epoch_batches(len(train_store), opts.batch_size, opts.random_seed, 0, rank, world))
    if per_rank < 1:
        raise ValueError("%d train tiles give no full batch of %d on each of %d ranks" %
                         (len(train_store), opts.batch_size, world))
    transform = _train_transform(opts, et)

    def epoch(e):
        for idx in epoch_batches(len(train_store), opts.batch_size, opts.random_seed, e, rank, world):
            yield transform.batch_resident(train_store, idx)
    # the reference's class weights: one pass of the AUGMENTED train loader (train.py:388-410), here epoch 0's order
    class_weights = calculate_class_weights_resident(epoch(0), dist.group.WORLD if world > 1 else None)
    if rank == 0:
        print("Class weights - Black: %.4f, White: %.4f" % (class_weights[0], class_weights[1]))
    return _run(opts, device, rank, world, epoch, per_rank, val_loader, class_weights)


def _main_loader(opts, train_dst, val_dst, device, rank, world):
    sampler = data.distributed.DistributedSampler(train_dst, world, rank, shuffle=True, drop_last=True) \
        if world > 1 else None
    train_transform = None
    if opts.device_augment:
        # the reference's train_transform (train.py:355-362) as one HIP kernel per batch over uint8 tiles on the GPU
        from .utils import ext_transforms as et
        train_transform = _train_transform(opts, et)
    train_loader = data.DataLoader(train_dst, batch_size=opts.batch_size, shuffle=sampler is None, sampler=sampler,
                                   num_workers=opts.num_workers, drop_last=True)
    val_loader = data.DataLoader(val_dst, batch_size=opts.val_batch_size, shuffle=False, num_workers=0)
    class_weights = calculate_class_weights(train_loader, dist.group.WORLD if world > 1 else None).to(device)
    if rank == 0:
        print("Class weights - Black: %.4f, White: %.4f" % (class_weights[0], class_weights[1]))

    def epoch(e):
        if sampler is not None:
            sampler.set_epoch(e)
        for images, labels in train_loader:
            if train_transform is not None:
                yield train_transform.batch(list(images.to(device, non_blocking=True)),
                                            list(labels.to(device, non_blocking=True)))
            else:
                yield (images.to(device, dtype=torch.float32, non_blocking=True), labels.to(device, non_blocking=True))
    return _run(opts, device, rank, world, epoch, len(train_loader), val_loader, class_weights)


def _run(opts, device, rank, world, epoch, batches_per_epoch, val_loader, class_weights):
    """model, optimizer, criterion, resume, then the step loop over `epoch(e)` -- an iterable of device batches
    (images float32 [B,3,H,W], labels) for epoch number e, `batches_per_epoch` of them on this rank"""
    class_weights = class_weights.to(device)
    model = setup_model(opts)
    cur_itrs, best_score = 0, -1.0
    ckpt = None
    if getattr(opts, "use_ema", False) and not os.path.isfile(opts.ckpt):
        raise FileNotFoundError("--use_ema: no checkpoint at %r" % (opts.ckpt,))
    if opts.ckpt is not None and os.path.isfile(opts.ckpt):
        ckpt = load_checkpoint(opts.ckpt)
        source = ema_model_state(ckpt) if getattr(opts, "use_ema", False) else ckpt["model_state"]
        state = {(k[7:] if k.startswith('module.') else k): v for k, v in source.items()}
        ret = model.load_state_dict(state, strict=False)
        print("Model restored from %s (missing %d, unexpected %d)" % (opts.ckpt, len(ret.missing_keys),
                                                                     len(ret.unexpected_keys)))
        if opts.continue_training:
            cur_itrs = ckpt["cur_itrs"]
            best_score = scalar_score(ckpt.get("best_score", best_score), ckpt.get("weighted_score"))
    model.to(device)
    if world > 1:
        torch.manual_seed(opts.random_seed + 1000003 * rank)       # dropout / augmentation streams differ per rank from here on
        random.seed(opts.random_seed + 1000003 * rank)
    optimizer = setup_optimizer(model, opts)
    optimizer.set_grad_clip(getattr(opts, "clip_grad_norm", 0.0))
    if getattr(opts, "ema_decay", 0.0):
        optimizer.enable_ema(opts.ema_decay, warmup=not opts.ema_no_warmup)
    scheduler = setup_scheduler(optimizer, opts)
    group = dist.group.WORLD if world > 1 else None
    criterion = setup_criterion(opts, class_weights, group).to(device)
    net = model
    if world > 1:
        net = DistributedDataParallelHIP(model, process_group=group)
        net.attach(optimizer)
    if ckpt is not None and opts.continue_training:
        optimizer.load_state_dict(ckpt["optimizer_state"])
        scheduler.load_state_dict(ckpt["scheduler_state"])
        if optimizer.ema_enabled and "ema_state" in ckpt:   # the resumed average continues where the checkpoint's stopped
            optimizer.load_ema_state_dict(model, ckpt["ema_state"])
    # with EMA on, everything that scores or draws the model runs on the averaged weights; the checkpoint is written outside
    # the context, from the live ones
    ema_weights = optimizer.ema_weights if optimizer.ema_enabled else contextlib.nullcontext
    clipping = bool(getattr(opts, "clip_grad_norm", 0.0))
    mining = isinstance(criterion, OhemCrossEntropyLoss)
    lovasz = isinstance(criterion, LovaszSoftmaxLoss)
    boundary = isinstance(criterion, BoundaryLoss)
    if boundary and rank == 0:
        print("Boundary term: CE x %g + BD x %g%s%s" %
              (opts.ce_weight, opts.boundary_weight, ", distance clamped at %g" % opts.boundary_clip if opts.boundary_clip else "",
               ", ramped over %d iterations" % opts.boundary_ramp_itrs if opts.boundary_ramp_itrs else ""))
    teacher = None
    if getattr(opts, 'distill_ckpt', None) is not None:
        teacher = setup_teacher(opts, device, getattr(opts, '_teacher_ck', None))
        opts._teacher_ck = None
        if rank == 0:
            print("Teacher %s (output stride %d%s): T=%g, CE x %g + KD x %g" %
                  (opts.distill_model, opts.distill_output_stride, ", EMA weights" if opts.distill_use_ema else "",
                   opts.distill_temperature, opts.ce_weight, opts.distill_weight))

    sequence_val = opts.val_metrics == 'sequence'
    if sequence_val:
        best_score = initialize_best_score()
        if ckpt is not None and opts.continue_training and isinstance(ckpt.get("best_score"), dict):
            best_score = ckpt["best_score"]
    if opts.test_only:
        score = (validate_sequence if sequence_val else validate)(model, val_loader, device, opts)
        print(score)
        if opts.save_val_results and rank == 0:
            weighted = logged_weighted_score(score) if sequence_val else \
                0.5 * score["Foreground IoU"] + 0.5 * score["Foreground F1"]
            save_validation_results(model, val_loader, device, opts, int(ckpt.get("cur_itrs", 0)) if ckpt else 0,
                                    weighted, prefix="test_only")
        return
    model.train()
    interval_loss = torch.zeros((), device=device)
    t_last, n_last = time.time(), 0
    # a resumed run continues the epoch count where it stopped (train.py:997): DistributedSampler.set_epoch would otherwise
    # replay the shuffles the run already consumed
    cur_epochs = cur_itrs // max(1, batches_per_epoch)
    if rank == 0 and cur_itrs:
        print("Resuming at iteration %d (epoch %d)" % (cur_itrs, cur_epochs))
    while cur_itrs < opts.total_itrs:
        cur_epochs += 1
        for images, labels in epoch(cur_epochs):
            cur_itrs += 1
            if teacher is not None:
                with torch.no_grad():                           # eval mode, nothing saved for a backward
                    teacher_logits = teacher(images)
                logits = net(images)
                loss = criterion(logits, labels, teacher_logits)
            else:
                if boundary:                                    # a host number: no synchronisation
                    criterion.boundary_weight = boundary_factor(opts, cur_itrs)
                logits = net(images)
                loss = criterion(logits, labels)
            optimizer.zero_grad()
            loss.backward()
            optimizer.step()
            interval_loss += loss.detach()
            n_last += images.shape[0] * world
            if cur_itrs % opts.print_interval == 0 and rank == 0:
                avg = float(interval_loss) / opts.print_interval
                dt = time.time() - t_last
                norm = ""
                if clipping:                                    # one read-back per interval; None until a step has clipped
                    last = optimizer.last_grad_norm
                    norm = ", grad norm=%s" % ("n/a" if last is None else "%.4e" % float(last))
                if mining:                                      # the last step's kept pixels of the global batch: one read-back
                    kept = int(criterion.last_kept)
                    norm += ", kept=%d (%.2f%%)" % (kept, 100.0 * kept / (labels.numel() * world))
                if lovasz:                                      # the last step's (image, class) pairs of the global batch: one read-back
                    norm += ", present=%d" % int(criterion.last_present)
                if teacher is not None:                         # the last step's KD term and agreement of the global batch: one read-back
                    kd, agree, nvalid = torch.stack([criterion.last_terms[1].double(), *criterion.last_agreement]).tolist()
                    norm += ", kd=%.6f, agree=%.2f%%" % (kd, 100.0 * agree / nvalid if nvalid else 0.0)
                if boundary:                                    # the last step's boundary term of the global batch: one read-back
                    norm += ", bd=%.6f, lbd=%.6g" % (float(criterion.last_terms[1]), criterion.boundary_weight)
                print("Epoch %d, Itrs %d/%d, Loss=%.6f, lr=%.3e, %.1f img/s%s" %
                      (cur_epochs, cur_itrs, opts.total_itrs, avg, optimizer.param_groups[0]['lr'], n_last / dt, norm))
                interval_loss.zero_()
                t_last, n_last = time.time(), 0
            if cur_itrs % opts.val_interval == 0 and world > 1:
                dist.barrier()               # the other ranks wait HERE (not inside the next step's all-reduce) while rank 0 validates
            if cur_itrs % opts.val_interval == 0 and rank == 0:
                if sequence_val:                                # train.py:686-731
                    with ema_weights():
                        score = validate_sequence(model, val_loader, device, opts)
                    print("Validation @%d: %s" % (cur_itrs, score))
                    if is_best_score(score, best_score):
                        best_score = update_best_score(score)
                        weighted = logged_weighted_score(score)
                        path = save_best_model(model, optimizer, scheduler, opts, score, weighted, cur_itrs, best_score)
                        print("saved", path)
                        if path and opts.save_val_results:          # train.py:733-737
                            with ema_weights():
                                save_validation_results(model, val_loader, device, opts, cur_itrs, weighted)
                else:
                    with ema_weights():
                        score = validate(model, val_loader, device, opts)
                    weighted = 0.5 * score["Foreground IoU"] + 0.5 * score["Foreground F1"]
                    print("Validation @%d: %s" % (cur_itrs, score))
                    if weighted > best_score:
                        best_score = weighted
                        path = save_best_model(model, optimizer, scheduler, opts, score, weighted, cur_itrs, best_score)
                        print("saved", path)
                        if path and opts.save_val_results:
                            with ema_weights():
                                save_validation_results(model, val_loader, device, opts, cur_itrs, weighted)
            if cur_itrs % opts.val_interval == 0 and world > 1:
                dist.barrier()
            scheduler.step()
            if cur_itrs >= opts.total_itrs:
                break
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
