"""Criteria of the training step on the fused HIP loss kernel -- counterpart of the
reference's utils/loss.py (FocalLoss :14-35, create_loss :37-39) and of the criterion
built by setup_criterion, train.py:454-459 (nn.CrossEntropyLoss(weight, ignore_index=255)).

``criterion(logits, labels)`` keeps the reference's call shape (train.py:1046): logits
NCHW fp32 on the GPU, labels [B,H,W] int64 (or uint8, as the dataset produces them).
One kernel pass computes the loss terms AND the unnormalised gradient; backward only
rescales it.  Under data parallelism ``group`` makes the weighted-mean normaliser global
(sum of class weights over ALL ranks' pixels), which is what the reference's
gathered-logits loss under nn.DataParallel computes (train.py:970,1045-1046).
"""
import math

import torch
import torch.nn as nn

from .. import ops
from ..network._hip import CONSUMED, once


def _scalar(upstream):
    """the upstream gradient as the fp32 device scalar [1] the backward kernels read"""
    return upstream.reshape(1).contiguous().to(torch.float32)


def _weight_for(weight, inputs):
    """a module's class weights as fp32 on the input's device (None without weights)"""
    return None if weight is None else weight.to(device=inputs.device, dtype=torch.float32)


class _LossFn(torch.autograd.Function):
    """The one-pass criteria: the forward stores the unnormalised gradient and the backward rescales it IN PLACE, so it is
    good for one backward; a second one through the same call (retain_graph) is refused, not handed a twice-scaled tensor."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, alpha, gamma, mode, group):
        loss, sums, grad = ops.loss_fwd(logits, labels, weight, ignore_index, alpha, gamma, mode)
        npix = labels.numel()
        if group is not None:
            import torch.distributed as dist
            world = dist.get_world_size(group)
            if mode == ops.MODE_WCE:
                dist.all_reduce(sums, group=group)              # global sum(w*nll), sum(w)
                loss = (sums[0] / sums[1]).reshape(1)
            else:
                if mode == ops.MODE_FOCAL_MEAN:
                    npix = npix * world
                dist.all_reduce(sums, group=group)
                loss = (sums[0] / npix if mode == ops.MODE_FOCAL_MEAN else sums[0]).reshape(1)
        ctx.save_for_backward(grad, sums)
        ctx.mode, ctx.npix, ctx.consumed = mode, npix, False
        return loss.reshape(())

    @staticmethod
    @once
    def backward(ctx, upstream):
        if ctx.consumed:
            raise RuntimeError("%s: %s" % (("CrossEntropyLoss" if ctx.mode == ops.MODE_WCE else "FocalLoss"), CONSUMED))
        ctx.consumed = True
        grad, sums = ctx.saved_tensors
        ops.loss_bwd_scale(grad, sums, _scalar(upstream), ctx.mode, ctx.npix)
        return grad, None, None, None, None, None, None, None


def _check(logits, labels):
    if not (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4):
        raise ValueError("loss expects fp32 CUDA logits [B,C,H,W] (there is no CPU fallback)")
    if labels.dtype not in (torch.int64, torch.uint8):
        labels = labels.long()
    return labels.to(logits.device)


class CrossEntropyLoss(nn.Module):
    """nn.CrossEntropyLoss(weight=w, ignore_index=255, reduction='mean') as train.py:454-459
    builds it ('ce_loss': weight=None; 'IWce_loss': weight=[1, sqrt(N_black/N_white)])."""

    def __init__(self, weight=None, ignore_index=255, reduction='mean', group=None):
        super().__init__()
        if reduction != 'mean':
            raise NotImplementedError("the training path uses reduction='mean'")
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.ignore_index = ignore_index
        self.group = group

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        w = _weight_for(self.weight, inputs)
        return _LossFn.apply(inputs, targets, w, self.ignore_index, 1.0, 0.0, ops.MODE_WCE, self.group)


class FocalLoss(nn.Module):
    """FocalLoss(alpha=1, gamma=0, size_average=True, ignore_index=255, weight=None) --
    reference utils/loss.py:14-35 (mean runs over ALL pixels, ignored ones included)."""

    def __init__(self, alpha=1, gamma=0, size_average=True, ignore_index=255, weight=None, group=None):
        super(FocalLoss, self).__init__()
        self.alpha = alpha
        self.gamma = gamma
        self.ignore_index = ignore_index
        self.size_average = size_average
        self.weight = weight
        self.group = group

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        w = _weight_for(self.weight, inputs)
        mode = ops.MODE_FOCAL_MEAN if self.size_average else ops.MODE_FOCAL_SUM
        return _LossFn.apply(inputs, targets, w, self.ignore_index, float(self.alpha), float(self.gamma), mode,
                             self.group)


class _OverlapLossFn(torch.autograd.Function):
    """ce_weight * weighted CE + overlap_weight * Tversky term on the two-pass kernels (csrc/loss.hip): the forward pass
    stores nothing per pixel, the backward pass reads the logits again and writes the finished gradient once.  With `group`
    the sums are all-reduced before the coefficients are formed, so every T_c is the global batch's and the SUM gradient
    all-reduce of parallel.py yields the gradient of the global loss."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, params, group):
        sums = ops.overlap_loss_fwd(logits, labels, weight, ignore_index)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        loss, coef = ops.overlap_loss_coeffs(sums, logits.shape[1], *params)
        ctx.save_for_backward(logits, labels, weight, coef)
        ctx.ignore_index = ignore_index
        return loss.reshape(())

    @staticmethod
    @once
    def backward(ctx, upstream):
        logits, labels, weight, coef = ctx.saved_tensors
        grad = ops.overlap_loss_bwd(logits, labels, weight, ctx.ignore_index, coef, _scalar(upstream))
        return grad, None, None, None, None, None


class TverskyLoss(nn.Module):
    """ce_weight * CrossEntropyLoss(weight, ignore_index) + overlap_weight * mean over the chosen classes of
    (1 - T_c)^gamma, T_c = (I_c + smooth) / (I_c + alpha FP_c + beta FN_c + smooth) on softmax probabilities over the
    pixels the CE counts.  beta > alpha favours recall; gamma != 1 is the focal-Tversky loss.  classes: 'foreground'
    (every class but 0) or 'all'.  At most 8 classes."""

    def __init__(self, alpha=0.3, beta=0.7, gamma=1.0, smooth=1.0, classes='foreground', ce_weight=0.0, overlap_weight=1.0,
                 weight=None, ignore_index=255, group=None):
        super().__init__()
        if not smooth > 0:
            raise ValueError("smooth must be positive (it keeps the empty and all-ignored cases finite)")
        if alpha < 0 or beta < 0 or not gamma > 0:
            raise ValueError("alpha and beta must not be negative and gamma must be positive")
        if ce_weight < 0 or overlap_weight < 0:
            raise ValueError("ce_weight and overlap_weight must not be negative")
        if classes not in ops.OVERLAP_CLASSES:
            raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.params = (float(ce_weight), float(overlap_weight), float(alpha), float(beta), float(gamma), float(smooth), classes)
        self.ignore_index = ignore_index
        self.group = group

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        w = _weight_for(self.weight, inputs)
        return _OverlapLossFn.apply(inputs, targets, w, self.ignore_index, self.params, self.group)


class DiceLoss(TverskyLoss):
    """soft Dice: TverskyLoss with alpha = beta = 0.5"""

    def __init__(self, **kw):
        if 'alpha' in kw or 'beta' in kw:
            raise TypeError("DiceLoss fixes alpha = beta = 0.5; use TverskyLoss for other values")
        super().__init__(alpha=0.5, beta=0.5, **kw)


class _OhemLossFn(torch.autograd.Function):
    """The weighted CE over the hard pixels (csrc/loss.hip): keys, an exact radix select of nu on the device, the kept sums;
    the backward pass decides `kept` from the stored keys and writes the finished gradient once.  Nothing is read back.  With
    `group`, |V|, every digit's histogram and the three sums are all-reduced between the kernel that writes and the kernel
    that reads them: nu, K and sum_K w are the global batch's, and the SUM gradient all-reduce of parallel.py yields the
    gradient of the global loss."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, thresh, min_kept, group):
        keys, nvalid = ops.ohem_keys(logits, labels, ignore_index)
        nu = ops.ohem_select(keys, nvalid, min_kept, thresh, group)
        sums = ops.ohem_sums(keys, labels, weight, nu)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        out = ops.ohem_loss(sums)
        ctx.save_for_backward(logits, labels, weight, keys, nu, out)
        ctx.mark_non_differentiable(sums, nu)
        return out[0].clone(), sums, nu

    @staticmethod
    @once
    def backward(ctx, upstream, _sums, _nu):
        logits, labels, weight, keys, nu, out = ctx.saved_tensors
        grad = ops.ohem_bwd(logits, labels, weight, keys, nu, out, _scalar(upstream))
        return grad, None, None, None, None, None, None


class OhemCrossEntropyLoss(nn.Module):
    """Online hard-example mining (bootstrapped cross-entropy): CrossEntropyLoss(weight, ignore_index) averaged over the
    pixels whose true-class probability is at most `thresh`, and over at least the `min_kept` hardest valid pixels of the
    batch (ties at the threshold are all kept).  thresh = 1 keeps every valid pixel: the plain weighted CE.  `min_kept`
    counts pixels of the whole batch (under `group`: of all ranks together).  At most 8 classes.

    `last_kept` is a 0-dim device view of the number of kept pixels of the last call and `last_nu` one of the loss threshold
    it selected; reading either synchronises."""

    def __init__(self, thresh=0.7, min_kept=100000, weight=None, ignore_index=255, group=None):
        super().__init__()
        if not 0.0 < thresh <= 1.0:
            raise ValueError("thresh must lie in (0, 1] (got %r)" % (thresh,))
        if int(min_kept) != min_kept or min_kept < 0:
            raise ValueError("min_kept must be a non-negative integer (got %r)" % (min_kept,))
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.thresh, self.min_kept = float(thresh), int(min_kept)
        self.ignore_index = ignore_index
        self.group = group
        self.last_kept = self.last_nu = None

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        w = _weight_for(self.weight, inputs)
        loss, sums, nu = _OhemLossFn.apply(inputs, targets, w, self.ignore_index, self.thresh, self.min_kept, self.group)
        self.last_kept, self.last_nu = sums[2], nu[0]
        return loss


class _LovaszLossFn(torch.autograd.Function):
    """ce_weight * weighted CE + lovasz_weight * per-image Lovasz-Softmax (csrc/lovasz.hip): keys, a stable segmented radix
    sort on the device, the Jaccard weights of every pixel; the backward pass reads the logits again and writes the finished
    gradient once.  Nothing is read back.  With `group` the four sums {sum w nll, sum w, sum L_bc, N} are all-reduced between
    the kernel that writes them and the one that reads them: the order statistic is per image, so no sort crosses a rank, and
    the SUM gradient all-reduce of parallel.py yields the gradient of the global loss."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, group):
        keys, counts, sums = ops.lovasz_keys(logits, labels, weight, ignore_index, classes)
        sorted_keys, perm = ops.lovasz_sort(keys)
        m, sums = ops.lovasz_weights(sorted_keys, perm, counts, sums)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        out = ops.lovasz_loss(sums, ce_weight, lovasz_weight)
        ctx.save_for_backward(logits, labels, weight, m, out)
        ctx.ignore_index, ctx.classes = ignore_index, classes
        ctx.mark_non_differentiable(sums)
        return out[0].clone(), sums

    @staticmethod
    @once
    def backward(ctx, upstream, _sums):
        logits, labels, weight, m, out = ctx.saved_tensors
        grad = ops.lovasz_bwd(logits, labels, weight, ctx.ignore_index, ctx.classes, m, out, _scalar(upstream))
        return grad, None, None, None, None, None, None, None


class LovaszSoftmaxLoss(nn.Module):
    """ce_weight * CrossEntropyLoss(weight, ignore_index) + lovasz_weight * Lovasz-Softmax (Berman et al. 2018), per image:
    for every image and class of `classes` ('foreground': every class but 0, or 'all') that occurs in the image, the errors
    |[y == c] - softmax_c| of the image's valid pixels, sorted descending, weighted by the increments of the Jaccard loss;
    averaged over those (image, class) pairs -- of all ranks together under `group`.  Absent classes are not counted; with
    none present the term is 0.  At most 8 classes.

    `last_present` is a 0-dim device view of the number of (image, class) pairs of the last call; reading it synchronises."""

    def __init__(self, classes='foreground', ce_weight=0.0, lovasz_weight=1.0, weight=None, ignore_index=255, group=None):
        super().__init__()
        if classes not in ops.OVERLAP_CLASSES:
            raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
        if not (0 <= ce_weight < math.inf and 0 <= lovasz_weight < math.inf):
            raise ValueError("ce_weight and lovasz_weight must be finite and not negative")
        if ce_weight == 0 and lovasz_weight == 0:
            raise ValueError("ce_weight 0 with lovasz_weight 0 leaves no loss term")
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.classes, self.ce_weight, self.lovasz_weight = classes, float(ce_weight), float(lovasz_weight)
        self.ignore_index = ignore_index
        self.group = group
        self.last_present = None

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        if self.classes == 'foreground' and inputs.shape[1] < 2:
            raise ValueError("no foreground class among %d (empty class set)" % inputs.shape[1])
        w = _weight_for(self.weight, inputs)
        loss, sums = _LovaszLossFn.apply(inputs, targets, w, self.ignore_index, self.classes, self.ce_weight,
                                         self.lovasz_weight, self.group)
        self.last_present = sums[3]
        return loss


class _DistillLossFn(torch.autograd.Function):
    """ce_weight * weighted CE + distill_weight * tau^2 * KL(teacher || student) at temperature tau on the two-pass kernels
    (csrc/distill.hip): the forward pass stores nothing per pixel, the backward pass reads both logit tensors again and writes
    the finished gradient once.  Nothing is read back.  With `group` the five sums {sum w nll, sum w, sum KL, N, A} are
    all-reduced before the coefficients are formed, so both normalisers are the global batch's and the SUM gradient all-reduce
    of parallel.py yields the gradient of the global loss.  The teacher gets no gradient.  Good for one backward: a second one
    through the same call (retain_graph) is refused."""

    @staticmethod
    def forward(ctx, logits, labels, teacher, weight, ignore_index, temperature, ce_weight, distill_weight, group):
        sums = ops.distill_loss_fwd(logits, teacher, labels, weight, ignore_index, temperature)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        out, coef = ops.distill_loss_coeffs(sums, ce_weight, distill_weight, temperature)
        ctx.save_for_backward(logits, labels, teacher, weight, coef)
        ctx.ignore_index, ctx.temperature, ctx.consumed = ignore_index, temperature, False
        ctx.mark_non_differentiable(sums, out)
        return out[0].clone(), sums, out

    @staticmethod
    @once
    def backward(ctx, upstream, _sums, _out):
        if ctx.consumed:
            raise RuntimeError("DistillationLoss: %s" % CONSUMED)
        ctx.consumed = True
        logits, labels, teacher, weight, coef = ctx.saved_tensors
        grad = ops.distill_loss_bwd(logits, teacher, labels, weight, ctx.ignore_index, ctx.temperature, coef, _scalar(upstream))
        return grad, None, None, None, None, None, None, None, None


class DistillationLoss(nn.Module):
    """ce_weight * CrossEntropyLoss(weight, ignore_index) + distill_weight * temperature^2 * mean over the valid pixels of
    KL(softmax(teacher / temperature) || softmax(student / temperature)) (Hinton et al. 2015), called as
    ``criterion(logits, labels, teacher_logits)``.  The pixels are the ones the CE counts; the teacher's logits are a constant
    (a tensor that requires grad is refused).  Under `group` both means run over all ranks' pixels.  At most 8 classes.

    `last_terms` is a device view of {CE term, KD term} of the last call and `last_agreement` a pair of 0-dim device views
    (A, N): the valid pixels on which student and teacher predict the same class, and the valid pixels (of all ranks under
    `group`); reading either synchronises."""

    def __init__(self, temperature=1.0, ce_weight=1.0, distill_weight=1.0, weight=None, ignore_index=255, group=None):
        super().__init__()
        if not (0 < temperature < math.inf):
            raise ValueError("temperature must be positive and finite (got %r)" % (temperature,))
        if not (0 <= ce_weight < math.inf and 0 <= distill_weight < math.inf):
            raise ValueError("ce_weight and distill_weight must be finite and not negative")
        if ce_weight == 0 and distill_weight == 0:
            raise ValueError("ce_weight 0 with distill_weight 0 leaves no loss term")
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.temperature, self.ce_weight, self.distill_weight = float(temperature), float(ce_weight), float(distill_weight)
        self.ignore_index = ignore_index
        self.group = group
        self.last_terms = self.last_agreement = None

    def forward(self, inputs, targets, teacher_logits):
        if not torch.is_tensor(teacher_logits):
            raise TypeError("DistillationLoss is called as criterion(logits, labels, teacher_logits)")
        if teacher_logits.requires_grad:
            raise ValueError("the teacher's logits are a constant of the distillation loss: pass them detached (run the "
                             "teacher under torch.no_grad())")
        if teacher_logits.shape != inputs.shape:
            raise ValueError("teacher logits %s do not have the student's shape %s" %
                             (tuple(teacher_logits.shape), tuple(inputs.shape)))
        targets = _check(inputs, targets)
        w = _weight_for(self.weight, inputs)
        loss, sums, out = _DistillLossFn.apply(inputs, targets, teacher_logits, w, self.ignore_index, self.temperature,
                                               self.ce_weight, self.distill_weight, self.group)
        self.last_terms, self.last_agreement = out[1:], (sums[4], sums[3])
        return loss


class _BoundaryLossFn(torch.autograd.Function):
    """ce_weight * weighted CE + boundary_weight * mean over the valid pixels and the selected classes of p * phi, phi the
    signed distance to the ground-truth contour, on the two-pass kernels (csrc/boundary.hip): the forward pass stores nothing
    per pixel besides the distance map it is given, the backward pass reads logits, labels and map again and writes the
    finished gradient once.  Nothing is read back.  With `group` the four sums {sum w nll, sum w, sum p phi, N} are
    all-reduced before the coefficients are formed, so both normalisers are the global batch's and the SUM gradient all-reduce
    of parallel.py yields the gradient of the global loss.  Good for one backward: a second one through the same call
    (retain_graph) is refused."""

    @staticmethod
    def forward(ctx, logits, labels, sd2, weight, ignore_index, classes, clip, ce_weight, boundary_weight, group):
        sums = ops.boundary_loss_fwd(logits, labels, sd2, weight, ignore_index, classes, clip)
        if group is not None:
            import torch.distributed as dist
            dist.all_reduce(sums, group=group)
        out, coef = ops.boundary_loss_coeffs(sums, sd2.shape[1], ce_weight, boundary_weight)
        ctx.save_for_backward(logits, labels, sd2, weight, coef)
        ctx.ignore_index, ctx.classes, ctx.clip, ctx.consumed = ignore_index, classes, clip, False
        ctx.mark_non_differentiable(sums, out)
        return out[0].clone(), sums, out

    @staticmethod
    @once
    def backward(ctx, upstream, _sums, _out):
        if ctx.consumed:
            raise RuntimeError("BoundaryLoss: %s" % CONSUMED)
        ctx.consumed = True
        logits, labels, sd2, weight, coef = ctx.saved_tensors
        grad = ops.boundary_loss_bwd(logits, labels, sd2, weight, ctx.ignore_index, coef, _scalar(upstream), ctx.classes, ctx.clip)
        return grad, None, None, None, None, None, None, None, None, None


class BoundaryLoss(nn.Module):
    """ce_weight * CrossEntropyLoss(weight, ignore_index) + boundary_weight * the boundary loss of Kervadec et al. (MIDL 2019):
    the mean over the valid pixels and the classes of `classes` ('foreground': 1 .. C-1, 'all': 0 .. C-1) of
    softmax probability x signed Euclidean distance to the class's ground-truth contour (negative inside the mask, clamped to
    +-clip pixels when clip > 0).  The distance map is built from `targets` in every call, on the device and without a
    gradient (ops.signed_edt: exact, sides up to 4096).  Under `group` both means run over all ranks' pixels.  At most 8 classes.

    `boundary_weight` may be set between calls (a ramp): it is a host number handed to the coefficient kernel, so changing it
    costs no synchronisation.  `last_terms` is a device view of {CE term, boundary term} of the last call and `last_valid` a
    0-dim device view of N (of all ranks under `group`); reading either synchronises."""

    def __init__(self, classes='foreground', ce_weight=1.0, boundary_weight=1.0, clip=0.0, weight=None, ignore_index=255,
                 group=None):
        super().__init__()
        if classes not in ops.OVERLAP_CLASSES:
            raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
        if not (0 <= ce_weight < math.inf and 0 <= boundary_weight < math.inf):
            raise ValueError("ce_weight and boundary_weight must be finite and not negative")
        if ce_weight == 0 and boundary_weight == 0:
            raise ValueError("ce_weight 0 with boundary_weight 0 leaves no loss term")
        if not (0 <= clip < math.inf):
            raise ValueError("clip must be finite and not negative, 0 = no clamp (got %r)" % (clip,))
        self.register_buffer('weight', None if weight is None else weight.detach().float().clone())
        self.classes, self.ce_weight, self.boundary_weight, self.clip = classes, float(ce_weight), float(boundary_weight), float(clip)
        self.ignore_index = ignore_index
        self.group = group
        self.last_terms = self.last_valid = None

    def forward(self, inputs, targets):
        targets = _check(inputs, targets)
        lbd = float(self.boundary_weight)
        if not (0 <= lbd < math.inf):
            raise ValueError("boundary_weight must be finite and not negative (got %r)" % (self.boundary_weight,))
        w = _weight_for(self.weight, inputs)
        with torch.no_grad():
            sd2 = ops.signed_edt(targets, inputs.shape[1], self.classes, self.ignore_index)
        loss, sums, out = _BoundaryLossFn.apply(inputs, targets, sd2, w, self.ignore_index, self.classes, self.clip,
                                                self.ce_weight, lbd, self.group)
        self.last_terms, self.last_valid = out[1:], sums[3]
        return loss


def create_loss(loss_type="focal",temporal_loss="none", temporal_weight=0.5, **kwargs):
    """reference utils/loss.py:37-39"""
    return FocalLoss(**kwargs)


def calculate_class_weights(loader, group=None):
    """[1, sqrt(N_black / N_white)] over one pass of the loader -- train.py:388-410.

    Under data parallelism every rank iterates its own shard of the train set (DistributedSampler); the reference counts
    the WHOLE set, and the criterion's global normaliser assumes one common weight vector, so the two pixel counts are
    summed over the process group (int64 all-reduce) before the ratio is taken: every rank gets the same weights."""
    black = white = 0
    for batch in loader:
        labels = batch['mask'] if isinstance(batch, dict) else batch[1]
        black += int((labels == 0).sum())
        white += int((labels == 1).sum())
    black, white = _sum_over_group(black, white, group)
    return torch.tensor([1.0, math.sqrt(black / white)], dtype=torch.float32)


def _sum_over_group(black, white, group):
    """the two pixel counts summed over the process group (int64 all-reduce); unchanged without one"""
    try:
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            dev = torch.device("cuda", torch.cuda.current_device()) if dist.get_backend(group) == "nccl" else torch.device("cpu")
            cnt = torch.tensor([black, white], dtype=torch.int64, device=dev)
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM, group=group)
            black, white = int(cnt[0]), int(cnt[1])
    except ImportError:
        pass
    return black, white


def calculate_class_weights_resident(batches, group=None, ignore_index=255):
    """calculate_class_weights for batches that already live on the device -- the reference's rule (train.py:388-410:
    [1, sqrt(N_black / N_white)] over ONE pass of the augmented train loader, which also consumes the random stream).
    `batches` yields (images, uint8 labels on the GPU); every batch is counted by iswm_label_count into one device
    accumulator, which is read back once at the end; then the same int64 all-reduce over `group`."""
    import ctypes
    from .. import _lib
    lib = _lib.load()
    acc = ws = None
    for batch in batches:
        labels = batch['mask'] if isinstance(batch, dict) else batch[1]
        if not (labels.is_cuda and labels.dtype == torch.uint8 and labels.is_contiguous()):
            raise ValueError("calculate_class_weights_resident counts contiguous uint8 CUDA label batches (got %s %s on %s)"
                             % (tuple(labels.shape), labels.dtype, labels.device))
        with torch.cuda.device(labels.device):
            if acc is None:
                acc = torch.zeros(3, dtype=torch.int64, device=labels.device)
            n = labels.numel()
            need = lib.iswm_label_count_workspace(n)
            if ws is None or ws.numel() < need:
                ws = torch.empty(need, dtype=torch.uint8, device=labels.device)
            _lib.call("iswm_label_count", labels.data_ptr(), n, ignore_index, acc.data_ptr(), ws.data_ptr(), ws.numel(),
                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    if acc is None:
        raise ValueError("calculate_class_weights_resident: no batches")
    black, white, _other = (int(v) for v in acc.cpu())
    black, white = _sum_over_group(black, white, group)
    if white == 0:
        raise ValueError("no foreground (class 1) pixel in the %d counted: the class weight sqrt(N_black / N_white) is "
                         "undefined -- check the masks" % (black + white))
    return torch.tensor([1.0, math.sqrt(black / white)], dtype=torch.float32)
