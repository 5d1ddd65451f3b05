"""Execution layer of the HIP backend: modules with a hand-written forward AND
backward over NHWC activations.

The reference is a tree of stock ``torch.nn`` modules driven by autograd
(network/utils.py:16-25).  Here every module keeps the reference's name, children
and parameters (so ``state_dict`` keys match) but implements

    fwd(x, save)  -> y          NHWC in, NHWC out; ``save`` keeps what bwd needs
    bwd(dy, sink) -> dx         hand-written backward; parameter gradients are
                                written straight into ``p.grad`` via ``sink``

and the whole model is ONE node in torch's autograd graph (``_Bridge``), so
``loss.backward()`` / ``optimizer.step()`` in train.py work unchanged while no
torch op ever touches an activation.  All compute is libiswm_hip.so kernels.
"""
import dataclasses
import functools
import itertools
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..ops import Act


# Test hook: when set to a dict, cba_fwd records {bn_module: (out > 0)} for every fused ReLU so a
# parity test can hand the CPU oracle the exact sign pattern this path used (tests/test_hip_modules.py).
MASK_RECORDER = None
# ... and {MaxPool2d module: uint8 NHWC tap index (kh * 3 + kw) chosen per output element}: two fp32 implementations pick different
# elements of a near-tie, which re-routes that window's gradient (same kind of discontinuity as a flipped ReLU)
POOL_RECORDER = None
# Calibration hook (iswm_amd.quant.calibrating): when set, the output of every fused conv stage, the stem's max-pool and the
# ASPP / decoder concat buffers report their max |x| to it (recorder.record(module, tensor[, channels])).  None, the default,
# leaves the forward exactly as it is.
CALIB_RECORDER = None


def pad4(c):
    return (c + 3) // 4 * 4


def pad_cin(c):
    """channel count a conv's INPUT buffer is padded to: groups of 4 (16-byte loads) always; wide inputs
    that are not a multiple of the K chunk (the decoder's 304 = 48 + 256) go up to the next multiple of 32
    so the tap-uniform / bf16x6 kernels apply -- 5 % more MACs on zero channels buys a 1.5x faster kernel"""
    if c % 32 == 0 or c < 128:
        return pad4(c)
    return (c + 31) // 32 * 32


def dense_flat(t):
    """1-D view over the dense memory of a parameter-shaped tensor (contiguous or
    channels_last)."""
    if t.dim() == 4 and not t.is_contiguous():
        v = t.permute(0, 2, 3, 1)
        assert v.is_contiguous(), "parameter is neither contiguous nor channels_last"
        return v.reshape(-1)
    assert t.is_contiguous()
    return t.reshape(-1)


class GradSink:
    """Where parameter gradients go.  ``target(p)`` returns a tensor shaped/strided
    like ``p`` for a kernel to overwrite; ``done(p)`` folds it into ``p.grad``
    (a no-op on the usual zero_grad(set_to_none=True) path) and fires the
    data-parallel ready hook.  A bridge also puts its call's serial on it, which ``take`` checks."""

    def __init__(self, on_ready=None, serial=None):
        self.on_ready = on_ready
        self.serial = serial             # of the forward call this backward belongs to (take); None: fwd / bwd driven by hand
        self._pending = {}

    def target(self, p):
        if p.grad is None:
            view = getattr(p, "_iswm_grad_view", None)
            p.grad = view if view is not None else torch.empty_like(p)
            return p.grad
        tmp = torch.empty_like(p)
        self._pending[id(p)] = tmp
        return tmp

    def done(self, p):
        tmp = self._pending.pop(id(p), None)
        if tmp is not None:
            ops.add_inplace(dense_flat(p.grad), dense_flat(tmp))
        if self.on_ready is not None:
            self.on_ready(p)


# ---------------------------------------------------------------------------------------
# What a forward saves for its backward lives on the modules (one slot each), not per call as under autograd.  So a
# backward must find the state ITS forward saved, or refuse: every bridge draws a serial per call and hands it down as
# `save` (a positive int: still truthy) and, on the GradSink, to the backward; `keep` stamps what it stores with it and
# enters the module in the call's list, `take` checks the stamp, and `claim` checks every module of the call before a
# bridge's backward launches anything.  Nothing here is thread-local: the autograd engine runs backward on a thread of
# its own.
# ---------------------------------------------------------------------------------------
_SERIALS = itertools.count(1)

REPLACED = ("a later forward of this module (or of a module containing / contained in it) replaced the state saved for "
            "this backward; run forward and backward of each batch in turn, gradients accumulate")
CONSUMED = ("the state saved for this backward was already consumed (a second backward through the same call, "
            "`retain_graph`, is not supported)")


class Serial(int):
    """the number of one forward call through a bridge, with the modules that kept state for it (`mods`, in the order
    their fwd finished).  The modules are stamped with the plain int, so they hold no reference back to the call."""

    def __new__(cls, value):
        self = int.__new__(cls, value)
        self.mods = []
        return self


def new_serial():
    """the Serial of a new forward call: a number no other call has (next() of itertools.count is atomic)"""
    return Serial(next(_SERIALS))


def _refuse(mod, why, root=None):
    name = type(mod).__name__
    if root is not None and root is not mod:
        name = "%s (at its %s)" % (type(root).__name__, name)
    return RuntimeError("%s: %s" % (name, why))


def keep(mod, save, payload):
    """the end of a module's fwd: store `payload` for the backward of call `save` (a bridge's Serial; True when fwd / bwd
    are driven by hand: no stamp to check).  A falsy `save` stores nothing and clears what an earlier call left -- and
    stamps the module all the same, so that the backward of that earlier call sees a forward came in between."""
    if not save:
        mod._saved, mod._stamp = None, next(_SERIALS)
    elif save is True:
        mod._saved, mod._stamp = payload, None
    else:
        mod._saved, mod._stamp = payload, int(save)
        save.mods.append(mod)


def peek(mod, sink):
    """what take(mod, sink) would return, left in place; None when the module holds nothing for this call"""
    serial = getattr(sink, "serial", None)
    if serial is not None and getattr(mod, "_stamp", None) != serial:
        return None
    return getattr(mod, "_saved", None)


def take(mod, sink):
    """the start of a module's bwd: the payload keep() stored for this call, cleared from the module.  RuntimeError when
    another forward's state stands there (REPLACED) or none (CONSUMED) -- never a wrong gradient."""
    payload, stamp = getattr(mod, "_saved", None), getattr(mod, "_stamp", None)
    mod._saved = None
    serial = getattr(sink, "serial", None)
    if serial is not None and stamp != serial:
        raise _refuse(mod, REPLACED)
    if payload is None:
        raise _refuse(mod, CONSUMED)
    return payload


def claim(root, serial):
    """A bridge's backward calls this first, before it launches a kernel or touches a .grad: every module that kept state
    for the forward call `serial` (the bridge's Serial) still holds it.  If another forward went through one of them since
    -- whole or in part, saving or not -- the state under `root` is dropped (the module is usable again) and REPLACED
    raised; if the call's state is gone already, CONSUMED."""
    for m in reversed(serial.mods):                     # `root` first: it kept last
        if m._stamp != serial:
            drop(root)
            raise _refuse(m, REPLACED, root)
        if m._saved is None:
            raise _refuse(m, CONSUMED, root)


def drop(root):
    """forget whatever the modules under `root` hold for a backward; a backward that still counts on it gets REPLACED"""
    for m in root.modules():
        if getattr(m, "_stamp", None) is not None or getattr(m, "_saved", None) is not None:
            m._saved, m._stamp = None, next(_SERIALS)


def once(backward):
    """torch's once_differentiable for a hand-written backward, and strict: under create_graph=True (the engine then runs
    backward with grad mode on) torch's decorator lets a gradient that is no function of anything through unless the
    upstream gradient itself requires grad; here the call is refused, so a gradient penalty cannot silently be zero."""
    inner = torch.autograd.function.once_differentiable(backward)

    @functools.wraps(backward)
    def wrapper(ctx, *args):
        if torch.is_grad_enabled():
            raise RuntimeError("trying to differentiate twice a function that was marked with @once_differentiable: %s is "
                               "a hand-written kernel pass and builds no graph (create_graph=True is not supported)" %
                               backward.__qualname__.split(".")[0])
        return inner(ctx, *args)
    return wrapper


def _bias_grad(bias, dy, sink):
    """gradient of a conv bias (possibly None or frozen) = the column sums of dy, into the sink"""
    if bias is not None and bias.requires_grad:
        ops.unpad_weights(ops.colsum(dy).view(-1, 1, 1, 1), sink.target(bias).view(-1, 1, 1, 1))
        sink.done(bias)


class HipModule(nn.Module):
    """Base: public ``forward`` takes/returns NCHW like the reference module and
    bridges to fwd/bwd."""

    def fwd(self, x, save):
        raise NotImplementedError

    def bwd(self, dy, sink):
        raise NotImplementedError

    def out_channels_of(self, cin):
        """logical channel count of the output (to strip channel padding)."""
        return None

    def forward(self, x):
        return run_module(self, x)


class _Bridge(torch.autograd.Function):
    """One autograd node for a whole HipModule call (NCHW tensors outside)."""

    @staticmethod
    def forward(ctx, mod, cout, x, *params):
        xh = ops.nchw_to_nhwc(x)
        ctx.serial = new_serial()
        yh = mod.fwd(xh, ctx.serial)
        ctx.mod, ctx.cin, ctx.need_dx = mod, x.shape[1], x.requires_grad
        return ops.nhwc_to_nchw(yh, cout or yh.shape[3])

    @staticmethod
    @once
    def backward(ctx, dy):
        mod = ctx.mod
        claim(mod, ctx.serial)
        dyh = ops.nchw_to_nhwc(dy.contiguous())
        sink = GradSink(getattr(mod, "_iswm_on_ready", None), ctx.serial)
        dxh = mod.bwd(dyh, sink)
        dx = ops.nhwc_to_nchw(dxh, ctx.cin) if (ctx.need_dx and dxh is not None) else None
        return (None, None, dx) + (None,) * (len(ctx.needs_input_grad) - 3)


def run_module(mod, x):
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
        raise ValueError("iswm_amd modules take a 4-D fp32 CUDA NCHW tensor (no CPU fallback); got %s" %
                         (x.shape if torch.is_tensor(x) else type(x),))
    params = [p for p in mod.parameters() if p.requires_grad]
    cout = mod.out_channels_of(x.shape[1])
    if torch.is_grad_enabled() and (x.requires_grad or params):
        return _Bridge.apply(mod, cout, x, *params)
    yh = mod.fwd(ops.nchw_to_nhwc(x), False)
    return ops.nhwc_to_nchw(yh, cout or yh.shape[3])


# ---------------------------------------------------------------------------------------
# leaf modules: same classes/keys as torch.nn so isinstance checks in the reference's
# _init_weight (network/_deeplab.py:63-69) and state_dict round-trips keep working
# ---------------------------------------------------------------------------------------
class Conv2d(HipModule, nn.Conv2d):
    """nn.Conv2d(groups=1) whose weight lives in channels_last memory format, i.e.
    physically OHWI -- the layout the implicit-GEMM kernels read directly."""

    def __init__(self, *args, **kwargs):
        nn.Conv2d.__init__(self, *args, **kwargs)
        if self.groups != 1 or self.padding_mode != "zeros":
            raise NotImplementedError("HIP conv supports groups=1, zero padding")
        if self.kernel_size[0] != self.kernel_size[1] or self.dilation[0] != self.dilation[1] or \
                self.stride[0] != self.stride[1] or self.padding[0] != self.padding[1]:
            raise NotImplementedError("HIP conv supports square kernels/strides/dilations")
        with torch.no_grad():
            self.weight.data = self.weight.data.contiguous(memory_format=torch.channels_last)
        self._saved = None

    # -- operand views -----------------------------------------------------------------
    @property
    def cin_p(self):
        return pad_cin(self.in_channels)

    @property
    def cout_p(self):
        return pad4(self.out_channels)

    def needs_pack(self):
        return self.cin_p != self.in_channels or self.cout_p != self.out_channels

    def ohwi(self):
        """OHWI weight for the kernels; zero-padded copy when Cin/Cout % 4 != 0
        (the 3-channel stem, the num_classes-wide classifier)."""
        w = self.weight
        v = w.permute(0, 2, 3, 1)
        if not self.needs_pack():
            return v if v.is_contiguous() else v.contiguous()
        return ops.pad_weights(w, self.cout_p, self.cin_p)

    def weight_for(self, kind):
        """the ops.ConvWeight of the forward (kind 0) / data gradient (1): the OHWI weight plus what the model's WeightPacker
        pre-packed from it for the bf16x6 ("x6") and the planes ("pl2") kernels.  Those buffers count only inside the
        forward/backward window they were made for and only while the parameter is untouched; the kernel wrappers pack the
        weight themselves otherwise."""
        w, e = self.ohwi(), getattr(self, "_iswm_wpk", None)
        if e is None or not e["live"] or e["epoch"] != ops.WEIGHTS_EPOCH or e["version"] != self.weight._version or \
                e["ptr"] != self.weight.data_ptr():
            return ops.ConvWeight(w)
        return ops.ConvWeight(w, {"x6": e["buf"][kind], "pl2": e["buf"][kind + 2]})

    def bias_p(self):
        if self.bias is None:
            return None
        if self.cout_p == self.out_channels:
            return self.bias
        return ops.pad_weights(self.bias.view(-1, 1, 1, 1), self.cout_p, 1).view(-1)

    def geometry(self, x):
        if x.shape[3] != self.cin_p:
            raise ValueError("conv expects %d (padded) input channels, got %d" % (self.cin_p, x.shape[3]))
        g = ops.ConvGeom(x, self.cout_p, self.kernel_size[0], self.kernel_size[1], self.stride[0],
                         self.padding[0], self.dilation[0])
        g.alg_cin, g.alg_cout = self.in_channels, self.out_channels
        return g

    def write_wgrad(self, x, dy, g, sink):
        """weight gradient straight into p.grad's memory when it is OHWI-dense."""
        p = self.weight
        if not p.requires_grad:
            return
        buf = sink.target(p)
        v = buf.permute(0, 2, 3, 1)
        if not self.needs_pack() and v.is_contiguous():
            ops.conv2d_wgrad(x, dy, g, v)
        else:
            ops.unpad_weights(ops.conv2d_wgrad(x, dy, g), buf)
        sink.done(p)

    # -- standalone conv (+bias), e.g. the final 1x1 classifier ---------------------------
    def fwd(self, x, save, out=None):
        g = self.geometry(x)
        y, _, _ = ops.conv2d_fwd(x, self.weight_for(0), g, bias=self.bias_p(), out=out)
        keep(self, save, (x, g))
        return y

    def bwd(self, dy, sink, need_dx=True, dx=None, accumulate=False):
        x, g = take(self, sink)
        _bias_grad(self.bias, dy, sink)
        self.write_wgrad(x, dy, g, sink)
        if not need_dx:
            return None
        return ops.conv2d_dgrad(dy, self.weight_for(1), g, tuple(x.shape), dx, accumulate)

    def out_channels_of(self, cin):
        return self.out_channels


class DepthwiseConv2d(HipModule, nn.Conv2d):
    """nn.Conv2d(C, C, k, groups=C): the depthwise half of AtrousSeparableConvolution (network/_deeplab.py:103).
    The parameter keeps torch's [C,1,KH,KW] layout; the activation may be a zero-padded buffer wider than C."""

    def __init__(self, *args, **kwargs):
        nn.Conv2d.__init__(self, *args, **kwargs)
        if self.groups != self.in_channels or self.out_channels != self.in_channels or self.padding_mode != "zeros":
            raise NotImplementedError("HIP depthwise conv needs groups == in_channels == out_channels, zero padding")
        if self.kernel_size[0] != self.kernel_size[1] or self.dilation[0] != self.dilation[1] or \
                self.stride[0] != self.stride[1] or self.padding[0] != self.padding[1]:
            raise NotImplementedError("HIP depthwise conv supports square kernels/strides/dilations")
        self._saved = None

    def geometry(self, x):
        c = x.shape[3]
        if c < self.in_channels or c % 4 != 0:
            raise ValueError("depthwise conv over %d channels got a %d-channel buffer" % (self.in_channels, c))
        return ops.ConvGeom(x, c, self.kernel_size[0], self.kernel_size[1], self.stride[0], self.padding[0],
                            self.dilation[0])

    def fwd(self, x, save, out=None):
        g = self.geometry(x)
        y = ops.dwconv2d_fwd(x, self.weight.contiguous(), g, self.bias, out)
        keep(self, save, (x, g))
        return y

    def is_dw3x3(self):
        """the geometry csrc/dwconv3.hip covers: 3x3, stride 1 / 2, padding == dilation, no bias (MobileNetV2's)"""
        return (self.kernel_size[0] == 3 and self.stride[0] in (1, 2) and self.padding[0] == self.dilation[0] and
                self.bias is None)

    def fwd_stats(self, x, save, want_stats):
        """forward of a depthwise -> BatchNorm stage (is_dw3x3): (y, partials | None, (tiles, tile_rows)), the tile
        statistics taken by the convolution's own launch"""
        g = self.geometry(x)
        y, partials, tiles = ops.dwconv3x3_fwd_stats(x, self.weight.contiguous(), g, want_stats)
        keep(self, save, (x, g))
        return y, partials, tiles

    def bwd_fused(self, dy, sink, need_dx=True, dx=None, accumulate=False):
        """backward of fwd_stats: data and weight gradient from one pass over dy and x"""
        x, g = take(self, sink)
        need_dw, buf, tgt = self.weight.requires_grad, None, None
        if need_dw:
            buf = sink.target(self.weight)
            tgt = buf if buf.is_contiguous() else None
        if not (need_dx or need_dw):
            return None
        dx, dw = ops.dwconv3x3_bwd(x, dy, self.weight.contiguous(), g, self.in_channels, dx, accumulate, tgt, need_dx, need_dw)
        if need_dw:
            if tgt is None:
                buf.copy_(dw)
            sink.done(self.weight)
        return dx

    def bwd(self, dy, sink, need_dx=True, dx=None, accumulate=False):
        x, g = take(self, sink)
        _bias_grad(self.bias, dy, sink)
        if self.weight.requires_grad:
            buf = sink.target(self.weight)
            if buf.is_contiguous():
                ops.dwconv2d_wgrad(x, dy, g, self.in_channels, buf)
            else:
                buf.copy_(ops.dwconv2d_wgrad(x, dy, g, self.in_channels))
            sink.done(self.weight)
        if not need_dx:
            return None
        return ops.dwconv2d_dgrad(dy, self.weight.contiguous(), g, tuple(x.shape), dx, accumulate)

    def out_channels_of(self, cin):
        return self.out_channels


class BatchNorm2d(nn.BatchNorm2d):
    pass


class ReLU(nn.ReLU):
    pass


class ReLU6(nn.ReLU6):
    """nn.ReLU6 (MobileNetV2's activation): fused into the BatchNorm pass like ReLU (clamp to [0, 6])"""
    pass


class Dropout(HipModule, nn.Dropout):
    """nn.Dropout(p) (network/_deeplab.py:165) with a Philox counter mask."""

    def __init__(self, *a, **k):
        nn.Dropout.__init__(self, *a, **k)
        self._calls = 0
        self._saved = None

    def fwd(self, x, save):
        if not self.training or self.p == 0.0:
            keep(self, save, (None,))                   # the identity: no mask
            return x
        self._calls += 1
        y, mask = ops.dropout_fwd(x, self.p, torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, self._calls)
        keep(self, save, (mask,))
        return y

    def bwd(self, dy, sink):
        mask, = take(self, sink)
        if mask is None:
            return dy
        return ops.dropout_bwd(dy.contiguous(), mask, self.p)


# ---------------------------------------------------------------------------------------
# conv -> BatchNorm -> (+residual) -> ReLU, the unit every stage of the net is made of
# ---------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Stage(object):
    """One fused unit of a module, as its `_stages()` describes it; it holds modules only, never a call's state.
    kind "cba": conv -> bn -> act (`conv` may be a SeparableBase or a DepthwiseConv2d); "conv": a Conv2d (+ bias) alone;
    "mod": any other HipModule, in `conv`."""
    kind: str
    conv: nn.Module
    bn: Optional[nn.Module] = None
    act: Act = Act.NONE

    def __post_init__(self):
        if self.kind not in ("cba", "conv", "mod") or not isinstance(self.act, Act):
            raise ValueError("bad stage: kind %r, act %r" % (self.kind, self.act))

    @property
    def bn_conv(self):
        """the convolution whose output the BatchNorm reads: the pointwise half of a separable conv, else `conv`"""
        return self.conv.body[1] if isinstance(self.conv, SeparableBase) else self.conv


class StageCtx(object):
    """What one forward of a "cba" stage keeps for its backward: x the input of `stage.bn_conv`, y its raw output, out the stage's
    output (None behind a folded classifier), coef [4, C] of the BatchNorm, g the conv geometry, res whether a residual was
    added, sep the SeparableBase / dw whether the conv is depthwise (both follow from the stage), bn_stats the ops.BnStats a
    consumer's data gradient filled for this stage's BatchNorm backward, cls / wc4 the classifier folded into the stage and its
    padded weight."""
    __slots__ = ("stage", "x", "y", "out", "coef", "g", "training", "res", "sep", "dw", "bn_stats", "cls", "wc4")

    def __init__(self, stage, x, y, coef, g, training, out=None, res=False, cls=None, wc4=None):
        self.stage, self.x, self.y, self.out, self.coef, self.g, self.training, self.res = stage, x, y, out, coef, g, training, res
        self.sep = stage.conv if isinstance(stage.conv, SeparableBase) else None
        self.dw = isinstance(stage.bn_conv, DepthwiseConv2d)
        self.bn_stats, self.cls, self.wc4 = None, cls, wc4


def cba_fwd(conv, bn, relu, x, save, residual=None, out=None, out_fmt=None):
    """Returns (out, ctx).  relu: an ops.Act, or True / False / 6.  Training-mode BN statistics come from the conv epilogue's
    per-tile partial sums (no extra pass over y).  The output is written pre-split (ops.Planes) when a convolution
    will consume it: `out` (a buffer slice) decides, else out_fmt ("planes" / "f32"), else the channel count."""
    stage = Stage("cba", conv, bn, Act.of(relu))
    if isinstance(conv, SeparableBase):         # depthwise first, then the pointwise conv carries the fused BN
        x = conv.body[0].fwd(x, save)
        conv = stage.bn_conv
    training = bn.training
    if bn.momentum is None or not bn.track_running_stats or not bn.affine:
        raise NotImplementedError("HIP BatchNorm2d supports affine=True, momentum!=None, running stats")
    g = conv.geometry(x)
    if isinstance(conv, DepthwiseConv2d):       # depthwise conv -> BN (MobileNetV2)
        if conv.is_dw3x3():                     # statistics from the convolution's own launch (csrc/dwconv3.hip)
            y, partials, tiles = conv.fwd_stats(x, save, training)
        else:                                   # other filter sizes: statistics from a column pass
            y = conv.fwd(x, save)
            partials, tiles = _colstat_partials(y, training)
    elif conv.bias is None:
        y, partials, tiles = ops.conv2d_fwd(x, conv.weight_for(0), g, want_stats=training)
    else:
        # a biased conv in front of a BatchNorm (only reachable through convert_to_separable_conv on a biased
        # conv): the fused epilogue statistics do not include the bias, so take them in a separate column pass
        y, _, _ = ops.conv2d_fwd(x, conv.weight_for(0), g, bias=conv.bias_p())
        partials, tiles = _colstat_partials(y, training)
    return _cba_finish(stage, x=x, y=y, g=g, partials=partials, tiles=tiles, training=training, save=save, residual=residual,
                       out=out, out_fmt=out_fmt)


def _colstat_partials(y, training):
    """(partials | None, (tiles, tile_rows)) of a stage whose producer publishes no tile statistics: a column pass over y"""
    if not training:
        return None, (0, 0)
    partials, nt, tr = ops.colstat(y)
    return partials, (nt, tr)


def _bn_coef(bn, y, partials, tiles, training):
    """coef [4, C] = (scale, shift, mean, invstd) of a stage's BatchNorm: from the tile statistics of y when training (the
    running buffers and the batch counter move), else from the running buffers"""
    if not training:
        return ops.bn_eval_coeffs(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    count = y.shape[0] * y.shape[1] * y.shape[2]
    if count <= 1:
        # same contract as torch (network/_deeplab.py:130-141 needs batch >= 2)
        raise ValueError("Expected more than 1 value per channel when training, got input size %s" % (tuple(y.shape),))
    coef = ops.bn_finalize(partials, tiles[0], count, tiles[1], bn.weight, bn.bias, bn.running_mean, bn.running_var,
                           bn.momentum, bn.eps)
    if not getattr(bn, "_iswm_nbt_fused", False):
        bn.num_batches_tracked.add_(1)     # models built by modeling.* bump all counters in ONE op
    return coef


def _bn_grad_targets(bn, sink):
    """(dgamma, dbeta) for the BatchNorm backward to write: the sink's targets, scratch for a frozen parameter"""
    return [sink.target(p) if p.requires_grad else torch.empty_like(p) for p in (bn.weight, bn.bias)]


def _bn_grads_done(bn, sink):
    for p in (bn.weight, bn.bias):
        if p.requires_grad:
            sink.done(p)


def _cba_finish(stage, *, x, y, g, partials, tiles, training, save, residual=None, out=None, out_fmt=None):
    """BatchNorm coefficients from the tile statistics of y, then the apply pass (+ residual, activation): (out, ctx)"""
    coef = _bn_coef(stage.bn, y, partials, tiles, training)
    if out_fmt is None:
        want_planes = ops.planes_on() and y.shape[3] % 64 == 0
    else:
        want_planes = out_fmt == "planes" and ops.planes_on() and y.shape[3] % 64 == 0
    o = ops.bn_apply(y, coef, stage.act, residual, out, planes=want_planes)
    if MASK_RECORDER is not None and stage.act is not Act.NONE:
        of = ops.as_f32(o)
        MASK_RECORDER[stage.bn] = (of > 0) & (of < 6) if stage.act is Act.RELU6 else (of > 0)
    if CALIB_RECORDER is not None:
        CALIB_RECORDER.record(stage.bn_conv, o)
    return o, StageCtx(stage, x, y, coef, g, training, out=o, res=residual is not None) if save else None


_BN3_FUSE = True      # False: residual stages reduce themselves (tests compare both paths)


def _bn_stats_request(up):
    """`up` = ctx of the stage that produced this stage's input, when ITS BatchNorm backward is the only consumer of the dx this
    stage returns: the planes data gradient then takes that backward's reduction pass in its epilogue (ops.BnStats)."""
    if up is None or not ops.planes_on() or up.bn_stats is not None:
        return None
    act = up.stage.act
    # a residual stage (bn3 + identity + ReLU): the pattern is read from its saved output planes and the data gradient
    # stores dx masked -- see ops.BnStats.mask
    if act is Act.RELU6 or (up.res and not (_BN3_FUSE and act is Act.RELU and ops.is_planes(up.out) and up.training)):
        return None
    return ops.BnStats(up.y, up.coef, act, mask=up.out if up.res else None)


def cba_bwd_bn(ctx, dout, sink, dy_out=None, need_dx=True, want_dres=True):
    """the BatchNorm (+ activation) backward of the stage that made `ctx`: parameter gradients into the sink, returns (dy, dres)
    with dy the gradient of the raw conv output -- pre-split when the conv's gradient kernels take planes; dy_out: write it there
    (a Planes slice of a wider buffer: the fused ASPP data gradient reads the four branches' gradients from one tensor);
    want_dres=False: the caller takes no gradient of the residual input from this stage"""
    conv, bn, act = ctx.stage.bn_conv, ctx.stage.bn, ctx.stage.act
    res = ctx.res and want_dres
    gw = bn.weight
    dgamma, dbeta = _bn_grad_targets(bn, sink)
    # planes only when a planes kernel will read them: the data gradient, or the weight gradient of a pre-split input (the stem
    # has neither: its gradient stays fp32 instead of being split here and joined again for the weight gradient)
    dyp = (not ctx.dw) and ops.planes_conv_ok(conv.cin_p, conv.cout_p, 1) and (need_dx or ops.is_planes(ctx.x))
    st, ctx.bn_stats = ctx.bn_stats, None
    if st is not None and st.partials is not None and st.masked:
        dout = ops.as_f32(dout)
        dy, _ = ops.bn_backward(dout, None, ctx.y, ctx.coef, gw, Act.NONE, ctx.training, dgamma, dbeta, want_dres=False,
                                dy=dy_out, dy_planes=dyp, stats=st)
        dres = dout if res else None
    else:
        dy, dres = ops.bn_backward(ops.as_f32(dout), ctx.out if act is not Act.NONE else None, ctx.y, ctx.coef, gw, act,
                                   ctx.training, dgamma, dbeta, want_dres=res, dy=dy_out, dy_planes=dyp, stats=st)
    _bn_grads_done(bn, sink)
    return dy, dres


def cba_bwd(ctx, dout, sink, need_dx=True, dx=None, accumulate=False, up=None, want_dres=True):
    """Backward of the stage that made `ctx`.  Returns (dx, dres): dres is the gradient of the residual input (if any; never with
    want_dres=False).  up: see _bn_stats_request."""
    x, g, sep, conv = ctx.x, ctx.g, ctx.sep, ctx.stage.bn_conv
    dy, dres = cba_bwd_bn(ctx, dout, sink, need_dx=need_dx or sep is not None, want_dres=want_dres)
    if ctx.dw:
        if conv.is_dw3x3():
            return conv.bwd_fused(dy, sink, need_dx, dx, accumulate), dres
        return conv.bwd(dy, sink, need_dx, dx, accumulate), dres
    conv.write_wgrad(x, dy, g, sink)
    _bias_grad(conv.bias, dy, sink)
    if sep is not None:
        dmid = ops.conv2d_dgrad(dy, conv.weight_for(1), g, tuple(x.shape))
        return sep.body[0].bwd(dmid, sink, need_dx, dx, accumulate), dres
    if need_dx:
        req = _bn_stats_request(up) if (up is not None and tuple(up.y.shape) == tuple(x.shape)) else None
        dx = ops.conv2d_dgrad(dy, conv.weight_for(1), g, tuple(x.shape), dx, accumulate, bn_stats=req)
        if req is not None and req.partials is not None:
            up.bn_stats = req
    else:
        dx = None
    return dx, dres


def fuse_batch_counters(root):
    """Re-home every BatchNorm's ``num_batches_tracked`` into one int64 tensor so a training forward
    bumps all of them with a single op (113 tiny launches per step for ResNet-101 otherwise).  The
    buffers stay registered under their usual state_dict keys (they become views)."""
    bns = [m for m in root.modules() if isinstance(m, nn.BatchNorm2d) and m.num_batches_tracked is not None]
    if not bns:
        return None
    flat = torch.stack([m.num_batches_tracked.detach().reshape(()) for m in bns]).contiguous()
    for i, m in enumerate(bns):
        m._buffers["num_batches_tracked"] = flat[i]
        m._iswm_nbt_fused = True
    return flat


class WeightPacker(object):
    """Packs the weights of every (unpadded) Conv2d under `root` for the bf16x6 kernels in ONE launch per forward
    pass -- the exact 3-way split in MFMA fragment order, csrc/conv_mfma_x6.hip k_pack_weights_batch -- instead of
    two tiny launches per conv per step.  Buffers and the device job table persist; they are rebuilt when a
    parameter moved.  `begin()` at the start of a model forward makes the buffers live, `end()` retires them."""

    def __init__(self, root):
        self.convs = [m for m in root.modules() if isinstance(m, Conv2d) and not m.needs_pack()]
        self.key, self.jobs, self.njobs, self.blocks, self.entries = None, None, 0, 0, []

    def _build(self, dev):
        from .. import _lib
        lib = _lib.load()
        jobs, entries, first = [], [], 0
        keep = []
        for m in self.convs:
            w = m.weight
            v = w.permute(0, 2, 3, 1)
            if not (w.is_cuda and v.is_contiguous()):
                continue
            taps = m.kernel_size[0] * m.kernel_size[1]
            bufs = {}
            # with pre-split activations the planes kernels take the conv (kinds 2 / 3); the fp32-input fragment order
            # (kinds 0 / 1) is packed only for the direction the planes kernels do not cover
            kinds = []
            for kind in (0, 1):
                if ops.planes_on() and lib.iswm_packed_weight_bytes(m.out_channels, taps, m.in_channels, kind + 2):
                    kinds.append(kind + 2)
                else:
                    kinds.append(kind)
            for kind in kinds:
                nb = lib.iswm_packed_weight_bytes(m.out_channels, taps, m.in_channels, kind)
                if nb == 0:
                    continue
                buf = torch.empty((nb // 4,), dtype=torch.float32, device=dev)
                bufs[kind] = buf
                jobs.append((w.data_ptr(), buf.data_ptr(), m.out_channels, taps, m.in_channels, kind, first, 0))
                first += lib.iswm_pack_job_blocks(m.out_channels, taps, m.in_channels, kind)
            if bufs:
                e = dict(live=False, epoch=-1, version=-1, ptr=w.data_ptr(), buf={k: bufs.get(k) for k in range(4)})
                m._iswm_wpk = e
                entries.append((m, e))
                keep.append(bufs)
        job = _lib.STRUCTS["iswm_pack_job"]
        arr = (job * max(1, len(jobs)))(*(job(*j) for j in jobs))
        self.jobs = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev) if jobs else None
        self.njobs, self.blocks, self.entries = len(jobs), first, entries

    def begin(self):
        from .. import _lib
        math = _lib.load().iswm_get_conv_math()
        if math < 1 or not ops._USE_PACKED or not self.convs:
            return
        key = (math, ops.planes_on()) + tuple(m.weight.data_ptr() for m in self.convs)      # bf16x6 packs 3 planes, bf16 one
        if key != self.key:
            self._build(self.convs[0].weight.device)
            self.key = key
        if self.njobs == 0:
            return
        ops.call("iswm_pack_weights_batch", ops._p(self.jobs), self.njobs, self.blocks, ops._stream())
        for m, e in self.entries:
            e["live"], e["epoch"], e["version"] = True, ops.WEIGHTS_EPOCH, m.weight._version

    def end(self):
        for _, e in self.entries:
            e["live"] = False


_CLS_FUSE = True      # False: the classifier as a conv of its own (tests compare both paths)


def cls_fusable(stage, cls):
    """[Conv2d(.., 256, k) -> BatchNorm2d -> ReLU] followed by the 1x1 classifier Conv2d(256, num_classes <= 4, 1): the tail of both
    DeepLab heads (network/_deeplab.py:44-52, 84-90).  The classifier is then folded into the stage's BatchNorm passes
    (csrc/bn_classify.hip).  Not while a calibration records ranges (it needs the stage's stored output); a test's ReLU-pattern
    recorder is served by cba_cls_fwd itself."""
    conv, bn = stage.conv, stage.bn
    return (_CLS_FUSE and CALIB_RECORDER is None and stage.act is Act.RELU and type(conv) is Conv2d and conv.out_channels == 256 and
            conv.bias is None and type(cls) is Conv2d and cls.in_channels == 256 and cls.out_channels <= 4 and
            tuple(cls.kernel_size) == (1, 1) and tuple(cls.stride) == (1, 1) and tuple(cls.padding) == (0, 0) and
            bn.momentum is not None and bn.track_running_stats and bn.affine)


def cba_cls_fwd(stage, cls, x, save):
    """conv -> BatchNorm -> ReLU -> 1x1 classifier with the activation never stored: returns (logits [N,H,W,4], ctx)"""
    conv, bn = stage.conv, stage.bn
    g = conv.geometry(x)
    training = bn.training
    y, partials, tiles = ops.conv2d_fwd(x, conv.weight_for(0), g, want_stats=training)
    coef = _bn_coef(bn, y, partials, tiles, training)
    wc4 = ops.pad_weights(cls.weight, 4, 256).view(4, 256)
    b4 = None if cls.bias is None else ops.pad_weights(cls.bias.view(-1, 1, 1, 1), 4, 1).view(-1)
    logits = ops.bn_apply_classify(y, coef, wc4, b4)
    if MASK_RECORDER is not None:
        # the stage's ReLU pattern, as _cba_finish records it: the unfused apply on the same y and coefficients evaluates the
        # fold's (y - mean) * scale + shift (tests/test_cls_fuse.py pins all of the fold's decisions to it bit for bit)
        MASK_RECORDER[bn] = ops.bn_apply(y, coef, Act.RELU) > 0
    return logits, StageCtx(stage, x, y, coef, g, training, cls=cls, wc4=wc4) if save else None


def cba_cls_bwd(ctx, dlogit, sink, need_dx=True, dx=None, accumulate=False):
    """backward of cba_cls_fwd: classifier bias / weight gradients, the stage's BatchNorm backward fed by dlogit, then the
    conv's weight and data gradients as in cba_bwd"""
    conv, bn = ctx.stage.conv, ctx.stage.bn
    cls, x, y, g = ctx.cls, ctx.x, ctx.y, ctx.g
    dlogit = ops.as_f32(dlogit)
    _bias_grad(cls.bias, dlogit, sink)
    gw = bn.weight
    dgamma, dbeta = _bn_grad_targets(bn, sink)
    dyp = ops.planes_conv_ok(conv.cin_p, conv.cout_p, 1)
    dy, dwc4 = ops.bn_backward_classify(dlogit, ctx.wc4, y, ctx.coef, gw, ctx.training, dgamma, dbeta, dyp)
    _bn_grads_done(bn, sink)
    if cls.weight.requires_grad:
        ops.unpad_weights(dwc4.view(4, 1, 1, 256), sink.target(cls.weight))
        sink.done(cls.weight)
    conv.write_wgrad(x, dy, g, sink)
    if not need_dx:
        return None
    return ops.conv2d_dgrad(dy, conv.weight_for(1), g, tuple(x.shape), dx, accumulate)


class SeparableBase(HipModule):
    """marker base of _deeplab.AtrousSeparableConvolution (body = [DepthwiseConv2d, pointwise Conv2d]) so that the
    conv -> BN -> ReLU stage logic here can recognise it without importing _deeplab"""
    pass


class HipSequential(HipModule, nn.Sequential):
    """nn.Sequential whose children are grouped into fused stages:
    [Conv2d, BatchNorm2d, ReLU?] -> cba;  Conv2d alone -> conv(+bias);  Dropout;  HipModule."""

    def _stages(self):
        mods = list(self.children())
        st, i = [], 0
        while i < len(mods):
            m = mods[i]
            if isinstance(m, (Conv2d, SeparableBase, DepthwiseConv2d)) and i + 1 < len(mods) and \
                    isinstance(mods[i + 1], nn.BatchNorm2d):
                nxt = mods[i + 2] if i + 2 < len(mods) else None
                act = Act.RELU6 if isinstance(nxt, nn.ReLU6) else Act.RELU if isinstance(nxt, nn.ReLU) else Act.NONE
                st.append(Stage("cba", m, mods[i + 1], act))
                i += 2 if act is Act.NONE else 3
            elif isinstance(m, Conv2d):
                st.append(Stage("conv", m))
                i += 1
            elif isinstance(m, HipModule):
                st.append(Stage("mod", m))
                i += 1
            else:
                raise NotImplementedError("no HIP implementation for %s inside a Sequential" % type(m).__name__)
        return st

    def fwd(self, x, save, out=None, out_fmt=None):
        st = self._stages()
        ctxs = []
        for k, s in enumerate(st):
            last = k == len(st) - 1
            if (s.kind == "cba" and k == len(st) - 2 and st[k + 1].kind == "conv" and out is None and
                    cls_fusable(s, st[k + 1].conv)):
                x, c = cba_cls_fwd(s, st[k + 1].conv, x, save)
                ctxs += [c, None]
                break                                   # the classifier conv, the last stage, is folded into this one (c.cls)
            if s.kind == "cba":
                # the stage's output is pre-split when the next stage is a convolution; the last stage follows `out`
                # / out_fmt (default fp32: the caller is not a conv unless it says so)
                if last:
                    fmt = out_fmt if out is None else None
                    if out is None and out_fmt is None:
                        fmt = "f32"
                else:
                    fmt = "planes" if st[k + 1].kind in ("cba", "conv") else "f32"
                x, c = cba_fwd(s.conv, s.bn, s.act, x, save, out=out if last else None, out_fmt=fmt)
                ctxs.append(c)
            elif s.kind == "conv":
                x = s.conv.fwd(x, save, out=out if last else None)
                ctxs.append(None)
            else:
                x = s.conv.fwd(x, save)
                ctxs.append(None)
        keep(self, save, (st, ctxs))
        return x

    def bwd(self, dy, sink, need_dx=True, dx=None, accumulate=False):
        st, ctxs = take(self, sink)
        for k in range(len(st) - 1, -1, -1):
            s, c = st[k], ctxs[k]
            rest = (need_dx or k > 0, dx if k == 0 else None, accumulate and k == 0)
            if s.kind == "conv" and k > 0 and ctxs[k - 1] is not None and ctxs[k - 1].cls is s.conv:
                continue                                # folded into the stage in front of it: cba_cls_bwd there covers it
            if s.kind == "cba" and c.cls is not None:
                dy = cba_cls_bwd(c, dy, sink, *rest)
            elif s.kind == "cba":
                dy, _ = cba_bwd(c, dy, sink, *rest)
            elif s.kind == "conv":
                dy = s.conv.bwd(dy, sink, *rest)
            else:
                dy = s.conv.bwd(dy, sink)
        return dy

    def out_channels_of(self, cin):
        c = None
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                c = m.out_channels
        return c
