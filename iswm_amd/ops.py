"""Tensor-level wrappers over the C ABI (include/iswm_hip.h).

torch supplies device memory, the current HIP stream and nothing else: every
function here validates its tensors, allocates outputs through torch's caching
allocator and enqueues hand-written gfx950 kernels from libiswm_hip.so on
``torch.cuda.current_stream()``.  There is no fallback path.

Activations are NHWC: a 4-D fp32 tensor ``[N, H, W, C]`` whose last dim is
contiguous and whose pixel pitch ``ld = t.stride(2)`` may exceed C (a channel
slice of a wider buffer -- that is how torch.cat disappears from the graph).
"""
import collections
import ctypes
import enum
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import ConvDesc, call

BN_EPS = 1e-5


class Act(enum.IntEnum):
    """activation fused behind a BatchNorm.  The values are the C ABI codes (include/iswm_hip.h, ISWM_ACT_*): int(act) is what
    the iswm_bn_apply* / iswm_bn_backward* entry points take."""
    NONE = _lib.CONSTANTS["ISWM_ACT_NONE"]
    RELU = _lib.CONSTANTS["ISWM_ACT_RELU"]
    RELU6 = _lib.CONSTANTS["ISWM_ACT_RELU6"]

    @classmethod
    def of(cls, v):
        """the only coercion: an Act; None / False / 0 -> NONE; True / 1 -> RELU; 6 -> RELU6.  Exactly bool and int count, so
        2, 6.0, "relu" or an instance of another int subclass are a ValueError, not an activation."""
        if isinstance(v, cls):
            return v
        if v is None:
            return cls.NONE
        if type(v) in (bool, int) and v in (0, 1, 6):
            return cls(int(v))
        raise ValueError("not an activation: %r (expected an Act, None, False, True, 0, 1 or 6)" % (v,))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def geom(t, dtype=torch.float32):
    """(N, H, W, C, ld) of an NHWC activation view; raises on any other layout."""
    if isinstance(t, Planes):
        raise ValueError("this operation takes an fp32 NHWC tensor, not Planes (use .f32())")
    if t.dim() != 4 or t.dtype != dtype or not t.is_cuda:
        raise ValueError("expected a 4-D fp32 CUDA NHWC tensor, got %s %s %s" % (tuple(t.shape), t.dtype, t.device))
    n, h, w, c = t.shape
    if w > 1:
        ld = t.stride(2)
    elif h > 1:
        ld = t.stride(1)
    elif n > 1:
        ld = t.stride(0)
    else:                                  # one pixel: a channel slice keeps its buffer's pitch in its strides
        ld = max(c, t.stride(2))
    ok = (c == 1 or t.stride(3) == 1) and (w == 1 or t.stride(2) == ld) and \
        (h == 1 or t.stride(1) == w * ld) and (n == 1 or t.stride(0) == h * w * ld)
    if not ok or ld < c:
        raise ValueError("tensor is not a pitched NHWC view: shape %s strides %s" % (tuple(t.shape), t.stride()))
    return n, h, w, c, ld


def new_act(n, h, w, c, device):
    return torch.empty((n, h, w, c), dtype=torch.float32, device=device)


# ---- "planes": activations stored pre-split for the bf16x6 convolution kernels (csrc/planes.h) -------------
# False keeps every activation fp32 (the round-1 data path, which tests compare against); conv math f32 does that too.
_PLANES_ENV = True


# conv math "bf16" (BASELINE configs[4], mixed precision): activations between convolutions are STORED as one bf16 plane
# (round to nearest even) -- 2 bytes per element through every memory-bound pass instead of 4 (fp32) or 6 (bf16x6 planes).


def nplanes():
    """bf16 planes an activation is stored as under the current conv math: 3 (bf16x6: exact split), 1 (bf16: rounded), 0 (fp32)"""
    math = _lib.load().iswm_get_conv_math()
    if not _PLANES_ENV:
        return 0
    return 3 if math == 1 else (1 if math == 2 else 0)


def planes_on():
    return nplanes() > 0


class Planes(object):
    """An NHWC fp32 activation held as its exact 3-way bf16 split: `t` is a bf16 tensor [3, N, H, W, C]
    (plane, then a pitched NHWC view), hi + mid + lo == the fp32 value bit for bit.  Producers (BatchNorm / pooling /
    resize passes) write it, the convolution kernels stage it into LDS by DMA; anything else asks for `.f32()`.
    Under conv math "bf16" there is ONE plane, [1, N, H, W, C]: the value rounded to nearest bf16 (C-ABI plane stride -1)."""

    __slots__ = ("t",)

    def __init__(self, t):
        assert t.dim() == 5 and t.dtype == torch.bfloat16 and t.shape[0] in (1, 3)
        self.t = t

    @property
    def shape(self):
        return self.t.shape[1:]

    @property
    def device(self):
        return self.t.device

    def dim(self):
        return 4

    def __getitem__(self, idx):
        if not (isinstance(idx, tuple) and len(idx) == 2 and idx[0] is Ellipsis and isinstance(idx[1], slice)):
            raise IndexError("Planes supports channel slices x[..., a:b] only")
        return Planes(self.t[..., idx[1]])

    def f32(self):
        n, h, w, c, ld, ps = pgeom(self)
        out = new_act(n, h, w, c, self.t.device)
        call("iswm_join_planes", _p(self.t), ld, ps, n * h * w, c, _p(out), c, _stream())
        return out

    def zero_(self):
        self.t.zero_()
        return self


def is_planes(x):
    return isinstance(x, Planes)


def as_f32(x):
    return x.f32() if isinstance(x, Planes) else x


def new_planes(n, h, w, c, device, zero=False):
    mk = torch.zeros if zero else torch.empty
    return Planes(mk((max(1, nplanes()), n, h, w, c), dtype=torch.bfloat16, device=device))


def pgeom(x):
    """(N, H, W, C, ld, plane stride) of a Planes tensor, both in bf16 elements"""
    n, h, w, c, ld = geom(x.t[0], torch.bfloat16)
    return n, h, w, c, ld, (x.t.stride(0) if x.t.shape[0] == 3 else -1)


def xgeom(x):
    """(pointer tensor, N, H, W, C, ld, ps) of an fp32 NHWC tensor (ps = 0) or a Planes tensor"""
    if isinstance(x, Planes):
        return (x.t,) + pgeom(x)
    return (x,) + geom(x) + (0,)


def pad_weights(w, cout_p, cin_p):
    """zero-padded OHWI [cout_p, KH, KW, cin_p] copy of an OIHW parameter (any strides)"""
    cout, cin, kh, kw = w.shape
    out = torch.empty((cout_p, kh, kw, cin_p), dtype=torch.float32, device=w.device)
    st = (ctypes.c_int64 * 4)(*w.stride())
    call("iswm_pad_weights", _p(w), cout, cin, kh, kw, st, cout_p, cin_p, _p(out), _stream())
    return out


def unpad_weights(dw_ohwi, grad):
    """grad (OIHW view, any strides) <- the leading [cout, :, :, cin] block of a padded OHWI gradient"""
    cout_p, kh, kw, cin_p = dw_ohwi.shape
    cout, cin = grad.shape[0], grad.shape[1]
    assert dw_ohwi.is_contiguous() and tuple(grad.shape[2:]) == (kh, kw)
    st = (ctypes.c_int64 * 4)(*grad.stride())
    call("iswm_unpad_weights", _p(dw_ohwi), cout_p, cin_p, cout, cin, kh, kw, _p(grad), st, _stream())
    return grad


def zero_channels(t, c0):
    """zero channels [c0, C) of an NHWC activation (fp32 tensor or Planes): the padding channels of a concatenation buffer"""
    if isinstance(t, Planes):
        n, h, w, c, ld, ps = pgeom(t)
        call("iswm_zero_cols", _p(t.t), n * h * w, ld * 2, c0 * 2, c * 2, (ps if ps > 0 else 0) * 2, t.t.shape[0], _stream())
    else:
        n, h, w, c, ld = geom(t)
        call("iswm_zero_cols", _p(t), n * h * w, ld * 4, c0 * 4, c * 4, 0, 1, _stream())
    return t


def split_planes(x, out=None):
    """fp32 NHWC -> Planes (one extra pass; producers normally write planes themselves)"""
    n, h, w, c, ld = geom(x)
    if out is None:
        out = new_planes(n, h, w, c, x.device)
    _, _, _, _, ldp, ps = pgeom(out)
    call("iswm_split_planes", _p(x), n * h * w, c, ld, _p(out.t), ldp, ps if ps > 0 else n * h * w * ldp, _stream())
    return out


class KernelProfile:
    """Optional per-launch timing of the conv kernels with HIP events recorded on the stream the
    kernels are launched on (torch's current stream).  bench.py turns it on for the timed region to
    report the MFMA roofline fraction; it is off (None) otherwise and costs nothing."""

    def __init__(self, only=None):
        self.records = []   # (kernel name, start event, end event, algorithmic flops, geometry tag)
        self.only = only    # when set: time launches of this kernel only (keeps the timed region light)
        self.scope = None   # free-form label stamped on the records added while it is set (bench: "head_fwd")

    def wants(self, name):
        return self.only is None or name == self.only or name + "+reduce" == self.only

    def add(self, name, a, b, flops, tag):
        self.records.append((name, a, b, flops, tag, self.scope))

    def _totals(self, key, records=None):
        """{key(record): dict(launches, ms, flops)} over the records -- call after torch.cuda.synchronize()"""
        out = {}
        for r in self.records if records is None else records:
            d = out.setdefault(key(r), dict(launches=0, ms=0.0, flops=0.0))
            d["launches"] += 1
            d["ms"] += r[1].elapsed_time(r[2])
            d["flops"] += r[3]
        return out

    def scope_total(self, scope):
        """dict(launches, ms, flops) over the records stamped with this scope"""
        tot = self._totals(lambda r: scope, [r for r in self.records if r[5] == scope])
        return tot.get(scope, dict(launches=0, ms=0.0, flops=0.0))

    def summary(self):
        """{name: dict(launches, ms, flops)}"""
        return self._totals(lambda r: r[0])

    def by_geometry(self):
        """{(name, geometry tag): dict(launches, ms, flops)}"""
        return self._totals(lambda r: (r[0], r[4]))


KPROF = None


def _valid_taps(h, ho, k, stride, pad, dil):
    """number of (output index, tap) pairs whose input index is in bounds"""
    n = 0
    for t in range(k):
        off = t * dil - pad
        # count o in [0, ho) with 0 <= o*stride + off < h
        o_min = 0 if off >= 0 else (-off + stride - 1) // stride
        o_max = min(ho - 1, (h - 1 - off) // stride) if h - 1 - off >= 0 else -1
        n += max(0, o_max - o_min + 1)
    return n


def conv_out_size(h, k, stride, pad, dil):
    return (h + 2 * pad - dil * (k - 1) - 1) // stride + 1


class ConvGeom:
    """Static geometry of one conv call (wraps iswm_conv_desc)."""

    def __init__(self, x, cout, kh, kw, stride, pad, dil):
        n, h, w, cin = x.shape
        self.n, self.h, self.w, self.cin, self.cout = n, h, w, cin, cout
        self.kh, self.kw, self.stride, self.pad, self.dil = kh, kw, stride, pad, dil
        self.ho = conv_out_size(h, kh, stride, pad, dil)
        self.wo = conv_out_size(w, kw, stride, pad, dil)
        self.alg_cin, self.alg_cout = cin, cout      # un-padded channel counts (set by the module)
        self._flops = None

    def tag(self):
        return "n%d %dx%d c%d->%d k%d s%d d%d" % (self.n, self.h, self.w, self.alg_cin, self.alg_cout, self.kh,
                                                  self.stride, self.dil)

    def flops(self):
        """algorithmic FLOPs = 2 x MACs over IN-BOUNDS taps only; identical for the
        forward, data-gradient and weight-gradient passes"""
        if self._flops is None:
            vh = _valid_taps(self.h, self.ho, self.kh, self.stride, self.pad, self.dil)
            vw = _valid_taps(self.w, self.wo, self.kw, self.stride, self.pad, self.dil)
            self._flops = 2.0 * self.n * vh * vw * self.alg_cin * self.alg_cout
        return self._flops

    def desc(self, ldx, ldy, cout=None):
        return ConvDesc(self.n, self.h, self.w, self.cin, self.ho, self.wo, cout or self.cout, self.kh, self.kw,
                        self.stride, self.pad, self.dil, ldx, ldy)


def _kernel_name(d, kind):
    """device kernel symbol the library launches for this geometry (labels profile records)"""
    buf = ctypes.create_string_buffer(64)
    _lib.load().iswm_conv2d_kernel_name(ctypes.byref(d), kind, buf, 64)
    return buf.value.decode()


def _geoms_tag(geoms):
    if len(geoms) == 1:
        return geoms[0].tag()
    g0 = geoms[0]
    return "n%d %dx%d c%d->%dx%d aspp d%s" % (g0.n, g0.h, g0.w, g0.alg_cin, len(geoms), g0.alg_cout,
                                             "/".join(str(g.dil) for g in geoms if g.kh > 1))


class _timed:
    """bracket one conv launch with HIP events on the launch stream when a KernelProfile is active; `geoms`: the conv
    geometries the launch computes (one, or the ASPP branches: flops add up)"""

    def __init__(self, name, geoms):
        self.on = KPROF is not None and KPROF.wants(name)
        self.name, self.geoms = name, geoms

    def __enter__(self):
        if self.on:
            self.a = torch.cuda.Event(enable_timing=True)
            self.a.record()

    def __exit__(self, *exc):
        if self.on:
            b = torch.cuda.Event(enable_timing=True)
            b.record()
            KPROF.add(self.name, self.a, b, sum(g.flops() for g in self.geoms), _geoms_tag(self.geoms))
        return False


def _check_w(w_ohwi, g):
    if tuple(w_ohwi.shape) != (g.cout, g.kh, g.kw, g.cin) or not w_ohwi.is_contiguous():
        raise ValueError("weight must be contiguous OHWI %s, got %s strides %s" %
                         ((g.cout, g.kh, g.kw, g.cin), tuple(w_ohwi.shape), w_ohwi.stride()))


WEIGHTS_EPOCH = 0     # bumped by the fused optimizers: packed-weight buffers made before a step are stale after it


def weights_changed():
    global WEIGHTS_EPOCH
    WEIGHTS_EPOCH += 1


_USE_PACKED = True      # False: the packed-weight kernels stay unused (tests compare both paths)
_BN_FUSE = True         # False: BatchNorm backward always reduces itself (tests compare both paths)


def _packed_bytes(d, kind):
    return _lib.load().iswm_conv2d_packed_weight_bytes(ctypes.byref(d), kind) if _USE_PACKED else 0


def _pl2_bytes(d, kind):
    """packed-weight bytes of the planes kernels for this geometry, 0 when they do not apply"""
    return _lib.load().iswm_conv2d_pl2_weight_bytes(ctypes.byref(d), kind) if planes_on() else 0


def planes_conv_ok(cin, cout, kind):
    """will a conv with these channel counts take a Planes operand (kind 0: x forward, 1: dy data gradient)?"""
    return planes_on() and (cout if kind else cin) % 64 == 0


# ---- one plan per conv call: THE entry-point ladder (planes kernel -> packed bf16x6 kernel -> transposed-weight data
# gradient -> plain) and everything the wrappers size from it.  tests/conv_ref.planned() restates it independently.
ConvPlan = collections.namedtuple("ConvPlan", "entry kind name wform wbytes planes tiles tile_rows rows_stored stat_tiles workspace")
ConvPlan.__doc__ = """How one conv call runs: `entry` point, its iswm_conv2d_kernel_name `kind` and the kernel `name`; the weight form
it reads (wform "ohwi" / "wt" transposed / "x6" packed / "pl2" packed for the planes kernels, None for a weight gradient) and
its size `wbytes`; `planes`: the operand is taken pre-split (False on a plan made for a Planes operand: join it and plan again).
Forward: the BatchNorm-partial layout (tiles, tile_rows) and rows_stored -- the halo-patch layout, whose per-tile row counts
follow the two planes.  Planes data gradient: stat_tiles of the BnStats epilogue.  Weight gradient: workspace bytes."""
_PLANS = {}
_PACK_ENTRY = {"x6": "iswm_conv2d_pack_weights", "pl2": "iswm_conv2d_pl2_pack_weights"}


def conv_plan(d, op, planes):
    """the ConvPlan of op ("fwd" / "dgrad" / "wgrad") on descriptor d whose operand (x; dy for the data gradient) is Planes or
    fp32 -- pure host queries of the C ABI, cached under everything they depend on: all descriptor fields (pitches route too),
    the conv math and the two switches"""
    lib = _lib.load()
    key = (bytes(d), op, planes, lib.iswm_get_conv_math(), planes_on(), _USE_PACKED)
    p = _PLANS.get(key)
    if p is not None:
        return p
    ref, dirn = ctypes.byref(d), int(op == "dgrad")
    entry = wform = None
    kind = wbytes = tiles = tile_rows = stat_tiles = workspace = 0
    rows_stored = False
    if op == "wgrad":
        if not planes:
            entry, kind, workspace = "iswm_conv2d_wgrad", 2, lib.iswm_conv2d_wgrad_workspace(ref)
        elif planes_on() and lib.iswm_conv2d_wgrad_planes_ok(ref):
            entry, kind, workspace = "iswm_conv2d_wgrad_planes", 7, lib.iswm_conv2d_wgrad_planes_workspace(ref)
    elif planes:
        wbytes = _pl2_bytes(d, dirn)
        if wbytes:
            entry, kind, wform = ("iswm_conv2d_dgrad_pl2", 6, "pl2") if dirn else ("iswm_conv2d_fwd_pl2", 5, "pl2")
            if dirn:
                stat_tiles = lib.iswm_conv2d_dgrad_pl2_stat_tiles(ref)
            else:
                tile_rows = lib.iswm_conv2d_pl2_tile_rows(ref, 0)
                tiles = (d.N * d.Ho * d.Wo + tile_rows - 1) // tile_rows
    else:
        wbytes = _packed_bytes(d, dirn)
        if wbytes:
            entry, kind, wform = ("iswm_conv2d_dgrad_packed", 4, "x6") if dirn else ("iswm_conv2d_fwd_packed", 3, "x6")
            if not dirn:
                nt, tr = ctypes.c_int(0), ctypes.c_int(0)
                call("iswm_conv2d_fwd_packed_stat_layout", ref, ctypes.byref(nt), ctypes.byref(tr))
                tiles, tile_rows, rows_stored = nt.value, tr.value, True
        else:
            wbytes = 4 * d.Cout * d.KH * d.KW * d.Cin
            if dirn:
                # bf16x6 math: the matrix cores want the K axis (tap, cout) contiguous -> transposed weights
                wt = lib.iswm_conv2d_dgrad_wants_wt(ref)
                entry, kind, wform = ("iswm_conv2d_dgrad_wt", 1, "wt") if wt else ("iswm_conv2d_dgrad", 1, "ohwi")
            else:
                entry, kind, wform = "iswm_conv2d_fwd", 0, "ohwi"
                tiles, tile_rows = lib.iswm_conv2d_stat_tiles(ref), lib.iswm_conv2d_stat_tile_rows(ref)
    p = _PLANS[key] = ConvPlan(entry, kind, _kernel_name(d, kind) if entry else None, wform, wbytes, bool(planes and entry),
                               tiles, tile_rows, rows_stored, stat_tiles, workspace)
    return p


class ConvWeight(object):
    """One conv weight for one direction: the OHWI tensor plus the live buffers a WeightPacker pre-packed from it
    ({"x6": ..., "pl2": ...}, network._hip.Conv2d.weight_for).  The op wrappers take this or a bare OHWI tensor."""
    __slots__ = ("ohwi", "packed")

    def __init__(self, ohwi, packed=None):
        self.ohwi, self.packed = ohwi, packed or {}


def _ohwi(w):
    return w.ohwi if isinstance(w, ConvWeight) else w


def conv_weight(w, p, d, dirn):
    """the weight of plan p (dirn 0 forward, 1 data gradient) in the form its entry point reads: the OHWI tensor itself, the
    handle's pre-packed buffer, else a buffer allocated and packed / transposed here"""
    ohwi = _ohwi(w)
    if p.wform == "ohwi":
        return ohwi
    buf = w.packed.get(p.wform) if isinstance(w, ConvWeight) else None
    if buf is None:
        buf = torch.empty((p.wbytes // 4,), dtype=torch.float32, device=ohwi.device)
        if p.wform == "wt":
            call("iswm_transpose_weights", ctypes.byref(d), _p(ohwi), _p(buf), _stream())
        else:
            call(_PACK_ENTRY[p.wform], ctypes.byref(d), dirn, _p(ohwi), _p(buf), _stream())
    return buf


def _plan_operand(t, op, desc):
    """(operand tensor, its plane stride | None, descriptor, plan) of a forward / data-gradient call; desc(ld) -> the descriptor
    for an operand pitch.  A Planes operand stays pre-split when a planes kernel takes the geometry, else it is joined first."""
    if isinstance(t, Planes):
        _, _, _, _, ld, ps = pgeom(t)
        d = desc(ld)
        p = conv_plan(d, op, True)
        if p.planes:
            return t.t, ps, d, p
        t = t.f32()
    d = desc(geom(t)[4])
    return t, None, d, conv_plan(d, op, False)


def conv2d_fwd(x, w, g, bias=None, out=None, want_stats=False):
    """y = conv(x, w) [+ bias]; returns (y, partials|None, (tiles, tile_rows)).  w: OHWI tensor or ConvWeight.  The partials
    describe the convolution BEFORE the bias (the same bits with and without one): a caller that normalises a biased output
    takes colstat(y) instead."""
    _check_w(_ohwi(w), g)
    if out is None:
        out = new_act(g.n, g.ho, g.wo, g.cout, x.device)
    on, oh, ow, oc, ldy = geom(out)
    assert (on, oh, ow, oc) == (g.n, g.ho, g.wo, g.cout)
    x, ps, d, p = _plan_operand(x, "fwd", lambda ld: g.desc(ld, ldy))
    partials, tiles = None, (0, 0)
    if want_stats:
        tiles, n2 = (p.tiles, p.tile_rows), 2 * p.tiles * g.cout
        flat = torch.empty((n2 + (p.tiles if p.rows_stored else 0),), dtype=torch.float32, device=out.device)
        partials = flat[:n2].view(2, p.tiles, g.cout)
    wk = conv_weight(w, p, d, 0)
    with _timed(p.name, [g]):
        call(p.entry, ctypes.byref(d), _p(x), *([ps] if p.planes else []), _p(wk), _p(bias), _p(out), _p(partials), _stream())
    return out, partials, tiles


# what iswm_conv2d_dgrad_pl2_bn applies to dx before it takes the sums (include/iswm_hip.h, ISWM_GATE_*):
#   NONE        the producer stage has no activation
#   RECOMPUTED  ReLU, no residual: the pattern recomputed from the producer's y and scale / shift
#   RESIDUAL    ReLU behind a residual add: the pattern read from the saved output's hi plane, dx stored masked
GATE_NONE, GATE_RECOMPUTED, GATE_RESIDUAL = (_lib.CONSTANTS["ISWM_GATE_" + n] for n in ("NONE", "RECOMPUTED", "RESIDUAL"))


class BnStats(object):
    """Request / result of the BatchNorm-backward statistics a planes data gradient can take in its epilogue: `y`, `coef`
    (scale, shift, mean, invstd) and `act` describe the stage that PRODUCED the conv's input (whose BatchNorm backward will
    consume dx); conv2d_dgrad fills `partials`, `tiles` when its kernel supports the fusion (they stay None otherwise)."""

    def __init__(self, y, coef, relu, mask=None):
        self.y, self.coef, self.act = y, coef, Act.of(relu)
        self.partials, self.tiles = None, 0
        # a RESIDUAL producer stage (out = relu(bn(y) + identity)): `mask` = its saved output (Planes); the data gradient then
        # stores dx MASKED by (out > 0) and sets `masked` -- that tensor is the stage's dout (relu already applied) AND the
        # gradient of its identity branch
        self.mask, self.masked = mask, False


def conv2d_dgrad(dy, w, g, x_like_shape, dx=None, accumulate=False, bn_stats=None):
    """dx (=|+=) conv^T(dy, w).  x_like_shape = (N,H,W,Cin) of the conv input.  w: OHWI tensor or ConvWeight.
    bn_stats: a BnStats to fill (planes kernel only)."""
    _check_w(_ohwi(w), g)
    if dx is None:
        assert not accumulate
        dx = new_act(*x_like_shape, dy.device)
    ldx = geom(dx)[4]
    dy, ps, d, p = _plan_operand(dy, "dgrad", lambda ld: g.desc(ldx, ld))
    wk = conv_weight(w, p, d, 1)
    entry, b = p.entry, bn_stats if (p.planes and _BN_FUSE and g.cin % 4 == 0) else None
    args = [ctypes.byref(d), _p(dy)] + ([ps] if p.planes else []) + [_p(wk), _p(dx), int(bool(accumulate))]
    if b is not None:                     # the BnStats epilogue, on top of the plan
        part = torch.empty((2, p.stat_tiles, g.cin), dtype=torch.float64, device=dx.device)
        masky = b.act is Act.RELU and b.mask is None
        pm, ldm, gate = None, 0, GATE_RECOMPUTED if masky else GATE_NONE
        if b.mask is not None:
            pm, _, _, ldm, _ = xrows(b.mask)            # plane 0 = hi
            gate = GATE_RESIDUAL
        entry += "_bn"
        args += [_p(b.y), rows(b.y)[2], _p(b.coef[2]), _p(b.coef[3]), _p(b.coef[0]) if masky else None,
                 _p(b.coef[1]) if masky else None, gate, _p(pm), ldm, _p(part), p.stat_tiles]
    with _timed(p.name, [g]):
        call(entry, *args, _stream())
    if b is not None:
        b.partials, b.tiles, b.masked = part, p.stat_tiles, b.mask is not None
    return dx


def conv2d_wgrad(x, dy, g, dw_ohwi=None):
    """dw[Cout,KH,KW,Cin] = sum_pixels dy (x) gathered x.  With a pre-split x the planes kernel runs, over Cout padded to 8
    (dy is split here when the producer did not: the few-channel classifier gradient)."""
    if dw_ohwi is None:
        dw_ohwi = torch.empty((g.cout, g.kh, g.kw, g.cin), dtype=torch.float32, device=x.device)
    _check_w(dw_ohwi, g)
    c8 = (g.cout + 7) // 8 * 8
    p, tgt = None, dw_ohwi
    if isinstance(x, Planes):
        # the descriptor the planes kernel would get: its plan holds every precondition (iswm_conv2d_wgrad_planes_ok)
        d = g.desc(pgeom(x)[4], pgeom(dy)[4] if (isinstance(dy, Planes) and c8 == g.cout) else c8, cout=c8)
        p = conv_plan(d, "wgrad", True)
    if p is not None and p.planes:
        if not isinstance(dy, Planes) or c8 != g.cout:
            dyf = as_f32(dy)
            dy = new_planes(g.n, g.ho, g.wo, c8, x.device)
            if c8 != g.cout:
                zero_channels(dy, g.cout)
                tgt = torch.empty((c8, g.kh, g.kw, g.cin), dtype=torch.float32, device=x.device)
            split_planes(dyf, out=dy[..., :g.cout] if c8 != g.cout else dy)
        args = (_p(x.t), pgeom(x)[5], _p(dy.t), pgeom(dy)[5], _p(tgt))
    else:
        x, dy = as_f32(x), as_f32(dy)
        d = g.desc(geom(x)[4], geom(dy)[4])
        p = conv_plan(d, "wgrad", False)
        args = (_p(x), _p(dy), _p(tgt))
    ws = torch.empty((p.workspace // 4,), dtype=torch.float32, device=x.device) if p.workspace else None
    with _timed(p.name + "+reduce", [g]):
        call(p.entry, ctypes.byref(d), *args, _p(ws), p.workspace, _stream())
    if tgt is not dw_ohwi:
        unpad_weights(tgt, dw_ohwi.permute(0, 3, 1, 2))
    return dw_ohwi


# ---- ASPP: the parallel branch convolutions as one launch (csrc/conv_mfma_pl2t.hip) ---------------------------------
ASPP_TILE_ROWS = 144
_ASPP_PLANS = {}
_ASPP_FUSED = True      # False: one launch per branch (tests compare both paths)


def _int_array(v):
    return (ctypes.c_int * len(v))(*[int(i) for i in v])


def _ptr_array(ts):
    return (ctypes.c_void_p * len(ts))(*[(t.data_ptr() if t is not None else None) for t in ts])


def aspp_desc(n, h, w, cin, cout, ldx, ldy):
    return ConvDesc(n, h, w, cin, h, w, cout, 1, 1, 1, 0, 1, ldx, ldy)


def aspp_plan(n, h, w, cin, cout, ksize, dil, kind, device):
    """device copy of the tile plan of iswm_aspp_fwd (kind 0) / iswm_aspp_bwd (kind 1) for this geometry (built on the host once
    and cached), or None when the fused kernel does not cover it"""
    if not (_ASPP_FUSED and nplanes() == 3):          # bf16x6 only (checked per call: the conv math can change at run time)
        return None
    key = (n, h, w, cin, cout, tuple(ksize), tuple(dil), kind, str(device))
    plan = _ASPP_PLANS.get(key)
    if plan is None:
        lib = _lib.load()
        d = aspp_desc(n, h, w, cin, cout, cin, cout)
        ks, dl = _int_array(ksize), _int_array(dil)
        nb = lib.iswm_aspp_plan_bytes(ctypes.byref(d), len(ksize), ks, dl, kind)
        if nb == 0:
            _ASPP_PLANS[key] = False
            return None
        host = torch.empty((nb,), dtype=torch.uint8)
        cus = torch.cuda.get_device_properties(device).multi_processor_count
        call("iswm_aspp_plan", ctypes.byref(d), len(ksize), ks, dl, kind, ctypes.c_void_p(host.data_ptr()), cus)
        plan = _ASPP_PLANS[key] = host.to(device)
    return None if plan is False else plan


def aspp_fwd(x, ksize, dil, cout, wpks, want_stats):
    """ys[b] = conv(x, w_b) for the parallel branches in one launch; x Planes; wpks[b] packed by iswm_conv2d_pl2_pack_weights
    (kind 0).  Returns (ys, partials | None, tiles) or None when the geometry is not covered."""
    _, n, h, w, cin, ldx, ps = xgeom(x)
    plan = aspp_plan(n, h, w, cin, cout, ksize, dil, 0, x.device)
    if plan is None:
        return None
    nb = len(ksize)
    tiles = (n * h * w + ASPP_TILE_ROWS - 1) // ASPP_TILE_ROWS
    ys = [new_act(n, h, w, cout, x.device) for _ in range(nb)]
    parts = [torch.empty((2, tiles, cout), dtype=torch.float32, device=x.device) for _ in range(nb)] if want_stats else None
    d = aspp_desc(n, h, w, cin, cout, ldx, cout)
    gs = [ConvGeom(x, cout, k, k, 1, dl * (k - 1) // 2, dl) for k, dl in zip(ksize, dil)]
    with _timed("k_conv_pl2t<false>", gs):
        call("iswm_aspp_fwd", ctypes.byref(d), nb, _int_array(ksize), _int_array(dil), _p(plan), _p(x.t), ps, _ptr_array(wpks),
             _ptr_array(ys), _ptr_array(parts) if parts else None, _stream())
    return ys, parts, tiles


def aspp_dgrad(dyc, ksize, dil, cin, cout, wpks, dx=None, accumulate=False, x=None, dws=None):
    """dx (=|+=) sum_b conv^T(dyc[..., b*cout:(b+1)*cout], w_b) in one launch; dyc Planes [N,H,W,nb*cout]; wpks[b] packed by
    iswm_conv2d_pl2_pack_weights (kind 1).  With x (Planes) and dws (OHWI tensors per branch) the same call also runs the
    branches' weight gradients (iswm_aspp_bwd's full form).  Returns dx or None when not covered."""
    _, n, h, w, ctot, ld, ps = xgeom(dyc)
    nb = len(ksize)
    assert ctot >= nb * cout
    plan = aspp_plan(n, h, w, cin, cout, ksize, dil, 1, dyc.device)
    if plan is None:
        return None
    if dx is None:
        assert not accumulate
        dx = new_act(n, h, w, cin, dyc.device)
    d = aspp_desc(n, h, w, cin, cout, geom(dx)[4], cout)
    gs = []
    for k, dl in zip(ksize, dil):
        g = ConvGeom(dx, cout, k, k, 1, dl * (k - 1) // 2, dl)
        g.alg_cin, g.alg_cout = cin, cout
        gs.append(g)
    px, xps, pdw, ws, need = None, 0, None, None, 0
    if dws is not None:
        px, xps = x.t, pgeom(x)[5]
        pdw = _ptr_array(dws)
        lib = _lib.load()
        for k, dl in zip(ksize, dil):
            db = ConvDesc(n, h, w, cin, h, w, cout, k, k, 1, dl * (k - 1) // 2, dl, pgeom(x)[4], ld)
            need = max(need, lib.iswm_conv2d_wgrad_planes_workspace(ctypes.byref(db)))
        ws = torch.empty((max(need, 16) // 4,), dtype=torch.float32, device=dyc.device)
        d = aspp_desc(n, h, w, cin, cout, pgeom(x)[4], cout)
        assert geom(dx)[4] == pgeom(x)[4], "iswm_aspp_bwd takes ONE pitch for x and dx"
    with _timed("k_conv_pl2t<true>", gs):
        call("iswm_aspp_bwd", ctypes.byref(d), nb, _int_array(ksize), _int_array(dil), _p(plan), _p(dyc.t), ps, ld, _ptr_array(wpks),
             _p(dx), int(bool(accumulate)), _p(px), xps, pdw, _p(ws), need, _stream())
    return dx


# ---- depthwise conv (groups == channels) -------------------------------------------------------------
def dwconv2d_fwd(x, w, g, bias=None, out=None):
    """x NHWC [N,H,W,C]; w the parameter [Cw,1,KH,KW] (contiguous), Cw <= C"""
    x = as_f32(x)
    ldx = geom(x)[4]
    if out is None:
        out = new_act(g.n, g.ho, g.wo, g.cin, x.device)
    d = g.desc(ldx, geom(out)[4])
    call("iswm_dwconv2d_fwd", ctypes.byref(d), _p(x), _p(w), w.shape[0], _p(bias), _p(out), _stream())
    return out


def dwconv2d_dgrad(dy, w, g, x_like_shape, dx=None, accumulate=False):
    if dx is None:
        assert not accumulate
        dx = new_act(*x_like_shape, dy.device)
    d = g.desc(geom(dx)[4], geom(dy)[4])
    call("iswm_dwconv2d_dgrad", ctypes.byref(d), _p(dy), _p(w), w.shape[0], _p(dx), int(bool(accumulate)), _stream())
    return dx


def dwconv2d_wgrad(x, dy, g, cw, dw=None):
    """dw [Cw,1,KH,KW]"""
    x, dy = as_f32(x), as_f32(dy)
    if dw is None:
        dw = torch.empty((cw, 1, g.kh, g.kw), dtype=torch.float32, device=x.device)
    d = g.desc(geom(x)[4], geom(dy)[4])
    need = _lib.load().iswm_dwconv2d_wgrad_workspace(ctypes.byref(d))
    ws = torch.empty((need // 8,), dtype=torch.float64, device=x.device)
    call("iswm_dwconv2d_wgrad", ctypes.byref(d), _p(x), _p(dy), cw, _p(dw), _p(ws), need, _stream())
    return dw


def dwconv3x3_fwd_stats(x, w, g, want_stats, out=None):
    """depthwise 3x3 (pad == dil, stride 1 / 2) with the BatchNorm tile statistics taken in the same launch
    (csrc/dwconv3.hip); w the parameter [Cw,1,3,3] (contiguous).  Returns (y, partials|None, (tiles, tile_rows))."""
    x = as_f32(x)
    if out is None:
        out = new_act(g.n, g.ho, g.wo, g.cin, x.device)
    d = g.desc(geom(x)[4], geom(out)[4])
    partials, tiles = None, (0, 0)
    if want_stats:
        lib = _lib.load()
        tiles = (lib.iswm_dwconv3x3_stat_tiles(ctypes.byref(d)), lib.iswm_dwconv3x3_stat_tile_rows(ctypes.byref(d)))
        partials = torch.empty((2, tiles[0], g.cin), dtype=torch.float32, device=x.device)
    call("iswm_dwconv3x3_fwd_stats", ctypes.byref(d), _p(x), _p(w), w.shape[0], _p(out), _p(partials), _stream())
    return out, partials, tiles


def dwconv3x3_bwd(x, dy, w, g, cw, dx=None, accumulate=False, dw=None, need_dx=True, need_dw=True):
    """data gradient (into dx, optionally accumulating) and weight gradient dw [Cw,1,3,3] of the depthwise 3x3 in one pass
    over dy and x.  Returns (dx|None, dw|None)."""
    x, dy = as_f32(x), as_f32(dy)
    if need_dx and dx is None:
        assert not accumulate
        dx = new_act(*x.shape, dy.device)
    if not need_dx:
        dx = None
    d = g.desc(geom(x)[4], geom(dy)[4])
    lddx = geom(dx)[4] if dx is not None else 0
    ws, need = None, 0
    if need_dw:
        if dw is None:
            dw = torch.empty((cw, 1, 3, 3), dtype=torch.float32, device=x.device)
        need = _lib.load().iswm_dwconv3x3_bwd_workspace(ctypes.byref(d))
        ws = torch.empty((need // 4,), dtype=torch.float32, device=x.device)
    else:
        dw = None
    call("iswm_dwconv3x3_bwd", ctypes.byref(d), _p(x), _p(dy), _p(w), cw, _p(dx), lddx, int(bool(accumulate)), _p(dw), _p(ws),
         need, _stream())
    return dx, dw


def dwconv3x3_pre_fwd(x, w, g, relu_in, out=None, planes=False):
    """y = dwconv3x3(relu?(x), w) with 1 <= g.pad <= g.dil and no statistics (csrc/dwconv3.hip, include/iswm_hip_sep.h): the
    depthwise half of a separable unit whose consumer is a 1x1 convolution.  `out`: an fp32 NHWC tensor or Planes whose pitch
    may exceed g.cin (a channel slice [..., :g.cin] of the consumer's padded input buffer); every column between g.cin and
    that pitch is written as zeros.  Without `out` the result is dense, Planes if `planes`."""
    x = as_f32(x)
    if out is None:
        out = new_planes(g.n, g.ho, g.wo, g.cin, x.device) if planes else new_act(g.n, g.ho, g.wo, g.cin, x.device)
    pt, n, h, wd, c, ldy, ps = xgeom(out)
    if (n, h, wd, c) != (g.n, g.ho, g.wo, g.cin):
        raise ValueError("dwconv3x3_pre_fwd: out is %s, expected %s" % ((n, h, wd, c), (g.n, g.ho, g.wo, g.cin)))
    d = g.desc(geom(x)[4], ldy)
    call("iswm_dwconv3x3_pre_fwd", ctypes.byref(d), _p(x), _p(w), w.shape[0], int(bool(relu_in)), _p(pt), ps, ldy, _stream())
    return out


def dwconv3x3_pre_bwd(x, dy, w, g, cw, relu_in, dx=None, accumulate=False, dw=None, need_dx=True, need_dw=True):
    """backward of dwconv3x3_pre_fwd in one pass over dy and x, the saved input BEFORE the ReLU: dw [Cw,1,3,3] from relu?(x),
    and dx (=|+=) (x > 0) * dgrad(dy, w) -- the mask only with relu_in.  Returns (dx|None, dw|None)."""
    x, dy = as_f32(x), as_f32(dy)
    if need_dx and dx is None:
        assert not accumulate
        dx = new_act(*x.shape, dy.device)
    if not need_dx:
        dx = None
    d = g.desc(geom(x)[4], geom(dy)[4])
    lddx = geom(dx)[4] if dx is not None else 0
    ws, need = None, 0
    if need_dw:
        if dw is None:
            dw = torch.empty((cw, 1, 3, 3), dtype=torch.float32, device=x.device)
        need = _lib.load().iswm_dwconv3x3_pre_bwd_workspace(ctypes.byref(d))
        ws = torch.empty((need // 4,), dtype=torch.float32, device=x.device)
    else:
        dw = None
    call("iswm_dwconv3x3_pre_bwd", ctypes.byref(d), _p(x), _p(dy), _p(w), cw, int(bool(relu_in)), _p(dx), lddx,
         int(bool(accumulate)), _p(dw), _p(ws), need, _stream())
    return dx, dw


def rows(t):
    n, h, w, c, ld = geom(t)
    return n * h * w, c, ld


def xrows(t):
    """(pointer tensor, rows, C, ld, ps) of an fp32 or Planes activation"""
    p, n, h, w, c, ld, ps = xgeom(t)
    return p, n * h * w, c, ld, ps


def colstat(x):
    """per-tile column statistics in the three-plane layout {S_t, M2_t, R_t} (iswm_colstat_res; R_t = sum (x - fp32(S_t / n_t)): what
    the fp32 tile sum lost, bn_finalize merges exactly with it); returns (partials [3, tiles, C], tiles, tile_rows).
    Only this column pass has the third plane.  The convolution epilogues and dwconv3 publish [2, tiles, C]: their variance keeps an
    error of ~2^-23 |mean| / sigma, which matters only for channels whose mean is thousands of standard deviations from 0."""
    m, c, ld = rows(x)
    tile_rows = _lib.load().iswm_colstat_tile_rows(m)
    tiles = (m + tile_rows - 1) // tile_rows
    partials = torch.empty((3, tiles, c), dtype=torch.float32, device=x.device)
    call("iswm_colstat_res", _p(x), m, c, ld, _p(partials), _stream())
    return partials, tiles, tile_rows


def bn_finalize(partials, tiles, count, tile_rows, gamma, beta, running_mean, running_var, momentum, eps=BN_EPS):
    """tile statistics -> coef [4, C] = (scale, beta, mean, invstd), running buffers updated.  The layout of `partials` is its first
    dimension: [2, tiles, C] = {S_t, M2_t} (convolution epilogues, dwconv3: iswm_bn_finalize), [3, tiles, C] = that pair plus the
    residual plane of colstat (iswm_bn_finalize_res, the exact merge)."""
    c = partials.shape[2]
    coef = torch.empty((4, c), dtype=torch.float32, device=partials.device)  # scale, beta, mean, invstd
    name = "iswm_bn_finalize_res" if (partials.dim() == 3 and partials.shape[0] == 3) else "iswm_bn_finalize"
    call(name, _p(partials), tiles, c, count, tile_rows, _p(gamma), _p(beta), _p(running_mean),
         _p(running_var), float(momentum), float(eps), _p(coef[0]), _p(coef[1]), _p(coef[2]), _p(coef[3]), _stream())
    return coef


def bn_eval_coeffs(gamma, beta, running_mean, running_var, eps=BN_EPS):
    c = running_mean.numel()
    coef = torch.empty((4, c), dtype=torch.float32, device=running_mean.device)
    call("iswm_bn_eval_coeffs", c, _p(gamma), _p(beta), _p(running_mean), _p(running_var), float(eps), _p(coef[0]),
         _p(coef[1]), _p(coef[2]), _p(coef[3]), _stream())
    return coef


def bn_apply(y, coef, relu, residual=None, out=None, planes=False):
    """out = act((y - mean) * scale + beta (+ residual)); `out` (fp32 or Planes, possibly a channel slice) decides the
    output format, else `planes` does"""
    act = Act.of(relu)
    m, c, ldy = rows(y)
    if out is None:
        out = new_planes(*y.shape, y.device) if planes else torch.empty(y.shape, dtype=torch.float32, device=y.device)
    po, mo, co, ldo, pso = xrows(out)
    assert (mo, co) == (m, c)
    pr, ldr, psr = None, 0, 0
    if residual is not None:
        pr, mr, cr, ldr, psr = xrows(residual)
        assert (mr, cr) == (m, c)
    call("iswm_bn_apply_pl", _p(y), m, c, ldy, _p(coef[0]), _p(coef[1]), _p(coef[2]), _p(pr), ldr, psr, int(act),
         _p(po), ldo, pso, _stream())
    return out


def bn_backward(dout, out, y, coef, gamma, relu, training, dgamma, dbeta, want_dres=False, dy=None, dy_planes=False,
                stats=None):
    """Returns (dy, dres|None); writes dgamma / dbeta (length-C fp32 tensors).  `out` (the saved activation, for the
    ReLU pattern) may be Planes; dy is written as Planes when dy_planes (the conv's data / weight gradient kernels
    take it pre-split).  stats: a filled BnStats from the data gradient that produced dout -- the reduction pass is skipped.
    want_dres also tells whether the stage added a residual: with ReLU and want_dres=False the pattern is recomputed from y alone,
    which is the forward's only if it added none -- a residual stage's backward must ask for dres."""
    act = Act.of(relu)
    m, c, ldy = rows(y)
    _, _, ldd = rows(dout)
    po, ldo, pso = None, 0, 0
    if out is not None:
        po, _, _, ldo, pso = xrows(out)
    need = _lib.load().iswm_bn_bwd_workspace(m, c)
    ws = torch.empty((need // 8,), dtype=torch.float64, device=y.device)
    if dy is None:
        dy = new_planes(*y.shape, y.device) if dy_planes else torch.empty(y.shape, dtype=torch.float32, device=y.device)
    pdy, _, _, lddy, psdy = xrows(dy)
    dres = torch.empty(y.shape, dtype=torch.float32, device=y.device) if want_dres else None
    # ReLU without a residual: hand over the forward's scale / shift so the sign pattern is recomputed from y and the
    # saved output is never read (a residual stage's pattern depends on the identity tensor: read `out` there)
    masky = act is Act.RELU and not want_dres
    fused = stats is not None and stats.partials is not None
    args = [_p(dout), ldd, _p(po), ldo, pso, _p(y), ldy, m, c, _p(coef[2]), _p(coef[3]), _p(gamma),
            _p(coef[0]) if masky else None, _p(coef[1]) if masky else None, int(act), int(bool(training)), _p(dgamma),
            _p(dbeta), _p(pdy), lddy, psdy, _p(dres), rows(dres)[2] if dres is not None else 0]
    if fused:
        args += [_p(stats.partials), stats.tiles]
    call("iswm_bn_backward_stats_pl" if fused else "iswm_bn_backward_pl", *args, _p(ws), need, _stream())
    return dy, dres


def bn_apply_classify(y, coef, wc4, bias4):
    """logits [N,H,W,4] = bias4 + wc4 . relu(bn(y)) in one pass over the raw conv output y (csrc/bn_classify.hip); wc4 = the 1x1
    classifier's weight zero-padded to [4, C] (pad_weights), C == 256"""
    m, c, ldy = rows(y)
    out = torch.empty(tuple(y.shape[:3]) + (4,), dtype=torch.float32, device=y.device)
    call("iswm_bn_apply_classify", _p(y), m, c, ldy, _p(coef[0]), _p(coef[1]), _p(coef[2]), _p(wc4), _p(bias4), _p(out), 4, _stream())
    return out


def bn_backward_classify(dlogit, wc4, y, coef, gamma, training, dgamma, dbeta, dy_planes):
    """BatchNorm + ReLU backward of the stage whose activation fed the folded classifier: returns (dy, dwc4) -- dy the gradient of
    the raw conv output (Planes when dy_planes), dwc4 [4, C] the classifier's weight gradient"""
    m, c, ldy = rows(y)
    _, cl, ldl = rows(dlogit)
    assert cl == 4
    need = _lib.load().iswm_bn_classify_bwd_workspace(m, c)
    ws = torch.empty((need // 8,), dtype=torch.float64, device=y.device)
    dy = new_planes(*y.shape, y.device) if dy_planes else torch.empty(y.shape, dtype=torch.float32, device=y.device)
    pdy, _, _, lddy, psdy = xrows(dy)
    dwc4 = torch.empty((4, c), dtype=torch.float32, device=y.device)
    call("iswm_bn_backward_classify", _p(dlogit), ldl, _p(wc4), _p(y), ldy, m, c, _p(coef[2]), _p(coef[3]), _p(gamma), _p(coef[0]),
         _p(coef[1]), int(bool(training)), _p(dgamma), _p(dbeta), _p(dwc4), _p(pdy), lddy, psdy, _p(ws), need, _stream())
    return dy, dwc4


def colsum(x):
    """per-channel sum over all pixels (bias gradient)"""
    x = as_f32(x)
    partials, tiles, _ = colstat(x)
    c = x.shape[3]
    out = torch.empty((2, c), dtype=torch.float32, device=x.device)
    call("iswm_colsum_finalize", _p(partials), tiles, c, _p(out[0]), _p(out[1]), _stream())
    return out[0]


def maxpool_fwd(x, planes=False):
    x = as_f32(x)
    n, h, w, c, ld = geom(x)
    assert ld == c
    ho, wo = (h + 2 - 3) // 2 + 1, (w + 2 - 3) // 2 + 1
    y = new_planes(n, ho, wo, c, x.device) if planes else new_act(n, ho, wo, c, x.device)
    py, _, _, _, _, _, ps = xgeom(y)
    idx = torch.empty((n, ho, wo, c), dtype=torch.uint8, device=x.device)
    call("iswm_maxpool3x3s2_fwd_pl", _p(x), n, h, w, c, _p(py), ps, _p(idx), ho, wo, _stream())
    return y, idx


def maxpool_bwd(dy, idx, in_shape):
    n, h, w, c = in_shape
    _, ho, wo, _, ld = geom(dy)
    assert ld == c
    dx = new_act(n, h, w, c, dy.device)
    call("iswm_maxpool3x3s2_bwd", _p(dy), _p(idx), n, h, w, c, ho, wo, _p(dx), _stream())
    return dx


def gap_fwd(x):
    px, n, h, w, c, ld, ps = xgeom(x)
    y = new_act(n, 1, 1, c, x.device)
    call("iswm_gap_fwd_pl", _p(px), ps, n, h * w, c, ld, _p(y), _stream())
    return y


def gap_bwd(dy, dx, accumulate):
    n, h, w, c, ld = geom(dx)
    call("iswm_gap_bwd", _p(dy), n, h * w, c, _p(dx), ld, int(bool(accumulate)), _stream())
    return dx


def bcast_fwd(v, out):
    po, n, h, w, c, ld, ps = xgeom(out)
    call("iswm_bcast_fwd_pl", _p(as_f32(v)), n, h * w, c, _p(po), ld, ps, _stream())
    return out


def bcast_bwd(dy):
    n, h, w, c, ld = geom(dy)
    dv = new_act(n, 1, 1, c, dy.device)
    call("iswm_bcast_bwd", _p(dy), ld, n, h * w, c, _p(dv), _stream())
    return dv


def bilinear_fwd(x, ho, wo, out=None):
    x = as_f32(x)
    n, hi, wi, c, ldx = geom(x)
    if out is None:
        out = new_act(n, ho, wo, c, x.device)
    po, _, _, _, _, ldy, ps = xgeom(out)
    call("iswm_bilinear_fwd_pl", _p(x), n, hi, wi, c, ldx, _p(po), ps, ho, wo, ldy, _stream())
    return out


def bilinear_bwd(dy, hi, wi):
    n, ho, wo, c, lddy = geom(dy)
    dx = new_act(n, hi, wi, c, dy.device)
    call("iswm_bilinear_bwd", _p(dy), n, hi, wi, c, lddy, ho, wo, _p(dx), c, _stream())
    return dx


def bilinear_to_nchw_fwd(x, c, ho, wo):
    """NHWC low-res logits (first c channels) -> NCHW [N,c,ho,wo]."""
    x = as_f32(x)
    n, hi, wi, cp, ldx = geom(x)
    y = torch.empty((n, c, ho, wo), dtype=torch.float32, device=x.device)
    call("iswm_bilinear_nhwc_to_nchw_fwd", _p(x), n, hi, wi, c, ldx, _p(y), ho, wo, _stream())
    return y


def bilinear_to_nchw_bwd(dy, hi, wi, cp):
    n, c, ho, wo = dy.shape
    assert dy.is_contiguous() and dy.dtype == torch.float32
    dx = new_act(n, hi, wi, cp, dy.device)
    call("iswm_bilinear_nhwc_to_nchw_bwd", _p(dy), n, hi, wi, c, cp, ho, wo, _p(dx), _stream())
    return dx


def nchw_to_nhwc(x, cp=None):
    assert x.dim() == 4 and x.dtype == torch.float32 and x.is_cuda
    x = x.contiguous()
    n, c, h, w = x.shape
    cp = cp or (c + 3) // 4 * 4
    y = new_act(n, h, w, cp, x.device)
    call("iswm_nchw_to_nhwc", _p(x), n, c, h * w, _p(y), cp, _stream())
    return y


def nhwc_to_nchw(x, c=None):
    x = as_f32(x)
    n, h, w, cc, ld = geom(x)
    c = c or cc
    y = torch.empty((n, c, h, w), dtype=torch.float32, device=x.device)
    call("iswm_nhwc_to_nchw", _p(x), n, c, h * w, ld, _p(y), _stream())
    return y


def copy_channels(src, dst):
    src = as_f32(src)
    m, c, lds = rows(src)
    md, cd, ldd = rows(dst)
    assert (m, c) == (md, cd)
    call("iswm_copy_channels", _p(src), lds, _p(dst), ldd, m, c, _stream())
    return dst


def add_inplace(dst, src):
    assert dst.is_contiguous() and src.is_contiguous() and dst.numel() == src.numel()
    call("iswm_add_inplace", _p(dst), _p(src), dst.numel(), _stream())
    return dst


def dropout_fwd(x, p, seed, offset):
    x = as_f32(x)
    assert x.is_contiguous()
    y = torch.empty_like(x)
    mask = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    call("iswm_dropout_fwd", _p(x), _p(y), _p(mask), x.numel(), float(p), int(seed), int(offset), _stream())
    return y, mask


def dropout_bwd(dy, mask, p):
    assert dy.is_contiguous()
    dx = torch.empty_like(dy)
    call("iswm_dropout_bwd", _p(dy), _p(mask), _p(dx), dy.numel(), float(p), _stream())
    return dx


MODE_WCE, MODE_FOCAL_MEAN, MODE_FOCAL_SUM = 0, 1, 2


def loss_fwd(logits, labels, weight, ignore_index, alpha, gamma, mode):
    """Returns (loss[1], sums[2], grad_unnorm) -- one pass over the logits."""
    assert logits.dim() == 4 and logits.dtype == torch.float32 and logits.is_cuda
    logits = logits.contiguous()
    b, c, h, w = logits.shape
    assert labels.shape == (b, h, w) and labels.dtype in (torch.uint8, torch.int64)
    labels = labels.contiguous()
    npix = b * h * w
    blocks = _lib.load().iswm_loss_blocks(npix)
    grad = torch.empty_like(logits)
    partials = torch.empty((2, blocks), dtype=torch.float32, device=logits.device)
    out = torch.empty((3,), dtype=torch.float32, device=logits.device)  # sums[2], loss
    call("iswm_loss_fwd", _p(logits), _p(labels), labels.element_size(), b, c, h * w, _p(weight), int(ignore_index),
         float(alpha), float(gamma), int(mode), _p(grad), _p(partials), _stream())
    call("iswm_loss_finalize", _p(partials), blocks, int(mode), npix, _p(out), _p(out[2:]), _stream())
    return out[2:], out[:2], grad


def loss_bwd_scale(grad, sums, upstream, mode, npix):
    call("iswm_loss_bwd_scale", _p(grad), grad.numel(), _p(sums), _p(upstream), int(mode), npix, _stream())
    return grad


OVERLAP_CLASSES = {"foreground": 0, "all": 1}


def _pixel_loss_args(logits, labels, weight, noun):
    """the checks the two-pass criteria share (`noun` names the criterion in the messages) -> logits, labels, B, C, H * W"""
    if not (logits.dim() == 4 and logits.dtype == torch.float32 and logits.is_cuda):
        raise ValueError("%s expects fp32 CUDA logits [B,C,H,W] (there is no CPU fallback)" % noun)
    logits = logits.contiguous()
    b, c, h, w = logits.shape
    if c > 8:
        raise ValueError("%s takes at most 8 classes (got %d)" % (noun, c))
    assert labels.shape == (b, h, w) and labels.dtype in (torch.uint8, torch.int64)
    assert weight is None or (weight.dtype == torch.float32 and weight.numel() == c and weight.is_cuda)
    return logits, labels.contiguous(), b, c, h * w


def overlap_loss_fwd(logits, labels, weight, ignore_index):
    """One pass over the logits, nothing stored per pixel -> sums (float64 [2 + 3C], on the device) =
    {sum w*nll, sum w, I_c [C], P_c [C], G_c [C]} over the valid pixels (include/iswm_hip.h)."""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "the overlap loss")
    blocks = _lib.load().iswm_loss_blocks(b * hw)
    nv = 2 + 3 * c
    partials = torch.empty((nv, blocks), dtype=torch.float32, device=logits.device)
    sums = torch.empty((nv,), dtype=torch.float64, device=logits.device)
    call("iswm_overlap_loss_fwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, _p(weight), int(ignore_index),
         _p(partials), _p(sums), _stream())
    return sums


def overlap_loss_coeffs(sums, C, ce_weight, overlap_weight, alpha, beta, gamma, smooth, classes):
    """sums (this process's, or all-reduced over the ranks) -> (loss fp32 [1], coef fp32 [1 + 2C]) on the device."""
    if classes not in OVERLAP_CLASSES:
        raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 2 + 3 * C
    out = torch.empty((2 + 2 * C,), dtype=torch.float32, device=sums.device)     # loss, coef[1 + 2C]
    call("iswm_overlap_loss_coeffs", _p(sums), int(C), float(ce_weight), float(overlap_weight), float(alpha), float(beta),
         float(gamma), float(smooth), OVERLAP_CLASSES[classes], _p(out), _p(out[1:]), _stream())
    return out[:1], out[1:]


def overlap_loss_bwd(logits, labels, weight, ignore_index, coef, upstream):
    """The second pass: upstream[0] * dL/dlogits, written once (upstream: fp32 device scalar [1])."""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "the overlap loss")
    assert coef.dtype == torch.float32 and coef.numel() == 1 + 2 * c and coef.is_cuda
    assert upstream.dtype == torch.float32 and upstream.numel() == 1 and upstream.is_cuda
    grad = torch.empty_like(logits)
    call("iswm_overlap_loss_bwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, _p(weight), int(ignore_index),
         _p(coef), _p(upstream), _p(grad), _stream())
    return grad


def _distill_args(student, teacher, labels, weight, temperature):
    """the checks of the distillation calls -> student, teacher, labels, B, C, H * W, float32(1 / temperature)"""
    student, labels, b, c, hw = _pixel_loss_args(student, labels, weight, "the distillation loss")
    if not (torch.is_tensor(teacher) and teacher.dtype == torch.float32 and teacher.is_cuda and teacher.device == student.device):
        raise ValueError("the distillation loss expects fp32 CUDA teacher logits on the student's device")
    if teacher.shape != student.shape:
        raise ValueError("teacher logits %s do not have the student's shape %s" % (tuple(teacher.shape), tuple(student.shape)))
    if not (0.0 < temperature < math.inf):
        raise ValueError("temperature must be positive and finite (got %r)" % (temperature,))
    inv_tau = float(torch.tensor(1.0 / float(temperature), dtype=torch.float32))
    if not (0.0 < inv_tau < math.inf):
        raise ValueError("1 / temperature is not a positive finite fp32 value (temperature %r)" % (temperature,))
    return student, teacher.contiguous(), labels, b, c, hw, inv_tau


def distill_loss_fwd(student, teacher, labels, weight, ignore_index, temperature):
    """One pass over both logit tensors, nothing stored per pixel -> sums (float64 [5], on the device) =
    {sum w*nll, sum w, sum KL, N, A} over the valid pixels (include/iswm_hip_kd.h)."""
    student, teacher, labels, b, c, hw, inv_tau = _distill_args(student, teacher, labels, weight, temperature)
    partials = torch.empty((_lib.load().iswm_distill_loss_partials(b * hw),), dtype=torch.float32, device=student.device)
    sums = torch.empty((5,), dtype=torch.float64, device=student.device)
    call("iswm_distill_loss_fwd", _p(student), _p(teacher), _p(labels), labels.element_size(), b, c, hw, _p(weight),
         int(ignore_index), inv_tau, _p(partials), _p(sums), _stream())
    return sums


def distill_loss_coeffs(sums, ce_weight, distill_weight, temperature):
    """sums (this process's, or all-reduced over the ranks) -> (out fp32 [3] = {loss, CE term, KD term}, coef fp32 [2]) on
    the device."""
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 5
    buf = torch.empty((5,), dtype=torch.float32, device=sums.device)
    call("iswm_distill_loss_coeffs", _p(sums), float(ce_weight), float(distill_weight), float(temperature), _p(buf),
         _p(buf[3:]), _stream())
    return buf[:3], buf[3:]


def distill_loss_bwd(student, teacher, labels, weight, ignore_index, temperature, coef, upstream):
    """The second pass: upstream[0] * dL/dstudent, written once (upstream: fp32 device scalar [1])."""
    student, teacher, labels, b, c, hw, inv_tau = _distill_args(student, teacher, labels, weight, temperature)
    assert coef.dtype == torch.float32 and coef.numel() == 2 and coef.is_cuda
    assert upstream.dtype == torch.float32 and upstream.numel() == 1 and upstream.is_cuda
    grad = torch.empty_like(student)
    call("iswm_distill_loss_bwd", _p(student), _p(teacher), _p(labels), labels.element_size(), b, c, hw, _p(weight),
         int(ignore_index), inv_tau, _p(coef), _p(upstream), _p(grad), _stream())
    return grad


EDT_MAX_SIDE = 4096


def _first_class(classes):
    """'foreground' -> 1 (the class planes 1 .. C-1), 'all' -> 0"""
    if classes not in OVERLAP_CLASSES:
        raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
    return 1 - OVERLAP_CLASSES[classes]


def signed_edt(labels, num_classes, classes='foreground', ignore_index=255):
    """The exact signed squared Euclidean distance map of labels [B,H,W] (uint8 or int64, on the GPU) -> int32 [B, |K|, H, W],
    K = the classes 1 .. C-1 ('foreground') or 0 .. C-1 ('all'): +d^2 to the nearest pixel of the class outside it, -d^2 to the
    nearest valid pixel of another class inside it, 0 at invalid pixels and over a plane with either set empty
    (include/iswm_hip_bd.h).  Sides up to 4096.  The workspace comes from torch's allocator; nothing is read back."""
    first = _first_class(classes)
    if not (torch.is_tensor(labels) and labels.dim() == 3 and labels.is_cuda and labels.dtype in (torch.uint8, torch.int64)):
        raise ValueError("the distance map expects uint8 or int64 CUDA labels [B,H,W] (there is no CPU fallback)")
    b, h, w = labels.shape
    c = int(num_classes)
    if c - first < 1:
        raise ValueError("%d classes with classes=%r leave no class plane" % (c, classes))
    if h > EDT_MAX_SIDE or w > EDT_MAX_SIDE:
        raise ValueError("a %d x %d plane: the distance map takes sides up to %d" % (h, w, EDT_MAX_SIDE))
    if b * h * w == 0:
        raise ValueError("the distance map of an empty label tensor %s" % (tuple(labels.shape),))
    nbytes = _lib.load().iswm_signed_edt_workspace(b, c, h, w, first)
    if nbytes < 0:
        raise ValueError("the distance map does not take labels %s with %d classes" % (tuple(labels.shape), c))
    labels = labels.contiguous()
    work = torch.empty((nbytes // 4,), dtype=torch.int32, device=labels.device)
    sd2 = torch.empty((b, c - first, h, w), dtype=torch.int32, device=labels.device)
    call("iswm_signed_edt", _p(labels), labels.element_size(), b, c, h, w, first, int(ignore_index), _p(sd2), _p(work), nbytes,
         _stream())
    return sd2


def boundary_metrics(pred, labels, num_classes, classes='foreground', ignore_index=255, tolerance=2, percent=95):
    """The contour statistics of predicted masks pred [B,H,W] against labels [B,H,W] (each uint8 or int64, on the GPU), per image,
    class of K (1 .. C-1 for 'foreground', 0 .. C-1 for 'all') and direction (0: predicted contour -> label contour, 1: the other
    way) -> (stats int64 [B, |K|, 2, 4] = n, within tolerance, max d^2, d^2 of the percent-th nearest rank; dsum float64
    [B, |K|, 2] = the sum of the distances), both on the device (include/iswm_hip_bm.h).  Sides up to 4096.  The workspace comes
    from torch's allocator; nothing is read back."""
    first = _first_class(classes)
    for name, t in (("predictions", pred), ("labels", labels)):
        if not (torch.is_tensor(t) and t.dim() == 3 and t.is_cuda and t.dtype in (torch.uint8, torch.int64)):
            raise ValueError("the boundary metrics expect uint8 or int64 CUDA %s [B,H,W] (there is no CPU fallback)" % name)
    if pred.shape != labels.shape or pred.device != labels.device:
        raise ValueError("the boundary metrics expect predictions and labels of one shape on one device (got %s on %s and %s on %s)" %
                         (tuple(pred.shape), pred.device, tuple(labels.shape), labels.device))
    b, h, w = labels.shape
    c = int(num_classes)
    if c - first < 1:
        raise ValueError("%d classes with classes=%r leave no class plane" % (c, classes))
    if h > EDT_MAX_SIDE or w > EDT_MAX_SIDE:
        raise ValueError("a %d x %d plane: the boundary metrics take sides up to %d" % (h, w, EDT_MAX_SIDE))
    if b * h * w == 0:
        raise ValueError("the boundary metrics of an empty label tensor %s" % (tuple(labels.shape),))
    if isinstance(tolerance, bool) or int(tolerance) != tolerance or not 0 <= tolerance <= EDT_MAX_SIDE:
        raise ValueError("tolerance is a whole number of pixels in [0, %d] (got %r)" % (EDT_MAX_SIDE, tolerance))
    if isinstance(percent, bool) or int(percent) != percent or not 1 <= percent <= 100:
        raise ValueError("percent is a whole number in [1, 100] (got %r)" % (percent,))
    nbytes = _lib.load().iswm_boundary_metrics_workspace(b, c, h, w, first)
    if nbytes < 0:
        raise ValueError("the boundary metrics do not take labels %s with %d classes" % (tuple(labels.shape), c))
    pred, labels = pred.contiguous(), labels.contiguous()
    work = torch.empty((nbytes // 4,), dtype=torch.int32, device=labels.device)
    stats = torch.empty((b, c - first, 2, 4), dtype=torch.int64, device=labels.device)
    dsum = torch.empty((b, c - first, 2), dtype=torch.float64, device=labels.device)
    call("iswm_boundary_metrics", _p(pred), pred.element_size(), _p(labels), labels.element_size(), b, c, h, w, first,
         int(ignore_index), int(tolerance), int(percent), _p(stats), _p(dsum), _p(work), nbytes, _stream())
    return stats, dsum


def _boundary_args(logits, labels, sd2, weight, classes, clip):
    """the checks of the boundary-loss calls -> logits, labels, sd2, B, C, H * W, first class"""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "the boundary loss")
    first = _first_class(classes)
    if c - first < 1:
        raise ValueError("%d classes with classes=%r leave no class plane" % (c, classes))
    if not (torch.is_tensor(sd2) and sd2.dtype == torch.int32 and sd2.is_cuda and sd2.device == logits.device):
        raise ValueError("the boundary loss expects an int32 CUDA distance map on the logits' device")
    want = (b, c - first) + tuple(logits.shape[2:])
    if tuple(sd2.shape) != want:
        raise ValueError("the distance map %s does not have the shape %s of these logits and classes=%r" %
                         (tuple(sd2.shape), want, classes))
    if not (0.0 <= clip < math.inf):
        raise ValueError("clip must be finite and not negative, 0 = no clamp (got %r)" % (clip,))
    return logits, labels, sd2.contiguous(), b, c, hw, first


def boundary_loss_fwd(logits, labels, sd2, weight, ignore_index, classes='foreground', clip=0.0):
    """One pass over the logits, the labels and the distance map of signed_edt, nothing stored per pixel -> sums (float64 [4],
    on the device) = {sum w*nll, sum w, sum p*phi, N} over the valid pixels (include/iswm_hip_bd.h)."""
    logits, labels, sd2, b, c, hw, first = _boundary_args(logits, labels, sd2, weight, classes, clip)
    partials = torch.empty((_lib.load().iswm_boundary_loss_partials(b * hw),), dtype=torch.float32, device=logits.device)
    sums = torch.empty((4,), dtype=torch.float64, device=logits.device)
    call("iswm_boundary_loss_fwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, first, _p(sd2), _p(weight),
         int(ignore_index), float(clip), _p(partials), _p(sums), _stream())
    return sums


def boundary_loss_coeffs(sums, nsel, ce_weight, boundary_weight):
    """sums (this process's, or all-reduced over the ranks) and nsel = |K| -> (out fp32 [3] = {loss, CE term, boundary term},
    coef fp32 [2]) on the device.  The two factors are host doubles: changing them between calls costs no synchronisation."""
    assert sums.dtype == torch.float64 and sums.is_cuda and sums.is_contiguous() and sums.numel() == 4
    buf = torch.empty((5,), dtype=torch.float32, device=sums.device)
    call("iswm_boundary_loss_coeffs", _p(sums), int(nsel), float(ce_weight), float(boundary_weight), _p(buf), _p(buf[3:]),
         _stream())
    return buf[:3], buf[3:]


def boundary_loss_bwd(logits, labels, sd2, weight, ignore_index, coef, upstream, classes='foreground', clip=0.0):
    """The second pass: upstream[0] * dL/dlogits, written once (upstream: fp32 device scalar [1])."""
    logits, labels, sd2, b, c, hw, first = _boundary_args(logits, labels, sd2, weight, classes, clip)
    assert coef.dtype == torch.float32 and coef.numel() == 2 and coef.is_cuda
    assert upstream.dtype == torch.float32 and upstream.numel() == 1 and upstream.is_cuda
    grad = torch.empty_like(logits)
    call("iswm_boundary_loss_bwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, first, _p(sd2), _p(weight),
         int(ignore_index), float(clip), _p(coef), _p(upstream), _p(grad), _stream())
    return grad


def ohem_nu0(thresh):
    """float32(-ln thresh): a pixel whose true-class probability is at most thresh has nll >= this (thresh 1 -> +0)"""
    if not 0.0 < thresh <= 1.0:
        raise ValueError("thresh must lie in (0, 1] (got %r)" % (thresh,))
    return float(torch.tensor(-math.log(thresh) + 0.0, dtype=torch.float32))


def ohem_keys(logits, labels, ignore_index):
    """-> (keys int32 [B,H,W]: the bit pattern of the pixel's nll, -1 at an invalid pixel; nvalid int64 [1] = |V|), on the device"""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, None, "hard-pixel mining")
    keys = torch.empty(labels.shape, dtype=torch.int32, device=logits.device)
    nvalid = torch.empty((1,), dtype=torch.int64, device=logits.device)
    counts = torch.empty((_lib.load().iswm_loss_blocks(b * hw),), dtype=torch.int32, device=logits.device)
    call("iswm_ohem_keys", _p(logits), _p(labels), labels.element_size(), b, c, hw, int(ignore_index), _p(keys), _p(counts),
         _p(nvalid), _stream())
    return keys, nvalid


def ohem_state(device):
    """the select state {prefix, remaining rank, k, -} (int64 [4]) and nu (fp32 [1]); scan(0) initialises the state"""
    return torch.zeros((4,), dtype=torch.int64, device=device), torch.empty((1,), dtype=torch.float32, device=device)


def ohem_hist(keys, state, digit, out=None):
    """-> hist int64 [2048]: the counts of digit `digit` among the keys carrying the prefix in `state` (digit 0: every valid
    key), ADDED to `out` (a zeroed buffer of the caller's; a fresh one without)"""
    assert keys.dtype == torch.int32 and keys.is_cuda and keys.is_contiguous()
    assert state.dtype == torch.int64 and state.numel() == 4 and state.is_cuda
    bins = _lib.load().iswm_ohem_bins()
    hist = torch.zeros((bins,), dtype=torch.int64, device=keys.device) if out is None else out
    assert hist.dtype == torch.int64 and hist.numel() == bins and hist.is_cuda and hist.is_contiguous()
    call("iswm_ohem_hist", _p(keys), keys.numel(), _p(state), int(digit), _p(hist), _stream())
    return hist


def ohem_scan(hist, nvalid, digit, min_kept, nu0, state, nu):
    """picks the bin of `hist` that holds the wanted rank: updates `state` in place; the last digit writes `nu`"""
    assert hist.dtype == torch.int64 and hist.is_cuda and hist.numel() == _lib.load().iswm_ohem_bins()
    assert nvalid.dtype == torch.int64 and nvalid.numel() == 1 and nvalid.is_cuda
    assert state.dtype == torch.int64 and state.numel() == 4 and nu.dtype == torch.float32 and nu.numel() == 1
    if min_kept < 0:
        raise ValueError("min_kept must not be negative (got %r)" % (min_kept,))
    call("iswm_ohem_scan", _p(hist), _p(nvalid), int(digit), int(min_kept), float(nu0), _p(state), _p(nu), _stream())
    return state


def ohem_select(keys, nvalid, min_kept, thresh, group=None):
    """nu = min(float32(-ln thresh), the min(min_kept, |V|)-th largest key) as an fp32 device scalar [1]: three histogram /
    scan rounds, nothing read back.  With `group`, |V| (in place) and every histogram are all-reduced: nu is the global batch's."""
    nu0 = ohem_nu0(thresh)
    state, nu = ohem_state(keys.device)
    if group is not None:
        import torch.distributed as dist
        dist.all_reduce(nvalid, group=group)
    digits = _lib.load().iswm_ohem_digits()
    hists = torch.zeros((digits, _lib.load().iswm_ohem_bins()), dtype=torch.int64, device=keys.device)   # one fill for all three
    for digit in range(digits):
        hist = ohem_hist(keys, state, digit, out=hists[digit])
        if group is not None:
            dist.all_reduce(hist, group=group)
        ohem_scan(hist, nvalid, digit, min_kept, nu0, state, nu)
    return nu


def ohem_sums(keys, labels, weight, nu):
    """-> float64 [3] on the device: {sum_K w nll, sum_K w, |K|}, K = the pixels whose stored key is >= the bits of nu"""
    assert keys.dtype == torch.int32 and keys.is_cuda and keys.is_contiguous() and keys.shape == labels.shape
    assert labels.dtype in (torch.uint8, torch.int64) and nu.dtype == torch.float32 and nu.numel() == 1 and nu.is_cuda
    labels = labels.contiguous()
    c = 8 if weight is None else weight.numel()
    assert weight is None or (weight.dtype == torch.float32 and weight.is_cuda and c <= 8)
    npix = keys.numel()
    blocks = _lib.load().iswm_loss_blocks(npix)
    partials = torch.empty((3, blocks), dtype=torch.float32, device=keys.device)
    sums = torch.empty((3,), dtype=torch.float64, device=keys.device)
    call("iswm_ohem_sums", _p(keys), _p(labels), labels.element_size(), npix, c, _p(weight), _p(nu), _p(partials), _p(sums),
         _stream())
    return sums


def ohem_loss(sums):
    """sums (this process's, or all-reduced) -> fp32 [2] on the device: {loss, 1 / sum_K w}, both 0 if nothing is kept"""
    assert sums.dtype == torch.float64 and sums.numel() == 3 and sums.is_cuda and sums.is_contiguous()
    out = torch.empty((2,), dtype=torch.float32, device=sums.device)
    call("iswm_ohem_loss", _p(sums), _p(out), _stream())
    return out


def ohem_bwd(logits, labels, weight, keys, nu, lossinv, upstream):
    """upstream[0] * dL/dlogits, written once: w (p - onehot) / sum_K w on the kept pixels, exactly 0 elsewhere"""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "hard-pixel mining")
    assert keys.dtype == torch.int32 and keys.is_cuda and keys.is_contiguous() and keys.shape == labels.shape
    assert nu.dtype == torch.float32 and nu.numel() == 1 and lossinv.dtype == torch.float32 and lossinv.numel() == 2
    assert upstream.dtype == torch.float32 and upstream.numel() == 1 and upstream.is_cuda
    grad = torch.empty_like(logits)
    call("iswm_ohem_bwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, _p(weight), _p(keys), _p(nu), _p(lossinv),
         _p(upstream), _p(grad), _stream())
    return grad


_LOVASZ_WS = {}


def lovasz_segments(b, c, classes):
    """the number of (image, class) segments of a [b, c, ...] batch: every class but 0 ('foreground') or all"""
    if classes not in OVERLAP_CLASSES:
        raise ValueError("classes is 'foreground' or 'all' (got %r)" % (classes,))
    return b * (c - (0 if classes == "all" else 1))


def lovasz_workspace(device, nseg, P):
    """the sort's ping-pong buffers and tables (uint8 on `device`), cached per (device, nseg, P): one criterion call after
    another on one stream reuses it"""
    key = (str(device), int(nseg), int(P))
    ws = _LOVASZ_WS.get(key)
    if ws is None:
        need = _lib.load().iswm_lovasz_workspace(int(nseg), int(P))
        if need <= 0:
            raise _lib.IswmError(_lib.load().iswm_last_error().decode())
        ws = _LOVASZ_WS[key] = torch.empty((need,), dtype=torch.uint8, device=device)
    return ws


def lovasz_keys(logits, labels, weight, ignore_index, classes, sums=None):
    """-> (keys int32 [nseg, HW]: the bits of ((bits(e) << 1) | g) + 1, 0 at an invalid pixel; counts int32 [nseg, 2] = {valid
    pixels of the image, G}; sums float64 [4] whose first two entries are {sum w nll, sum w}) on the device.  The keys are
    uint32 values held in int32 tensors."""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "the Lovasz loss")
    nseg = lovasz_segments(b, c, classes)
    keys = torch.empty((max(nseg, 0), hw), dtype=torch.int32, device=logits.device)
    counts = torch.empty((max(nseg, 0), 2), dtype=torch.int32, device=logits.device)
    partials = torch.empty((2, _lib.load().iswm_loss_blocks(b * hw)), dtype=torch.float32, device=logits.device)
    if sums is None:
        sums = torch.zeros((4,), dtype=torch.float64, device=logits.device)
    call("iswm_lovasz_keys", _p(logits), _p(labels), labels.element_size(), b, c, hw, _p(weight), int(ignore_index),
         OVERLAP_CLASSES[classes], _p(keys), _p(counts), _p(partials), _p(sums), _stream())
    return keys, counts, sums


def lovasz_sort(keys):
    """keys int32 [nseg, P] (uint32 values) -> (sorted [nseg, P], perm [nseg, P]): every segment in descending order of the
    unsigned keys, equal keys in input order; perm is the key's index in its segment"""
    assert keys.dtype == torch.int32 and keys.is_cuda and keys.is_contiguous() and keys.dim() == 2
    nseg, P = keys.shape
    ws = lovasz_workspace(keys.device, nseg, P)
    out = torch.empty((2, nseg, P), dtype=torch.int32, device=keys.device)
    call("iswm_lovasz_sort", _p(keys), nseg, P, _p(ws), ws.numel(), _p(out[0]), _p(out[1]), _stream())
    return out[0], out[1]


def lovasz_weights(sorted_keys, perm, counts, sums=None):
    """-> (m fp32 [nseg, P]: m[seg, perm[j]] = omega_j, 0 at invalid pixels and in absent segments; sums float64 [4] whose last
    two entries are {sum over present segments of L_bc, N})"""
    assert sorted_keys.dtype == torch.int32 and sorted_keys.is_cuda and sorted_keys.is_contiguous() and sorted_keys.dim() == 2
    nseg, P = sorted_keys.shape
    assert perm.dtype == torch.int32 and perm.shape == sorted_keys.shape and perm.is_contiguous() and perm.is_cuda
    assert counts.dtype == torch.int32 and counts.shape == (nseg, 2) and counts.is_contiguous() and counts.is_cuda
    ws = lovasz_workspace(sorted_keys.device, nseg, P)
    m = torch.empty((nseg, P), dtype=torch.float32, device=sorted_keys.device)
    if sums is None:
        sums = torch.zeros((4,), dtype=torch.float64, device=sorted_keys.device)
    assert sums.dtype == torch.float64 and sums.numel() == 4 and sums.is_contiguous() and sums.is_cuda
    call("iswm_lovasz_weights", _p(sorted_keys), _p(perm), _p(counts), nseg, P, _p(ws), ws.numel(), _p(m), _p(sums[2:]), _stream())
    return m, sums


def lovasz_loss(sums, ce_weight, lovasz_weight):
    """sums (this process's, or all-reduced) -> fp32 [3] on the device: {loss, ce_weight / sum w, lovasz_weight / N}"""
    assert sums.dtype == torch.float64 and sums.numel() == 4 and sums.is_cuda and sums.is_contiguous()
    out = torch.empty((3,), dtype=torch.float32, device=sums.device)
    call("iswm_lovasz_loss", _p(sums), float(ce_weight), float(lovasz_weight), _p(out), _stream())
    return out


def lovasz_bwd(logits, labels, weight, ignore_index, classes, m, out, upstream):
    """upstream[0] * dL/dlogits, written once, CE term included (out: lovasz_loss's result); exactly 0 at invalid pixels"""
    logits, labels, b, c, hw = _pixel_loss_args(logits, labels, weight, "the Lovasz loss")
    nseg = lovasz_segments(b, c, classes)
    assert m.dtype == torch.float32 and m.shape == (nseg, hw) and m.is_contiguous() and m.is_cuda
    assert out.dtype == torch.float32 and out.numel() == 3 and out.is_cuda and out.is_contiguous()
    assert upstream.dtype == torch.float32 and upstream.numel() == 1 and upstream.is_cuda
    grad = torch.empty_like(logits)
    call("iswm_lovasz_bwd", _p(logits), _p(labels), labels.element_size(), b, c, hw, _p(weight), int(ignore_index),
         OVERLAP_CLASSES[classes], _p(m), _p(out[1:]), _p(upstream), _p(grad), _stream())
    return grad


def argmax_nchw(logits):
    logits = logits.contiguous()
    b, c, h, w = logits.shape
    out = torch.empty((b, h, w), dtype=torch.int64, device=logits.device)
    call("iswm_argmax_nchw", _p(logits), b, c, h * w, _p(out), _stream())
    return out


def _int_code(t):
    if t.dtype == torch.uint8:
        return 0
    if t.dtype == torch.int64:
        return 1
    raise TypeError("expected a uint8 or int64 tensor, got %s" % t.dtype)


def confusion_matrix(labels, preds, n_classes, hist=None):
    """hist[n_classes, n_classes] (int64, device) += bincount(n_classes*label + pred) over valid labels"""
    labels, preds = labels.contiguous(), preds.contiguous()
    if labels.numel() != preds.numel():
        raise ValueError("labels and predictions differ in size: %d vs %d" % (labels.numel(), preds.numel()))
    if hist is None:
        hist = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=labels.device)
    call("iswm_confusion_matrix", _p(labels), _int_code(labels), _p(preds), _int_code(preds), labels.numel(), n_classes,
         _p(hist), _stream())
    return hist


def confusion_matrix_logits(labels, logits, n_classes, hist=None):
    """the same with pred = logits.max(1)[1] computed on the fly (logits NCHW fp32)"""
    labels, logits = labels.contiguous(), logits.contiguous()
    b, c, h, w = logits.shape
    if labels.numel() != b * h * w:
        raise ValueError("labels %s do not match logits %s" % (tuple(labels.shape), tuple(logits.shape)))
    if hist is None:
        hist = torch.zeros((n_classes, n_classes), dtype=torch.int64, device=labels.device)
    call("iswm_confusion_matrix_logits", _p(labels), _int_code(labels), _p(logits), b, c, h * w, n_classes, _p(hist),
         _stream())
    return hist


def _masks(t):
    """[N, H, W] (or [H, W]) uint8 / int64 class map on the device, contiguous"""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError("expected [N, H, W] masks, got %s" % (tuple(t.shape),))
    return t.contiguous()


def mask_morph(src, radius, dilate):
    """dilate / erode (src > 0) by a (2*radius+1)^2 rectangle, neutral border -> uint8 [N, H, W]"""
    src = _masks(src)
    n, h, w = src.shape
    out = torch.empty((n, h, w), dtype=torch.uint8, device=src.device)
    call("iswm_mask_morph", _p(src), _int_code(src), n, h, w, int(radius), int(bool(dilate)), _p(out), _stream())
    return out


def ccl(mask):
    """8-connected components of a uint8 mask: (labels int32 [N, H, W], the component's smallest raster index or -1;
    areas int32 [N, H, W], the component's size at that root, 0 elsewhere)"""
    mask = _masks(mask)
    if mask.dtype != torch.uint8:
        raise TypeError("ccl takes a uint8 mask, got %s" % mask.dtype)
    n, h, w = mask.shape
    labels = torch.empty((n, h, w), dtype=torch.int32, device=mask.device)
    areas = torch.empty_like(labels)
    call("iswm_ccl", _p(mask), n, h, w, _p(labels), _p(areas), _stream())
    return labels, areas


def mask_preprocess(src):
    """MaskUtils.preprocess_mask per frame: (mask uint8 [N, H, W], weight float64 [N], area int64 [N]); the
    reference's result is mask * weight"""
    src = _masks(src)
    n, h, w = src.shape
    dev = src.device
    out = torch.empty((n, h, w), dtype=torch.uint8, device=dev)
    weight = torch.empty(n, dtype=torch.float64, device=dev)
    area = torch.empty(n, dtype=torch.int64, device=dev)
    nbytes = _lib.load().iswm_mask_preprocess_workspace(n, h, w)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    call("iswm_mask_preprocess", _p(src), _int_code(src), n, h, w, _p(out), _p(weight), _p(area), _p(ws), nbytes,
         _stream())
    return out, weight, area


def mask_fronts(mask, weight=None):
    """leftmost column per row where mask * weight == 1 (-1: none): (fronts int32 [N, H], stats int64 [N, 3] =
    count, sum of rows, sum of columns)"""
    mask = _masks(mask)
    if mask.dtype != torch.uint8:
        raise TypeError("mask_fronts takes a uint8 mask, got %s" % mask.dtype)
    n, h, w = mask.shape
    fronts = torch.empty((n, h), dtype=torch.int32, device=mask.device)
    stats = torch.empty((n, 3), dtype=torch.int64, device=mask.device)
    weight = weight.contiguous() if weight is not None else None
    call("iswm_mask_fronts", _p(mask), _p(weight), n, h, w, _p(fronts), _p(stats), _stream())
    return fronts, stats


def front_error(pred_fronts, gt_fronts, tau):
    """FrontTrackingMetrics.calculate_error per (pred, gt) pair of front rows [N, H] -> float64 [N]"""
    pred_fronts, gt_fronts = pred_fronts.contiguous(), gt_fronts.contiguous()
    if pred_fronts.shape != gt_fronts.shape or pred_fronts.dtype != torch.int32 or gt_fronts.dtype != torch.int32:
        raise ValueError("front rows must be two int32 [N, H] tensors of one shape")
    n, h = pred_fronts.shape
    out = torch.empty(n, dtype=torch.float64, device=pred_fronts.device)
    call("iswm_front_error", _p(pred_fronts), _p(gt_fronts), n, h, float(tau), _p(out), _stream())
    return out


def mask_pair_scores(curr_fronts, curr_stats, prev_mask, prev_weight, prev_stats):
    """MaskUtils.calculate_stability / calculate_motion of (current, previous) preprocessed frames, given the
    current frames' fronts and the previous frames' masks -> (stability, motion) float64 [N]"""
    prev_mask = _masks(prev_mask)
    n, h, w = prev_mask.shape
    if tuple(curr_fronts.shape) != (n, h):
        raise ValueError("fronts %s do not match masks %s" % (tuple(curr_fronts.shape), tuple(prev_mask.shape)))
    stab = torch.empty(n, dtype=torch.float64, device=prev_mask.device)
    motion = torch.empty_like(stab)
    call("iswm_mask_pair_scores", _p(curr_fronts.contiguous()), _p(curr_stats.contiguous()), _p(prev_mask),
         _p(prev_weight.contiguous()), _p(prev_stats.contiguous()), n, h, w, _p(stab), _p(motion), _stream())
    return stab, motion


def region_score(pred, gt):
    """RegionMetrics.calculate_region_metrics per frame -> (final_score float64 [N], valid int32 [N])"""
    pred, gt = _masks(pred), _masks(gt)
    if pred.shape != gt.shape:
        raise ValueError("pred %s and gt %s differ in shape" % (tuple(pred.shape), tuple(gt.shape)))
    n, h, w = pred.shape
    score = torch.empty(n, dtype=torch.float64, device=pred.device)
    valid = torch.empty(n, dtype=torch.int32, device=pred.device)
    nbytes = _lib.load().iswm_region_workspace(n, h, w)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=pred.device)
    call("iswm_region_score", _p(pred), _int_code(pred), _p(gt), _int_code(gt), n, h, w, _p(score), _p(valid), _p(ws),
         nbytes, _stream())
    return score, valid


def predict_normalize(img, mean, std):
    """uint8 [N, H, W, 3] RGB on the device -> normalised fp32 NCHW [N, 3, H, W]: (v / 255 - mean) / std in fp32,
    bit-identical to ToTensor + Normalize on the CPU"""
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8 or not img.is_cuda:
        raise ValueError("expected a uint8 CUDA [N, H, W, 3] image batch, got %s %s" % (tuple(img.shape), img.dtype))
    img = img.contiguous()
    n, h, w, _ = img.shape
    out = torch.empty((n, 3, h, w), dtype=torch.float32, device=img.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    call("iswm_predict_normalize", _p(img), n, h, w, m, s, _p(out), _stream())
    return out


@functools.lru_cache(maxsize=64)
def band_bounds(min_prob, max_prob):
    """(lo, hi) with lo <= k <= hi exactly for the confidence values k in 0..255 that binarize_confidence_map marks
    (predict.py:229-234: k / 255.0 >= min_prob and k / 255.0 <= max_prob, fp64); an empty band gives (1, 0)"""
    ks = [k for k in range(256) if k / 255.0 >= min_prob and k / 255.0 <= max_prob]
    return (ks[0], ks[-1]) if ks else (1, 0)


def _align16(v):
    return (v + 15) // 16 * 16


def predict_maps_layout(n, h, w):
    """byte offsets of stats (fp64 [n, 5]), pred, conf, band (uint8 [n, h, w]) in predict_maps' packed buffer and its
    size: a prefix up to the last map a caller needs can be copied to the host in one transfer"""
    stats = 0
    pred = _align16(40 * n)
    conf = pred + _align16(n * h * w)
    band = conf + _align16(n * h * w)
    return {"stats": stats, "pred": pred, "conf": conf, "band": band, "end": band + _align16(n * h * w)}


class PredictMaps(tuple):
    """(pred, conf, band, prob, stats, packed): pred / conf / band uint8 [N, H, W], prob fp32 [N, H, W] or None,
    stats fp64 [N, 5] = (min p, max p, sum p, count(p < thr), count(pred)); every tensor but prob is a view of the
    uint8 buffer `packed` (predict_maps_layout)"""
    __slots__ = ()
    pred = property(lambda self: self[0])
    conf = property(lambda self: self[1])
    band = property(lambda self: self[2])
    prob = property(lambda self: self[3])
    stats = property(lambda self: self[4])
    packed = property(lambda self: self[5])


def predict_maps(yl, num_classes, fg, H, W, thr, min_prob, max_prob, want_prob=False):
    """low-resolution NHWC logits (the model's forward_lowres) -> PredictMaps at [N, H, W]: the reference's
    predict_mask / binarize_confidence_map maps in one pass (bilinear upsample, softmax, p = prob[fg], pred = p > thr,
    conf = uint8(p * 255), band = min_prob <= conf / 255 <= max_prob).  Enqueues only; never synchronises."""
    yl = as_f32(yl)
    n, hl, wl, c, ld = geom(yl)
    if ld % 4 or ld < (num_classes + 3) // 4 * 4 or num_classes > c:
        raise ValueError("logits %s (pitch %d) do not hold %d classes" % (tuple(yl.shape), ld, num_classes))
    if not 0 <= fg < num_classes:
        raise ValueError("foreground class %d outside [0, %d)" % (fg, num_classes))
    dev = yl.device
    lay = predict_maps_layout(n, H, W)
    packed = torch.empty(lay["end"], dtype=torch.uint8, device=dev)
    stats = packed[:40 * n].view(torch.float64).view(n, 5)
    pred, conf, band = (packed[lay[k]:lay[k] + n * H * W].view(n, H, W) for k in ("pred", "conf", "band"))
    prob = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_prob else None
    lo, hi = band_bounds(min_prob, max_prob)
    nbytes = _lib.load().iswm_predict_maps_workspace(n, H, W)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    call("iswm_predict_maps", _p(yl), n, hl, wl, ld, int(num_classes), int(fg), int(H), int(W), float(thr),
         lo, hi, _p(pred), _p(conf), _p(band), _p(prob), _p(stats), _p(ws), nbytes, _stream())
    return PredictMaps((pred, conf, band, prob, stats, packed))


def prob_maps(prob, thr, min_prob, max_prob):
    """fp32 CUDA probability [N, H, W] -> PredictMaps with predict_maps' rules, layout and order of summation (prob is the input
    itself): fed the prob of a predict_maps call it gives that call's packed bytes (include/iswm_hip_cr.h).  Enqueues only."""
    if not (torch.is_tensor(prob) and prob.dim() == 3 and prob.is_cuda and prob.dtype == torch.float32):
        raise ValueError("the maps of a probability expect an fp32 CUDA tensor [N,H,W] (there is no CPU fallback)")
    n, H, W = prob.shape
    nbytes = _lib.load().iswm_prob_maps_workspace(n, H, W)
    if nbytes < 0:
        raise ValueError("the maps of a probability do not take the shape %s" % (tuple(prob.shape),))
    prob = prob.contiguous()
    dev = prob.device
    lay = predict_maps_layout(n, H, W)
    packed = torch.empty(lay["end"], dtype=torch.uint8, device=dev)
    stats = packed[:40 * n].view(torch.float64).view(n, 5)
    pred, conf, band = (packed[lay[k]:lay[k] + n * H * W].view(n, H, W) for k in ("pred", "conf", "band"))
    lo, hi = band_bounds(min_prob, max_prob)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    call("iswm_prob_maps", _p(prob), n, H, W, float(thr), lo, hi, _p(pred), _p(conf), _p(band), _p(stats), _p(ws), nbytes,
         _stream())
    return PredictMaps((pred, conf, band, prob, stats, packed))


CRF_MAX_RADIUS, CRF_MAX_STEP, CRF_MAX_ITERS, CRF_MAX_SIDE = 7, 4, 20, 8192


def crf_check(iters, radius, step, w_bilateral, w_spatial, theta_alpha, theta_beta, theta_gamma):
    """the parameter ranges of crf_refine (include/iswm_hip_cr.h); ValueError with the offending name"""
    for name, v, hi in (("iters", iters, CRF_MAX_ITERS), ("radius", radius, CRF_MAX_RADIUS), ("step", step, CRF_MAX_STEP)):
        if isinstance(v, bool) or int(v) != v or not (0 if name == "iters" else 1) <= v <= hi:
            raise ValueError("%s is a whole number in [%d, %d] (got %r)" % (name, 0 if name == "iters" else 1, hi, v))
    for name, v in (("w_bilateral", w_bilateral), ("w_spatial", w_spatial)):
        if not (math.isfinite(v) and v >= 0):
            raise ValueError("%s must be finite and not negative (got %r)" % (name, v))
    for name, v in (("theta_alpha", theta_alpha), ("theta_beta", theta_beta), ("theta_gamma", theta_gamma)):
        if not (math.isfinite(v) and v > 0):
            raise ValueError("%s must be finite and positive (got %r)" % (name, v))


def crf_refine(prob, img_u8, iters, radius=5, step=2, w_bilateral=10.0, w_spatial=3.0, theta_alpha=80.0, theta_beta=13.0,
               theta_gamma=3.0):
    """Local dense-CRF refinement of the foreground probability prob (fp32 CUDA [N,H,W]) on the frames img_u8 (uint8 CUDA
    [N,H,W,3], RGB): `iters` mean-field updates over the (2 radius + 1)^2 window dilated by `step` (include/iswm_hip_cr.h, DESIGN.md
    section 25) -> fp32 [N,H,W].  iters == 0 returns prob itself.  The defaults are ConvCRF's published values, unvalidated on this
    project's data.  The workspace comes from torch's allocator; one launch per iteration, nothing is read back."""
    crf_check(iters, radius, step, w_bilateral, w_spatial, theta_alpha, theta_beta, theta_gamma)
    if not (torch.is_tensor(prob) and prob.dim() == 3 and prob.dtype == torch.float32):
        raise ValueError("the refinement expects an fp32 probability [N,H,W]")
    if not (torch.is_tensor(img_u8) and img_u8.dim() == 4 and img_u8.dtype == torch.uint8 and
            tuple(img_u8.shape) == tuple(prob.shape) + (3,)):
        raise ValueError("the refinement expects uint8 frames [N,H,W,3] for a probability %s (got %s %s)" %
                         (tuple(prob.shape), tuple(img_u8.shape) if torch.is_tensor(img_u8) else type(img_u8).__name__,
                          getattr(img_u8, "dtype", None)))
    if not (prob.is_cuda and img_u8.is_cuda) or prob.device != img_u8.device:
        raise ValueError("the refinement expects the probability and the frames on one CUDA device (got %s and %s; there is no "
                         "CPU fallback)" % (prob.device, img_u8.device))
    n, h, w = prob.shape
    if n * h * w == 0 or h > CRF_MAX_SIDE or w > CRF_MAX_SIDE:
        raise ValueError("the refinement takes planes of 1 to %d pixels a side (got %s)" % (CRF_MAX_SIDE, tuple(prob.shape)))
    if iters == 0:
        return prob
    nbytes = _lib.load().iswm_crf_refine_workspace(n, h, w)
    if nbytes < 0:
        raise ValueError("the refinement does not take the shape %s" % (tuple(prob.shape),))
    prob, img_u8 = prob.contiguous(), img_u8.contiguous()
    work = torch.empty((nbytes // 4,), dtype=torch.float32, device=prob.device)
    out = torch.empty_like(prob)
    call("iswm_crf_refine", _p(prob), _p(img_u8), n, h, w, int(radius), int(step), int(iters), float(w_bilateral),
         float(w_spatial), float(theta_alpha), float(theta_beta), float(theta_gamma), _p(out), _p(work), nbytes, _stream())
    return out


VAL_PANELS = ("original", "target_rgb", "pred_rgb", "overlay", "error", "pred", "conf")     # the packed order


def val_palette(num_classes):
    """uint8 [256, 3] RGB colour of every class index.  num_classes == 2: the reference's decode_target
    (train.py:611-618) -- index 1 white, every other index (255 included) black.  Any other class count: the PASCAL VOC
    bit-interleave colour map over all 256 indices (the reference paints everything black there)."""
    pal = np.zeros((256, 3), dtype=np.uint8)
    if num_classes == 2:
        pal[1] = 255
        return pal
    for i in range(256):
        c, rgb = i, [0, 0, 0]
        for j in range(8):
            for k in range(3):
                rgb[k] |= ((c >> k) & 1) << (7 - j)
            c >>= 3
        pal[i] = rgb
    return pal


def denorm_constants(mean, std):
    """(M, S) of the reference's Denormalize (utils/utils.py:14-24): -mean / std and 1 / std per channel, the
    quotients taken in fp64 and rounded once to fp32 (torchvision's normalize casts them to the tensor's dtype)"""
    mean, std = np.array(mean, dtype=np.float64), np.array(std, dtype=np.float64)
    return (-mean / std).astype(np.float32), (1 / std).astype(np.float32)


def val_panels_layout(n, h, w, want=VAL_PANELS):
    """byte offsets of the wanted panels in val_panels' packed uint8 buffer, in VAL_PANELS order, each 16-byte aligned
    (RGB panels [n, h, w, 3], pred / conf [n, h, w]), and its size under "end": the whole buffer comes back to the
    host in one transfer"""
    lay, off = {}, 0
    for k in VAL_PANELS:
        if k in want:
            lay[k] = off
            off += _align16(n * h * w * (1 if k in ("pred", "conf") else 3))
    lay["end"] = off
    return lay


class ValPanels(tuple):
    """(original, target_rgb, pred_rgb, overlay, error, pred, conf, prob, packed): uint8 RGB panels [N, H, W, 3], the
    class-index map pred and the confidence map conf uint8 [N, H, W], prob = max softmax probability fp32 [N, H, W];
    a panel that was not asked for is None; every uint8 tensor is a view of `packed` (val_panels_layout)"""
    __slots__ = ()
    original = property(lambda self: self[0])
    target_rgb = property(lambda self: self[1])
    pred_rgb = property(lambda self: self[2])
    overlay = property(lambda self: self[3])
    error = property(lambda self: self[4])
    pred = property(lambda self: self[5])
    conf = property(lambda self: self[6])
    prob = property(lambda self: self[7])
    packed = property(lambda self: self[8])


@functools.lru_cache(maxsize=8)
def _palette_on(num_classes, device):
    return torch.from_numpy(val_palette(num_classes)).to(device)


def val_panels(x, yl, labels, num_classes, mean, std, want=VAL_PANELS, want_prob=False):
    """the image panels of the reference's save_validation_results (train.py:461-523) for a batch, one launch:
    x normalised fp32 NCHW [N, 3, H, W], yl the model's forward_lowres logits, labels uint8 / int64 [N, H, W] class
    indices (255 = ignore) -> ValPanels with the panels named in `want` (VAL_PANELS; see iswm_hip.h for each).
    Enqueues only; never synchronises."""
    want = tuple(want)
    if [k for k in want if k not in VAL_PANELS] or not (want or want_prob):
        raise ValueError("val_panels: want %r must name at least one of %r" % (want, VAL_PANELS))
    if not (torch.is_tensor(x) and x.is_cuda and x.dim() == 4 and x.shape[1] == 3 and x.dtype == torch.float32):
        raise ValueError("expected a fp32 CUDA [N, 3, H, W] batch, got %s" %
                         ((tuple(x.shape), x.dtype, x.device) if torch.is_tensor(x) else type(x),))
    x = x.contiguous()
    n, _, H, W = x.shape
    dev = x.device
    if not (torch.is_tensor(labels) and labels.is_cuda) or tuple(labels.shape) != (n, H, W):
        raise ValueError("expected CUDA labels [%d, %d, %d], got %s" %
                         (n, H, W, (tuple(labels.shape), labels.device) if torch.is_tensor(labels) else type(labels)))
    labels = labels.contiguous()
    code = _int_code(labels)
    yl = as_f32(yl)
    ny, hl, wl, c, ld = geom(yl)
    if ld % 4 or ld < (num_classes + 3) // 4 * 4 or num_classes > c or not 1 <= num_classes <= 256:
        raise ValueError("logits %s (pitch %d) do not hold %d classes" % (tuple(yl.shape), ld, num_classes))
    if ny != n:
        raise ValueError("logits of %d images for a batch of %d" % (ny, n))
    lay = val_panels_layout(n, H, W, want)
    packed = torch.empty(max(lay["end"], 16), dtype=torch.uint8, device=dev)
    views = {k: packed[lay[k]:lay[k] + n * H * W * (1 if k in ("pred", "conf") else 3)].view(
        (n, H, W) if k in ("pred", "conf") else (n, H, W, 3)) for k in want}
    prob = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_prob else None
    dm, ds = denorm_constants(mean, std)
    m3 = (ctypes.c_float * 3)(*[float(v) for v in dm])
    s3 = (ctypes.c_float * 3)(*[float(v) for v in ds])
    pal = _palette_on(int(num_classes), dev)
    out = [views.get(k) for k in VAL_PANELS]
    call("iswm_val_panels", _p(x), _p(yl), _p(labels), code, n, hl, wl, ld, int(num_classes), int(H),
         int(W), m3, s3, _p(pal), _p(out[0]), _p(out[5]), _p(out[6]), _p(prob), _p(out[1]), _p(out[2]), _p(out[3]),
         _p(out[4]), _stream())
    return ValPanels(tuple(out) + (prob, packed))


def scene_plan(H, W, tile, overlap):
    """the sliding-window plan of an H x W scene (iswm_scene_plan_make, a pure host function): a _lib.ScenePlan.
    Raises IswmError for tile < 1, overlap outside [0, 1024] or above half a window"""
    plan = _lib.ScenePlan()
    call("iswm_scene_plan_make", int(H), int(W), int(tile), int(overlap), ctypes.byref(plan))
    return plan


def scene_tiles_normalize(scene_u8, plan, first, count, mean, std):
    """windows first .. first + count - 1 of a uint8 [H, W, 3] RGB scene on the device -> normalised fp32 NCHW
    [count, 3, th, tw], bit-identical to predict_normalize of the cropped windows"""
    if scene_u8.dim() != 3 or scene_u8.shape[2] != 3 or scene_u8.dtype != torch.uint8 or not scene_u8.is_cuda:
        raise ValueError("expected a uint8 CUDA [H, W, 3] scene, got %s %s" % (tuple(scene_u8.shape), scene_u8.dtype))
    if tuple(scene_u8.shape[:2]) != (plan.H, plan.W):
        raise ValueError("scene %s does not match the plan's %d x %d" % (tuple(scene_u8.shape), plan.H, plan.W))
    if first < 0 or count < 1 or first + count > plan.ntiles:
        raise ValueError("windows [%d, %d) outside the plan's %d" % (first, first + count, plan.ntiles))
    scene_u8 = scene_u8.contiguous()
    out = torch.empty((count, 3, plan.th, plan.tw), dtype=torch.float32, device=scene_u8.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    call("iswm_scene_tiles_normalize", _p(scene_u8), ctypes.byref(plan), int(first), int(count), m, s, _p(out),
         _stream())
    return out


def scene_maps(yl_tiles, num_classes, fg, plan, thr, min_prob, max_prob, want_prob=False):
    """low-resolution NHWC logits of all windows of one scene [plan.ntiles, hl, wl, ld] -> PredictMaps at
    [1, H, W]: every pixel blends the windows that cover it (a gather; weights ramp over the overlap), then
    predict_maps's outputs.  A scene of one window gives predict_maps's bytes.  Enqueues only."""
    yl = as_f32(yl_tiles)
    n, hl, wl, c, ld = geom(yl)
    if n != plan.ntiles:
        raise ValueError("logits %s do not hold the plan's %d windows" % (tuple(yl.shape), plan.ntiles))
    if ld % 4 or ld < (num_classes + 3) // 4 * 4 or num_classes > c:
        raise ValueError("logits %s (pitch %d) do not hold %d classes" % (tuple(yl.shape), ld, num_classes))
    if not 0 <= fg < num_classes:
        raise ValueError("foreground class %d outside [0, %d)" % (fg, num_classes))
    dev = yl.device
    H, W = plan.H, plan.W
    lay = predict_maps_layout(1, H, W)
    packed = torch.empty(lay["end"], dtype=torch.uint8, device=dev)
    stats = packed[:40].view(torch.float64).view(1, 5)
    pred, conf, band = (packed[lay[k]:lay[k] + H * W].view(1, H, W) for k in ("pred", "conf", "band"))
    prob = torch.empty((1, H, W), dtype=torch.float32, device=dev) if want_prob else None
    lo, hi = band_bounds(min_prob, max_prob)
    nbytes = _lib.load().iswm_scene_maps_workspace(H, W)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    call("iswm_scene_maps", _p(yl), ctypes.byref(plan), hl, wl, ld, int(num_classes), int(fg), float(thr), lo, hi,
         _p(pred), _p(conf), _p(band), _p(prob), _p(stats), _p(ws), nbytes, _stream())
    return PredictMaps((pred, conf, band, prob, stats, packed))


PREDICT_MAX_VIEWS = _lib.CONSTANTS["ISWM_PREDICT_MAX_VIEWS"]
TTA_MAX_SCALES = 8
TTA_SCALE_RANGE = (0.25, 4.0)


def tta_views(H, W, scales, flip):
    """the ordered views (Hv, Wv, flip) of an H x W frame under test-time augmentation (a pure host function):
    per scale s in the order given, Hv = max(1, int(H * s + 0.5)) and the same for Wv, the unflipped view and, with
    `flip`, the horizontally flipped one after it.  1 to 8 distinct scales in [0.25, 4.0], at most 16 views; two
    scales that round to the same size are still two views.  Anything else raises ValueError naming the value."""
    if isinstance(H, bool) or isinstance(W, bool) or not isinstance(H, int) or not isinstance(W, int) or H < 1 or W < 1:
        raise ValueError("tta_views: bad frame size %r x %r" % (H, W))
    if not isinstance(flip, (bool, int)) or flip not in (0, 1):
        raise ValueError("tta_views: flip %r is neither False nor True" % (flip,))
    try:
        scales = list(scales)
    except TypeError:
        raise ValueError("tta_views: scales %r is no list of numbers" % (scales,)) from None
    if not 1 <= len(scales) <= TTA_MAX_SCALES:
        raise ValueError("tta_views: %d scales %r, need 1 to %d" % (len(scales), scales, TTA_MAX_SCALES))
    seen = []
    for s in scales:
        if isinstance(s, bool) or not isinstance(s, (int, float)):
            raise ValueError("tta_views: scale %r is no number" % (s,))
        s = float(s)
        if not TTA_SCALE_RANGE[0] <= s <= TTA_SCALE_RANGE[1]:             # a NaN fails both compares
            raise ValueError("tta_views: scale %r outside [%g, %g]" % ((s,) + TTA_SCALE_RANGE))
        if s in seen:
            raise ValueError("tta_views: scale %r is given twice" % (s,))
        seen.append(s)
    views = []
    for s in seen:
        hv, wv = max(1, int(H * s + 0.5)), max(1, int(W * s + 0.5))
        views.append((hv, wv, False))
        if flip:
            views.append((hv, wv, True))
    if len(views) > PREDICT_MAX_VIEWS:
        raise ValueError("tta_views: %d views exceed the limit of %d" % (len(views), PREDICT_MAX_VIEWS))
    return views


def predict_view_normalize(img, Hv, Wv, flip, mean, std):
    """uint8 [N, H, W, 3] RGB on the device -> one test-time-augmentation view as normalised fp32 NCHW [N, 3, Hv, Wv]:
    the frame resampled (bilinear, align_corners=False), mirrored left to right when `flip`, then predict_normalize's
    arithmetic.  (H, W, False) is bit-identical to predict_normalize, (H, W, True) to that of the mirrored frame."""
    if img.dim() == 3:
        img = img.unsqueeze(0)
    if img.dim() != 4 or img.shape[3] != 3 or img.dtype != torch.uint8 or not img.is_cuda:
        raise ValueError("expected a uint8 CUDA [N, H, W, 3] image batch, got %s %s" % (tuple(img.shape), img.dtype))
    Hv, Wv = int(Hv), int(Wv)
    if Hv < 1 or Wv < 1:
        raise ValueError("bad view size %d x %d" % (Hv, Wv))
    img = img.contiguous()
    n, h, w, _ = img.shape
    out = torch.empty((n, 3, Hv, Wv), dtype=torch.float32, device=img.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean])
    s = (ctypes.c_float * 3)(*[float(v) for v in std])
    call("iswm_predict_view_normalize", _p(img), n, h, w, Hv, Wv, int(bool(flip)), m, s, _p(out), _stream())
    return out


def predict_views_maps(yls, flips, num_classes, fg, H, W, thr, min_prob, max_prob, want_prob=False):
    """the low-resolution NHWC logits of every view of one frame batch (a list of the model's forward_lowres outputs
    [N, hl_v, wl_v, ld], one per view, and the views' flip flags) -> PredictMaps at [N, H, W]: per pixel the mean over
    the views of predict_maps's probability, each view sampled straight from its logits (a flipped one at the
    mirrored column), then predict_maps's outputs.  A gather: no canvas, no atomics.  One unflipped view gives
    predict_maps's bytes.  Enqueues only; never synchronises."""
    yls, flips = list(yls), [bool(f) for f in flips]
    if not 1 <= len(yls) <= PREDICT_MAX_VIEWS or len(flips) != len(yls):
        raise ValueError("%d views (%d flip flags), need 1 to %d" % (len(yls), len(flips), PREDICT_MAX_VIEWS))
    yls = [as_f32(y) for y in yls]
    n, _, _, c, ld = geom(yls[0])
    views = (_lib.PredictView * len(yls))()
    for v, (y, f) in enumerate(zip(yls, flips)):
        nv, hl, wl, cv, ldv = geom(y)
        if (nv, cv, ldv) != (n, c, ld) or y.device != yls[0].device:
            raise ValueError("view %d: logits %s (pitch %d) do not match view 0's %s (pitch %d)" %
                             (v, tuple(y.shape), ldv, tuple(yls[0].shape), ld))
        views[v] = _lib.PredictView(y.data_ptr(), hl, wl, int(f))
    if ld % 4 or ld < (num_classes + 3) // 4 * 4 or num_classes > c:
        raise ValueError("logits %s (pitch %d) do not hold %d classes" % (tuple(yls[0].shape), ld, num_classes))
    if not 0 <= fg < num_classes:
        raise ValueError("foreground class %d outside [0, %d)" % (fg, num_classes))
    dev = yls[0].device
    lay = predict_maps_layout(n, H, W)
    packed = torch.empty(lay["end"], dtype=torch.uint8, device=dev)
    stats = packed[:40 * n].view(torch.float64).view(n, 5)
    pred, conf, band = (packed[lay[k]:lay[k] + n * H * W].view(n, H, W) for k in ("pred", "conf", "band"))
    prob = torch.empty((n, H, W), dtype=torch.float32, device=dev) if want_prob else None
    lo, hi = band_bounds(min_prob, max_prob)
    nbytes = _lib.load().iswm_predict_views_maps_workspace(n, H, W)
    ws = torch.empty(max(1, nbytes), dtype=torch.uint8, device=dev)
    call("iswm_predict_views_maps", views, len(yls), n, ld, int(num_classes), int(fg), int(H), int(W), float(thr),
         lo, hi, _p(pred), _p(conf), _p(band), _p(prob), _p(stats), _p(ws), nbytes, _stream())
    return PredictMaps((pred, conf, band, prob, stats, packed))


def sgd_step(p, g, buf, lr_dev, momentum, weight_decay, nesterov):
    call("iswm_sgd_step", _p(p), _p(g), _p(buf), p.numel(), _p(lr_dev), float(momentum), float(weight_decay),
         int(bool(nesterov)), _stream())


def adam_step(p, g, m, v, hyper_dev, beta1, beta2, eps, weight_decay, decoupled):
    call("iswm_adam_step", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper_dev), float(beta1), float(beta2),
         float(eps), float(weight_decay), int(bool(decoupled)), _stream())


# ---- gradient-norm clipping and EMA weights inside the step (csrc/optim.hip) --------------------
CLIP_COEF, CLIP_NORM = 0, 1          # slots of the 4-float clip block; floats 2..3 hold the sum of squares as one double


def new_clip_state(device):
    """(slots, clip): the double partials iswm_grad_sqnorm leaves and the 4-float block iswm_clip_finalize writes"""
    return (torch.zeros(_lib.load().iswm_grad_sqnorm_slots(), dtype=torch.float64, device=device),
            torch.zeros(4, dtype=torch.float32, device=device))


def grad_sqnorm(g, slots, accumulate=False):
    """adds sum(g^2) of a flat fp32 range into `slots` (accumulate) or starts a new total there; enqueues only"""
    if g.dtype != torch.float32 or g.dim() != 1 or not g.is_contiguous() or slots.dtype != torch.float64 or \
            slots.numel() < _lib.load().iswm_grad_sqnorm_slots() or not slots.is_contiguous():
        raise ValueError("grad_sqnorm: a flat fp32 range and the fp64 slots of new_clip_state expected")
    call("iswm_grad_sqnorm", _p(g), g.numel(), _p(slots), int(bool(accumulate)), _stream())


def clip_finalize(slots, max_norm, clip):
    """clip[0] = min(1, max_norm / (norm + 1e-6)), clip[1] = norm, clip[2:4] (as one double) = sum of squares"""
    if clip.dtype != torch.float32 or clip.numel() != 4 or not clip.is_contiguous():
        raise ValueError("clip_finalize: a 4-float device block expected")
    call("iswm_clip_finalize", _p(slots), float(max_norm), _p(clip), _stream())


def clip_sumsq(clip):
    """the double sum of squares behind floats 2..3 of a clip block (a 0-dim view, no copy)"""
    return clip[2:4].view(torch.float64)[0]


def sgd_step_ex(p, g, buf, hyper_dev, momentum, weight_decay, nesterov, clip=None, ema=None):
    """iswm_sgd_step with g * clip[0] at the load of g (g itself untouched) and ema += hyper_dev[3] * (p_new - ema)"""
    if hyper_dev.numel() < 4 or (ema is not None and ema.numel() != p.numel()):
        raise ValueError("sgd_step_ex: a 4-float hyper block and an ema range of p's size expected")
    call("iswm_sgd_step_ex", _p(p), _p(g), _p(buf), p.numel(), _p(hyper_dev), float(momentum), float(weight_decay),
         int(bool(nesterov)), _p(clip), _p(ema), _stream())


def adam_step_ex(p, g, m, v, hyper_dev, beta1, beta2, eps, weight_decay, decoupled, clip=None, ema=None):
    if hyper_dev.numel() < 4 or (ema is not None and ema.numel() != p.numel()):
        raise ValueError("adam_step_ex: a 4-float hyper block and an ema range of p's size expected")
    call("iswm_adam_step_ex", _p(p), _p(g), _p(m), _p(v), p.numel(), _p(hyper_dev), float(beta1), float(beta2),
         float(eps), float(weight_decay), int(bool(decoupled)), _p(clip), _p(ema), _stream())


def swap_f32(a, b):
    """a <-> b in place (two disjoint flat fp32 ranges of one size)"""
    if a.dtype != torch.float32 or b.dtype != torch.float32 or a.numel() != b.numel() or \
            not a.is_contiguous() or not b.is_contiguous():
        raise ValueError("swap_f32: two contiguous fp32 ranges of one size expected")
    call("iswm_swap_f32", _p(a), _p(b), a.numel(), _stream())


# ---- INT8 post-training quantized inference (csrc/qconv.hip, csrc/quant.hip; iswm_amd/quant.py) ---------------------
# int8 activations are NHWC torch.int8 tensors (pitched views allowed, pitch in bytes); one symmetric scale per tensor.
def i8geom(t):
    return geom(t, torch.int8)


def qconv_desc(x, cout, k, stride, pad, dil, ldy, cstore, relu, lo, out_f32, ldr=0):
    n, h, w, cin, ldx = i8geom(x)
    ho, wo = conv_out_size(h, k, stride, pad, dil), conv_out_size(w, k, stride, pad, dil)
    return _lib.QConvDesc(n, h, w, cin, ho, wo, cout, k, k, stride, pad, dil, ldx, ldy, ldr, int(bool(relu)), int(lo),
                          int(bool(out_f32)), cstore)


def qconv_fwd(x, w, mul, add, k, stride, pad, dil, relu, lo, inv_s_out, out=None, res=None, s_res=0.0, out_f32=False,
              cstore=None):
    """int8 implicit-GEMM convolution: x int8 NHWC [N,H,W,Cin] (Cin % 64 == 0), w int8 [Cout_p, KH*KW*Cin] (OHWI,
    Cout_p % 16 == 0), mul / add fp64 [Cout_p] -> `out` (int8, or fp32 when out_f32) of which the first `cstore`
    channels are written (default Cout_p; the default `out` has cstore channels on a pad4(cstore) pitch).  Epilogue: see
    iswm_qconv_fwd."""
    cout = w.shape[0]
    cstore = cout if cstore is None else cstore
    if w.dtype != torch.int8 or not w.is_contiguous() or mul.dtype != torch.float64 or add.dtype != torch.float64:
        raise ValueError("qconv: int8 contiguous weights and fp64 mul / add expected")
    n, h, wd, cin, _ = i8geom(x)
    ho, wo = conv_out_size(h, k, stride, pad, dil), conv_out_size(wd, k, stride, pad, dil)
    if out is None:                                       # the C ABI wants ldy % 4 == 0: a pad4 pitch under a cstore view
        out = torch.empty((n, ho, wo, (cstore + 3) // 4 * 4), dtype=torch.float32 if out_f32 else torch.int8,
                          device=x.device)[..., :cstore]
    on, oh, ow, oc, ldy = geom(out, torch.float32 if out_f32 else torch.int8)
    if (on, oh, ow) != (n, ho, wo) or oc < cstore:
        raise ValueError("qconv: out %s cannot hold [%d, %d, %d, %d]" % (tuple(out.shape), n, ho, wo, cstore))
    ldr = 0
    if res is not None:
        rn, rh, rw, rc, ldr = i8geom(res)
        if (rn, rh, rw) != (n, ho, wo) or rc < cstore:
            raise ValueError("qconv: residual %s does not cover [%d, %d, %d, %d]" % (tuple(res.shape), n, ho, wo, cstore))
    d = qconv_desc(x, cout, k, stride, pad, dil, ldy, cstore, relu, lo, out_f32, ldr)
    if w.numel() != _lib.load().iswm_qconv_weight_bytes(ctypes.byref(d)):
        raise ValueError("qconv: weights %s do not match the geometry" % (tuple(w.shape),))
    call("iswm_qconv_fwd", ctypes.byref(d), _p(x), _p(w), _p(mul), _p(add), _p(res), float(s_res), float(inv_s_out),
         _p(out), _stream())
    return out


def absmax(x, amax, c=None, slab=None):
    """amax (a 1-element fp32 device tensor) = max(amax, max |x|) over the first c channels of an fp32 NHWC or
    Planes tensor.  Enqueues only."""
    px, n, h, w, cc, ld, ps = xgeom(x)
    c = cc if c is None else c
    rows = n * h * w
    nbytes = _lib.load().iswm_absmax_workspace(rows, c)
    if slab is None or slab.numel() * 4 < nbytes:
        slab = torch.empty((max(1, nbytes // 4),), dtype=torch.float32, device=amax.device)
    call("iswm_absmax", _p(px), ps, rows, c, ld, _p(slab), nbytes, _p(amax), _stream())
    return amax


def quantize_i8(x, inv_s, lo, ldy=None, c=None, out=None):
    """fp32 NHWC / Planes -> int8 NHWC: clamp(rint(x * inv_s), lo, 127) for the first c channels, 0 up to ldy"""
    px, n, h, w, cc, ld, ps = xgeom(x)
    c = cc if c is None else c
    if out is None:
        out = torch.empty((n, h, w, ldy or (c + 63) // 64 * 64), dtype=torch.int8, device=px.device)
    _, _, _, _, ldo = i8geom(out)
    if out.shape[3] != ldo:
        raise ValueError("quantize_i8 writes whole pixels: out must not be a channel slice")
    call("iswm_quantize_i8", _p(px), ps, n * h * w, c, ld, float(inv_s), int(lo), _p(out), ldo, _stream())
    return out


def qgap(x, s_in, inv_s_in, ldy=None):
    """int8 global average pool [N,H,W,C] -> int8 [N,1,1,ldy] re-quantized with the input's scale"""
    n, h, w, c, ldx = i8geom(x)
    ldy = ldy or c
    y = torch.zeros((n, 1, 1, ldy), dtype=torch.int8, device=x.device)
    call("iswm_qgap", _p(x), n, h * w, c, ldx, float(s_in), float(inv_s_in), _p(y), ldy, _stream())
    return y


def qbcast(v, out):
    """int8 [N,1,1,C] -> every pixel of `out` (an int8 [N,H,W,C] channel slice)"""
    n, h, w, c, ldy = i8geom(out)
    _, _, _, cv, ldv = i8geom(v)
    if cv < c:
        raise ValueError("qbcast: %d source channels for a %d-wide slice" % (cv, c))
    call("iswm_qbcast", _p(v), n, h * w, c, ldv, _p(out), ldy, _stream())
    return out


def qbilinear(x, s_in, inv_s_out, out):
    """int8 bilinear resize (align_corners=False) of x into `out` (an int8 channel slice of the destination size)"""
    n, hi, wi, c, ldx = i8geom(x)
    no, ho, wo, co, ldy = i8geom(out)
    if no != n or co != c:
        raise ValueError("qbilinear: %s does not fit %s" % (tuple(x.shape), tuple(out.shape)))
    call("iswm_qbilinear", _p(x), n, hi, wi, c, ldx, float(s_in), ho, wo, float(inv_s_out), _p(out), ldy, _stream())
    return out
