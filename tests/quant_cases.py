"""Edge cases of the INT8 kernels (csrc/qconv.hip, csrc/quant.hip), shared by tests/test_quant_cpu.py and
tests/test_quant_edges_gpu.py.  Every case exists for one property, named in its `why`; the CPU tests assert that
property from the geometry restated here and from tests/quant_ref.py alone, the GPU tests hold the kernels to
tests/quant_ref.py bit for bit.  Operands come from a fixed seed per case id (crc32 of the id)."""
import collections
import zlib

import numpy as np
import torch

from tests import quant_ref as R


def rng_of(case_id):
    return np.random.default_rng(zlib.crc32(case_id.encode()))


def pad4(c):
    return (c + 3) // 4 * 4


def ceil16(c):
    return (c + 15) // 16 * 16


# ---- the launch geometry, restated ----
QC_WAVE_ROWS = 64          # pixels of one wave: four row blocks of 16
QC_WG_ROWS = 256           # pixels of one workgroup: four waves
STREAM_BLOCK = 256         # threads of a streaming workgroup
STREAM_CAP = 2048          # workgroups of a streaming grid at the most


def stream_grid(items, block=STREAM_BLOCK):
    return max(1, min(STREAM_CAP, (items + block - 1) // block))


def conv_out(n, k, stride, pad, dil):
    return (n + 2 * pad - dil * (k - 1) - 1) // stride + 1


# ---- qconv ----
QConv = collections.namedtuple("QConv", "id N H W Cin Cout k stride pad dil relu residual f32 why")


def _q(id_, geom, relu=False, residual=False, f32=False, why=""):
    return QConv(id_, *geom, relu, residual, f32, why)


_CS = (1, 3, 5, 64)      # N, H, W, Cin of the cstore cases
QCONV = [
    _q("one_pixel", (1, 1, 1, 64, 16, 1, 1, 0, 1), why="M = 1, one K step"),
    _q("pooled", (3, 1, 1, 128, 256, 1, 1, 0, 1), relu=True, why="M = 3, 64-wide kernel, 4 column blocks"),
    _q("centre_only_1x1", (2, 1, 1, 64, 16, 3, 1, 2, 2), why="8 of 9 taps out of bounds at every pixel"),
    _q("rate_ge_map", (1, 5, 7, 64, 64, 3, 1, 18, 18), relu=True,
       why="only the centre tap in bounds; M = 35: one wave, third row block ragged; equals the 1x1 conv of the centre"),
    _q("rate_partial", (1, 9, 11, 64, 16, 3, 1, 6, 6),
       why="each of the eight outer taps is in bounds for one pixel and out of bounds for another"),
    _q("s2_even", (2, 8, 10, 64, 16, 3, 2, 1, 1), relu=True,
       why="Ho x Wo = 4 x 5; the last row and column read no bottom / right padding"),
    _q("s2_1x1_even", (2, 8, 10, 128, 64, 1, 2, 0, 1), why="Ho x Wo = 4 x 5"),
    _q("valid_pad0", (1, 6, 7, 64, 16, 3, 1, 0, 1), why="Ho x Wo = 4 x 5, no padding tap anywhere"),
    _q("over_pad", (1, 4, 5, 64, 16, 3, 1, 3, 1), residual=True,
       why="Ho x Wo = 8 x 9; border pixels have all nine taps out of bounds: the epilogue of add"),
    _q("m256", (1, 16, 16, 64, 16, 1, 1, 0, 1), why="M = 256 fills one workgroup exactly"),
    _q("m257", (1, 1, 257, 64, 16, 1, 1, 0, 1), why="M = 257 leaves one pixel to a second workgroup"),
    _q("chunks3", (1, 5, 5, 192, 16, 3, 1, 1, 1), relu=True, why="3 chunks per tap, 27 steps"),
    _q("x_slice", (1, 5, 5, 128, 16, 3, 1, 1, 1),
       why="x is channels [64, 192) of a 256-wide buffer whose other channels hold 127"),
    _q("extreme_pos", (1, 3, 3, 2048, 16, 3, 1, 1, 1), f32=True, why="centre accumulator +128 * 128 * 18432"),
    _q("extreme_neg", (1, 3, 3, 2048, 16, 3, 1, 1, 1), f32=True, why="centre accumulator -128 * 127 * 18432"),
]
for _c in (1, 2, 3, 17, 61):
    _where = {17: ": second block of the 16-wide kernel", 61: ": last group of the 64-wide kernel"}.get(_c, "")
    QCONV.append(_q("cstore_%d_i8" % _c, _CS + (_c, 1, 1, 0, 1), why="tail of %d channels%s" % (_c % 4, _where)))
    QCONV.append(_q("cstore_%d_f32" % _c, _CS + (_c, 1, 1, 0, 1), f32=True, why="the same tail, fp32 stores"))
    if _c in (17, 61):
        QCONV.append(_q("cstore_%d_res" % _c, _CS + (_c, 1, 1, 0, 1), residual=True, relu=True,
                        why="the same tail with a residual of pitch pad4(cstore)"))
_TIES = (1, 8, 16, 64, 64, 1, 1, 0, 1)
QCONV += [
    _q("ties", _TIES, why="acc over [-300, 300], mul 0.5: exact ties of both signs and both clamps"),
    _q("ties_res", _TIES, residual=True, why="the ties moved by a residual with s_res 0.5"),
    _q("ties_relu", _TIES, relu=True, why="ReLU and lo = 0: every negative gives 0"),
]
QCONV_BY_ID = {c.id: c for c in QCONV}
X_SLICE = (256, 64)        # x_slice: buffer width and first channel


def qconv_tiles(c):
    """where the kernel puts the case: M, K steps, grid and the column block / group that holds the store tail"""
    ho, wo = conv_out(c.H, c.k, c.stride, c.pad, c.dil), conv_out(c.W, c.k, c.stride, c.pad, c.dil)
    m = c.N * ho * wo
    cout_p = ceil16(c.Cout)
    wide = cout_p % 64 == 0
    per_block = 64 if wide else 16
    tail = c.Cout - 1                                   # the last stored channel
    return dict(Ho=ho, Wo=wo, M=m, chunks=c.Cin // 64, steps=c.k * c.k * (c.Cin // 64), Cout_p=cout_p, wide=wide,
                grid=((m + QC_WG_ROWS - 1) // QC_WG_ROWS, cout_p // per_block), waves=(m + QC_WAVE_ROWS - 1) // QC_WAVE_ROWS,
                row_blocks=(m + 15) // 16, ragged_rows=m % 16,
                tail_block=tail // per_block, tail_group=(tail % per_block) // 16, tail_len=c.Cout % 4)


def qconv_taps(c):
    """[Ho, Wo, k, k] bool: tap (i, j) of output pixel (oh, ow) lies inside the map"""
    ho, wo = conv_out(c.H, c.k, c.stride, c.pad, c.dil), conv_out(c.W, c.k, c.stride, c.pad, c.dil)
    ih = np.arange(ho)[:, None] * c.stride - c.pad + np.arange(c.k)[None, :] * c.dil
    iw = np.arange(wo)[:, None] * c.stride - c.pad + np.arange(c.k)[None, :] * c.dil
    okh, okw = (ih >= 0) & (ih < c.H), (iw >= 0) & (iw < c.W)
    return okh[:, None, :, None] & okw[None, :, None, :]


def _ties_operands(c):
    """out channel o < 32 reads x[o] + 2 x[o + 32] = t, o >= 32 reads -t; t runs over the integers [-300, 300]"""
    m = c.N * c.H * c.W
    t = (np.arange(m * 32) % 601 - 300).reshape(m, 32)
    b = np.rint(t / 3.0).astype(np.int64)
    a = t - 2 * b
    assert np.abs(a).max() <= 127 and np.abs(b).max() <= 127
    x = np.concatenate([a, b], axis=1).astype(np.int8).reshape(c.N, c.H, c.W, 64)
    w = np.zeros((64, 64, 1, 1), np.int8)
    for o in range(32):
        w[o, o, 0, 0], w[o, o + 32, 0, 0] = 1, 2
        w[o + 32, o, 0, 0], w[o + 32, o + 32, 0, 0] = -1, -2
    return x, w


def qconv_operands(c):
    """dict: xbuf int8 [N,H,W,ld] with x = xbuf[..., x0:x0+Cin]; w int8 [Cout,Cin,k,k]; mul, add fp64 [Cout]; inv_s
    (None: fp32 output), lo; res int8 [N,Ho,Wo,Cout] or None, s_res"""
    rng = rng_of(c.id)
    t = qconv_tiles(c)
    kk = c.k * c.k * c.Cin
    x0 = 0
    if c.id.startswith("ties"):
        x, w = _ties_operands(c)
        mul, add, inv_s, s_res = np.full(c.Cout, 0.5), np.zeros(c.Cout), 1.0, 0.5
    elif c.id.startswith("extreme"):
        x = np.full((c.N, c.H, c.W, c.Cin), -128, np.int8)
        w = np.full((c.Cout, c.Cin, c.k, c.k), -128 if c.id == "extreme_pos" else 127, np.int8)
        mul, add, inv_s, s_res = np.ones(c.Cout), np.zeros(c.Cout), None, 0.0
    else:
        x = rng.integers(-128, 128, (c.N, c.H, c.W, c.Cin)).astype(np.int8)
        w = rng.integers(-128, 128, (c.Cout, c.Cin, c.k, c.k)).astype(np.int8)
        x.reshape(-1)[0] = w.reshape(-1)[0] = -128
        # acc of uniform int8 operands has std about 74^2 sqrt(K): v spreads over about +-2 and the scale clamps some
        mul = rng.uniform(0.5, 1.5, c.Cout) / (5476.0 * np.sqrt(kk))
        add = rng.normal(0, 0.05, c.Cout)
        inv_s, s_res = 127.0 / 2.0, 0.013
    if c.f32:
        inv_s = None
    xbuf = x
    if c.id == "x_slice":
        ld, x0 = X_SLICE
        xbuf = np.full((c.N, c.H, c.W, ld), 127, np.int8)
        xbuf[..., x0:x0 + c.Cin] = x
    res = rng.integers(-128, 128, (c.N, t["Ho"], t["Wo"], c.Cout)).astype(np.int8) if c.residual else None
    return dict(xbuf=xbuf, x0=x0, w=w, mul=mul, add=add, inv_s=inv_s, lo=0 if c.relu else -127, res=res, s_res=s_res)


def qconv_v(c, o):
    """the epilogue's fp64 value before ReLU, rounding and clamping"""
    x = o["xbuf"][..., o["x0"]:o["x0"] + c.Cin]
    v = R.conv_int(x, o["w"], c.stride, c.pad, c.dil).astype(np.float64) * o["mul"] + o["add"]
    if o["res"] is not None:
        v = v + o["res"].astype(np.float64) * o["s_res"]
    return v


def qconv_expected(c, o):
    x = o["xbuf"][..., o["x0"]:o["x0"] + c.Cin]
    acc = R.conv_int(x, o["w"], c.stride, c.pad, c.dil)
    return R.epilogue(acc, o["mul"], o["add"], c.relu, o["inv_s"], o["lo"], o["res"], o["s_res"])


def tie_counts(v, inv_s, lo):
    """of the fp64 values v * inv_s: exact ties inside the clamps that round down / up to even, by sign, and the
    values clamped at each end"""
    u = np.asarray(v, np.float64) * inv_s
    tie = (u - np.floor(u) == 0.5) & (u > lo) & (u < 127)
    down = tie & (np.rint(u) == np.floor(u))
    up = tie & (np.rint(u) == np.ceil(u))
    return dict(down_pos=int((down & (u > 0)).sum()), up_pos=int((up & (u > 0)).sum()),
                down_neg=int((down & (u < 0)).sum()), up_neg=int((up & (u < 0)).sum()),
                clamp_hi=int((np.rint(u) > 127).sum()), clamp_lo=int((np.rint(u) < lo).sum()))


# ---- absmax ----
# id -> (shape of the buffer [N, H, W, ld], C, first channel, source form, amax before); channels outside
# [first, first + C) hold 1e6
Absmax = collections.namedtuple("Absmax", "id shape C c0 planes amax0 peak why")
ABSMAX = [Absmax("c%d_f32" % c, (2, 3, 5, pad4(c) + 4), c, 0, False, 0.0, "neg",
                 "C = %d on a pad4(C) + 4 pitch; the maximum is negative" % c) for c in (1, 2, 3, 5, 7)]
ABSMAX += [Absmax("c%d_planes" % c, (2, 3, 5, pad4(c) + 4), c, 0, True, 0.0, "neg", "the same from planes") for c in (3, 5)]
ABSMAX += [
    Absmax("planes_slice", (2, 3, 5, 16), 7, 4, True, 0.0, "neg", "planes channels [4, 11) of 16"),
    Absmax("cap_last_row", (1, 257, 256, 32), 32, 0, False, 0.0, "last", "526 336 groups; the maximum in the last row"),
    Absmax("cap_row0", (1, 257, 256, 32), 32, 0, False, 0.0, "first", "526 336 groups; the maximum in row 0"),
    Absmax("preset", (2, 3, 5, 8), 5, 0, False, 1e4, "neg", "an amax above the data survives"),
]


def absmax_operands(c):
    """fp32 buffer [N, H, W, ld]; the tensor measured is buf[..., c0:c0 + C]"""
    rng = rng_of("absmax_" + c.id)
    buf = rng.normal(0, 1, c.shape).astype(np.float32)
    n, h, w, _ = c.shape
    sl = buf[..., c.c0:c.c0 + c.C]
    np.clip(sl, -4, 4, out=sl)
    if c.peak == "neg":                                 # in the last real channel: the last lane of a ragged group
        sl[n - 1, h // 2, w // 2, c.C - 1] = -7.3125
    elif c.peak == "last":
        sl[0, h - 1, w - 1, c.C - 1] = -7.3125
    else:
        sl[0, 0, 0, 0] = 7.3125
    buf[..., :c.c0] = 1e6
    buf[..., c.c0 + c.C:] = 1e6
    return buf


# ---- quantize_i8 ----
# values along whole rows of a [1, 8, W, C] tensor at inv_s = 1: ties of both signs and both clamps
TIE_ROWS = [0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 1e3, -1e3]
# a planes source: the bfloat16 of each value is the tie itself, the lower planes decide the side
NEAR_TIES = [0.5 + 2.0 ** -20, 0.5 - 2.0 ** -20, 1.5 + 2.0 ** -20, 1.5 - 2.0 ** -20, -2.5 + 2.0 ** -20, -2.5 - 2.0 ** -20]
Quantize = collections.namedtuple("Quantize", "id shape C ldy planes inv_s lo why")
QUANTIZE = [Quantize("c%d_ldy%d" % (c, ldy), (2, 5, 7), c, ldy, False, 127.0 / 5.3, -127,
                     "C = %d: channels past C are 0 up to %d" % (c, ldy)) for c in (3, 6) for ldy in (pad4(c), 64)]
QUANTIZE += [
    Quantize("tie_rows_lo-127", (1, 8, 9), 12, 12, False, 1.0, -127, "ties and clamps along whole rows"),
    Quantize("tie_rows_lo0", (1, 8, 9), 12, 64, False, 1.0, 0, "the same under lo = 0"),
    Quantize("tie_rows_planes", (1, 8, 9), 12, 12, True, 1.0, -127, "the same from a split planes source"),
    Quantize("near_ties_planes", (1, 6, 5), 8, 8, True, 1.0, -127, "the hi plane on the tie, the low planes decide"),
    Quantize("cap", (1, 129, 128), 128, 128, False, 127.0 / 4.0, -127, "528 384 words: past the grid cap"),
]


def quantize_operands(c):
    """fp32 [N, H, W, C] (the caller pads it to a pad4 pitch)"""
    rng = rng_of("quantize_" + c.id)
    n, h, w = c.shape
    if c.id.startswith("tie_rows"):
        x = np.broadcast_to(np.array(TIE_ROWS, np.float32)[None, :, None, None], (n, h, w, c.C)).copy()
    elif c.id == "near_ties_planes":
        x = np.broadcast_to(np.array(NEAR_TIES, np.float32)[None, :, None, None], (n, h, w, c.C)).copy()
    else:
        x = rng.normal(0, 2, (n, h, w, c.C)).astype(np.float32)
    return x


def planes_by_rounding(x):
    """fp32 -> bf16 [3, ...] with hi = the nearest bfloat16, mid = the nearest bfloat16 of the rest, lo = what is left:
    hi + mid + lo == x exactly (asserted), as a Planes tensor requires"""
    x = torch.as_tensor(x, dtype=torch.float32)
    hi = x.bfloat16()
    r1 = x - hi.float()
    mid = r1.bfloat16()
    lo = (r1 - mid.float()).bfloat16()
    assert torch.equal((hi.float() + mid.float()) + lo.float(), x)
    return torch.stack([hi, mid, lo])


# ---- qgap ----
QGap = collections.namedtuple("QGap", "id N H W C ldy s_in fill why")
QGAP = [
    QGap("c1_hw1", 1, 1, 1, 1, 4, 0.037, "rand", "one channel, one pixel; ldy > C"),
    QGap("c255_n5", 5, 5, 7, 255, 255, 0.037, "rand", "HW = 35; the last thread of the block idle"),
    QGap("c256_ties", 1, 1, 2, 256, 256, 2.0 ** -5, "ties", "HW = 2 pixel pairs on exact ties"),
    QGap("c257_ties_n5", 5, 2, 1, 257, 264, 2.0 ** -5, "ties", "a second block of one channel; the tail of y stays 0"),
    QGap("c600", 1, 5, 7, 600, 600, 0.037, "rand", "three blocks, the last ragged"),
    QGap("c600_min", 5, 1, 2, 600, 604, 0.037, "min", "every value -128"),
]
QGAP_PITCH = 8             # x is channels [0, C) of a C + 8 wide buffer whose tail holds 99
TIE_PAIRS = [(1, 0), (1, 2), (-1, 0), (-1, -2)]


def qgap_operands(c):
    rng = rng_of("qgap_" + c.id)
    buf = np.full((c.N, c.H, c.W, c.C + QGAP_PITCH), 99, np.int8)
    if c.fill == "min":
        x = np.full((c.N, c.H, c.W, c.C), -128, np.int8)
    elif c.fill == "ties":
        pairs = np.array(TIE_PAIRS, np.int8)[np.arange(c.N * c.C) % 4].reshape(c.N, c.C, 2)
        x = pairs.transpose(0, 2, 1).reshape(c.N, c.H, c.W, c.C).copy()
    else:
        x = rng.integers(-128, 128, (c.N, c.H, c.W, c.C)).astype(np.int8)
    buf[..., :c.C] = x
    return buf


# ---- qbcast ----
QBcast = collections.namedtuple("QBcast", "id N H W C ldv why")
QBCAST = [
    QBcast("c4", 2, 3, 5, 4, 4, "C = 4: one word per pixel"),
    QBcast("ldv", 3, 3, 5, 8, 24, "the source is a channel slice"),
    QBcast("hw1", 3, 1, 1, 8, 8, "H * W = 1"),
    QBcast("cap", 1, 129, 128, 128, 128, "528 384 words: past the grid cap"),
]

# ---- qbilinear ----
QBil = collections.namedtuple("QBil", "id N Hi Wi Ho Wo C s_in inv_s why")
QBILINEAR = [
    QBil("identity", 2, 5, 7, 5, 7, 4, 0.25, 4.0, "the output is the input (|x| <= 127: -128 would clamp)"),
    QBil("down_33_9", 1, 33, 33, 9, 9, 260, 0.021, 127.0 / 2.9, "downscale"),
    QBil("down_7x5_3x2", 2, 7, 5, 3, 2, 4, 0.021, 127.0 / 2.9, "downscale, unequal"),
    QBil("mixed_5x9_13x4", 1, 5, 9, 13, 4, 260, 0.021, 127.0 / 2.9, "up in one axis, down in the other"),
    QBil("src_1x6", 2, 1, 6, 3, 11, 4, 0.021, 127.0 / 2.9, "a one-row source"),
    QBil("src_6x1", 2, 6, 1, 11, 3, 4, 0.021, 127.0 / 2.9, "a one-column source"),
    QBil("src_1x1", 2, 1, 1, 4, 5, 260, 0.021, 127.0 / 2.9, "every pixel is the source value requantized"),
    QBil("dst_1x1", 2, 9, 11, 1, 1, 4, 0.021, 127.0 / 2.9, "a one-pixel destination"),
]
QBIL_PITCH = (8, 12)       # source and destination are channels [8, 8 + C) of a C + 20 wide buffer


def qbilinear_operands(c):
    rng = rng_of("qbilinear_" + c.id)
    lo = -127 if c.id == "identity" else -128
    x = rng.integers(lo, 128, (c.N, c.Hi, c.Wi, c.C)).astype(np.int8)
    x.reshape(-1)[0] = lo
    return x


# ---- the network at its smallest maps, and tiled scenes on an INT8 model ----
NETWORK = [(16, 1, 33, 33), (16, 3, 33, 49), (8, 1, 33, 33), (8, 3, 33, 49)]      # (output stride, N, H, W)
SCENE = dict(H=97, W=129, tile=65, overlap=16, windows=6, tile_batches=(1, 4, 6))
