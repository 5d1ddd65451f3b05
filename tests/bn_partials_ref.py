"""Float64 restatements of the BatchNorm partials every producer publishes, the fp32 floors they are judged by, the cases of
tests/test_bn_partials_gpu.py and the mutants tests/test_bn_partials_cpu.py shows those cases to catch.

What is compared.  Every producer check starts from the tensor the kernel itself STORED (y forward, dx backward), so the
convolution arithmetic drops out and the only legitimate error is the fp32 summation and centring inside the epilogue:
  forward   S_t = sum of the tile's rows, M2_t = sum of squared deviations from the tile's own mean; tile t covers rows
            [t * tile_rows, min(M, (t + 1) * tile_rows)) of the stored y (minus the bias: the partials describe the convolution
            BEFORE the bias)
  backward  sum dz and sum dz * xhat over all rows, dz = stored dx * [pattern], xhat = (y - mean) * invstd
  finalize  the exact merge of given partials (synthetic: no producer)

Rule (the one of tests/conv_ref.py): rel_err = max|a - b| / max|b| against float64, <= 4 x FLOOR[check]; FLOOR[check] is a plain
fp32 restatement of the same quantity on the same kind of stored values, the largest over the check's cases.  The tile sums are
judged TILE BY TILE (tile_err: the metric of each tile's row of channels, the largest over the tiles -- a short last tile is
held to its own magnitude, not to that of the full tiles).  The fp32 restatement adds a tile's rows one after another in fp32,
centres about fp32(S_t / n_t) and adds the squared deviations the same way: a kernel may chain its adds, so torch's pairwise
`sum` would be too favourable (and torch's CPU `cumsum` accumulates fp32 input in double -- hence the explicit loop).  The
backward sums form dz * ((y - mean) * invstd) in fp32, add runs of <= 10 rows in fp32 and the runs in double (DESIGN.md
section 3.3).  On the CPU the "stored" tensor is torch's fp32 rounding of the float64 convolution of the same operands.
tests/test_bn_partials_cpu.py measures the floors again and ties them to profiles/bn_partials_tests.txt."""
import collections
import ctypes

import torch

from tests import conv_ref as R
from tests import streaming_ref as SR
from tests.util import rel_err

EPS = 1e-5
SENTINEL = -12345.0
PAD = 64                                           # sentinel floats / doubles in front of a partials buffer

# ---- forward cases ---------------------------------------------------------------------------------------------------------------
# routes added so that every raster-tiled kernel family has a last tile of tile_rows - 1 rows (the table of conv_ref has
# one-row and mid-sized last tiles only); tests/test_bn_partials_cpu.py checks the remainders through the host queries
EXTRA = [
    R._r("pl_short", "pl", (1, 1, 255, 64, 128, 1, 1, 0, 1), "k_conv_pl2<8, 1, 3, false>"),           # 255 = 128 + 127
    R._r("pl_narrow_short", "pl", (1, 1, 255, 64, 64, 1, 1, 0, 1), "k_conv_pl2<4, 2, 3, false>"),
    R._r("x6_short", "x6", (1, 1, 127, 64, 128, 1, 1, 0, 1), "k_conv_x6<64, 64, false, true, 3>"),    # 127 = 64 + 63
    R._r("f32_u_short", "f32", (1, 1, 127, 64, 128, 1, 1, 0, 1), "k_conv_fwd_u<64, 64>"),
    R._r("f32_short", "f32", (1, 1, 255, 48, 48, 1, 1, 0, 1), "k_conv_fwd<64>"),
    R._r("stem_short", "x6", (1, 9, 229, 4, 64, 7, 2, 3, 1), "k_stem_fwd<6>"),                        # 575 = 5 x 96 + 95
    # the tall tiles and the wide kernel have epilogues and row masks of their own
    R._r("pl_r9_short", "pl", (1, 1, 9071, 64, 512, 1, 1, 0, 1), "k_conv_pl2<9, 1, 3, false>"),       # 9071 = 62 x 144 + 143
    R._r("pl_r10_short", "pl", (1, 1, 9919, 64, 512, 1, 1, 0, 1), "k_conv_pl2<10, 1, 3, false>"),     # 9919 = 61 x 160 + 159
    R._r("pl_wide_short", "pl", (1, 1, 10367, 512, 512, 1, 1, 0, 1), "k_conv_pl2w<8, 3, false>"),     # 10367 = 80 x 128 + 127
]
FWD_ROUTES = [rt for rt in R.ROUTES if "fwd" in rt.names] + EXTRA
ROUTE = dict((rt.id, rt) for rt in FWD_ROUTES)
ONE_ROW_LAST = ("pl_1x1", "x6_1x1", "f32_u", "bf16_1x1")             # 385 rows: the last tile holds ONE row
SHORT_LAST = tuple(rt.id for rt in EXTRA)                            # the last tile holds tile_rows - 1 rows
PATCH = ("x6_patch", "x6_patch_d2", "bf16_patch")                    # layout tile_rows == 0: merge-level checks
# Cout no multiple of the 128-column block (MobileNetV2's 96 / 160 columns, and 32 on the 64-column layout)
RAGGED = ("pl_c200_d2", "pl_c320_fwd", "mb_384_96", "mb_576_160", "mb_960_320", "mb_576_160_r9", "mb_192_32", "mb_192_32_r5",
          "mb_960_320_w9")
# the pair-merge identity (+ DW_IDENTITY).  pl_3x3 (a padded border: |mean| / sigma 5) and the depthwise case (K = 9: 9) keep the
# terms of the identity below the bound, so there the check adds little beyond M2_t's; the three 1 x 1 routes (no border, K = 64:
# |mean| / sigma ~ 130) are where leaving the terms out fails it (tests/test_bn_partials_cpu.py)
IDENTITY = ("pl_3x3", "pl_1x1", "x6_1x1", "f32_u")
# the bias convention: conv_ref.SLICE_ROUTES and one route of every forward kernel family they lack
# (mb_192_32: k_conv_pl2<4, 2, 3, false> writing 32 of its 64 columns)
BIAS_ROUTES = list(R.SLICE_ROUTES) + ["stem_even", "f32_narrow", "pl_wide", "mb_192_32"]
ASPP_TILE_ROWS = 144


def fwd_kinds(rt):
    """dense, exact integers, and "offset": non-negative activations and weights (what a post-ReLU input does to a convolution:
    |mean| / sigma of a channel in the tens to hundreds).  The statistics do not depend on the K length, so the routes of
    conv_ref.NO_DENSE keep int and offset; the extra short-tile routes run offset and int"""
    if rt.id in R.NO_DENSE or rt.id in SHORT_LAST:
        return ["int", "offset"]
    return ["dense", "int", "offset"]


FWD_CASES = [(rt.id, kind) for rt in FWD_ROUTES for kind in fwd_kinds(rt)]
ASPP_KINDS = ["dense", "int", "offset"]
ASPP_CASES = [(cid, kind) for cid in R.ASPP for kind in ASPP_KINDS]


# activations of the offset kind: 1 + OFFSET_SPREAD |randn|.  With |randn| weights a channel of a K-term convolution then has
# |mean| / sigma ~ 14 sqrt(K) away from padded borders -- 115 at K = 64, 330 at K = 512 -- and the cross term of the pair merge
# (identity_terms) stands 3 x or more above the bound it is asserted within (tests/test_bn_partials_cpu.py)
OFFSET_SPREAD = 0.1


def _offset(o, rt):
    x = o["x"].abs() * OFFSET_SPREAD + 1.0
    if rt.id.startswith("stem"):
        x[..., 3] = 0
    o.update(x=x, w_f=o["w_f"].abs())
    if R.MATH[rt.mode] == 2:
        o["x_r"], o["w_f_r"] = o["x"].bfloat16().float(), o["w_f"].bfloat16().float()
    return o


def operands(rt, kind, xkey=None):
    if kind != "offset":
        return R.operands(rt, kind, xkey)
    return _offset(R.operands(rt, "dense", xkey), rt)


def aspp_operands(cid, kind):
    return [operands(rt, kind, xkey=cid) for rt in R.aspp_routes(cid)]


def stored_y_cpu(rt, o, bias=None):
    """the CPU stand-in of the stored output: fp32 rounding of the float64 convolution, [M, Cout] -- EVERY channel, also on the
    routes whose convolution tests sample a channel subset: the GPU file compares every channel"""
    y = R.conv_fwd(rt._replace(sub=0), R.rounded(rt, o)["x"], R.rounded(rt, o)["w_f"], torch.float64, bias)
    return y.float().reshape(-1, y.shape[-1])


# ---- tile statistics -------------------------------------------------------------------------------------------------------------
def _tiled(y, tile_rows):
    """[M, C] -> ([T, tile_rows, C] zero-padded, n_t [T, 1], valid [T, tile_rows, 1])"""
    m, c = y.shape
    t = (m + tile_rows - 1) // tile_rows
    buf = torch.zeros(t * tile_rows, c, dtype=y.dtype)
    buf[:m] = y
    n = torch.full((t, 1), float(tile_rows), dtype=y.dtype)
    n[-1, 0] = m - (t - 1) * tile_rows
    valid = (torch.arange(t * tile_rows) < m).view(t, tile_rows, 1)
    return buf.view(t, tile_rows, c), n, valid


def _seq_sum(v):
    """sum over dim 1, one row after another in v's own precision"""
    acc = torch.zeros_like(v[:, 0])
    for i in range(v.shape[1]):
        acc = acc + v[:, i]
    return acc


def tile_stats(y, tile_rows, dtype=torch.float64):
    """(S [T, C], M2 [T, C]) of the rows of y [M, C] (fp32 values).  float64: the restatement.  float32: the floor's -- rows
    added one after another in fp32, centred about fp32(S_t / n_t)"""
    v, n, valid = _tiled(y.to(dtype), tile_rows)
    if dtype == torch.float64:
        s = v.sum(1)
        dev = (v - (s / n)[:, None]) * valid
        return s, (dev * dev).sum(1)
    s = _seq_sum(v)
    dev = (v - (s / n)[:, None]) * valid
    return s, _seq_sum(dev * dev)


def tile_err(a, b):
    """the metric tile by tile: max over tiles of max_c|a - b| / max_c|b|; a tile whose reference is all zeros must be all zeros"""
    a, b = a.double(), b.double()
    num, den = (a - b).abs().amax(1), b.abs().amax(1)
    err = torch.where(den > 0, num / den.clamp_min(1e-300), torch.where(num > 0, torch.full_like(num, float("inf")), num))
    return float(err.max())


def merge(s, m2, n):
    """exact pair merge (Chan) in float64 of partials S, M2 [T, C] with row counts n [T]: (mean [C], biased variance [C]) --
    what iswm_bn_finalize computes: S_t taken as the tile's exact sum"""
    s, m2, n = s.double(), m2.double(), n.double().view(-1, 1)
    tot = n.sum()
    mean = s.sum(0) / tot
    d = s / n - mean
    return mean, (m2 + n * d * d).sum(0) / tot


def counts(m, tile_rows):
    t = (m + tile_rows - 1) // tile_rows
    return torch.tensor([min(tile_rows, m - i * tile_rows) for i in range(t)], dtype=torch.float64)


def batch_stats(y):
    y = y.double()
    return y.mean(0), y.var(0, unbiased=False)


def identity_terms(y, s_pub, tile_rows):
    """the pair-merge identity: with mu_t = fp32(S_t / n_t) from the PUBLISHED S_t and R_t = sum (y - mu_t) over the tile (float64),
         var_true = (1/N) sum [M2_t(about mu_t) + 2 (mu_t - mean) R_t + n_t (mu_t - mean)^2]          (iswm_bn_finalize_res)
         var_pair = (1/N) sum [M2_t + n_t (S_t / n_t - mean_pair)^2]                                  (iswm_bn_finalize)
    so var_true - var_pair = cross + shift + (error of the published M2_t), cross = (2/N) sum (mu_t - mean) R_t and
    shift = (1/N) sum n_t [(mu_t - mean)^2 - (S_t / n_t - mean_pair)^2].  Returns (cross + shift [C], M2_t about mu_t [T, C])"""
    v, n, valid = _tiled(y.double(), tile_rows)
    mu = (s_pub.float() / n.float()).double()
    dev = (v - mu[:, None]) * valid
    r, m2_mu = dev.sum(1), (dev * dev).sum(1)
    tot = float(y.shape[0])
    mean = (n * mu + r).sum(0) / tot
    mean_pair = s_pub.double().sum(0) / tot
    cross = 2.0 * ((mu - mean) * r).sum(0) / tot
    shift = (n * ((mu - mean) ** 2 - (s_pub.double() / n - mean_pair) ** 2)).sum(0) / tot
    return cross + shift, m2_mu


# ---- depthwise 3 x 3 ---------------------------------------------------------------------------------------------------------------
# (N, H, W, C, Cw, stride, dil, sliced): the first eight cases of tests/dw3_ref.CASES, a last tile of tile_rows - 1 = 63 rows, the
# two fallback-layout cases (idle quad lanes) and the two shapes of dw3_ref.BIG_FWD, whose statistic tiles are the 8-pixel
# ones production uses: 128 rows at 144 channels, 256 rows at 32 (4169 tiles: more than 2048, from a real producer)
def dw_cases():
    from tests import dw3_ref as D
    return list(D.CASES[:8]) + [(1, 1, 127, 96, 96, 1, 1, False)] + [D.CASES[i] for i in D.FALLBACK] + list(D.BIG_FWD)


DW_SINGLE_ROW, DW_SHORT, DW_IDENTITY = 3, 8, 1               # indices into dw_cases()
DW_FALLBACK, DW_BIG = (9, 10), (11, 12)
DW_KINDS = ["dense", "int", "offset"]
# a ~100 MB shape runs once: the offset kind (the only one that sees a tile centred about a wrong count, NEEDS_MEAN)
DW_CASE_KINDS = [(i, k) for i in range(13) for k in (["offset"] if i in DW_BIG else DW_KINDS)]


def dw_inputs(i, kind):
    n, h, w, c, cw, s, d, _ = dw_cases()[i]
    g = R.gen("dw3", i, kind)
    if kind == "int":
        x = torch.randint(-4, 5, (n, h, w, c), generator=g).float()
        wt = torch.randint(-3, 4, (cw, 1, 3, 3), generator=g).float()
    else:
        x, wt = torch.randn(n, h, w, c, generator=g), torch.randn(cw, 1, 3, 3, generator=g) * 0.5
        if kind == "offset":
            x, wt = x.abs() * OFFSET_SPREAD + 1.0, wt.abs()
    return x, wt


def dw_stored_y_cpu(i, x, wt):
    import torch.nn.functional as F
    n, h, w, c, cw, s, d, _ = dw_cases()[i]
    y = F.conv2d(x[..., :cw].permute(0, 3, 1, 2).double(), wt.double(), None, s, d, d, cw).permute(0, 2, 3, 1)
    return F.pad(y, (0, c - cw)).float().reshape(-1, c)


# ---- finalize on synthetic partials --------------------------------------------------------------------------------------------------
FIN_C = [1, 5, 16, 67]                              # every CPB variant (16, 4, 1 channels per block) has a ragged last block
FIN_TILES = [1, 2, 32, 33, 512, 513, 2048, 2049, 2081]   # dispatch switches after 32 and 512; <1>'s tail loop starts at 2049
FIN_ROWS = 7                                        # rows of a full tile; the last tile holds 3 (5 when there is one tile)
FIN_CASES = [(c, t, lay) for c in FIN_C for t in FIN_TILES for lay in ("rows",)] + \
            [(5, t, "counts") for t in (20, 100, 600)]       # tile_rows = 0 with unequal counts, once per variant


def fin_partials(c, tiles, layout, planes=2, zero_m2_channel=None, count_one=False):
    """synthetic partials as a producer would publish them: random float64 tiles, their sums rounded to fp32.  Returns
    (flat fp32 buffer, counts [T] float64, tile_rows)"""
    g = R.gen("fin", c, tiles, layout, planes)
    if count_one:
        n = torch.ones(1, dtype=torch.float64)
    elif layout == "counts":
        n = torch.randint(1, 129, (tiles,), generator=g).double()
    else:
        n = torch.full((tiles,), float(FIN_ROWS), dtype=torch.float64)
        n[-1] = 3.0 if tiles > 1 else 5.0
    off = torch.randn(c, generator=g, dtype=torch.float64) * 3
    mu = off + torch.randn(tiles, c, generator=g, dtype=torch.float64) * 0.3
    s = (mu * n.view(-1, 1)).float()
    m2 = (torch.rand(tiles, c, generator=g, dtype=torch.float64) * (n.view(-1, 1) - 1)).float()
    if zero_m2_channel is not None:                 # a constant channel: every tile mean equal (a power of two: S_t exact), M2 zero
        s[:, zero_m2_channel] = (0.5 * n).float()
        m2[:, zero_m2_channel] = 0
    parts = [s.reshape(-1), m2.reshape(-1)]
    if planes == 3:
        parts.append((torch.randn(tiles, c, generator=g, dtype=torch.float64) * 1e-3).float().reshape(-1))
    if layout == "counts":
        parts.append(n.float())
    return torch.cat(parts), n, (0 if layout == "counts" else FIN_ROWS)


def fin_expected(flat, n, c, planes, gamma, beta, rmean, rvar, momentum, eps=EPS):
    """float64 merge of those very partials.  planes == 3: the identity of iswm_bn_finalize_res (centres fp32(S_t / n_t))"""
    tiles = n.numel()
    p = flat[:planes * tiles * c].view(planes, tiles, c)
    tot = n.sum()
    nn = n.view(-1, 1)
    if planes == 2:
        mean, var = merge(p[0], p[1], n)
    else:
        mu = (p[0] / nn.float()).double()
        r = p[2].double()
        mean = (nn * mu + r).sum(0) / tot
        d = mu - mean
        var = (p[1].double() + 2 * d * r + nn * d * d).sum(0) / tot
    var = var.clamp_min(0)
    eps64 = float(torch.tensor(eps, dtype=torch.float32))
    momentum = float(torch.tensor(momentum, dtype=torch.float32))      # the entry point takes eps and momentum as floats
    invstd = 1.0 / torch.sqrt(var + eps64)
    g = torch.ones(c, dtype=torch.float64) if gamma is None else gamma.double()
    out = dict(mean=mean, var=var, invstd=invstd, scale=g * invstd,
               shift=torch.zeros(c) if beta is None else beta.clone())
    if rmean is not None:
        unb = var * tot / (tot - 1) if float(tot) > 1 else var
        out["rmean"] = (1 - momentum) * rmean.double() + momentum * mean
        out["rvar"] = (1 - momentum) * rvar.double() + momentum * unb
        out["unbiased"] = unb
    return out


def fin_key(k, mom, c):
    """the FLOOR key of a finalize output.  The running mean at momentum 0.1 of a ONE-channel case is judged on its own: with a
    single channel the metric is that number's own relative error, and 0.9 rm + 0.1 mean may cancel (it does at C = 1 here)"""
    if k[0] != "r":
        return "fin." + k
    return "fin.%s.m%g%s" % (k, mom, ".c1" if (k == "rmean" and mom != 1.0 and c == 1) else "")


def fin_fp32(exp, gamma, rmean, rvar, momentum):
    """the floor's restatement: the float64 results rounded to fp32, scale and the running buffers formed in fp32 from them"""
    f = dict(var=exp["var"].float(), invstd=exp["invstd"].float())
    f["scale"] = (torch.ones_like(f["invstd"]) if gamma is None else gamma) * f["invstd"]
    if rmean is not None:
        m = torch.tensor(momentum, dtype=torch.float32)
        f["rmean"] = (1 - m) * rmean + m * exp["mean"].float()
        f["rvar"] = (1 - m) * rvar + m * exp["unbiased"].float()
    return f


# ---- backward: the sums iswm_conv2d_dgrad_pl2_bn takes and their consumer -----------------------------------------------------------
BWD_ROUTES = ["pl_3x3", "pl_1x1", "pl_s2", "pl_narrow", "pl_s2_1x1"]
BWD_CASES = [(rid, code, acc) for rid in BWD_ROUTES for code in (0, 2, 3) for acc in (False, True)]
RUN = 10


def bwd_inputs(rid):
    """the producer stage of the conv's input: raw output y, saved activation (zeros, negative zeros, 2^-100 -- its hi plane is
    positive -- and the fp32 denormal 2^-140, which is positive while its hi plane is ZERO), mean, invstd, gamma, beta,
    scale = fp32(gamma * invstd), shift = beta"""
    n, h, w, cin = R.ROUTE[rid].geom[:4]
    g = R.gen(rid, "bnp")
    saved = torch.randn(n, h, w, cin, generator=g)
    flat = saved.view(-1)
    flat[0::7] = 0.0
    flat[3::11] = -0.0
    flat[5::13] = 2.0 ** -100
    flat[2::17] = 2.0 ** -140
    y = torch.randn(n, h, w, cin, generator=g) * 0.7 + 0.3
    mean, invstd = torch.randn(cin, generator=g) * 0.2 + 0.3, torch.rand(cin, generator=g) + 0.9
    gamma, beta = torch.randn(cin, generator=g) * 0.3 + 1, torch.randn(cin, generator=g) * 0.3
    return dict(saved=saved, y=y, mean=mean, invstd=invstd, gamma=gamma, beta=beta, scale=gamma * invstd, shift=beta)


def hi_plane(x):
    return R.split3(x)[0]


def pattern(code, b, variant=None):
    """the pass pattern of a relu code, evaluated in fp32 exactly as the kernels write it.  variant: a mutant"""
    if code == 0:
        return torch.ones_like(b["y"], dtype=torch.bool)
    if code == 2:
        if variant == "y>0":
            return b["y"] > 0
        return (b["y"] - b["mean"]) * b["scale"] + b["shift"] > 0
    if variant == "full":
        return b["saved"] > 0
    return hi_plane(b["saved"]) > 0


def bwd_sums(dx, pat, b, dtype=torch.float64):
    """(sum dz [C], sum dz * xhat [C]) over all rows of the stored dx.  float32: the floor's restatement -- the products in
    fp32, runs of <= RUN rows added in fp32, the runs in double"""
    c = dx.shape[-1]
    dz = (dx * pat).reshape(-1, c)
    y = b["y"].reshape(-1, c)
    if dtype == torch.float64:
        dz = dz.double()
        xhat = (y.double() - b["mean"].double()) * b["invstd"].double()
        return dz.sum(0), (dz * xhat).sum(0)
    t = dz * ((y - b["mean"]) * b["invstd"])
    out = []
    for v in (dz, t):
        runs, _, _ = _tiled(v, RUN)
        out.append(_seq_sum(runs).double().sum(0))
    return tuple(out)


def nchw(t):
    return t.permute(0, 3, 1, 2)


def bn_backward_ref(dz, b, training):
    """float64 (dy NHWC, dgamma, dbeta) through tests/streaming_ref.bn_bwd_ref; dz = the activation's gradient, pattern applied"""
    inv = b["invstd"].double()
    fwd = dict(xhat=nchw((b["y"].double() - b["mean"].double()) * inv), var=1.0 / (inv * inv) - SR.BN_EPS)
    dy, dgamma, dbeta, _ = SR.bn_bwd_ref(fwd, b["gamma"], nchw(dz), torch.ones_like(nchw(dz), dtype=torch.bool), training)
    return dy.permute(0, 2, 3, 1), dgamma, dbeta


def bn_backward_fp32(dz, b, training, sums):
    """the floor's dy: per-element fp32 expression on fp32-rounded sums"""
    k = b["gamma"] * b["invstd"]
    if not training:
        return k * dz
    m = dz.numel() // dz.shape[-1]
    xhat = (b["y"] - b["mean"]) * b["invstd"]
    return k * (dz - (sums[0] / m).float() - xhat * (sums[1] / m).float())


def parity_rows(rt):
    """rows of dx [N*H*W] in the strided data gradient's parity-major order (class (h % s, w % s), raster inside), and the mask
    of rows some filter tap reaches"""
    n, h, w, cin, cout, k, s, pad, dil = rt.geom
    ho, wo = R.out_size(h, k, s, pad, dil), R.out_size(w, k, s, pad, dil)
    reach = torch.zeros(h, w, dtype=torch.bool)
    for a in range(k):
        for oh in range(ho):
            ih = oh * s - pad + a * dil
            if 0 <= ih < h:
                for bb in range(k):
                    iw = torch.arange(wo) * s - pad + bb * dil
                    reach[ih, iw[(iw >= 0) & (iw < w)]] = True
    return reach.unsqueeze(0).expand(n, h, w)


def untouched_tiles(rt, tile_rows):
    """tiles of the parity-major row order that hold no reached row"""
    n, h, w = rt.geom[:3]
    s = rt.geom[6]
    reach = parity_rows(rt)
    hh, ww = torch.arange(h).view(1, h, 1).expand(n, h, w), torch.arange(w).view(1, 1, w).expand(n, h, w)
    cls = ((hh % s) * s + (ww % s)).reshape(-1)
    order = torch.sort(cls, stable=True)[1]
    r = reach.reshape(-1)[order]
    t = (r.numel() + tile_rows - 1) // tile_rows
    return [i for i in range(t) if not r[i * tile_rows:(i + 1) * tile_rows].any()]


# ---- host queries ----------------------------------------------------------------------------------------------------------------------
def fwd_layout(rt):
    """(entry point, kernel name, M, tiles, tile_rows) of a route's forward statistics, from the library's host queries"""
    from iswm_amd import _lib
    e, name = R.planned(rt)["fwd"]
    with R.conv_math(rt) as lib:
        d = R.desc(rt)
        ref = ctypes.byref(d)
        m = d.N * d.Ho * d.Wo
        if e == "iswm_conv2d_fwd_pl2":
            tr = lib.iswm_conv2d_pl2_tile_rows(ref, 0)
            t = (m + tr - 1) // tr
        elif e == "iswm_conv2d_fwd_packed":
            nt, trr = ctypes.c_int(0), ctypes.c_int(0)
            assert lib.iswm_conv2d_fwd_packed_stat_layout(ref, ctypes.byref(nt), ctypes.byref(trr)) == 0
            t, tr = nt.value, trr.value
        else:
            t, tr = lib.iswm_conv2d_stat_tiles(ref), lib.iswm_conv2d_stat_tile_rows(ref)
    del _lib
    return e, name, m, t, tr


def dw_layout(i):
    from iswm_amd import _lib
    n, h, w, c, cw, s, d, _ = dw_cases()[i]
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    dd = _lib.ConvDesc(n, h, w, c, ho, wo, c, 3, 3, s, d, d, c, c)
    lib = _lib.load()
    return n * ho * wo, lib.iswm_dwconv3x3_stat_tiles(ctypes.byref(dd)), lib.iswm_dwconv3x3_stat_tile_rows(ctypes.byref(dd))


def dgrad_layout(rt):
    with R.conv_math(rt) as lib:
        d = R.desc(rt)
        return d.N * d.H * d.W, lib.iswm_conv2d_dgrad_pl2_stat_tiles(ctypes.byref(d)), lib.iswm_conv2d_pl2_tile_rows(ctypes.byref(d), 1)


# ---- mutants of the float64 restatement (tests/test_bn_partials_cpu.py: each must miss an assertion by >= 3 x its bound) -------------
def fwd_mutants(y, tile_rows, bias=None):
    """{name: (S, M2)} of plausible wrong epilogues on the stored y [M, C]; a mutant that is a no-op on this shape is left out"""
    m, c = y.shape
    t = (m + tile_rows - 1) // tile_rows
    last = m - (t - 1) * tile_rows
    s, m2 = tile_stats(y, tile_rows)
    out = collections.OrderedDict()
    v, n, valid = _tiled(y.double(), tile_rows)
    if last < tile_rows:                          # the last tile centred as if it were full
        dev = (v - (s / float(tile_rows))[:, None]) * valid
        out["last count = tile_rows"] = (s, (dev * dev).sum(1))
    if m > 1:                                     # the last valid row masked out
        out["last row dropped"] = tile_stats(y[:-1], tile_rows) if last > 1 else (s[:-1], m2[:-1])
        if last == 1:                             # (the tile disappears: judged as a zero tile)
            z = torch.zeros(1, c, dtype=torch.float64)
            out["last row dropped"] = (torch.cat([s[:-1], z]), torch.cat([m2[:-1], z]))
    if last < tile_rows:                          # one row past M taken in (what lies there: a copy of row 0), count unchanged
        s2 = s.clone()
        s2[-1] += y[0].double()
        dev = torch.cat([v[-1][:last], y[:1].double()]) - (s2[-1] / last)
        m2b = m2.clone()
        m2b[-1] = (dev * dev).sum(0)
        out["row past M included"] = (s2, m2b)
    if t > 1:
        mean = y.double().mean(0)
        out["M2 about the batch mean"] = (s, m2 + n * (s / n - mean) ** 2)
        idx = list(range(t))
        idx[0], idx[1] = 1, 0
        out["tiles 0 and 1 swapped"] = (s[idx], m2[idx])
    if bias is not None:
        out["bias in S_t"] = (s + n * bias.double(), m2)
    out["planes swapped"] = (m2, s)
    if c > 1:
        out["neighbouring channel"] = (s.roll(1, 1), m2.roll(1, 1))
    return out


# a last tile one row short that is centred as if it were full moves M2_t by n_t (mu_t / tile_rows)^2: with zero-mean operands
# (dense, int) that is below the bound, so on the tile_rows - 1 shapes this mutant is required of the offset kind only -- every
# such shape has one; the checks of the other kinds stay
NEEDS_MEAN = ("last count = tile_rows",)


def exempt(mutant, kind, short):
    return short and mutant in NEEDS_MEAN and kind != "offset"


def bound(key):
    return 4.0 * FLOOR[key]


# ---- recorded floors (profiles/bn_partials_tests.txt carries the same figures; tests/test_bn_partials_cpu.py ties the two) -------------
FLOOR = {
    "aspp_large.mean": 5.1e-07,
    "aspp_large.var": 4.4e-06,
    "aspp_small.mean": 5.0e-07,
    "aspp_small.var": 4.7e-07,
    "bf16_1x1.M2": 1.0e-06,
    "bf16_1x1.S": 3.4e-07,
    "bf16_patch.mean": 4.3e-07,
    "bf16_patch.var": 6.9e-07,
    "bf16_pl.M2": 1.2e-06,
    "bf16_pl.S": 4.3e-07,
    "bwd.pl_1x1.dy": 1.1e-07,
    "bwd.pl_1x1.dy_eval": 6.0e-08,
    "bwd.pl_1x1.sum_dz": 8.8e-08,
    "bwd.pl_1x1.sum_dzx": 8.8e-08,
    "bwd.pl_3x3.dy": 1.4e-07,
    "bwd.pl_3x3.dy_eval": 7.1e-08,
    "bwd.pl_3x3.sum_dz": 7.3e-08,
    "bwd.pl_3x3.sum_dzx": 1.5e-07,
    "bwd.pl_narrow.dy": 1.2e-07,
    "bwd.pl_narrow.dy_eval": 8.7e-08,
    "bwd.pl_narrow.sum_dz": 6.8e-08,
    "bwd.pl_narrow.sum_dzx": 7.0e-08,
    "bwd.pl_s2.dy": 1.1e-07,
    "bwd.pl_s2.dy_eval": 8.6e-08,
    "bwd.pl_s2.sum_dz": 8.7e-08,
    "bwd.pl_s2.sum_dzx": 1.1e-07,
    "bwd.pl_s2_1x1.dy": 1.3e-07,
    "bwd.pl_s2_1x1.dy_eval": 5.3e-08,
    "bwd.pl_s2_1x1.sum_dz": 9.8e-08,
    "bwd.pl_s2_1x1.sum_dzx": 9.1e-08,
    "dw3_0.M2": 1.8e-06,
    "dw3_0.S": 4.3e-07,
    "dw3_1.M2": 1.2e-06,
    "dw3_1.S": 3.9e-07,
    "dw3_1.identity": 9.6e-08,
    "dw3_2.M2": 1.0e-06,
    "dw3_2.S": 2.1e-07,
    "dw3_3.M2": 1.0e-07,
    "dw3_3.S": 7.9e-08,
    "dw3_4.M2": 1.2e-06,
    "dw3_4.S": 2.6e-07,
    "dw3_5.M2": 1.4e-06,
    "dw3_5.S": 3.8e-07,
    "dw3_6.M2": 1.9e-06,
    "dw3_6.S": 3.1e-07,
    "dw3_7.M2": 6.0e-07,
    "dw3_7.S": 2.4e-07,
    "dw3_8.M2": 1.1e-06,
    "dw3_8.S": 2.4e-07,
    "dw3_9.M2": 5.5e-07,
    "dw3_9.S": 3.1e-07,
    "dw3_10.M2": 8.6e-07,
    "dw3_10.S": 2.6e-07,
    "dw3_11.M2": 7.6e-07,
    "dw3_11.S": 6.2e-07,
    "dw3_12.M2": 1.2e-06,
    "dw3_12.S": 9.1e-07,
    "f32_narrow.M2": 1.3e-06,
    "f32_narrow.S": 3.0e-07,
    "f32_short.M2": 1.4e-06,
    "f32_short.S": 4.6e-07,
    "f32_u.M2": 1.2e-06,
    "f32_u.S": 3.5e-07,
    "f32_u.identity": 1.1e-07,
    "f32_u_m128.M2": 2.2e-06,
    "f32_u_m128.S": 6.6e-07,
    "f32_u_s2.M2": 2.3e-07,
    "f32_u_s2.S": 3.0e-07,
    "f32_u_short.M2": 7.8e-07,
    "f32_u_short.S": 2.5e-07,
    "f32_wide_fwd.M2": 2.3e-06,
    "f32_wide_fwd.S": 7.0e-07,
    "fin.invstd": 4.9e-08,
    "fin.rmean.m0.1": 1.2e-07,
    "fin.rmean.m0.1.c1": 5.9e-06,
    "fin.rmean.m1": 5.1e-08,
    "fin.rvar.m0.1": 1.3e-07,
    "fin.rvar.m1": 5.6e-08,
    "fin.scale": 8.0e-08,
    "fin.var": 5.7e-08,
    "mb_144_24.M2": 1.5e-06,
    "mb_144_24.S": 6.6e-07,
    "mb_144_32.M2": 1.4e-06,
    "mb_144_32.S": 3.3e-07,
    "mb_160_960.M2": 1.2e-06,
    "mb_160_960.S": 3.5e-07,
    "mb_16_96.M2": 1.7e-06,
    "mb_16_96.S": 3.2e-07,
    "mb_16_96_m128.M2": 2.2e-06,
    "mb_16_96_m128.S": 6.8e-07,
    "mb_192_32.M2": 1.4e-06,
    "mb_192_32.S": 5.0e-07,
    "mb_192_32_r5.M2": 2.6e-06,
    "mb_192_32_r5.S": 7.7e-07,
    "mb_24_144.M2": 1.9e-06,
    "mb_24_144.S": 3.8e-07,
    "mb_32_16.M2": 9.8e-07,
    "mb_32_16.S": 4.9e-07,
    "mb_32_192.M2": 8.2e-07,
    "mb_32_192.S": 3.5e-07,
    "mb_32_192_m128.M2": 2.0e-06,
    "mb_32_192_m128.S": 6.1e-07,
    "mb_384_96.M2": 1.4e-06,
    "mb_384_96.S": 3.9e-07,
    "mb_576_160.M2": 1.8e-06,
    "mb_576_160.S": 4.7e-07,
    "mb_576_160_r9.M2": 2.2e-06,
    "mb_576_160_r9.S": 6.6e-07,
    "mb_960_320.M2": 1.3e-06,
    "mb_960_320.S": 6.0e-07,
    "mb_96_576.M2": 9.1e-07,
    "mb_96_576.S": 3.4e-07,
    "mb_stem.M2": 1.7e-06,
    "mb_stem.S": 3.8e-07,
    "mb_960_320_w9.M2": 1.9e-06,
    "mb_960_320_w9.S": 8.0e-07,
    "pl_1x1.M2": 1.5e-06,
    "pl_1x1.S": 4.6e-07,
    "pl_1x1.identity": 2.7e-07,
    "pl_3x3.M2": 1.3e-06,
    "pl_3x3.S": 4.8e-07,
    "pl_3x3.identity": 3.6e-07,
    "pl_5x5.M2": 3.8e-07,
    "pl_5x5.S": 4.5e-07,
    "pl_c200_d2.M2": 1.4e-06,
    "pl_c200_d2.S": 5.6e-07,
    "pl_c320_fwd.M2": 1.8e-06,
    "pl_c320_fwd.S": 4.6e-07,
    "pl_c4.M2": 1.0e-06,
    "pl_c4.S": 3.3e-07,
    "pl_c48.M2": 1.3e-06,
    "pl_c48.S": 5.2e-07,
    "pl_d18.M2": 3.0e-07,
    "pl_d18.S": 3.6e-07,
    "pl_map1.M2": 5.3e-08,
    "pl_map1.S": 6.1e-08,
    "pl_narrow.M2": 1.3e-06,
    "pl_narrow.S": 4.6e-07,
    "pl_narrow3.M2": 1.0e-06,
    "pl_narrow3.S": 4.4e-07,
    "pl_narrow_short.M2": 1.1e-06,
    "pl_narrow_short.S": 3.0e-07,
    "pl_pad0.M2": 4.1e-07,
    "pl_pad0.S": 3.4e-07,
    "pl_r10_fwd.M2": 2.5e-06,
    "pl_r10_fwd.S": 6.6e-07,
    "pl_r10_short.M2": 2.4e-06,
    "pl_r10_short.S": 6.2e-07,
    "pl_r5_narrow.M2": 2.5e-06,
    "pl_r5_narrow.S": 7.7e-07,
    "pl_r9_fwd.M2": 2.4e-06,
    "pl_r9_fwd.S": 6.6e-07,
    "pl_r9_short.M2": 2.3e-06,
    "pl_r9_short.S": 5.7e-07,
    "pl_rect.M2": 3.2e-07,
    "pl_rect.S": 3.1e-07,
    "pl_s2_1x1.M2": 3.9e-07,
    "pl_s2_1x1.S": 3.5e-07,
    "pl_s2_fwd.M2": 5.8e-07,
    "pl_s2_fwd.S": 4.1e-07,
    "pl_short.M2": 1.7e-06,
    "pl_short.S": 5.3e-07,
    "pl_wide.M2": 2.2e-06,
    "pl_wide.S": 6.5e-07,
    "pl_wide3.M2": 2.2e-06,
    "pl_wide3.S": 5.9e-07,
    "pl_wide_short.M2": 2.1e-06,
    "pl_wide_short.S": 5.9e-07,
    "stem_even.M2": 1.0e-06,
    "stem_even.S": 4.2e-07,
    "stem_odd.M2": 1.3e-06,
    "stem_odd.S": 3.4e-07,
    "stem_short.M2": 1.3e-06,
    "stem_short.S": 4.0e-07,
    "x6_1x1.M2": 1.0e-06,
    "x6_1x1.S": 3.4e-07,
    "x6_1x1.identity": 9.8e-08,
    "x6_m128.M2": 2.0e-06,
    "x6_m128.S": 6.3e-07,
    "bf16_m128.M2": 2.0e-06,
    "bf16_m128.S": 6.0e-07,
    "f32_u_fwd128.M2": 1.9e-06,
    "f32_u_fwd128.S": 9.0e-07,
    "x6w_1x1.M2": 1.0e-06,
    "x6w_1x1.S": 4.0e-07,
    "x6w_m128.M2": 1.9e-06,
    "x6w_m128.S": 5.9e-07,
    "x6w_wide.M2": 1.9e-06,
    "x6w_wide.S": 7.6e-07,
    "x6_patch.mean": 4.0e-07,
    "x6_patch.var": 7.0e-07,
    "x6_patch_d2.mean": 2.1e-07,
    "x6_patch_d2.var": 5.7e-07,
    "x6_s2.M2": 3.0e-07,
    "x6_s2.S": 2.9e-07,
    "x6_short.M2": 8.2e-07,
    "x6_short.S": 3.7e-07,
}
