"""Cases, seeded inputs, float64 restatement and tap-level model of the pre-activation depthwise 3 x 3 kernels (csrc/dwconv3.hip,
iswm_dwconv3x3_pre_*; include/iswm_hip_sep.h), shared by tests/test_dwconv3_pre_gpu.py (the kernels) and
tests/test_dw3_pre_ref_cpu.py (no GPU: ties every case to the layout / chunking it reaches and shows which faults the GPU
assertions catch).

Rule (the one of tests/dw3_ref.py): rel_err = max|a - b| / max|b| against float64 must be <= 4 x FLOOR, FLOOR = torch's own
fp32 grouped convolution (and its autograd) on the same inputs, CPU, one thread -- computed per case by `floors`, in the test
that uses it (nothing recorded).  The equalities (y against iswm_dwconv2d_fwd, dx against mask x iswm_dwconv2d_dgrad, planes,
zeros) carry no bound.

The restatement is F.conv2d(relu?(x), groups) in float64 with torch's ReLU gradient (0 at x <= 0); `y_by_taps` / `dx_by_taps` /
`dw_by_chunks` restate the kernels' own index arithmetic (taps at -pad + k dil, the mask, the chunking of both pixel grids), so
that a fault of that arithmetic can be emulated on the CPU."""
import ctypes

import torch
import torch.nn.functional as F

# (N, H, W, C, pitch of y, Cw, stride, dil, pad, relu_in)
CASES = [
    (2, 13, 11, 64, 64, 64, 1, 1, 1, True),
    (2, 13, 11, 128, 128, 128, 1, 2, 1, True),         # pad < dil: 11 x 9 out
    (2, 13, 11, 728, 768, 728, 1, 2, 2, True),         # the middle flow: 728 channels written into the 768-wide operand buffer
    (2, 13, 11, 728, 736, 728, 1, 2, 1, False),        # ... and into a 736-wide one (23 channel blocks of 8 quads)
    (1, 13, 11, 1536, 1536, 1536, 1, 4, 1, False),     # conv4 at output stride 8: 7 x 5 out
    (2, 13, 11, 20, 20, 20, 1, 1, 1, True),            # fallback layout: 5 quads, 11 idle quad lanes
    (2, 13, 11, 64, 64, 64, 1, 4, 4, False),
    (2, 13, 11, 64, 64, 62, 1, 2, 1, True),            # channels 62, 63 see zero weights
    (2, 13, 11, 128, 128, 128, 2, 1, 1, True),         # stride 2 is kept
    (2, 13, 11, 64, 64, 64, 2, 2, 1, True),            # ... with pad < dil: 6 x 5 out
    (2, 17, 15, 128, 128, 128, 1, 2, 1, True),         # 390 output and 510 input pixels: two chunks of 195 / 255
    # -- small geometry
    (1, 1, 1, 64, 64, 64, 1, 1, 1, True),              # one pixel
    (2, 9, 1, 128, 128, 128, 1, 2, 2, True),           # one column
    (1, 3, 4, 64, 64, 64, 1, 4, 4, True),              # H, W <= dil: only the centre tap is ever in bounds
    (1, 2, 2, 20, 20, 20, 1, 2, 2, False),             # ... in the fallback layout
    (1, 7, 9, 128, 128, 128, 1, 4, 1, True),           # the smallest map with an output at dil 4, pad 1: 1 x 3
]
# the backward under the 2048-chunk cap (the shape of dw3_ref.BIG_BWD): out_chunk = in_chunk = 257.  Backward only.
BIG_BWD = [(1, 725, 725, 32, 32, 32, 1, 1, 1, True)]
DIL_PAD_OS16, DIL_PAD_OS8 = {(1, 1), (2, 2), (2, 1)}, {(1, 1), (2, 2), (4, 4), (4, 1)}     # what the Xception models use


def case_id(c):
    return "n%d_%dx%d_c%d_ld%d_cw%d_s%d_d%d_p%d_%s" % (c[:9] + ("relu" if c[9] else "lin",))


def out_hw(case):
    n, h, w, c, ld, cw, s, d, p, _ = case
    return (h + 2 * p - 2 * d - 1) // s + 1, (w + 2 * p - 2 * d - 1) // s + 1


def layout(cols):
    """dw3_ref.layout: (CQ, RL, channel blocks, fallback) -- the forward lays its quads over the PITCH of y (so that 728
    channels in a 768-wide buffer are 192 quads = 12 blocks of 16), the backward over C"""
    from tests.dw3_ref import layout as lay
    return lay(cols)


def bwd_layout(c):
    """the backward's layout: over C, or over the next multiple of 32 channels when C has no layout free of idle lanes and is
    more than one block wide (728 -> 736: CQ 8, RL 32) -- then its pixel lanes differ from iswm_dwconv3x3_bwd's"""
    cq, rl, blocks, fallback = layout(c)
    return layout((c + 31) // 32 * 32) if fallback and c // 4 >= 16 else (cq, rl, blocks, fallback)


def queries(case):
    """backward chunks (from the workspace query) and the pixels per chunk on the output / input grid"""
    from iswm_amd import _lib
    n, h, w, c, ld, cw, s, d, p, _ = case
    ho, wo = out_hw(case)
    dd = _lib.ConvDesc(n, h, w, c, ho, wo, c, 3, 3, s, p, d, c, c)
    ws = _lib.load().iswm_dwconv3x3_pre_bwd_workspace(ctypes.byref(dd))
    assert ws % (9 * c * 4) == 0
    chunks, pout, pin = ws // (9 * c * 4), n * ho * wo, n * h * w
    return dict(pout=pout, pin=pin, chunks=chunks, out_chunk=(pout + chunks - 1) // chunks, in_chunk=(pin + chunks - 1) // chunks)


def inputs(case):
    """seeded inputs: x (about half of it negative; exact 0.0 and -0.0 planted), w [Cw,1,3,3], dy, dx0"""
    n, h, w, c, ld, cw, s, d, p, _ = case
    g = torch.Generator().manual_seed(sum(v * k for v, k in zip(case[:9], (3, 5, 7, 11, 13, 17, 19, 23, 29))) % 1000)
    x = torch.randn(n, h, w, c, generator=g) + 0.1
    flat = x.view(-1)
    flat[::7] = 0.0
    flat[3::11] = -0.0
    wt = torch.randn(cw, 1, 3, 3, generator=g) * 0.5 + 0.1
    ho, wo = out_hw(case)
    dy = torch.randn(n, ho, wo, c, generator=g) + 0.2
    dx0 = torch.randn(n, h, w, c, generator=g)
    return dict(x=x, w=wt, dy=dy, dx0=dx0, ho=ho, wo=wo)


def subset_channels(c, cw):
    from tests.dw3_ref import subset_channels as sub
    return sub(c, cw)


def restate(case, r, ch=None, dtype=torch.float64, parts=("y", "dx", "dw")):
    """{y [N,Ho,Wo,len(ch)], dx, dx_acc, dw [len(ch),1,3,3]} of the channels ch (all: every channel, those past Cw zero)"""
    n, h, w, c, ld, cw, s, d, p, relu = case
    full = ch is None
    ch = list(range(cw)) if full else ch
    need_grad = "dx" in parts or "dw" in parts
    xr = r["x"][..., ch].permute(0, 3, 1, 2).to(dtype).requires_grad_(need_grad)
    wr = r["w"][ch].to(dtype).requires_grad_(need_grad)
    y = F.conv2d(F.relu(xr) if relu else xr, wr, None, s, p, d, len(ch))
    pad = lambda t: F.pad(t.detach().permute(0, 2, 3, 1), (0, c - cw)) if full else t.detach().permute(0, 2, 3, 1)
    out = dict(y=pad(y))
    if need_grad:
        y.backward(r["dy"][..., ch].permute(0, 3, 1, 2).to(dtype))
        base = r["dx0"] if full else r["dx0"][..., ch]
        out.update(dx=pad(xr.grad), dw=wr.grad.detach())
        out["dx_acc"] = out["dx"] + base.to(dtype)
    return out


def floors(case, r, ref, ch=None, parts=("y", "dx", "dw")):
    """{y, dx, dx_acc, dw: rel_err of torch's fp32 operator against the float64 restatement `ref`}, one thread"""
    from tests.conv_ref import one_thread
    from tests.util import rel_err
    with one_thread():
        f32 = restate(case, r, ch, torch.float32, parts)
    return {q: rel_err(f32[q], ref[q]) for q in f32}


# ---- the kernels' index arithmetic, restated (float64; channels < Cw) ---------------------------------------------------------
def _x_op(case, r, relu_of=None):
    x = r["x"][..., :case[5]].double()
    relu = case[9] if relu_of is None else relu_of
    return x.clamp(min=0) if relu else x


def y_by_taps(case, r, pad=None):
    """y[n, oh, ow, c] = sum over taps with ih = oh s - pad + kh dil in [0, H) (likewise iw) of relu?(x)[n, ih, iw, c] w[c, kh, kw];
    pad: the offset the taps use (a fault: dil), the output size stays the descriptor's"""
    n, h, w, c, ld, cw, s, d, p, _ = case
    pad = p if pad is None else pad
    ho, wo = out_hw(case)
    x, wt = _x_op(case, r), r["w"].double()
    y = torch.zeros(n, ho, wo, cw, dtype=torch.float64)
    for kh in range(3):
        ih = torch.arange(ho) * s - pad + kh * d
        okh = (ih >= 0) & (ih < h)
        for kw in range(3):
            iw = torch.arange(wo) * s - pad + kw * d
            okw = (iw >= 0) & (iw < w)
            m = (okh[:, None] & okw[None, :])[None, :, :, None]
            y += x[:, ih.clamp(0, h - 1)][:, :, iw.clamp(0, w - 1)] * wt[:, 0, kh, kw] * m
    return y


def dx_by_taps(case, r, mask="x>0", pad=None, drop_last_of_chunk=0):
    """dx[n, ih, iw, c] = mask x sum over taps with th = ih + pad - kh dil >= 0, divisible by the stride, th / s < Ho (likewise w) of
    dy[n, oh, ow, c] w[c, kh, kw].  mask: "x>0" (the kernel), "relu(x)>0" (from the rectified value: the same set), "x>=0"
    (passes the planted zeros), "none" (unmasked).  drop_last_of_chunk = in_chunk: the last input pixel of every chunk is left 0"""
    n, h, w, c, ld, cw, s, d, p, relu = case
    pad = p if pad is None else pad
    ho, wo = out_hw(case)
    dy, wt = r["dy"][..., :cw].double(), r["w"].double()
    dx = torch.zeros(n, h, w, cw, dtype=torch.float64)

    def axis(size, osize, k):
        t = torch.arange(size) + pad - k * d
        o = torch.div(t, s, rounding_mode="floor")
        return (t >= 0) & (t % s == 0) & (o < osize), o.clamp(0, osize - 1)
    for kh in range(3):
        okh, oh = axis(h, ho, kh)
        for kw in range(3):
            okw, ow = axis(w, wo, kw)
            m = (okh[:, None] & okw[None, :])[None, :, :, None]
            dx += dy[:, oh][:, :, ow] * wt[:, 0, kh, kw] * m
    x = r["x"][..., :cw].double()
    if relu and mask != "none":
        dx = dx * {"x>0": x > 0, "relu(x)>0": x.clamp(min=0) > 0, "x>=0": x >= 0}[mask]
    if drop_last_of_chunk:
        lin = torch.zeros(n * h * w, dtype=torch.bool)
        lin[drop_last_of_chunk - 1::drop_last_of_chunk] = True
        dx = dx * (~lin).view(n, h, w, 1)
    return dx


def dw_by_chunks(case, r, out_chunk, drop_last=False, relu_of=None):
    """dw[c, kh, kw] = sum over chunks of out_chunk consecutive output pixels of the chunk's sum of dy[p] relu?(x)[pin(p, tap)];
    drop_last: every chunk loses its last output pixel"""
    n, h, w, c, ld, cw, s, d, p, _ = case
    ho, wo = out_hw(case)
    x, dy = _x_op(case, r, relu_of), r["dy"][..., :cw].double().contiguous().clone()
    if drop_last:
        flat = dy.view(-1, cw)
        flat[out_chunk - 1::out_chunk] = 0
    dw = torch.zeros(cw, 1, 3, 3, dtype=torch.float64)
    for kh in range(3):
        ih = torch.arange(ho) * s - p + kh * d
        okh = (ih >= 0) & (ih < h)
        for kw in range(3):
            iw = torch.arange(wo) * s - p + kw * d
            okw = (iw >= 0) & (iw < w)
            m = (okh[:, None] & okw[None, :])[None, :, :, None]
            dw[:, 0, kh, kw] = (x[:, ih.clamp(0, h - 1)][:, :, iw.clamp(0, w - 1)] * dy * m).sum((0, 1, 2))
    return dw
