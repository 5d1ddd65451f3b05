"""Cases, seeded inputs, float64 restatement and fp32 floors of the depthwise 3 x 3 kernels (csrc/dwconv3.hip), shared by
tests/test_dwconv3_gpu.py (the kernels), tests/test_dw3_ref_cpu.py (no GPU: ties every case to the branch it reaches through
the library's host queries, measures the floors, emulates the faults those branches can have) and tests/bn_partials_ref.py.

Rule (the one of tests/streaming_ref.py and tests/conv_ref.py): rel_err = max|a - b| / max|b| against float64 must be
<= 4 x FLOOR[check]; FLOOR[check] is torch's own fp32 grouped convolution (and its autograd) on the same inputs, CPU, one
thread.  The floor is kept PER CASE ("dw3.<case id>.<y | dx | dx_acc | dw>"): torch's fp32 weight gradient degrades with the pixel
count (2e-8 .. 8e-7 on the small maps, 3e-5 at half a million pixels), and one floor over all cases would hand the largest
figure to the small maps.

The restatement is F.conv2d(groups) in float64, which tests/test_streaming_ref_cpu.py ties to a direct tap loop.  Depthwise
is per channel, so on a channel subset it is exact: the ~100 MB shapes are compared on the first and the last channel quad of
the first and the last workgroup channel block (subset_channels), over every pixel."""
import ctypes

import torch
import torch.nn.functional as F

# (N, H, W, C, Cw, stride, dil, slices)
CASES = [
    (2, 19, 23, 32, 32, 1, 1, False),
    (2, 19, 23, 96, 96, 2, 1, False),
    (3, 5, 7, 96, 96, 1, 4, False),          # the dilation reaches past the image: only centre taps are valid
    (1, 1, 9, 144, 144, 1, 2, False),        # a single row
    (2, 18, 22, 144, 144, 2, 1, False),      # even size under stride 2
    (2, 65, 49, 144, 144, 1, 1, False),      # 6 370 pixels: many tiles, many workgroup partials
    (2, 33, 17, 32, 30, 1, 2, False),        # padded buffer: channels 30, 31 see zero weights
    (2, 11, 13, 48, 48, 2, 1, True),         # x, y, dy, dx are channel slices of wider buffers (ldx, ldy > C)
    # -- the fallback layout (quad count no multiple of 8, 12 or 16: CQ = 16 with idle quad lanes)
    (2, 9, 11, 20, 20, 1, 1, False),         # 5 quads: one channel block, 11 idle quad lanes
    (2, 9, 11, 72, 70, 1, 1, False),         # 18 quads: the second block two quads wide; channels 70, 71 see zero weights
    # -- small geometry
    (2, 14, 18, 32, 32, 2, 2, False),        # stride 2 with dilation 2, even map
    (2, 13, 17, 96, 96, 2, 2, False),        # ... odd map
    (2, 9, 1, 32, 32, 1, 1, False),          # one column
    (1, 9, 1, 48, 48, 2, 1, False),          # one column under stride 2
    (3, 1, 1, 144, 144, 1, 1, False),        # 1 x 1 maps
    (1, 1, 1, 20, 20, 2, 2, False),          # one pixel in all, fallback layout
]
FALLBACK, SMALL_GEOMETRY = (8, 9), (10, 11, 12, 13, 14, 15)      # indices into CASES
# the tiles production uses.  Forward: 8 pixels per thread (dw3_ppt: P / (RL 8) x colblocks >= 4096).  Backward: the chunk cap
# (dw3_chunks clamps to 2048, so out_chunk exceeds 256 above 524 288 output pixels).  Each shape runs ONE direction.
BIG_FWD = [
    (1, 419, 419, 144, 144, 1, 1, False),    # CQ 12, RL 16: tile_rows 128; 175 561 = 1371 x 128 + 73
    (1, 1031, 1035, 32, 32, 1, 1, False),    # CQ 8, RL 32: tile_rows 256; 1 067 085 = 4168 x 256 + 77 (the threshold: 1 048 576)
]
BIG_FWD_NEIGHBOUR = [(1, 418, 418, 144, 144, 1, 1, False), (1, 1023, 1025, 32, 32, 1, 1, False)]      # still 4 pixels per thread
BIG_BWD = [
    (1, 725, 725, 32, 32, 1, 1, False),      # 525 625 = 2045 x 257 + 60 output pixels: out_chunk = in_chunk = 257, chunk 2045 ragged, 2046 and 2047 empty
    (1, 1449, 1449, 8, 8, 2, 1, False),      # stride 2: out_chunk 257 over 725 x 725, in_chunk 1026 over 1449 x 1449; fallback layout
]
BIG_BWD_NEIGHBOUR = [(1, 724, 724, 32, 32, 1, 1, False), (1, 1447, 1447, 8, 8, 2, 1, False)]          # 256-pixel chunks, fewer than 2048


def case_id(c):
    return "n%d_%dx%d_c%d_cw%d_s%d_d%d%s" % (c[:7] + ("_sliced" if c[7] else "",))


# ---- the layout of csrc/dwconv3.hip, restated --------------------------------------------------------------------------------
def layout(c):
    """(CQ, RL, colblocks, fallback): channel quads per workgroup -- the widest of 16 / 12 / 8 that divides the quad count, 16
    when none does (fallback: idle quad lanes); pixel lanes; channel blocks"""
    c4 = c // 4
    cq = 16 if c4 % 16 == 0 else (12 if c4 % 12 == 0 else (8 if c4 % 8 == 0 else 16))
    return cq, (32 if cq == 8 else 16), (c4 + cq - 1) // cq, c4 % cq != 0


def out_hw(case):
    n, h, w, c, cw, s, d, _ = case
    return (h - 1) // s + 1, (w - 1) // s + 1


def queries(case):
    """what the library's host queries say about a case: output pixels, statistic tiles and tile rows, backward chunks (from
    the workspace size) and the pixels per chunk on the output / input grid that follow from them"""
    from iswm_amd import _lib
    n, h, w, c, cw, s, d, _ = case
    ho, wo = out_hw(case)
    dd = _lib.ConvDesc(n, h, w, c, ho, wo, c, 3, 3, s, d, d, c, c)
    lib = _lib.load()
    ws = lib.iswm_dwconv3x3_bwd_workspace(ctypes.byref(dd))
    assert ws % (9 * c * 4) == 0
    chunks, pout, pin = ws // (9 * c * 4), n * ho * wo, n * h * w
    return dict(pout=pout, pin=pin, tiles=lib.iswm_dwconv3x3_stat_tiles(ctypes.byref(dd)),
                tile_rows=lib.iswm_dwconv3x3_stat_tile_rows(ctypes.byref(dd)), chunks=chunks,
                out_chunk=(pout + chunks - 1) // chunks, in_chunk=(pin + chunks - 1) // chunks)


def subset_channels(c, cw):
    """first and last quad of the first and of the last workgroup channel block, below Cw"""
    cq, _, blocks, _ = layout(c)
    quads = set()
    for b in (0, blocks - 1):
        q0, q1 = b * cq, min(c // 4, (b + 1) * cq) - 1
        quads.update((q0, q1))
    return [ch for q in sorted(quads) for ch in range(4 * q, 4 * q + 4) if ch < cw]


# ---- inputs and the restatement ------------------------------------------------------------------------------------------------
def inputs(case):
    """seeded inputs (|x| of order 1, non-zero mean): x, w [Cw,1,3,3], dy, dx0 (what the accumulating form adds into)"""
    n, h, w, c, cw, s, d, _ = case
    g = torch.Generator().manual_seed(hash(case[:7]) % 1000)
    x = torch.randn(n, h, w, c, generator=g) + 0.7
    wt = torch.randn(cw, 1, 3, 3, generator=g) * 0.5 + 0.1
    ho, wo = out_hw(case)
    dy = torch.randn(n, ho, wo, c, generator=g) + 0.2
    dx0 = torch.randn(n, h, w, c, generator=g)
    return dict(x=x, w=wt, dy=dy, dx0=dx0, ho=ho, wo=wo)


def restate(case, r, ch=None, dtype=torch.float64, parts=("y", "dx", "dw")):
    """{y [N,Ho,Wo,len(ch)], dx [N,H,W,len(ch)], dx_acc, dw [len(ch),1,3,3]} of the channels ch (all: every channel, those past
    Cw zero) in `dtype`: float64 is the restatement, float32 torch's own operator (the floor)"""
    n, h, w, c, cw, s, d, _ = case
    full = ch is None
    ch = list(range(cw)) if full else ch
    assert max(ch) < cw
    need_grad = "dx" in parts or "dw" in parts
    xr = r["x"][..., ch].permute(0, 3, 1, 2).to(dtype).requires_grad_(need_grad)
    wr = r["w"][ch].to(dtype).requires_grad_(need_grad)
    y = F.conv2d(xr, wr, None, s, d, d, len(ch))
    pad = lambda t: F.pad(t.detach().permute(0, 2, 3, 1), (0, c - cw)) if full else t.detach().permute(0, 2, 3, 1)
    out = dict(y=pad(y))
    if need_grad:
        y.backward(r["dy"][..., ch].permute(0, 3, 1, 2).to(dtype))
        base = r["dx0"] if full else r["dx0"][..., ch]
        out.update(dx=pad(xr.grad), dw=wr.grad.detach())
        out["dx_acc"] = out["dx"] + base.to(dtype)
    return out


def key(case, q):
    return "dw3.%s.%s" % (case_id(case), q)


def bound(case, q):
    return 4.0 * FLOOR[key(case, q)]


def big_parts(case):
    """what a ~100 MB shape runs: the forward of BIG_FWD, the backward of BIG_BWD"""
    return ("y",) if case in BIG_FWD else ("dx", "dx_acc", "dw")


# ---- recorded floors (profiles/streaming_kernel_tests.txt carries the same figures; tests/test_dw3_ref_cpu.py ties the two) --------
FLOOR = {
    "dw3.n2_19x23_c32_cw32_s1_d1.y": 9.3e-08,
    "dw3.n2_19x23_c32_cw32_s1_d1.dx": 9.2e-08,
    "dw3.n2_19x23_c32_cw32_s1_d1.dx_acc": 1.1e-07,
    "dw3.n2_19x23_c32_cw32_s1_d1.dw": 7.0e-07,
    "dw3.n2_19x23_c96_cw96_s2_d1.y": 1.1e-07,
    "dw3.n2_19x23_c96_cw96_s2_d1.dx": 8.2e-08,
    "dw3.n2_19x23_c96_cw96_s2_d1.dx_acc": 7.9e-08,
    "dw3.n2_19x23_c96_cw96_s2_d1.dw": 4.3e-07,
    "dw3.n3_5x7_c96_cw96_s1_d4.y": 7.0e-08,
    "dw3.n3_5x7_c96_cw96_s1_d4.dx": 4.8e-08,
    "dw3.n3_5x7_c96_cw96_s1_d4.dx_acc": 6.5e-08,
    "dw3.n3_5x7_c96_cw96_s1_d4.dw": 7.0e-08,
    "dw3.n1_1x9_c144_cw144_s1_d2.y": 8.2e-08,
    "dw3.n1_1x9_c144_cw144_s1_d2.dx": 6.2e-08,
    "dw3.n1_1x9_c144_cw144_s1_d2.dx_acc": 5.6e-08,
    "dw3.n1_1x9_c144_cw144_s1_d2.dw": 6.9e-08,
    "dw3.n2_18x22_c144_cw144_s2_d1.y": 1.0e-07,
    "dw3.n2_18x22_c144_cw144_s2_d1.dx": 6.4e-08,
    "dw3.n2_18x22_c144_cw144_s2_d1.dx_acc": 7.7e-08,
    "dw3.n2_18x22_c144_cw144_s2_d1.dw": 4.7e-07,
    "dw3.n2_65x49_c144_cw144_s1_d1.y": 1.6e-07,
    "dw3.n2_65x49_c144_cw144_s1_d1.dx": 1.1e-07,
    "dw3.n2_65x49_c144_cw144_s1_d1.dx_acc": 1.1e-07,
    "dw3.n2_65x49_c144_cw144_s1_d1.dw": 3.2e-06,
    "dw3.n2_33x17_c32_cw30_s1_d2.y": 1.2e-07,
    "dw3.n2_33x17_c32_cw30_s1_d2.dx": 1.1e-07,
    "dw3.n2_33x17_c32_cw30_s1_d2.dx_acc": 8.2e-08,
    "dw3.n2_33x17_c32_cw30_s1_d2.dw": 7.7e-07,
    "dw3.n2_11x13_c48_cw48_s2_d1_sliced.y": 8.3e-08,
    "dw3.n2_11x13_c48_cw48_s2_d1_sliced.dx": 7.2e-08,
    "dw3.n2_11x13_c48_cw48_s2_d1_sliced.dx_acc": 9.0e-08,
    "dw3.n2_11x13_c48_cw48_s2_d1_sliced.dw": 2.3e-07,
    "dw3.n2_9x11_c20_cw20_s1_d1.y": 6.3e-08,
    "dw3.n2_9x11_c20_cw20_s1_d1.dx": 8.6e-08,
    "dw3.n2_9x11_c20_cw20_s1_d1.dx_acc": 9.5e-08,
    "dw3.n2_9x11_c20_cw20_s1_d1.dw": 5.3e-07,
    "dw3.n2_9x11_c72_cw70_s1_d1.y": 1.0e-07,
    "dw3.n2_9x11_c72_cw70_s1_d1.dx": 1.4e-07,
    "dw3.n2_9x11_c72_cw70_s1_d1.dx_acc": 1.2e-07,
    "dw3.n2_9x11_c72_cw70_s1_d1.dw": 3.7e-07,
    "dw3.n2_14x18_c32_cw32_s2_d2.y": 1.1e-07,
    "dw3.n2_14x18_c32_cw32_s2_d2.dx": 1.1e-07,
    "dw3.n2_14x18_c32_cw32_s2_d2.dx_acc": 1.1e-07,
    "dw3.n2_14x18_c32_cw32_s2_d2.dw": 7.2e-08,
    "dw3.n2_13x17_c96_cw96_s2_d2.y": 9.1e-08,
    "dw3.n2_13x17_c96_cw96_s2_d2.dx": 1.1e-07,
    "dw3.n2_13x17_c96_cw96_s2_d2.dx_acc": 9.6e-08,
    "dw3.n2_13x17_c96_cw96_s2_d2.dw": 9.5e-08,
    "dw3.n2_9x1_c32_cw32_s1_d1.y": 5.5e-08,
    "dw3.n2_9x1_c32_cw32_s1_d1.dx": 2.9e-08,
    "dw3.n2_9x1_c32_cw32_s1_d1.dx_acc": 4.7e-08,
    "dw3.n2_9x1_c32_cw32_s1_d1.dw": 1.0e-07,
    "dw3.n1_9x1_c48_cw48_s2_d1.y": 5.9e-08,
    "dw3.n1_9x1_c48_cw48_s2_d1.dx": 3.4e-08,
    "dw3.n1_9x1_c48_cw48_s2_d1.dx_acc": 6.4e-08,
    "dw3.n1_9x1_c48_cw48_s2_d1.dw": 4.1e-08,
    "dw3.n3_1x1_c144_cw144_s1_d1.y": 2.7e-08,
    "dw3.n3_1x1_c144_cw144_s1_d1.dx": 3.2e-08,
    "dw3.n3_1x1_c144_cw144_s1_d1.dx_acc": 4.5e-08,
    "dw3.n3_1x1_c144_cw144_s1_d1.dw": 4.8e-08,
    "dw3.n1_1x1_c20_cw20_s2_d2.y": 3.8e-08,
    "dw3.n1_1x1_c20_cw20_s2_d2.dx": 1.9e-08,
    "dw3.n1_1x1_c20_cw20_s2_d2.dx_acc": 3.2e-08,
    "dw3.n1_1x1_c20_cw20_s2_d2.dw": 2.1e-08,
    "dw3.n1_419x419_c144_cw144_s1_d1.y": 1.5e-07,
    "dw3.n1_1031x1035_c32_cw32_s1_d1.y": 1.2e-07,
    "dw3.n1_725x725_c32_cw32_s1_d1.dx": 1.3e-07,
    "dw3.n1_725x725_c32_cw32_s1_d1.dx_acc": 1.3e-07,
    "dw3.n1_725x725_c32_cw32_s1_d1.dw": 3.4e-05,
    "dw3.n1_1449x1449_c8_cw8_s2_d1.dx": 7.8e-08,
    "dw3.n1_1449x1449_c8_cw8_s2_d1.dx_acc": 8.9e-08,
    "dw3.n1_1449x1449_c8_cw8_s2_d1.dw": 2.8e-05,
}
