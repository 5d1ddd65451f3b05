"""Depthwise 3x3 kernels of csrc/dwconv3.hip (forward + BatchNorm tile statistics, one-launch backward) against torch's own
grouped convolution in float64 on the CPU, and bit for bit against the general depthwise kernels of csrc/dwconv.hip.

Bounds: y / dx within 1e-5 of max|.| and dw within 2e-4 of max|dw| (the figures of test_depthwise_bn_relu6_stage); the batch
mean / variance iswm_bn_finalize derives from the kernel's partials within 1e-5 of the fp64 statistics of y."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_err

pytestmark = pytest.mark.gpu

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
]
IDS = ["n%d_%dx%d_c%d_cw%d_s%d_d%d%s" % (c[:7] + ("_sliced" if c[7] else "",)) for c in CASES]


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def _view(t, sliced, off):
    """t [N,H,W,C] on the GPU, as a dense tensor or as channels [off, off + C) of a buffer 12 channels wider"""
    t = t.to(dev())
    if not sliced:
        return t.contiguous()
    n, h, w, c = t.shape
    buf = torch.full((n, h, w, c + 12), 7.0, device=dev())
    buf[..., off:off + c] = t
    return buf[..., off:off + c]


@functools.lru_cache(maxsize=None)
def _case(case):
    """seeded inputs (|x| of order 1, non-zero mean) and the float64 results, computed once per case"""
    n, h, w, c, cw, s, d, _ = case
    g = torch.Generator().manual_seed(hash(case[:7]) % 1000)
    x = torch.randn(n, h, w, c, generator=g) + 0.7
    wt = torch.randn(cw, 1, 3, 3, generator=g) * 0.5 + 0.1
    ho, wo = (h - 1) // s + 1, (w - 1) // s + 1
    dy = torch.randn(n, ho, wo, c, generator=g) + 0.2
    dx0 = torch.randn(n, h, w, c, generator=g)
    x64 = x[..., :cw].permute(0, 3, 1, 2).double().requires_grad_(True)
    w64 = wt.double().requires_grad_(True)
    y64 = F.conv2d(x64, w64, None, s, d, d, cw)
    y64.backward(dy[..., :cw].permute(0, 3, 1, 2).double())
    pad = lambda t: F.pad(t.detach().permute(0, 2, 3, 1), (0, c - cw))       # channels past Cw: zero
    return dict(x=x, w=wt, dy=dy, dx0=dx0, y=pad(y64), dx=pad(x64.grad), dw=w64.grad.detach(), ho=ho, wo=wo)


def _geom(x, case):
    from iswm_amd import ops
    _, _, _, c, _, s, d, _ = case
    return ops.ConvGeom(x, c, 3, 3, s, d, d)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_and_statistics(case):
    from iswm_amd import ops
    n, h, w, c, cw, s, d, sliced = case
    r = _case(case)
    x, wt = _view(r["x"], sliced, 4), r["w"].to(dev())
    g = _geom(x, case)

    def out():
        return _view(torch.zeros(n, r["ho"], r["wo"], c), sliced, 8)
    y, part, (tiles, tile_rows) = ops.dwconv3x3_fwd_stats(x, wt, g, True, out=out())
    y_old = ops.dwconv2d_fwd(x, wt, g, None, out())
    assert torch.equal(y, y_old), "not bit-identical to iswm_dwconv2d_fwd"
    err = rel_err(y, r["y"])
    print("y rel err %.2e" % err)
    assert err <= 1e-5
    if cw < c:
        assert float(y[..., cw:].abs().max()) == 0.0
    # statistics: the layout iswm_bn_finalize consumes (momentum 1: the running buffers become the batch statistics)
    p = n * r["ho"] * r["wo"]
    assert tiles == (p + tile_rows - 1) // tile_rows and tuple(part.shape) == (2, tiles, c)
    ones, zeros = torch.ones(c, device=dev()), torch.zeros(c, device=dev())
    rm, rv = torch.zeros(c, device=dev()), torch.zeros(c, device=dev())
    coef = ops.bn_finalize(part, tiles, p, tile_rows, ones, zeros, rm, rv, 1.0)
    flat = r["y"].reshape(-1, c)
    mean64, var64 = flat.mean(0), flat.var(0, unbiased=p > 1)
    em, ev = rel_err(rm, mean64), rel_err(rv, var64)
    print("mean rel err %.2e  var rel err %.2e  (%d tiles of %d)" % (em, ev, tiles, tile_rows))
    assert em <= 1e-5 and ev <= 1e-5
    assert rel_err(coef[2], mean64) <= 1e-5
    # eval-mode form (no partials) writes the same y; a second run of either form gives the same bits
    y_eval, none, _ = ops.dwconv3x3_fwd_stats(x, wt, g, False, out=out())
    assert none is None and torch.equal(y_eval, y)
    y2, part2, _ = ops.dwconv3x3_fwd_stats(x, wt, g, True, out=out())
    assert torch.equal(y2, y) and torch.equal(part2, part)
    if sliced:
        assert float((y2._base[..., :8] - 7.0).abs().max()) == 0.0 and float((y2._base[..., 8 + c:] - 7.0).abs().max()) == 0.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward(case):
    from iswm_amd import ops
    n, h, w, c, cw, s, d, sliced = case
    r = _case(case)
    x, dy, wt = _view(r["x"], sliced, 4), _view(r["dy"], sliced, 8), r["w"].to(dev())
    g = _geom(x, case)

    def dx_buf(t):
        return _view(t, sliced, 0)
    dx, dw = ops.dwconv3x3_bwd(x, dy, wt, g, cw, dx=dx_buf(torch.zeros(n, h, w, c)))
    dx_old = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), dx_buf(torch.zeros(n, h, w, c)))
    assert torch.equal(dx, dx_old), "not bit-identical to iswm_dwconv2d_dgrad"
    e_dx, e_dw = rel_err(dx, r["dx"]), rel_err(dw, r["dw"])
    print("dx rel err %.2e  dw rel err %.2e" % (e_dx, e_dw))
    assert e_dx <= 1e-5
    assert tuple(dw.shape) == (cw, 1, 3, 3) and e_dw <= 2e-4
    if cw < c:
        assert float(dx[..., cw:].abs().max()) == 0.0
    # a fresh dx of the entry point's own (no buffer handed in) holds the same values
    dx_own, _ = ops.dwconv3x3_bwd(x, dy, wt, g, cw)
    assert torch.equal(dx_own, dx)
    # accumulate form
    acc, dw_b = ops.dwconv3x3_bwd(x, dy, wt, g, cw, dx=dx_buf(r["dx0"]), accumulate=True)
    acc_old = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), dx_buf(r["dx0"]), True)
    assert torch.equal(acc, acc_old)
    assert rel_err(acc, r["dx"] + r["dx0"].double()) <= 1e-5
    # run-to-run identical bits (fixed-order merge, no atomics); either half alone gives the same values
    assert torch.equal(dw_b, dw)
    dx_only, none = ops.dwconv3x3_bwd(x, dy, wt, g, cw, need_dw=False)
    assert none is None and torch.equal(dx_only, dx)
    none, dw_only = ops.dwconv3x3_bwd(x, dy, wt, g, cw, need_dx=False)
    assert none is None and torch.equal(dw_only, dw)
    if sliced:
        assert float((acc._base[..., c:] - 7.0).abs().max()) == 0.0


def test_rejects_other_geometries():
    from iswm_amd import _lib, ops
    x = torch.zeros(1, 8, 8, 8, device=dev())
    w5 = torch.zeros(8, 1, 5, 5, device=dev())
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_fwd_stats(x, w5, ops.ConvGeom(x, 8, 5, 5, 1, 2, 1), False)
    w3 = torch.zeros(8, 1, 3, 3, device=dev())
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_fwd_stats(x, w3, ops.ConvGeom(x, 8, 3, 3, 1, 0, 1), False)      # pad != dil
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_fwd_stats(x, w3, ops.ConvGeom(x, 8, 3, 3, 3, 1, 1), False)      # stride 3
