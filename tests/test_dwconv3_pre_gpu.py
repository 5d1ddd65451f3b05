"""Pre-activation depthwise 3x3 kernels (csrc/dwconv3.hip: iswm_dwconv3x3_pre_fwd / _pre_bwd, include/iswm_hip_sep.h) bit for bit
against the general depthwise kernels of csrc/dwconv.hip on relu?(x), and against torch's grouped convolution in float64.

Per case of tests/dw3_pre_ref.py (tests/test_dw3_pre_ref_cpu.py ties each to the layout / chunking it reaches and shows on the
CPU which faults these assertions catch):
  y (fp32)      == iswm_dwconv2d_fwd(relu?(x)); columns [C, pitch) of the output buffer exactly zero
  y (planes)    joined by iswm_join_planes == the fp32 y; pad columns exactly zero in all three planes
  y (bf16)      == the fp32 y rounded to nearest-even bf16; pad columns zero
  dx, dx + base == (x > 0) x iswm_dwconv2d_dgrad (+ base); exactly 0 where x <= 0 (0.0 and -0.0 are planted in x)
  dw            == iswm_dwconv3x3_bwd on relu?(x) where pad == dil and the layout is that kernel's (not at 728 channels, which
                   the backward lays over 736 columns); everywhere within 4 x FLOOR of float64, FLOOR = torch's own
                   fp32 grouped convolution on the same inputs, computed here (the rule of tests/test_dwconv3_gpu.py)
  two runs give the same bits; either half of the backward alone gives the same values; bad geometry raises IswmError."""
import functools

import pytest
import torch

from tests import dw3_pre_ref as D
from tests.util import rel_err

pytestmark = pytest.mark.gpu

IDS = [D.case_id(c) for c in D.CASES]


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(case):
    r = D.inputs(case)
    r.update(D.restate(case, r))
    r["floor"] = D.floors(case, r, r)
    return r


def within(case, q, got, ref, floor):
    err = rel_err(got, ref)
    print("dw3pre %-44s %-6s err %.3e  bound %.3e" % (D.case_id(case), q, err, 4 * floor))
    assert err <= 4 * floor, (D.case_id(case), q, err, 4 * floor)


def _geom(x, case):
    from iswm_amd import ops
    n, h, w, c, ld, cw, s, d, p, _ = case
    return ops.ConvGeom(x, c, 3, 3, s, p, d)


def _rect(x, case):
    return torch.relu(x) if case[9] else x


def round_bf16(t):
    """round to nearest even on the bit pattern (finite values), as csrc/planes.h round_bf16x4"""
    u = t.contiguous().view(torch.int32)
    r = (u + 0x7FFF + ((u >> 16) & 1)) & ~0xFFFF
    return r.view(torch.float32)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_forward(case):
    from iswm_amd import ops
    n, h, w, c, ld, cw, s, d, p, relu = case
    r = _case(case)
    x, wt = r["x"].to(dev()), r["w"].to(dev())
    g = _geom(x, case)
    ho, wo = r["ho"], r["wo"]

    def f32_out():
        return torch.full((n, ho, wo, ld), 7.0, device=dev())
    buf = f32_out()
    y = ops.dwconv3x3_pre_fwd(x, wt, g, relu, out=buf[..., :c])
    y_old = ops.dwconv2d_fwd(_rect(x, case), wt, g, None)
    assert torch.equal(y, y_old), "not bit-identical to iswm_dwconv2d_fwd on relu?(x)"
    if ld > c:
        assert float(buf[..., c:].abs().max()) == 0.0, "pad columns of the fp32 output are not zero"
    if cw < c:
        assert float(y[..., cw:].abs().max()) == 0.0
    within(case, "y", y, r["y"], r["floor"]["y"])
    buf2 = f32_out()
    assert torch.equal(ops.dwconv3x3_pre_fwd(x, wt, g, relu, out=buf2[..., :c]), y) and torch.equal(buf2, buf)      # run to run
    if relu:                                                       # the flag is what rectifies: off, the kernel is linear in x
        assert torch.equal(ops.dwconv3x3_pre_fwd(x, wt, g, False), ops.dwconv2d_fwd(x, wt, g, None))
    # three planes in a buffer of the pitch, filled with ones beforehand
    pl = ops.Planes(torch.ones((3, n, ho, wo, ld), dtype=torch.bfloat16, device=dev()))
    yp = ops.dwconv3x3_pre_fwd(x, wt, g, relu, out=pl[..., 0:c])
    assert torch.equal(yp.f32(), y), "planes do not join to the fp32 y"
    assert torch.equal(pl.f32()[..., :c], y)
    if ld > c:
        assert float(pl.t[..., c:].float().abs().max()) == 0.0, "pad columns of the planes are not zero"
    # one rounded bf16 plane
    one = ops.Planes(torch.ones((1, n, ho, wo, ld), dtype=torch.bfloat16, device=dev()))
    ops.dwconv3x3_pre_fwd(x, wt, g, relu, out=one[..., 0:c])
    assert torch.equal(one.t[0, ..., :c].float(), round_bf16(y)), "the single plane is not round_bf16(y)"
    if ld > c:
        assert float(one.t[..., c:].float().abs().max()) == 0.0


def _backward_checks(case, r, ch=None):
    """dx / dx + base / dw of one case; ch: the channel subset the float64 reference covers (None: all)"""
    from iswm_amd import ops
    n, h, w, c, ld, cw, s, d, p, relu = case
    x, dy, wt = r["x"].to(dev()), r["dy"].to(dev()), r["w"].to(dev())
    g = _geom(x, case)
    sel = (lambda t: t) if ch is None else (lambda t: t[..., ch].cpu())
    dx, dw = ops.dwconv3x3_pre_bwd(x, dy, wt, g, cw, relu)
    lin = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c))
    mask = (x > 0) if relu else torch.ones_like(x, dtype=torch.bool)
    want = torch.where(mask, lin, torch.zeros_like(lin))
    assert torch.equal(dx, want), "not bit-identical to (x > 0) x iswm_dwconv2d_dgrad"
    if relu:
        assert int((x == 0).sum()) > 0 and float(dx[x <= 0].abs().max()) == 0.0            # +0.0 and -0.0 planted: gradient 0
    if cw < c:
        assert float(dx[..., cw:].abs().max()) == 0.0
    base = r["dx0"].to(dev())
    acc, dw_b = ops.dwconv3x3_pre_bwd(x, dy, wt, g, cw, relu, dx=base.clone(), accumulate=True)
    assert torch.equal(acc, want + base), "accumulating form is not base + mask x dgrad"
    assert torch.equal(dw_b, dw)                                                           # run to run
    assert tuple(dw.shape) == (cw, 1, 3, 3)
    if p == d and D.bwd_layout(c) == D.layout(c):           # same pixel lanes: the same fp32 sums in the same order
        _, dw_old = ops.dwconv3x3_bwd(_rect(x, case), dy, wt, ops.ConvGeom(x, c, 3, 3, s, d, d), cw, need_dx=False)
        assert torch.equal(dw, dw_old), "dw not bit-identical to iswm_dwconv3x3_bwd on relu?(x)"
    fl = r["floor"]
    within(case, "dx", sel(dx), r["dx"], fl["dx"])
    within(case, "dx_acc", sel(acc), r["dx_acc"], fl["dx_acc"])
    within(case, "dw", dw if ch is None else dw[ch].cpu(), r["dw"], fl["dw"])
    dx_only, none = ops.dwconv3x3_pre_bwd(x, dy, wt, g, cw, relu, need_dw=False)
    assert none is None and torch.equal(dx_only, dx)
    none, dw_only = ops.dwconv3x3_pre_bwd(x, dy, wt, g, cw, relu, need_dx=False)
    assert none is None and torch.equal(dw_only, dw)


@pytest.mark.parametrize("case", D.CASES, ids=IDS)
def test_backward(case):
    _backward_checks(case, _case(case))


@pytest.mark.parametrize("case", D.BIG_BWD, ids=[D.case_id(c) for c in D.BIG_BWD])
def test_backward_under_the_chunk_cap(case):
    """more than 2048 x 256 output pixels: a chunk holds 257 pixels of either grid, the last chunk fewer"""
    n, h, w, c, ld, cw, s, d, p, relu = case
    q = D.queries(case)
    assert q["chunks"] == 2048 and q["pout"] > 2048 * 256 and q["out_chunk"] == 257 and q["pout"] % 257 != 0
    r, ch = D.inputs(case), D.subset_channels(c, cw)
    r.update(D.restate(case, r, ch))
    r["floor"] = D.floors(case, r, r, ch)
    _backward_checks(case, r, ch)


def test_refusals():
    from iswm_amd import _lib, ops
    x = torch.zeros(1, 9, 9, 8, device=dev())
    w3 = torch.zeros(8, 1, 3, 3, device=dev())
    dy = torch.zeros(1, 9, 9, 8, device=dev())
    bad = [ops.ConvGeom(x, 8, 3, 3, 1, 2, 1),       # pad > dil
           ops.ConvGeom(x, 8, 3, 3, 1, 0, 1),       # pad == 0
           ops.ConvGeom(x, 8, 3, 3, 3, 1, 1),       # stride 3
           ops.ConvGeom(x, 8, 5, 5, 1, 2, 1)]       # 5 x 5
    for g in bad:
        with pytest.raises(_lib.IswmError):
            ops.dwconv3x3_pre_fwd(x, w3, g, True)
        with pytest.raises(_lib.IswmError):
            ops.dwconv3x3_pre_bwd(x, torch.zeros(1, g.ho, g.wo, 8, device=dev()), w3, g, 8, True)
    x6 = torch.zeros(1, 9, 9, 6, device=dev())      # C % 4
    w6 = torch.zeros(6, 1, 3, 3, device=dev())
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_pre_fwd(x6, w6, ops.ConvGeom(x6, 6, 3, 3, 1, 1, 1), True)
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_pre_bwd(x6, x6.clone(), w6, ops.ConvGeom(x6, 6, 3, 3, 1, 1, 1), 6, True)
    wide = torch.zeros(1, 9, 9, 10, device=dev())   # pitch 10: not a multiple of 4
    g = ops.ConvGeom(x, 8, 3, 3, 1, 1, 1)
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_pre_fwd(wide[..., :8], w3, g, True)
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_pre_fwd(x, w3, g, True, out=wide[..., :8])
    with pytest.raises(_lib.IswmError):
        ops.dwconv3x3_pre_bwd(x, dy, w3, g, 8, True, dx=wide[..., :8])
    with pytest.raises(_lib.IswmError):             # a map with no output: 3 + 2 - 8 - 1 < 0
        small = torch.zeros(1, 3, 3, 8, device=dev())
        d = _lib.ConvDesc(1, 3, 3, 8, 1, 1, 8, 3, 3, 1, 1, 4, 8, 8)
        import ctypes
        _lib.call("iswm_dwconv3x3_pre_fwd", ctypes.byref(d), ops._p(small), ops._p(w3), 8, 1, ops._p(small), 0, 8, ops._stream())
