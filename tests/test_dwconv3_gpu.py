"""Depthwise 3x3 kernels of csrc/dwconv3.hip (forward + BatchNorm tile statistics, one-launch backward) against torch's own
grouped convolution in float64 on the CPU, and bit for bit against the general depthwise kernels of csrc/dwconv.hip.

Rule (tests/dw3_ref.py): y, dx, dx + base and dw within 4 x FLOOR of the float64 restatement, FLOOR = torch's own fp32 grouped
convolution on the same inputs, per case (tests/test_dw3_ref_cpu.py measures it again, ties every case to the kernel branch it
reaches through the host queries and shows which faults of those branches these assertions catch).  The older bounds stay
beside it: y / dx within 1e-5 of max|.| and dw within 2e-4 of max|dw| (the figures of test_depthwise_bn_relu6_stage); the batch
mean / variance iswm_bn_finalize derives from the kernel's partials within 1e-5 of the fp64 statistics of y (the partials
themselves are pinned tile by tile in tests/test_bn_partials_gpu.py).

The ~100 MB shapes (8 pixels per thread forward, the backward under the 2048-chunk cap) run one direction each; their float64
reference covers every pixel of a channel subset (dw3_ref.subset_channels), the bit-identity with csrc/dwconv.hip every channel."""
import functools

import pytest
import torch

from tests import dw3_ref as D
from tests.dw3_ref import CASES
from tests.util import rel_err

pytestmark = pytest.mark.gpu

IDS = [D.case_id(c) for c in CASES]


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
    r = D.inputs(case)
    r.update(D.restate(case, r))
    return r


def within(case, q, got, ref):
    """the rule of tests/dw3_ref.py: print the figure, then assert it"""
    err = rel_err(got, ref)
    print("dw3 %-34s %-6s err %.3e  bound %.3e" % (D.case_id(case), q, err, D.bound(case, q)))
    assert err <= D.bound(case, q), (D.case_id(case), q, err, D.bound(case, q))


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
    within(case, "y", y, r["y"])
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
    within(case, "dx", dx, r["dx"])
    within(case, "dw", dw, r["dw"])
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
    within(case, "dx_acc", acc, r["dx_acc"])
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


# ---- the tiles production uses: ~100 MB shapes, one direction each ---------------------------------------------------------------
@pytest.mark.parametrize("case", D.BIG_FWD, ids=[D.case_id(c) for c in D.BIG_FWD])
def test_forward_at_eight_pixels_per_thread(case):
    """k_dw3_fwd_stats<8>: tile_rows = 8 RL with a short last tile (tests/test_dw3_ref_cpu.py holds the neighbouring shape to
    the 4-pixel answer).  Bit-identity over every channel; float64 on the channel subset over every pixel"""
    from iswm_amd import ops
    n, h, w, c, cw, s, d, _ = case
    q, (cq, rl, blocks, _) = D.queries(case), D.layout(c)
    assert q["tile_rows"] == 8 * rl and 0 < q["pout"] % q["tile_rows"] < q["tile_rows"]
    r, ch = D.inputs(case), D.subset_channels(c, cw)
    ref = D.restate(case, r, ch, parts=("y",))["y"]
    x, wt = r["x"].to(dev()), r["w"].to(dev())
    g = _geom(x, case)
    y, part, lay = ops.dwconv3x3_fwd_stats(x, wt, g, True)
    assert tuple(lay) == (q["tiles"], q["tile_rows"]) and tuple(part.shape) == (2, q["tiles"], c)
    y_old = ops.dwconv2d_fwd(x, wt, g, None, torch.zeros_like(y))
    assert torch.equal(y, y_old), "not bit-identical to iswm_dwconv2d_fwd"
    del y_old
    got = y[..., ch].cpu()
    assert rel_err(got, ref) <= 1e-5
    within(case, "y", got, ref)
    # the merge of the partials (more than 2048 tiles at 32 channels: the finalize's tail loop on real partials)
    p = q["pout"]
    ones, zeros = torch.ones(c, device=dev()), torch.zeros(c, device=dev())
    rm, rv = torch.zeros(c, device=dev()), torch.zeros(c, device=dev())
    ops.bn_finalize(part, q["tiles"], p, q["tile_rows"], ones, zeros, rm, rv, 1.0)
    flat = ref.reshape(-1, len(ch))
    em, ev = rel_err(rm[ch], flat.mean(0)), rel_err(rv[ch], flat.var(0, unbiased=True))
    print("mean rel err %.2e  var rel err %.2e  (%d tiles of %d)" % (em, ev, q["tiles"], q["tile_rows"]))
    assert em <= 1e-5 and ev <= 1e-5
    y_eval, none, _ = ops.dwconv3x3_fwd_stats(x, wt, g, False)
    assert none is None and torch.equal(y_eval, y)
    del y_eval
    y2, part2, _ = ops.dwconv3x3_fwd_stats(x, wt, g, True)
    assert torch.equal(y2, y) and torch.equal(part2, part)


@pytest.mark.parametrize("case", D.BIG_BWD, ids=[D.case_id(c) for c in D.BIG_BWD])
def test_backward_under_the_chunk_cap(case):
    """k_dw3_bwd with dw3_chunks clamped to 2048: more than 2048 x 256 output pixels, so a chunk holds 257 output pixels (the
    last chunk fewer) -- and, under stride 2, 1026 input pixels.  dx, accumulating dx and dw"""
    from iswm_amd import ops
    n, h, w, c, cw, s, d, _ = case
    q = D.queries(case)
    assert q["chunks"] == 2048 and q["pout"] > 2048 * 256 and q["out_chunk"] == 257 and q["pout"] % q["out_chunk"] != 0
    r, ch = D.inputs(case), D.subset_channels(c, cw)
    ref = D.restate(case, r, ch)
    x, dy, wt = r["x"].to(dev()), r["dy"].to(dev()), r["w"].to(dev())
    g = _geom(x, case)
    dx, dw = ops.dwconv3x3_bwd(x, dy, wt, g, cw)
    dx_old = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), torch.zeros_like(dx))
    assert torch.equal(dx, dx_old), "not bit-identical to iswm_dwconv2d_dgrad"
    del dx_old
    got_dx, got_dw = dx[..., ch].cpu(), dw[ch].cpu()
    assert tuple(dw.shape) == (cw, 1, 3, 3) and rel_err(got_dx, ref["dx"]) <= 1e-5 and rel_err(got_dw, ref["dw"]) <= 2e-4
    within(case, "dx", got_dx, ref["dx"])
    within(case, "dw", got_dw, ref["dw"])
    acc, dw_b = ops.dwconv3x3_bwd(x, dy, wt, g, cw, dx=r["dx0"].to(dev()), accumulate=True)
    acc_old = ops.dwconv2d_dgrad(dy, wt, g, (n, h, w, c), r["dx0"].to(dev()), True)
    assert torch.equal(acc, acc_old) and torch.equal(dw_b, dw)               # fixed-order merge: run-to-run identical bits
    del acc_old
    within(case, "dx_acc", acc[..., ch].cpu(), ref["dx_acc"])
