"""The 1x1 classifier folded into the BatchNorm passes of the stage in front of it (csrc/bn_classify.hip; network/_deeplab.py:44-52
`classifier`): the folded kernels against float64 ATen and a float64 restatement at production and edge shapes, their three ReLU
decisions bit for bit against the unfused apply on data built to sit on rounding boundaries, their dy output formats bit for bit,
and the folded head against the unfolded one."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.util import rel_err

C = 256


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


@pytest.fixture
def conv_math(request):
    from iswm_amd import _lib
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    lib.iswm_set_conv_math(request.param)
    yield request.param
    lib.iswm_set_conv_math(old)


# ---- ReLU decisions on rounding boundaries ------------------------------------------------------------------------------------
ULPS = (-3, -2, -1, 0, 1, 2, 3)


def adversarial_bn(reps=64, seed=5):
    """y [7 reps, C] and per-channel mean / scale / shift (fp32 numpy) on which the order of evaluation of (y - mean) * scale + shift
    decides ReLUs: per channel a y0 with d0 = fl32(y0 - mean) and shift = -fl32(d0 * scale), so that at y = y0 mul-then-add gives
    exactly 0 and an fma gives the product's rounding error -- positive (ReLU on) in 3/4 of the channels, negative in the rest;
    row r of channel c holds y0 moved by ULPS[(r + c) % 7] ulps."""
    rng = np.random.default_rng(seed)
    mean = (rng.standard_normal(C) * 0.5).astype(np.float32)
    y0 = (mean + rng.uniform(0.5, 2.0, C) * rng.choice([-1.0, 1.0], C)).astype(np.float32)
    d0 = y0 - mean
    cand = rng.uniform(0.25, 2.0, (C, 64)).astype(np.float32)               # candidate scales per channel
    err = d0[:, None].astype(np.float64) * cand - (d0[:, None] * cand).astype(np.float64)
    want = np.where(np.arange(C) % 4 == 3, -1.0, 1.0)[:, None]
    pick = np.argmax(err * want > 0, axis=1)
    scale = cand[np.arange(C), pick]
    assert (err[np.arange(C), pick] * want[:, 0] > 0).all()
    shift = -(d0 * scale)
    y = np.empty((len(ULPS) * reps, C), np.float32)
    for r in range(y.shape[0]):
        k = np.array([ULPS[(r + c) % len(ULPS)] for c in range(C)])
        v = y0.copy()
        for step in range(3):
            v = np.where(k > step, np.nextafter(v, np.float32(np.inf)), v)
            v = np.where(-k > step, np.nextafter(v, np.float32(-np.inf)), v)
        y[r] = v
    return y, mean, scale.astype(np.float32), shift.astype(np.float32)


def relu_orders(y, mean, scale, shift):
    """the ReLU decision (pre-activation > 0) of (y - mean) * scale + shift under the two evaluation orders: fma (the sign of the
    float64 value -- the product of two fp32 numbers is exact there) and mul-then-add (two fp32 roundings)"""
    d = y - mean
    fma = d.astype(np.float64) * scale.astype(np.float64) + shift.astype(np.float64) > 0
    mad = (d * scale) + shift > 0
    return fma, mad


def test_adversarial_data_separate_the_evaluation_orders():
    """CPU self-check of adversarial_bn: the data really tell an fma from mul-then-add in >= 1 % of the elements (else the bit-exact
    decision test below could not see a kernel that rounds the expression differently)"""
    y, mean, scale, shift = adversarial_bn()
    fma, mad = relu_orders(y, mean, scale, shift)
    assert (fma != mad).mean() >= 0.01, (fma != mad).mean()
    assert 0.2 < fma.mean() < 0.8


@pytest.mark.gpu
@pytest.mark.parametrize("conv_math", [1, 0], ids=["bf16x6", "f32mfma"], indirect=True)
def test_folded_relu_decisions_bit_exact(conv_math):
    """each of the fold's three ReLU decisions -- forward (k_bn_apply_cls), backward reduce (k_bn_bwd_reduce_cls -> k_cls_finalize)
    and backward apply (k_bn_bwd_apply_cls) -- equals the unfused apply's pattern (ops.bn_apply(y, coef, True) > 0, what the same-mask
    recorder stores) element for element on adversarial_bn's data, and that pattern is the fma's"""
    from iswm_amd import ops
    d = dev()
    y, mean, scale, shift = adversarial_bn()
    fma, mad = relu_orders(y, mean, scale, shift)
    m = y.shape[0]
    coef = torch.from_numpy(np.stack([scale, shift, mean, np.ones(C, np.float32)])).to(d)
    yd = torch.from_numpy(y).view(1, 1, m, C).to(d)
    act = ops.bn_apply(yd, coef, True).view(m, C)
    on = act > 0
    assert torch.equal(on.cpu(), torch.from_numpy(fma)), int((on.cpu() != torch.from_numpy(fma)).sum())
    # forward: one-hot classifier rows (class k reads channel c0 + k), zero bias -> the logits ARE that channel's activation
    for c0 in range(0, C, 4):
        wc4 = torch.zeros(4, C, device=d)
        wc4[torch.arange(4), c0 + torch.arange(4)] = 1.0
        lg = ops.bn_apply_classify(yd, coef, wc4, torch.zeros(4, device=d)).view(m, 4)
        assert torch.equal(lg, act[:, c0:c0 + 4]), (c0, int((lg != act[:, c0:c0 + 4]).sum()))
    gamma = torch.ones(C, device=d)
    dgamma, dbeta = torch.empty(C, device=d), torch.empty(C, device=d)
    # backward apply, eval mode: dlogit = e_0 and Wc4[0] = 1 -> dy = gamma * invstd = 1 exactly where the ReLU is on, 0 elsewhere
    wc4 = torch.zeros(4, C, device=d)
    wc4[0] = 1.0
    dl = torch.zeros(1, 1, m, 4, device=d)
    dl[..., 0] = 1.0
    dy, _ = ops.bn_backward_classify(dl, wc4, yd, coef, gamma, False, dgamma, dbeta, False)
    assert torch.equal(dy.view(m, C) != 0, on), int(((dy.view(m, C) != 0) != on).sum())
    assert torch.equal(dy.view(m, C)[on], torch.ones_like(dy.view(m, C)[on]))
    # backward reduce: dlogit one-hot on four probe rows (row p0 + k for class k) -> dWc4[k] = that row's activation, exactly
    wc4 = torch.randn(4, C, generator=torch.Generator().manual_seed(3)).to(d)
    for p0 in range(0, m, 4):
        dl = torch.zeros(m, 4, device=d)
        dl[p0 + torch.arange(4), torch.arange(4)] = 1.0
        _, dwc4 = ops.bn_backward_classify(dl.view(1, 1, m, 4), wc4, yd, coef, gamma, True, dgamma, dbeta, False)
        assert torch.equal(dwc4, act[p0:p0 + 4]), (p0, int((dwc4 != act[p0:p0 + 4]).sum()))


# ---- production and edge shapes against a float64 restatement --------------------------------------------------------------------
CHUNK = 1 << 15           # rows per float64 block: at 16 x 129 x 129 x 256 one float64 tensor would be 545 MB


class FoldCase:
    """random BatchNorm -> ReLU -> 1x1 classifier data of one shape and its float64 forward / backward, computed in row blocks.
    The ReLU decisions are the fold's fp32 expression (the sign of fl32(y - mean) * scale + shift with one rounding, which
    test_folded_relu_decisions_bit_exact pins): at 68 M pre-activations a few sit within rounding of zero, and a flipped ReLU is a
    discontinuity, not an error (tests/test_hip_modules.py docstring)."""

    def __init__(self, shape, k, training, bias, seed, ld=C):
        n, h, w, _ = shape
        self.shape, self.k, self.training, self.m = shape, k, training, n * h * w
        g = torch.Generator().manual_seed(seed)
        self.y = torch.randn(self.m, C, generator=g) * (torch.rand(C, generator=g) + 0.5) + torch.randn(C, generator=g) * 0.3
        self.gamma, self.beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
        self.wc = torch.randn(k, C, generator=g) * 0.1
        self.bias = torch.randn(k, generator=g) if bias else None
        self.dl = torch.randn(self.m, k, generator=g)
        self.ld = ld
        if training:
            mean = sum(self.y[i:i + CHUNK].double().sum(0) for i in range(0, self.m, CHUNK)) / self.m
            var = sum(((self.y[i:i + CHUNK].double() - mean) ** 2).sum(0) for i in range(0, self.m, CHUNK)) / self.m
        else:
            mean, var = torch.randn(C, generator=g).double() * 0.1, (torch.rand(C, generator=g) + 0.5).double()
        self.mean64, self.inv64 = mean, 1.0 / torch.sqrt(var + 1e-5)
        # HIP: coefficients as bn_finalize would give them (scale, shift, mean, invstd)
        self.coef = torch.stack([(self.gamma.double() * self.inv64).float(), self.beta, mean.float(), self.inv64.float()])
        self._forward()

    def _rows(self, i):
        """float64 (xhat, ReLU pattern, activation) of rows i .. i + CHUNK"""
        y = self.y[i:i + CHUNK]
        d32 = (y - self.coef[2]).double()
        on = d32 * self.coef[0].double() + self.coef[1].double() > 0
        xh = (y.double() - self.mean64) * self.inv64
        act = (xh * self.gamma.double() + self.beta.double()) * on
        return xh, on, act

    def _forward(self):
        wc, dl = self.wc.double(), self.dl.double()
        self.logits = torch.empty(self.m, self.k, dtype=torch.float64)
        sdz, sdzx, self.dwc = torch.zeros(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64), 0.0
        for i in range(0, self.m, CHUNK):
            xh, on, act = self._rows(i)
            self.logits[i:i + CHUNK] = act @ wc.t() + (0.0 if self.bias is None else self.bias.double())
            dz = (dl[i:i + CHUNK] @ wc) * on
            sdz += dz.sum(0)
            sdzx += (dz * xh).sum(0)
            self.dwc = self.dwc + dl[i:i + CHUNK].t() @ act
        self.dbeta, self.dgamma = sdz, sdzx

    def dy_err(self, dy):
        """rel_err of an fp32 [M, C] dy against the float64 data gradient, block by block"""
        wc, dl, gi = self.wc.double(), self.dl.double(), self.gamma.double() * self.inv64
        worst = scale = 0.0
        for i in range(0, self.m, CHUNK):
            xh, on, _ = self._rows(i)
            dz = (dl[i:i + CHUNK] @ wc) * on
            ref = gi * (dz - self.dbeta / self.m - xh * self.dgamma / self.m) if self.training else gi * dz
            worst = max(worst, float((dy[i:i + CHUNK].double() - ref).abs().max()))
            scale = max(scale, float(ref.abs().max()))
        return worst / scale

    def device_y(self, d):
        """y on the device as an NHWC view with row pitch self.ld (a channel slice of a wider buffer when ld > C)"""
        n, h, w, _ = self.shape
        if self.ld == C:
            return self.y.view(n, h, w, C).to(d)
        buf = torch.zeros(n, h, w, self.ld, device=d)
        off = (self.ld - C) // 2 // 4 * 4
        buf[..., off:off + C] = self.y.view(n, h, w, C).to(d)
        return buf[..., off:off + C]

    def run(self, d, planes):
        """the fold on the device: (logits [M, 4], dy, dwc4, dgamma, dbeta)"""
        from iswm_amd import ops
        n, h, w, _ = self.shape
        yd = self.device_y(d)
        wc4 = torch.zeros(4, C)
        wc4[:self.k] = self.wc
        b4 = None
        if self.bias is not None:
            b4 = torch.zeros(4)
            b4[:self.k] = self.bias
            b4 = b4.to(d)
        dl4 = torch.zeros(self.m, 4)
        dl4[:, :self.k] = self.dl
        coef = self.coef.to(d)
        logits = ops.bn_apply_classify(yd, coef, wc4.to(d), b4)
        dgamma, dbeta = torch.empty(C, device=d), torch.empty(C, device=d)
        dy, dwc4 = ops.bn_backward_classify(dl4.view(n, h, w, 4).to(d), wc4.to(d), yd, coef, self.gamma.to(d), self.training,
                                            dgamma, dbeta, planes)
        return logits.view(self.m, 4), dy, dwc4, dgamma, dbeta


FOLD_CASES = {
    # production: deeplabv3plus at 513 x 513, batch 16 (stride-4 map 129 x 129) -- tile caps of colstat / plan_rows / the apply grid
    "prod_train": ((16, 129, 129, C), 2, True, True),
    "prod_eval": ((16, 129, 129, C), 2, False, True),
    "os8_769": ((2, 193, 193, C), 2, True, True),       # the stride-4 map of the 769 x 769 output-stride-8 configuration
    # small and ragged row counts, classifier variants
    "m1_eval": ((1, 1, 1, C), 3, False, True),
    "m7": ((1, 1, 7, C), 1, True, True),
    "m8": ((1, 1, 8, C), 2, True, False),
    "m9": ((1, 1, 9, C), 3, True, True),
    "m33": ((1, 3, 11, C), 4, True, True),
    "m4097": ((1, 17, 241, C), 4, True, False),
    "k1": ((2, 33, 33, C), 1, True, True),
    "k3_nobias": ((2, 33, 33, C), 3, True, False),
    "k4_eval_nobias": ((2, 33, 33, C), 4, False, False),
}


@functools.lru_cache(maxsize=1)           # the conv-math variants of a case run back to back: one float64 evaluation
def fold_case(tag, ld=C):
    shape, k, training, bias = FOLD_CASES[tag]
    return FoldCase(shape, k, training, bias, seed=len(tag) * 31 + shape[1], ld=ld)


def check_fold(case, d, report=""):
    """the fold against float64 at the bounds of test_folded_classifier_kernels_vs_float64; under bf16x6 the pre-split dy joins to
    the fp32 dy bit for bit"""
    from iswm_amd import ops
    logits, dy, dwc4, dgamma, dbeta = case.run(d, False)
    k = case.k
    errs = dict(logits=rel_err(logits[:, :k].cpu(), case.logits), dwc4=rel_err(dwc4[:k].cpu(), case.dwc),
                dgamma=rel_err(dgamma.cpu(), case.dgamma), dbeta=rel_err(dbeta.cpu(), case.dbeta),
                dy=case.dy_err(dy.view(case.m, C).cpu()))
    import os
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write("fold %s: %s\n" % (report, "  ".join("%s %.2e" % kv for kv in errs.items())))
    for key in ("logits", "dwc4", "dgamma", "dbeta"):
        assert errs[key] < 2e-6, (key, errs)
    assert errs["dy"] < 5e-6, errs
    assert not logits[:, k:].any() and not dwc4[k:].any()              # zero-padded classes: zero weights, zero bias
    if ops.nplanes() == 3:                          # bf16x6: the data gradient kernels take dy pre-split (exactly)
        _, dyp, dwc4p, dgp, dbp = case.run(d, True)
        assert torch.equal(ops.as_f32(dyp), dy) and torch.equal(dwc4p, dwc4) and torch.equal(dgp, dgamma) and torch.equal(dbp, dbeta)


@pytest.mark.gpu
@pytest.mark.parametrize("conv_math", [1, 0], ids=["bf16x6", "f32mfma"], indirect=True)
@pytest.mark.parametrize("tag", list(FOLD_CASES))
def test_folded_classifier_shapes_vs_float64(tag, conv_math):
    """the folded kernels at production shapes (266 256 and 74 498 rows: the 1024-tile cap of iswm_colstat_tiles, the 4096-block cap
    of the apply grid, plan_rows' row-block caps), at 1 / 7 / 8 / 9 / 33 / 4097 rows, with 1 - 4 classes and without a bias, against
    the float64 restatement (FoldCase)"""
    check_fold(fold_case(tag), dev(), "%s math %d" % (tag, conv_math))


@pytest.mark.gpu
def test_folded_classifier_strided_rows_vs_float64():
    """y a 256-channel slice of a 320-channel buffer (row pitch 320, cls_shape_ok takes any ldy % 4 == 0 >= 256): same results"""
    case = fold_case("k1", ld=320)
    assert case.device_y(dev()).stride(2) == 320
    check_fold(case, dev(), "strided ld 320")


@pytest.mark.gpu
def test_folded_dy_formats_bit_exact():
    """the backward's dy stores: under bf16x6 the three planes join to the fp32 dy bit for bit; under conv math "bf16" the single
    plane is the fp32 dy rounded to nearest even (torch's .bfloat16()) bit for bit"""
    from iswm_amd import _lib, ops
    lib = _lib.load()
    d = dev()
    case = fold_case("k3_nobias")
    old = lib.iswm_get_conv_math()
    try:
        for math, nplanes in ((1, 3), (2, 1)):
            lib.iswm_set_conv_math(math)
            dy = case.run(d, False)[1]
            dyp = case.run(d, True)[1]
            assert ops.is_planes(dyp) and dyp.t.shape[0] == nplanes, math
            if nplanes == 3:
                assert torch.equal(ops.as_f32(dyp), dy)
            else:
                want = dy.to(torch.bfloat16)
                assert torch.equal(dyp.t[0].view(torch.int16), want.view(torch.int16)), \
                    int((dyp.t[0].view(torch.int16) != want.view(torch.int16)).sum())
                assert not torch.equal(want.float(), dy)         # the data are not all bf16-representable
    finally:
        lib.iswm_set_conv_math(old)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,k,training", [((2, 9, 11, 256), 2, True), ((3, 33, 33, 256), 3, True), ((1, 7, 5, 256), 4, False)])
def test_folded_classifier_kernels_vs_float64(shape, k, training):
    from iswm_amd import ops
    d = dev()
    g = torch.Generator().manual_seed(7)
    n, h, w, c = shape
    y = torch.randn(shape, generator=g)
    gamma, beta = torch.rand(c, generator=g) + 0.5, torch.randn(c, generator=g) * 0.3
    wc = torch.randn(k, c, generator=g) * 0.1
    bias = torch.randn(k, generator=g)
    dl = torch.randn(n, h, w, k, generator=g)
    # float64 reference: BatchNorm (batch or running statistics) -> ReLU -> 1x1 conv
    y64 = y.double().requires_grad_(True)
    g64, b64, w64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True), wc.double().requires_grad_(True)
    if training:
        mean, var = y64.mean((0, 1, 2)), y64.var((0, 1, 2), unbiased=False)
    else:
        mean, var = torch.randn(c, generator=g).double() * 0.1, (torch.rand(c, generator=g) + 0.5).double()
    inv = 1.0 / torch.sqrt(var + 1e-5)
    act = F.relu((y64 - mean) * inv * g64 + b64)
    lg = act @ w64.t() + bias.double()
    lg.backward(dl.double())
    # HIP: coefficients as bn_finalize would give them (scale, shift, mean, invstd)
    coef = torch.stack([(g64 * inv).detach().float(), beta, mean.detach().float(), inv.detach().float()]).to(d).contiguous()
    wc4 = torch.zeros(4, c)
    wc4[:k] = wc
    b4 = torch.zeros(4)
    b4[:k] = bias
    yd = y.to(d)
    logits = ops.bn_apply_classify(yd, coef, wc4.to(d), b4.to(d))
    assert rel_err(logits[..., :k].cpu(), lg.detach()) < 2e-6
    assert torch.equal(logits[..., k:].cpu(), b4[k:].expand(n, h, w, 4 - k))
    dl4 = torch.zeros(n, h, w, 4)
    dl4[..., :k] = dl
    dgamma, dbeta = torch.empty(c, device=d), torch.empty(c, device=d)
    for planes in (False, True):
        dy, dwc4 = ops.bn_backward_classify(dl4.to(d), wc4.to(d), yd, coef, gamma.to(d), training, dgamma, dbeta, planes)
        dyf = ops.as_f32(dy)
        assert rel_err(dyf.cpu(), y64.grad) < 5e-6, planes
        assert rel_err(dwc4[:k].cpu(), w64.grad) < 2e-6
        assert not dwc4[k:].any()
        assert rel_err(dgamma.cpu(), g64.grad) < 2e-6 and rel_err(dbeta.cpu(), b64.grad) < 2e-6


@pytest.mark.gpu
def test_folded_head_equals_unfolded_head():
    """DeepLabHeadV3Plus forward + backward with the classifier folded vs as a conv of its own: logits and every gradient"""
    from iswm_amd.network import _deeplab, _hip
    d = dev()
    torch.manual_seed(3)
    head = _deeplab.DeepLabHeadV3Plus(2048, 256, 2, [6, 12, 18]).to(d).train()
    head.aspp.project[3].p = 0.0                     # nn.Dropout(0.1): the two passes must see the same activations
    feats = {"low_level": torch.randn(2, 256, 33, 33, device=d), "out": torch.randn(2, 2048, 9, 9, device=d)}
    dy = torch.randn(2, 2, 33, 33, device=d)
    res = []
    for fold in (True, False):
        _hip._CLS_FUSE = fold
        for p in head.parameters():
            p.grad = None
        f = {k: v.clone().requires_grad_(True) for k, v in feats.items()}
        sd = {k: v.clone() for k, v in head.state_dict().items()}
        out = head(f)
        out.backward(dy)
        res.append((out.detach().clone(), {k: p.grad.detach().clone() for k, p in head.named_parameters()},
                    {k: v.grad.detach().clone() for k, v in f.items()}))
        head.load_state_dict(sd)                      # same running statistics for the second pass
    _hip._CLS_FUSE = True
    (o1, g1, x1), (o0, g0, x0) = res
    assert rel_err(o1, o0) < 5e-6
    for k in g0:
        assert rel_err(g1[k], g0[k]) < 2e-5, k
    for k in x0:
        assert rel_err(x1[k], x0[k]) < 2e-5, k
