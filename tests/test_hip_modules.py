"""Module- and model-level parity of the HIP path (iswm_amd.network, through the
reference's construction API) against the golden vectors produced by the reference's
own modules and against the CPU oracle on the same seeded inputs.

Tolerance: 1e-3 relative fp32 (BASELINE.json north_star), argmax masks bit-exact.

How gradients are compared.  Forward results are compared element-wise.  A gradient passes
through every ReLU's sign pattern, and two fp32 implementations legitimately disagree on the
sign of the ~1e-6 fraction of pre-activations that are within rounding of zero (the same
near-tie effect as argmax flips); with a few hundred pixels per channel one flipped ReLU
moves that channel's gradients by O(1/pixels).  So:
  * ``same-mask`` checks hand the HIP path's recorded ReLU sign patterns to the CPU oracle
    (oracle.relu_masks) and require ELEMENT-WISE 1e-3 agreement of every gradient, plus that
    every sign disagreement is a true near-tie (|pre-activation| <= 1e-3 of the site's scale,
    i.e. inside the forward tolerance)
    and that they are rare (<= 1e-4 of the elements);
  * against the reference-generated golden gradients (own sign patterns on both sides) the
    relative L2 error must be <= 5e-2 (tests/util.robust_err explains why not element-wise);
    the oracle itself is pinned to those golden gradients on the CPU at 1e-4
    (tests/test_oracle_golden.py), which closes the chain reference -> oracle -> HIP.
"""
from collections import OrderedDict

import numpy as np
import pytest
import torch

from tests.util import RTOL, check, check_grad_robust, check_robust, load, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(params=[1, 0], ids=["bf16x6", "f32mfma"], autouse=True)
def conv_math(request):
    """every module/model parity test runs under both conv arithmetics (default bf16x6, and exact fp32 MFMA)"""
    from iswm_amd import _lib
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    lib.iswm_set_conv_math(request.param)
    yield request.param
    lib.iswm_set_conv_math(old)


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def load_sd(module, sd, prefix):
    own = module.state_dict()
    mapped = OrderedDict((k, sd[prefix + k]) for k in own)
    module.load_state_dict(mapped, strict=True)
    return module.to(dev())


def upstream(shape, seed):
    from oracle.make_golden import upstream as up
    return up(shape, seed)


class record_masks:
    """context manager: collect the HIP path's ReLU sign patterns keyed like the oracle's sites"""

    def __init__(self, module, prefix):
        self.module, self.prefix, self.rec = module, prefix, {}

    def __enter__(self):
        from iswm_amd.network import _hip
        self.pools = {}
        _hip.MASK_RECORDER, _hip.POOL_RECORDER = self.rec, self.pools
        return self

    def __exit__(self, *a):
        from iswm_amd.network import _hip
        _hip.MASK_RECORDER = _hip.POOL_RECORDER = None

    def masks(self):
        names = {m: n for n, m in self.module.named_modules()}
        return {self.prefix + names[bn]: v.permute(0, 3, 1, 2).cpu() for bn, v in self.rec.items()}

    def apply_to(self, o):
        """hand the oracle this path's ReLU sign patterns and (whole models) the stem max-pool's window choices, and make it
        record its pre-activations; check_sign_patterns() then verifies that every imposed decision is a near-tie"""
        o.relu_masks, o.preact = self.masks(), {}
        if self.pools:
            o.pool_index = next(iter(self.pools.values())).permute(0, 3, 1, 2).cpu()


class spy_calls:
    """context manager: every library entry point called through ops.call while it is open, as (name, arguments with each
    pointer replaced by "P") -- what ran, in order, independent of where torch's allocator put the tensors"""

    def __enter__(self):
        import ctypes
        from iswm_amd import ops
        self.ops, self.real, self.seq = ops, ops.call, []

        def arg(a):
            if a is None or isinstance(a, (int, float)):
                return a
            return "P" if isinstance(a, ctypes.c_void_p) else type(a).__name__

        def spy(name, *a):
            self.seq.append((name,) + tuple(arg(x) for x in a))
            return self.real(name, *a)
        ops.call = spy
        return self

    def __exit__(self, *a):
        self.ops.call = self.real

    def count(self, name):
        return sum(1 for c in self.seq if c[0] == name)


def assert_fold_ran(calls, steps=1):
    """the training step under comparison ran the folded classifier (csrc/bn_classify.hip), forward and backward: the same-mask
    comparisons record ReLU patterns, and before the recorder served the fold they silently took the unfolded head"""
    assert calls.count("iswm_bn_apply_classify") == steps and calls.count("iswm_bn_backward_classify") == steps, \
        (calls.count("iswm_bn_apply_classify"), calls.count("iswm_bn_backward_classify"))


def check_sign_patterns(o, masks):
    """every disagreement between the oracle's own ReLU signs and the HIP path's is a near-tie"""
    total = bad = 0
    for site, mk in masks.items():
        z = o.preact[site]
        mism = (z > 0) != mk
        total += mk.numel()
        bad += int(mism.sum())
        if mism.any():
            assert float(z[mism].abs().max()) <= RTOL * float(z.abs().max()), site
    assert bad <= max(3, 1e-4 * total), (bad, total)
    if getattr(o, "pool_index", None) is not None:
        check_pool_choices(o)
    return bad, total


POOL_GAP = 1e-5     # of max |x|: fp32 vs bf16x6 / fp32-MFMA stems put genuine near-ties at ~1e-6


def check_pool_choices(o):
    """the stem max-pool's imposed window choices are near-ties of the oracle's own maxima (gap <= POOL_GAP of max |x|) and,
    like ReLU flips, rare: at most max(3, 1e-4 of the windows) differ from the oracle's own argmax"""
    import os
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write("pool choices: gap %.3e, %d of %d windows re-routed\n" % (o.pool_gap, o.pool_moved, o.pool_windows))
    assert o.pool_gap <= POOL_GAP, o.pool_gap
    assert o.pool_moved <= max(3, 1e-4 * o.pool_windows), (o.pool_moved, o.pool_windows)


def oracle_for(sd, rates=(6, 12, 18)):
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg
    cfg = ArchCfg(output_stride=16 if tuple(rates) == (6, 12, 18) else 8)
    return OracleDeepLab(cfg, sd, dropout_p=0.0).train()


@pytest.mark.parametrize("tag,rates,hw", [("os16_17", (6, 12, 18), 17), ("os16_25", (6, 12, 18), 25),
                                          ("os8_41", (12, 24, 36), 41)])
def test_aspp(tag, rates, hw):
    from iswm_amd.network._deeplab import ASPP
    from oracle.synth import aspp_shapes, synth_from_shapes, synth_images
    fx = load("aspp_%s.npz" % tag)
    sd = synth_from_shapes(aspp_shapes("aspp", 64))
    m = load_sd(ASPP(64, list(rates)), sd, "aspp.")
    m.project[3].p = 0.0
    x = synth_images(2, hw, hw, seed=11, c=64)
    m.eval()
    with torch.no_grad():
        check(m(x.to(dev())), fx, "eval_out")
    m.train()
    xg = x.to(dev()).requires_grad_(True)
    with record_masks(m, "aspp.") as rec:
        y = m(xg)
    check(y, fx, "train_out")
    up = upstream(y.shape, 5)
    (y * up.to(dev())).sum().backward()
    for k in fx.files:
        if k.startswith("buf."):
            assert rel_err(m.state_dict()[k[4:]], fx[k]) <= RTOL, k
    # golden gradients from the reference (own sign patterns): robust metric
    check_robust(xg.grad, fx, "grad_x")
    for k, p in m.named_parameters():
        check_grad_robust(p.grad, fx, "grad." + k)
    # same-mask: element-wise 1e-3 against the oracle
    o = oracle_for(sd, rates)
    rec.apply_to(o)
    xo = x.clone().requires_grad_(True)
    yo = o.aspp(xo, "aspp")
    (yo * up).sum().backward()
    check_sign_patterns(o, o.relu_masks)
    assert rel_err(y, yo.detach()) <= RTOL
    assert rel_err(xg.grad, xo.grad) <= RTOL
    for k, p in m.named_parameters():
        assert rel_err(p.grad, o.sd["aspp." + k].grad) <= RTOL, k


def test_head_v3plus():
    from iswm_amd.network._deeplab import DeepLabHeadV3Plus
    from oracle.synth import head_v3plus_shapes, synth_from_shapes, synth_images
    fx = load("head_v3plus.npz")
    sd = synth_from_shapes(head_v3plus_shapes("classifier", 64, 16, 2))
    m = load_sd(DeepLabHeadV3Plus(64, 16, 2, [6, 12, 18]), sd, "classifier.")
    m.aspp.project[3].p = 0.0
    low = synth_images(2, 65, 65, seed=21, c=16)
    hi = synth_images(2, 17, 17, seed=22, c=64)
    m.eval()
    with torch.no_grad():
        check(m({"low_level": low.to(dev()), "out": hi.to(dev())}), fx, "eval_out")
    m.train()
    lg, hg = low.to(dev()).requires_grad_(True), hi.to(dev()).requires_grad_(True)
    with record_masks(m, "classifier.") as rec:
        y = m({"low_level": lg, "out": hg})
    check(y, fx, "train_out")
    up = upstream(y.shape, 6)
    (y * up.to(dev())).sum().backward()
    check_robust(lg.grad, fx, "grad_low")
    check_robust(hg.grad, fx, "grad_out")
    for k, p in m.named_parameters():
        check_grad_robust(p.grad, fx, "grad." + k)
    o = oracle_for(sd)
    rec.apply_to(o)
    lo_, ho_ = low.clone().requires_grad_(True), hi.clone().requires_grad_(True)
    yo = o.head({"low_level": lo_, "out": ho_})
    (yo * up).sum().backward()
    check_sign_patterns(o, o.relu_masks)
    assert rel_err(lg.grad, lo_.grad) <= RTOL and rel_err(hg.grad, ho_.grad) <= RTOL
    for k, p in m.named_parameters():
        assert rel_err(p.grad, o.sd["classifier." + k].grad) <= RTOL, k


def test_bottleneck():
    from iswm_amd.network import _hip
    from iswm_amd.network.backbone import resnet
    from oracle.make_golden import BOTTLENECK_CASES
    from oracle.synth import bottleneck_shapes, synth_from_shapes, synth_images
    import torch.nn as nn
    fx = load("bottleneck.npz")
    for tag, (inpl, pl, s, d, down, hw) in BOTTLENECK_CASES.items():
        ds = nn.Sequential(resnet.conv1x1(inpl, pl * 4, s), _hip.BatchNorm2d(pl * 4)) if down else None
        sd = synth_from_shapes(bottleneck_shapes("block", inpl, pl, down))
        m = load_sd(resnet.Bottleneck(inpl, pl, s, ds, 1, 64, d), sd, "block.")
        x = synth_images(2, hw, hw, seed=31, c=inpl)
        m.eval()
        with torch.no_grad():
            check(m(x.to(dev())), fx, tag + ".eval_out")
        m.train()
        xg = x.to(dev()).requires_grad_(True)
        with record_masks(m, "block.") as rec:
            y = m(xg)
        check(y, fx, tag + ".train_out")
        up = upstream(y.shape, 7)
        (y * up.to(dev())).sum().backward()
        check_robust(xg.grad, fx, tag + ".grad_x")
        for k, p in m.named_parameters():
            check_grad_robust(p.grad, fx, tag + ".grad." + k)
        for k in fx.files:
            if k.startswith(tag + ".buf."):
                assert rel_err(m.state_dict()[k[len(tag) + 5:]], fx[k]) <= RTOL, k
        o = oracle_for(sd)
        rec.apply_to(o)
        xo = x.clone().requires_grad_(True)
        yo = o._bottleneck(xo, "block", s, d, down)
        (yo * up).sum().backward()
        check_sign_patterns(o, o.relu_masks)
        assert rel_err(xg.grad, xo.grad) <= RTOL, tag
        for k, p in m.named_parameters():
            assert rel_err(p.grad, o.sd["block." + k].grad) <= RTOL, (tag, k)


def _build(backbone, os_, num_classes=2):
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    cfg = ArchCfg("deeplabv3plus", backbone, num_classes, os_)
    m = modeling._segm_resnet("deeplabv3plus", backbone, num_classes, os_, False)
    sd = synth_state_dict(cfg)
    assert list(m.state_dict().keys()) == list(sd.keys())         # drop-in key layout (374 / 680 keys)
    m.load_state_dict(sd, strict=True)
    m.classifier.aspp.project[3].p = 0.0
    return m.to(dev()), cfg, sd


@pytest.mark.parametrize("tag,backbone,os_,fold", [
    pytest.param("r50_os16", "resnet50", 16, True, id="r50_os16-resnet50-16"),
    pytest.param("r50_os16", "resnet50", 16, False, id="r50_os16-resnet50-16-unfolded"),
    pytest.param("r101_os8", "resnet101", 8, True, id="r101_os8-resnet101-8")])
def test_whole_model(tag, backbone, os_, fold):
    """logits, bit-exact argmax mask, loss, gradients and BN running stats of one training
    step on [2,3,65,65] vs the reference's _segm_resnet + nn.CrossEntropyLoss(weight).  The training step runs the folded
    classifier (the product's step); `unfolded` pins the classifier as a conv of its own (_hip._CLS_FUSE = False)."""
    from iswm_amd.network import _hip
    try:
        _hip._CLS_FUSE = fold
        _whole_model(tag, backbone, os_, fold)
    finally:
        _hip._CLS_FUSE = True


def _whole_model(tag, backbone, os_, fold):
    from iswm_amd import ops
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.make_golden import WATCH
    from oracle.synth import synth_images
    from oracle.make_golden import model_input, model_state
    fx = load("model_%s.npz" % tag)
    m, cfg, sd = _build(backbone, os_)
    sd = model_state(tag, cfg)
    m.load_state_dict(sd, strict=True)
    x = model_input(tag)[0]
    labels = torch.from_numpy(fx["labels"].astype(np.int64))
    m.eval()
    with torch.no_grad():
        lg = m(x.to(dev()))
    assert rel_err(lg, fx["eval_logits"]) <= RTOL
    mask = ops.argmax_nchw(lg).cpu().numpy()
    margin = np.abs(fx["eval_logits"][:, 1] - fx["eval_logits"][:, 0])
    sure = margin > 2 * RTOL * np.abs(fx["eval_logits"]).max()       # pixels that are not near-ties
    assert sure.mean() > 0.95
    assert (mask[sure] == fx["eval_mask"][sure]).all()
    assert torch.equal(ops.argmax_nchw(lg).cpu(), lg.cpu().max(1)[1])   # the argmax kernel itself: bit-exact
    m.train()
    with record_masks(m, "") as rec:
        lg = m(x.to(dev()))
    # plain RTOL against the reference's own train-mode logits (the os8 case runs on 4 x 97 x 97 so that its BatchNorm
    # layers see 676 values per channel: oracle/make_golden.py MODEL_INPUT) ...
    assert rel_err(lg, fx["train_logits"]) <= RTOL
    # ... and, as an extra, against the float64 evaluation of the same graph
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    with torch.no_grad():
        ref64 = OracleDeepLab(cfg, sd64, dropout_p=0.0).train()(x.double())
    assert rel_err(lg, ref64) <= RTOL
    w = torch.tensor([1.0, 3.0])
    loss = CrossEntropyLoss(weight=w, ignore_index=255)(lg, labels.to(dev()))
    assert rel_err(loss, fx["loss"]) <= RTOL
    for k in fx.files:
        if k.startswith("buf."):
            assert rel_err(m.state_dict()[k[4:]], fx[k]) <= RTOL, k
    # Backward of the whole network, element-wise, every parameter: both sides get the SAME upstream
    # dL/dlogits and the same ReLU sign patterns, so what is compared is the backward arithmetic
    # (dgrad/wgrad/BN/pool/bilinear backward through 50-100 layers), not the forward's 1e-4
    # logit differences re-entering through softmax.  (The criterion's own gradient is checked
    # against the reference's golden vectors in test_hip_kernels.py::test_loss_golden.)
    # Batch 8 here: with the golden case's batch of 2 the ASPP image-pooling BatchNorm normalises
    # over TWO values per channel, where dy cancels to eps/(var+eps) of its terms (xhat = +-a exactly)
    # and any fp32 implementation is only good to ~1e-2 on that branch's contribution.
    m.load_state_dict(sd, strict=True)
    x4 = synth_images(8, 65, 65, seed=72)
    with spy_calls() as calls:
        with record_masks(m, "") as rec:
            lg4 = m(x4.to(dev()))
        for p in m.parameters():
            p.grad = None
        up = upstream(lg4.shape, 12)
        lg4.backward(up.to(dev()))
    if fold:
        assert_fold_ran(calls)
    else:
        assert calls.count("iswm_bn_apply_classify") == 0 and calls.count("iswm_bn_backward_classify") == 0
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).train()
    rec.apply_to(o)
    lgo = o(x4)
    assert rel_err(lg4, lgo.detach()) <= RTOL
    lgo.backward(up)
    check_sign_patterns(o, o.relu_masks)
    params = dict(m.named_parameters())
    worst = max((rel_err(params[k].grad, v.grad), k) for k, v in o.named_parameters())
    # 3e-3: the saved activations that enter every weight gradient already differ by up to 1e-3 (the
    # forward tolerance) after 50-100 train-mode BatchNorm layers on a 5x5 / 9x9 map
    assert worst[0] <= 3 * RTOL, worst


def test_train_steps_match_oracle():
    """three full SGD-nesterov steps (the train.py:1045-1049 sequence: forward, weighted CE,
    zero_grad, backward, step; torch's default lr 1e-3 as train.py:426-432 uses it) from the same
    initial state: HIP path vs CPU oracle.  Compared: the loss of every step (1e-3), the parameter
    UPDATES after three steps (1e-2 of the tensor's update scale -- the loss gradient inherits the
    forward's ~3e-4 logit differences through softmax -- plus 4 ulp of the parameter itself) and the
    BatchNorm running statistics (1e-3)."""
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.optim import OracleSGD
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    # residual branches damped (bn3.weight x 0.3, as oracle/make_golden.py does for its r101 case and for the same reason): with
    # the synthetic rule's gamma ~ 1 on all 16 residual branches the THREE-step comparison of the stem's update -- the
    # quantity at the far end of every chain in the graph -- moved between 2.9e-3 and 1.1e-2 under changes of summation
    # order alone (fused / per-branch ASPP, fused / stand-alone bn3 reduction: profiles/r03_train_steps_sensitivity.txt)
    sd = {k: (v * 0.3 if k.endswith(".bn3.weight") else v) for k, v in sd.items()}
    m.load_state_dict(sd, strict=True)
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).train()
    lr = 1e-3
    oopt = OracleSGD(o.parameters(), lr=lr)
    opt = FusedSGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True)
    w = torch.tensor([1.0, 3.0])
    crit = CrossEntropyLoss(weight=w)
    m.train()
    for it in range(3):
        x = synth_images(6, 81, 81, seed=100 + it)      # batch 6: see the image-pooling note above
        lab = synth_labels(6, 81, 81, seed=100 + it, p_fg=0.2, p_ignore=0.05)
        with spy_calls() as calls:
            with record_masks(m, "") as rec:
                lg = m(x.to(dev()))
            l = crit(lg, lab.to(dev()))
            opt.zero_grad()
            l.backward()
        assert_fold_ran(calls)
        opt.step()
        rec.apply_to(o)
        lo = oloss.weighted_ce(o(x), lab, w)
        o.zero_grad()
        lo.backward()
        oopt.step()
        assert rel_err(l, lo.detach()) <= RTOL, it
    osd = o.state_dict()
    msd = m.state_dict()
    worst_u, worst_b = (0.0, ""), (0.0, "")
    for k in osd:
        if not osd[k].is_floating_point():
            continue
        if "running_" in k:
            worst_b = max(worst_b, (rel_err(msd[k], osd[k]), k))
        else:
            du_h, du_o = (msd[k].cpu() - sd[k]).double(), (osd[k] - sd[k]).double()
            slack = 4 * 1.2e-7 * float(sd[k].abs().max())
            err = max(0.0, float((du_h - du_o).abs().max()) - slack) / float(du_o.abs().max())
            worst_u = max(worst_u, (err, k))
    import os
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write("train_steps: worst update err %.4e (%s), worst buffer err %.3e (%s)\n" % (worst_u + worst_b))
    assert worst_b[0] <= RTOL, worst_b
    assert worst_u[0] <= 1e-2, worst_u
    assert int(msd["backbone.bn1.num_batches_tracked"]) == 3


def test_train_steps_undamped_vs_float64():
    """test_train_steps_match_oracle's three SGD-nesterov steps WITHOUT its bn3 damping -- gamma ~ 1 on every residual branch,
    torchvision's default initialisation and the ill-conditioned case -- against a float64 oracle, with an fp32 oracle as the
    yardstick; both oracles follow the HIP path's ReLU patterns and max-pool choices at every step.  Every step's loss and the
    BatchNorm buffers within 1e-3 of float64; per parameter tensor, the HIP update's error against float64 at most
    3 x max(the fp32 oracle's, 1e-3): no worse than a plain fp32 evaluation of the same steps.  Measured on an MI355X (bf16x6 /
    fp32 MFMA): loss 3.0e-5 / 1.0e-5, buffers 9.6e-5 / 8.0e-5, worst update error 1.19e-3 / 1.57e-3 against the fp32 oracle's
    9.8e-4 / 1.53e-3, worst ratio to max(fp32, 1e-3) 1.19 / 1.38."""
    import os
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.optim import OracleSGD
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    o32, o64 = OracleDeepLab(cfg, sd, dropout_p=0.0).train(), OracleDeepLab(cfg, sd64, dropout_p=0.0).train()
    lr = 1e-3
    opt32, opt64 = OracleSGD(o32.parameters(), lr=lr), OracleSGD(o64.parameters(), lr=lr)
    opt = FusedSGD(m.parameters(), lr=lr, momentum=0.9, weight_decay=1e-4, nesterov=True)
    w = torch.tensor([1.0, 3.0])
    crit = CrossEntropyLoss(weight=w)
    m.train()
    loss_err = 0.0
    for it in range(3):
        x = synth_images(6, 81, 81, seed=100 + it)
        lab = synth_labels(6, 81, 81, seed=100 + it, p_fg=0.2, p_ignore=0.05)
        with spy_calls() as calls:
            with record_masks(m, "") as rec:
                lg = m(x.to(dev()))
            l = crit(lg, lab.to(dev()))
            opt.zero_grad()
            l.backward()
        assert_fold_ran(calls)
        opt.step()
        for o, oopt, xx, ww in ((o32, opt32, x, w), (o64, opt64, x.double(), w.double())):
            rec.apply_to(o)
            lo = oloss.weighted_ce(o(xx), lab, ww)
            o.zero_grad()
            lo.backward()
            oopt.step()
        # (no near-tie rule on the imposed patterns here: undamped, two fp32 evaluations of the decoder's last stage already
        # differ by ~2e-3 of its scale after the first update -- the ill-conditioning this test is about)
        loss_err = max(loss_err, rel_err(l, lo.detach()))
    s32, s64, sh = o32.state_dict(), o64.state_dict(), m.state_dict()
    worst_b, worst_h, worst_32, worst_r = (0.0, ""), (0.0, ""), (0.0, ""), (0.0, "")
    for k in s64:
        if not s64[k].is_floating_point():
            continue
        if "running_" in k:
            worst_b = max(worst_b, (rel_err(sh[k], s64[k]), k))
            continue
        du64 = s64[k] - sd64[k]
        slack = 4 * 1.2e-7 * float(sd[k].abs().max())          # the fp32 parameters' own rounding
        def err(p):
            return max(0.0, float((p.cpu().double() - sd64[k] - du64).abs().max()) - slack) / float(du64.abs().max())
        eh, e32 = err(sh[k]), err(s32[k])
        worst_h, worst_32 = max(worst_h, (eh, k)), max(worst_32, (e32, k))
        worst_r = max(worst_r, (eh / max(e32, 1e-3), k))
    if os.environ.get("ISWM_TEST_REPORT"):
        with open(os.environ["ISWM_TEST_REPORT"], "a") as f:
            f.write("undamped steps vs fp64: loss %.2e, buffers %.2e (%s), update err hip %.3e (%s) fp32 oracle %.3e (%s), "
                    "worst hip / max(fp32, 1e-3) %.3f (%s)\n" % ((loss_err,) + worst_b + worst_h + worst_32 + worst_r))
    assert loss_err <= RTOL, loss_err
    assert worst_b[0] <= RTOL, worst_b
    assert worst_r[0] <= 3.0, (worst_r, worst_h, worst_32)
    assert int(sh["backbone.bn1.num_batches_tracked"]) == 3


def test_mask_recorder_leaves_the_step_alone():
    """the same-mask recorder does not change what a training step runs: with MASK_RECORDER / POOL_RECORDER set, the library calls
    of one forward + loss + backward are the plain step's, in order and with the same arguments, plus one iswm_bn_apply_pl (ReLU,
    fp32 out, no residual) right after the folded classifier's forward -- the pattern it records -- and the recorder's reads of
    pre-split stage outputs (iswm_join_planes)"""
    from iswm_amd.network import _hip
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    m.train()
    x = synth_images(4, 65, 65, seed=41).to(dev())
    lab = synth_labels(4, 65, 65, seed=41, p_fg=0.2).to(dev())
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))

    def step(record):
        for p in m.parameters():
            p.grad = None
        rec = {}
        with spy_calls() as calls:
            _hip.MASK_RECORDER, _hip.POOL_RECORDER = (rec, {}) if record else (None, None)
            try:
                lg = m(x)
            finally:
                _hip.MASK_RECORDER = _hip.POOL_RECORDER = None
            crit(lg, lab).backward()
        torch.cuda.synchronize()
        return calls.seq, rec
    step(False)                                   # one-time setup (weight packing, plans) out of the comparison
    plain, _ = step(False)
    recorded, masks = step(True)
    assert step(False)[0] == plain
    folds = [j + 1 for j, c in enumerate(recorded) if c[0] == "iswm_bn_apply_classify"]
    assert len(folds) == 1 and m.classifier.classifier[1] in masks
    for j in folds:
        # iswm_bn_apply_pl(y, M, C, ldy, scale, shift, mean, residual None, 0, 0, relu 1, out, ldo C, plane stride 0, stream)
        assert recorded[j][:5] == ("iswm_bn_apply_pl",) + recorded[j - 1][1:5], (recorded[j - 1], recorded[j])
        assert recorded[j][8:] == (None, 0, 0, 1, "P", 256, 0, "P"), recorded[j]
    i = 0
    for c in (c for j, c in enumerate(recorded) if j not in folds):
        if i < len(plain) and c == plain[i]:
            i += 1
        else:
            assert c[0] == "iswm_join_planes", (i, c)
    assert i == len(plain)
    mk = masks[m.classifier.classifier[1]]
    assert mk.dtype == torch.bool and mk.shape == (4, 17, 17, 256) and 0.2 < float(mk.float().mean()) < 0.8


def test_full_size_step_vs_oracle():
    """BASELINE.json configs[1] geometry (deeplabv3plus_resnet50, output_stride 16, 513 x 513) against the CPU oracle at
    FULL size: eval logits, train logits and weighted-CE loss element-wise at 1e-3, and every parameter gradient
    element-wise at 3e-3 with the oracle's ReLUs following this path's recorded sign patterns (same-mask; the docstring
    of this file says why).  Batch 4, not 2: the ASPP image-pooling BatchNorm normalises over `batch` values per channel
    and is ill-conditioned at two (test_whole_model).  At this size the production tile planners run (129 x 129, 65 x 65
    and 33 x 33 maps: > 256 tiles per launch, multi-split weight gradients, parity-ordered strided data gradients)."""
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    x = synth_images(4, 513, 513, seed=31)
    lab = synth_labels(4, 513, 513, seed=31, p_fg=0.1, p_ignore=0.02)
    w = torch.tensor([1.0, 3.0])
    m.eval()
    with torch.no_grad():
        lg_e = m(x[:2].to(dev())).cpu()
        ref_e = OracleDeepLab(cfg, sd, dropout_p=0.0).eval()(x[:2])
    assert rel_err(lg_e, ref_e) <= RTOL
    del lg_e, ref_e
    m.train()
    with spy_calls() as calls:
        with record_masks(m, "") as rec:
            lg = m(x.to(dev()))
        loss = CrossEntropyLoss(weight=w, ignore_index=255)(lg, lab.to(dev()))
        for p in m.parameters():
            p.grad = None
        loss.backward()
    assert_fold_ran(calls)                # M = 4 x 129 x 129: the fold's 1024-tile cap is reached end to end
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).train()
    rec.apply_to(o)
    lgo = o(x)
    assert rel_err(lg, lgo.detach()) <= RTOL
    lo = oloss.weighted_ce(lgo, lab, w)
    assert rel_err(loss, lo.detach()) <= RTOL
    lo.backward()
    check_sign_patterns(o, o.relu_masks)
    params = dict(m.named_parameters())
    worst = max((rel_err(params[k].grad, v.grad), k) for k, v in o.named_parameters())
    assert worst[0] <= 3 * RTOL, worst
    msd = m.state_dict()
    for k, v in o.state_dict().items():
        if "running_" in k:
            assert rel_err(msd[k], v) <= RTOL, k


def test_full_size_properties():
    """513x513 (BASELINE size), batch 2, resnet50: size-independent properties --
    finite logits of the right shape, bit-identical repeat of logits and gradients (no atomics
    anywhere), and the argmax kernel agrees bit-exactly with logits.max(1)[1]."""
    from iswm_amd import ops
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    x = synth_images(2, 513, 513, seed=5).to(dev())
    lab = synth_labels(2, 513, 513, seed=5).to(dev())
    m.train()
    outs = []
    for rep in range(2):
        m.load_state_dict(sd, strict=True)
        lg = m(x)
        assert lg.shape == (2, 2, 513, 513) and bool(torch.isfinite(lg).all())
        loss = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))(lg, lab)
        for p in m.parameters():
            p.grad = None
        loss.backward()
        outs.append((lg.detach().clone(), m.backbone.conv1.weight.grad.clone(),
                     m.classifier.classifier[6].weight.grad.clone()))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    m.eval()
    with torch.no_grad():
        lg = m(x)
    assert torch.equal(ops.argmax_nchw(lg).cpu(), lg.cpu().max(1)[1])


@pytest.mark.parametrize("os_,size", [(8, 769), (16, 1024)], ids=["r101_os8_769", "r101_os16_1024"])
def test_baseline_large_tile_configs(os_, size):
    """BASELINE.json configs[3] / configs[4] geometry (resnet101, output_stride 8 at 769x769 with ASPP rates
    12/24/36, and output_stride 16 at 1024x1024), batch 2: one training step is finite, repeats bit-identically,
    and the two conv arithmetics agree on the loss to well under the 1e-3 contract."""
    from iswm_amd import _lib
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet101", os_)
    x = synth_images(2, size, size, seed=9).to(dev())
    lab = synth_labels(2, size, size, seed=9).to(dev())
    m.train()
    lib = _lib.load()
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))
    res = []
    for math in (lib.iswm_get_conv_math(), lib.iswm_get_conv_math(), 0):
        old = lib.iswm_get_conv_math()
        lib.iswm_set_conv_math(math)
        try:
            m.load_state_dict(sd, strict=True)
            lg = m(x)
            assert lg.shape == (2, 2, size, size) and bool(torch.isfinite(lg).all())
            loss = crit(lg, lab)
            for p in m.parameters():
                p.grad = None
            loss.backward()
            g = m.backbone.layer3[0].conv2.weight.grad
            assert bool(torch.isfinite(g).all())
            res.append((float(loss.detach()), lg.detach().clone(), g.clone()))
        finally:
            lib.iswm_set_conv_math(old)
    assert torch.equal(res[0][1], res[1][1]) and torch.equal(res[0][2], res[1][2])     # bit-identical repeat
    assert abs(res[0][0] - res[2][0]) <= 1e-4 * abs(res[2][0])                          # bf16x6 vs exact fp32 MFMA


def test_separable_conv_and_conversion():
    """AtrousSeparableConvolution and convert_to_separable_conv (network/_deeplab.py:95-119,176-188) vs vectors
    produced by the reference's own classes: same state_dict keys, forward and every gradient."""
    from iswm_amd.network import _deeplab, _hip
    from oracle.make_golden import SEPCONV_CASES
    from oracle.synth import synth_images, synth_tensor
    fx = load("sepconv.npz")
    for tag, (cin, cout, k, s, p, d, bias, h, w) in SEPCONV_CASES.items():
        m = _deeplab.AtrousSeparableConvolution(cin, cout, k, s, p, d, bias)
        pre = "sep.%s." % tag
        m.load_state_dict(OrderedDict((key, synth_tensor(pre + key, tuple(v.shape))) for key, v in m.state_dict().items()),
                          strict=True)
        m = m.to(dev())
        xg = synth_images(2, h, w, seed=31, c=cin).to(dev()).requires_grad_(True)
        y = m(xg)
        check(y, fx, tag + ".out")
        (y * upstream(y.shape, 7).to(dev())).sum().backward()
        check(xg.grad, fx, tag + ".grad_x")
        for key, prm in m.named_parameters():
            assert rel_err(prm.grad, fx["%s.grad.%s" % (tag, key)]) <= RTOL, (tag, key)
    # conversion of a conv -> BN -> ReLU stage
    m = _deeplab.convert_to_separable_conv(_deeplab.ASPPConv(32, 16, 3))
    assert isinstance(m[0], _deeplab.AtrousSeparableConvolution) and isinstance(m[0].body[0], _hip.DepthwiseConv2d)
    assert list(m.state_dict().keys()) == [str(s_) for s_ in fx["asppconv.keys"]]
    m.load_state_dict(OrderedDict((key, synth_tensor("sep.asppconv." + key, tuple(v.shape)))
                                  for key, v in m.state_dict().items()), strict=True)
    m = m.to(dev())
    x = synth_images(4, 19, 19, seed=32, c=32)
    m.eval()
    with torch.no_grad():
        check(m(x.to(dev())), fx, "asppconv.eval_out")
    m.train()
    xg = x.to(dev()).requires_grad_(True)
    y = m(xg)
    check(y, fx, "asppconv.train_out")
    (y * upstream(y.shape, 8).to(dev())).sum().backward()
    check_robust(xg.grad, fx, "asppconv.grad_x")
    for key, prm in m.named_parameters():
        check_grad_robust(prm.grad, fx, "asppconv.grad." + key)
    for key in ("1.running_mean", "1.running_var"):
        assert rel_err(m.state_dict()[key], fx["asppconv.buf." + key]) <= RTOL, key


def test_converted_head_trains():
    """network.convert_to_separable_conv(model.classifier) -- the upstream use of the function -- yields a model
    that steps: ASPP branches and both decoder 3x3s become depthwise + pointwise (decoder input stays the padded
    320-wide concat buffer), logits and all gradients finite, repeat bit-identical."""
    from iswm_amd.network import _deeplab
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    m.classifier = _deeplab.convert_to_separable_conv(m.classifier).to(dev())
    assert isinstance(m.classifier.classifier[0], _deeplab.AtrousSeparableConvolution)
    assert isinstance(m.classifier.aspp.convs[1][0], _deeplab.AtrousSeparableConvolution)
    m.classifier.aspp.project[3].p = 0.0
    x = synth_images(4, 65, 65, seed=3).to(dev())
    lab = synth_labels(4, 65, 65, seed=3).to(dev())
    m.train()
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))
    init = {k: v.clone() for k, v in m.state_dict().items()}
    outs = []
    for _ in range(2):
        m.load_state_dict(init, strict=True)
        for p in m.parameters():
            p.grad = None
        lg = m(x)
        assert lg.shape == (4, 2, 65, 65) and bool(torch.isfinite(lg).all())
        crit(lg, lab).backward()
        gs = [p.grad.clone() for p in m.parameters()]
        assert all(bool(torch.isfinite(g).all()) for g in gs) and all(float(g.abs().max()) > 0 for g in gs)
        outs.append((lg.detach().clone(), gs))
    assert torch.equal(outs[0][0], outs[1][0]) and all(torch.equal(a, b) for a, b in zip(outs[0][1], outs[1][1]))


def test_baseline_config0_plumbing_size():
    """BASELINE.json configs[0] geometry -- 256x256 two-class tiles, batch 2 (the reference has no mobilenet, SURVEY
    F1, so resnet50 as SURVEY 8d prescribes): eval logits and the training loss vs the CPU oracle on the same
    weights, argmax bit-exact away from near-ties."""
    from iswm_amd import ops
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    x = synth_images(2, 256, 256, seed=41)
    lab = synth_labels(2, 256, 256, seed=41)
    m.eval()
    with torch.no_grad():
        lg = m(x.to(dev()))
        lo = OracleDeepLab(cfg, sd, dropout_p=0.0).eval()(x)
    assert lg.shape == (2, 2, 256, 256) and rel_err(lg, lo) <= RTOL
    margin = (lo[:, 1] - lo[:, 0]).abs()
    sure = margin > 2 * RTOL * lo.abs().max()
    assert float(sure.float().mean()) > 0.95
    assert torch.equal(ops.argmax_nchw(lg).cpu()[sure], lo.max(1)[1][sure])
    m.train()
    lg = m(x.to(dev()))
    with torch.no_grad():
        lt = OracleDeepLab(cfg, sd, dropout_p=0.0).train()(x)
    w = torch.tensor([1.0, 3.0])
    assert rel_err(lg, lt) <= RTOL
    assert rel_err(CrossEntropyLoss(weight=w)(lg, lab.to(dev())), oloss.weighted_ce(lt, lab, w)) <= RTOL


def test_whole_model_v3_head_5_channel_stem():
    """the other constructor path: modeling._segm_resnet('deeplabv3', ..., in_channels=5) -- DeepLabHead (ASPP -> 3x3 ->
    1x1, network/_deeplab.py:71-93) on a 5-channel stem (network/modeling.py:25-43) -- same keys as the reference,
    logits / mask / loss vs its vectors, gradients vs the oracle under the HIP path's ReLU sign patterns"""
    from iswm_amd import ops
    from iswm_amd.network import modeling
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg, synth_images, synth_state_dict
    fx = load("model_v3_in5.npz")
    cfg = ArchCfg("deeplabv3", "resnet50", 2, 16, in_channels=5)
    sd = synth_state_dict(cfg)
    m = modeling._segm_resnet("deeplabv3", "resnet50", 2, 16, False, in_channels=5)
    assert list(m.state_dict().keys()) == [str(k) for k in fx["keys"]]
    m.load_state_dict(sd, strict=True)
    m.classifier.classifier[0].project[3].p = 0.0
    m = m.to(dev())
    x = synth_images(4, 65, 65, seed=73, c=5)
    labels = torch.from_numpy(fx["labels"].astype(np.int64))
    m.eval()
    with torch.no_grad():
        lg = m(x.to(dev()))
    assert rel_err(lg, fx["eval_logits"]) <= RTOL
    margin = np.abs(fx["eval_logits"][:, 1] - fx["eval_logits"][:, 0])
    sure = margin > 2 * RTOL * np.abs(fx["eval_logits"]).max()
    assert (ops.argmax_nchw(lg).cpu().numpy()[sure] == fx["eval_mask"][sure]).all()
    m.train()
    with spy_calls() as calls:
        with record_masks(m, "") as rec:
            lg = m(x.to(dev()))
        assert rel_err(lg, fx["train_logits"]) <= RTOL
        loss = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]), ignore_index=255)(lg, labels.to(dev()))
        assert rel_err(loss, fx["loss"]) <= RTOL
        for p in m.parameters():
            p.grad = None
        up = upstream(lg.shape, 14)
        lg.backward(up.to(dev()))
    assert_fold_ran(calls)                # DeepLabHead: ASPP -> 3x3 -> BN -> ReLU -> folded 1x1
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).train()
    rec.apply_to(o)
    lgo = o(x)
    lgo.backward(up)
    check_sign_patterns(o, o.relu_masks)
    params = dict(m.named_parameters())
    worst = max((rel_err(params[k].grad, v.grad), k) for k, v in o.named_parameters())
    assert worst[0] <= 3 * RTOL, worst


def close_up_to_bf16_ties(a, b, tol=RTOL, l2_tol=3e-3):
    """two evaluations of a stage whose OUTPUT is stored as bf16: they agree to `tol` (of the tensor's scale) before the store,
    each side then rounds to nearest bf16 -- so every element must agree to tol + one bf16 step (2^-7 of its magnitude: half a
    step per side, the steps at a binade edge differing by two), and the relative L2 distance must stay at the bf16 rounding level
    (2^-9 rms): a wrong rounding mode or a wrong value anywhere shows in one of the two.  (That the store itself IS
    round-to-nearest-even, bit for bit, is test_bf16_store_is_round_to_nearest_even.)"""
    a = a.detach().cpu().double()
    b = b.detach().cpu().double()
    d = (a - b).abs()
    scale = float(b.abs().max())
    bad = d > tol * scale + 2.0 ** -7 * torch.maximum(a.abs(), b.abs())
    assert not bool(bad.any()), "%d elements differ by more than tol + a bf16 step: worst %.3e at value %.3e (scale %.3e)" % (
        int(bad.sum()), float(d[bad].max()), float(b[bad][d[bad].argmax()]), scale)
    l2 = float((a - b).norm() / b.norm())
    assert l2 <= l2_tol, "relative L2 %.3e" % l2
    return True


def test_bf16_store_is_round_to_nearest_even():
    """conv math "bf16": what the memory-bound passes store as the single plane is x.bfloat16() bit for bit (split pass, and the
    BatchNorm apply pass against its own fp32 form rounded by torch), ties to even included"""
    from iswm_amd import _lib, ops
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    try:
        lib.iswm_set_conv_math(2)
        if not ops.planes_on():
            pytest.skip("activation planes switched off (ops._PLANES_ENV)")
        g = torch.Generator().manual_seed(3)
        x = torch.randn(2, 9, 11, 128, generator=g)
        x[0, 0, 0, :6] = torch.tensor([1.00390625, 1.01171875, -1.00390625, 3.0e38, 1e-30, 0.0])     # exact ties (to even), range ends
        xd = x.to(dev())
        p = ops.split_planes(xd)
        assert p.t.shape[0] == 1 and torch.equal(p.t[0], xd.bfloat16())
        assert torch.equal(p.f32(), xd.bfloat16().float())
        coef = torch.stack([torch.rand(128, generator=g) + 0.5, torch.randn(128, generator=g) * 0.1,
                            torch.randn(128, generator=g) * 0.1, torch.rand(128, generator=g) + 0.5]).to(dev())
        lib.iswm_set_conv_math(1)
        ref = ops.bn_apply(xd, coef, True, None)                      # fp32 output of the same kernel family
        lib.iswm_set_conv_math(2)
        o = ops.bn_apply(xd, coef, True, None, planes=True)
        assert ops.is_planes(o) and torch.equal(o.t[0], ref.bfloat16())
    finally:
        lib.iswm_set_conv_math(old)


def test_bf16_mixed_precision_mode():
    """conv math 2 (BASELINE configs[4] "bf16 mixed precision": activations between convolutions STORED as one bf16 plane,
    bf16 MFMA inputs, fp32 accumulation, fp32 BatchNorm statistics / master weights / loss / gradients of tensors).
    The reference has no such mode, so the oracle is the fp32 oracle with the SAME rounding applied to the operands of
    every conv GEMM (oracle/deeplab.py _Bf16Conv) and to every activation the product stores as planes (OracleDeepLab.act_bf16,
    straight-through gradient) -- parity with the reference itself is unpinned for this mode.
      * one stage at a time (a Bottleneck, the ASPP block: identical inputs on both sides) the usual bars hold: outputs
        1e-3, every gradient 3e-3 under the HIP path's ReLU sign patterns;
      * through the whole network two bf16 pipelines are only defined up to bf16-sized noise -- a 1e-7 difference in an
        activation flips a round-to-nearest decision (a 2^-8 jump), and that compounds over ~50 layers to ~1e-2 -- so
        logits / loss are held to 3e-2 against the same-rounding oracle and against the fp32 model, argmax agreement
        > 97 %, and repeats must be bit-identical;
      * the 1024 x 1024 tile of configs[4] runs and its loss stays within 3e-2 of the fp32 path."""
    from iswm_amd import _lib, ops
    from iswm_amd.network import _hip
    from iswm_amd.network._deeplab import ASPP
    from iswm_amd.network.backbone import resnet
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import aspp_shapes, bottleneck_shapes, synth_from_shapes, synth_images, synth_labels
    import torch.nn as nn
    lib = _lib.load()
    old = lib.iswm_get_conv_math()
    try:
        lib.iswm_set_conv_math(2)
        # ---- single stages vs the same-rounding oracle
        for inpl, pl, stride, dil, down, hw in ((64, 32, 2, 1, True, 33), (128, 32, 1, 2, False, 17)):
            ds = nn.Sequential(resnet.conv1x1(inpl, pl * 4, stride), _hip.BatchNorm2d(pl * 4)) if down else None
            bsd = synth_from_shapes(bottleneck_shapes("block", inpl, pl, down))
            blk = load_sd(resnet.Bottleneck(inpl, pl, stride, ds, 1, 64, dil), bsd, "block.").train()
            xb = synth_images(4, hw, hw, seed=31, c=inpl)
            xg = xb.to(dev()).requires_grad_(True)
            with record_masks(blk, "block.") as rec:
                y = blk(xg)
            up = upstream(y.shape, 7)
            (y * up.to(dev())).sum().backward()
            o = oracle_for(bsd)
            o.conv_math = "bf16"
            o.act_bf16 = True
            rec.apply_to(o)
            xo = xb.clone().requires_grad_(True)
            yo = o._bottleneck(xo, "block", stride, dil, down)
            assert close_up_to_bf16_ties(y, yo)
            (yo * up).sum().backward()
            assert rel_err(xg.grad, xo.grad) <= 3 * RTOL
            for k, p in blk.named_parameters():
                assert rel_err(p.grad, o.sd["block." + k].grad) <= 3 * RTOL, k
        asd = synth_from_shapes(aspp_shapes("aspp", 64))
        aspp = load_sd(ASPP(64, [6, 12, 18]), asd, "aspp.").train()
        aspp.project[3].p = 0.0
        xa = synth_images(4, 25, 25, seed=11, c=64)
        xg = xa.to(dev()).requires_grad_(True)
        with record_masks(aspp, "aspp.") as rec:
            y = aspp(xg)
        up = upstream(y.shape, 5)
        (y * up.to(dev())).sum().backward()
        o = oracle_for(asd)
        o.conv_math = "bf16"
        o.act_bf16 = True
        rec.apply_to(o)
        xo = xa.clone().requires_grad_(True)
        yo = o.aspp(xo, "aspp")
        assert close_up_to_bf16_ties(y, yo)
        (yo * up).sum().backward()
        assert rel_err(xg.grad, xo.grad) <= 3 * RTOL
        for k, p in aspp.named_parameters():
            assert rel_err(p.grad, o.sd["aspp." + k].grad) <= 3 * RTOL, k
        # ---- whole model
        fx = load("model_r50_os16.npz")
        m, cfg, sd = _build("resnet50", 16)
        x = synth_images(2, 65, 65, seed=71)
        m.eval()
        with torch.no_grad():
            e2 = m(x.to(dev()))
            e2b = m(x.to(dev()))
        assert torch.equal(e2, e2b)                                                  # deterministic
        ob = OracleDeepLab(cfg, sd, dropout_p=0.0)
        ob.conv_math = "bf16"
        ob.act_bf16 = True
        with torch.no_grad():
            eo = ob.eval()(x)
        assert rel_err(e2, eo) <= 3e-2
        assert 1e-4 < rel_err(e2, fx["eval_logits"]) <= 5e-2                         # vs fp32: bf16-sized, not fp32-sized
        agree = (ops.argmax_nchw(e2).cpu() == torch.from_numpy(fx["eval_mask"].astype(np.int64))).float().mean()
        assert float(agree) > 0.97
        x8 = synth_images(8, 65, 65, seed=72)
        lab8 = synth_labels(8, 65, 65, seed=72, p_fg=0.2)
        m.train()
        w = torch.tensor([1.0, 3.0])
        losses = []
        for _ in range(2):
            m.load_state_dict(sd, strict=True)
            for p in m.parameters():
                p.grad = None
            loss = CrossEntropyLoss(weight=w)(m(x8.to(dev())), lab8.to(dev()))
            loss.backward()
            losses.append((float(loss.detach()), m.backbone.conv1.weight.grad.clone()))
            assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())
        assert losses[0][0] == losses[1][0] and torch.equal(losses[0][1], losses[1][1])
        with torch.no_grad():
            lo = oloss.weighted_ce(ob.train()(x8), lab8, w)
        assert abs(losses[0][0] - float(lo)) <= 3e-2 * abs(float(lo))
        del m
        torch.cuda.empty_cache()
        # configs[4] tile size
        m, cfg, sd = _build("resnet101", 16)
        x = synth_images(2, 1024, 1024, seed=9).to(dev())
        lab = synth_labels(2, 1024, 1024, seed=9).to(dev())
        m.train()
        losses = {}
        for math in (0, 2):
            lib.iswm_set_conv_math(math)
            m.load_state_dict(sd, strict=True)
            lg = m(x)
            assert lg.shape == (2, 2, 1024, 1024) and bool(torch.isfinite(lg).all())
            loss = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))(lg, lab)
            for p in m.parameters():
                p.grad = None
            loss.backward()
            assert bool(torch.isfinite(m.backbone.conv1.weight.grad).all())
            losses[math] = float(loss.detach())
        assert abs(losses[2] - losses[0]) < 3e-2 * abs(losses[0]), losses
    finally:
        lib.iswm_set_conv_math(old)


def test_depthwise_bn_relu6_stage():
    """nn.Conv2d(groups=C) -> BatchNorm2d -> ReLU6 (the stage MobileNetV2-style backbones are made of) through the fused
    stage logic: statistics from a column pass, clamp fused into the BatchNorm pass; vs torch on the CPU"""
    import torch.nn as nn
    import torch.nn.functional as F
    from iswm_amd.network import _hip
    torch.manual_seed(3)
    c = 48
    seq = _hip.HipSequential(_hip.DepthwiseConv2d(c, c, 3, stride=2, padding=1, groups=c, bias=False),
                             _hip.BatchNorm2d(c), _hip.ReLU6(inplace=True))
    ref = nn.Sequential(nn.Conv2d(c, c, 3, stride=2, padding=1, groups=c, bias=False), nn.BatchNorm2d(c), nn.ReLU6())
    with torch.no_grad():
        seq[1].weight.fill_(4.0)                   # normalised values x 4: the clamp at 6 is exercised on both sides
    ref.load_state_dict(seq.state_dict())
    seq = seq.to(dev()).train()
    ref.train()
    x = torch.randn(4, c, 21, 17) * 2
    xg, xr = x.to(dev()).requires_grad_(True), x.clone().requires_grad_(True)
    y, yr = seq(xg), ref(xr)
    assert float((yr == 6).float().mean()) > 0.01 and float((yr == 0).float().mean()) > 0.05
    assert rel_err(y, yr.detach()) <= 1e-5
    up = torch.randn(yr.shape)
    y.backward(up.to(dev()))
    yr.backward(up)
    assert rel_err(xg.grad, xr.grad) <= 2e-4
    for (k, p), (_, q) in zip(seq.named_parameters(), ref.named_parameters()):
        assert rel_err(p.grad, q.grad) <= 2e-4, k
    assert rel_err(seq[1].running_var, ref[1].running_var) <= 1e-5


@pytest.mark.parametrize("os_,n,h,w", [(16, 3, 97, 131), (8, 2, 73, 49), (16, 2, 33, 200)])
def test_whole_model_odd_sizes(os_, n, h, w):
    """non-square / odd input sizes and batch 3 (nothing in the path assumes 65 or 513): logits in eval and train mode and
    the loss vs the CPU oracle"""
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", os_)
    x = synth_images(n, h, w, seed=51)
    lab = synth_labels(n, h, w, seed=51, p_fg=0.2, p_ignore=0.05)
    o = OracleDeepLab(cfg, sd, dropout_p=0.0)
    m.eval()
    with torch.no_grad():
        assert rel_err(m(x.to(dev())), o.eval()(x)) <= RTOL
    m.train()
    lg = m(x.to(dev()))
    with torch.no_grad():
        lo = o.train()(x)
    assert lg.shape == (n, 2, h, w) and rel_err(lg, lo) <= RTOL
    wgt = torch.tensor([1.0, 3.0])
    loss = CrossEntropyLoss(weight=wgt, ignore_index=255)(lg, lab.to(dev()))
    assert rel_err(loss, oloss.weighted_ce(lo, lab, wgt, 255)) <= RTOL
    loss.backward()
    assert all(bool(torch.isfinite(p.grad).all()) for p in m.parameters())


def test_fix_bn_training_step():
    """utils.fix_bn of the reference (utils/utils.py:30-33): BatchNorm layers frozen in eval mode while the model trains -- the fused
    stage normalises with the running statistics, leaves them untouched, and its backward is the eval-mode one.  Logits,
    loss and every gradient vs the oracle evaluated the same way (its eval mode, dropout off)."""
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    m.train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.eval()
    x = synth_images(4, 65, 65, seed=61)
    lab = synth_labels(4, 65, 65, seed=61, p_fg=0.2)
    with spy_calls() as calls:
        with record_masks(m, "") as rec:
            lg = m(x.to(dev()))
        for p in m.parameters():
            p.grad = None
        up = upstream(lg.shape, 15)
        lg.backward(up.to(dev()))
    assert_fold_ran(calls)                # eval-mode BatchNorm in a training step: k_bn_bwd_apply_cls<false>
    for k, v in m.state_dict().items():
        if "running" in k or "num_batches" in k:
            assert torch.equal(v.cpu(), sd[k]), k                # frozen statistics
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).eval()
    rec.apply_to(o)
    lgo = o(x)
    assert rel_err(lg, lgo.detach()) <= RTOL
    w = torch.tensor([1.0, 3.0])
    assert rel_err(CrossEntropyLoss(weight=w)(lg, lab.to(dev())), oloss.weighted_ce(lgo.detach(), lab, w)) <= RTOL
    lgo.backward(up)
    check_sign_patterns(o, o.relu_masks)
    params = dict(m.named_parameters())
    worst = max((rel_err(params[k].grad, v.grad), k) for k, v in o.named_parameters())
    assert worst[0] <= 3 * RTOL, worst


def test_autograd_semantics_accumulation_and_frozen_parameters():
    """what the reference's training scripts may rely on from torch.autograd: a second backward without zero_grad()
    ACCUMULATES into .grad; parameters with requires_grad=False get no gradient and do not change the others';
    set_to_none=False zero_grad keeps the same gradient tensors."""
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle.synth import synth_images, synth_labels
    m, cfg, sd = _build("resnet50", 16)
    m.train()
    crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0]))
    xa, xb = synth_images(4, 65, 65, seed=81).to(dev()), synth_images(4, 65, 65, seed=82).to(dev())
    la, lb = synth_labels(4, 65, 65, seed=81).to(dev()), synth_labels(4, 65, 65, seed=82).to(dev())

    def grads_of(x, lab):
        m.load_state_dict(sd, strict=True)
        for p in m.parameters():
            p.grad = None
        crit(m(x), lab).backward()
        return {k: p.grad.clone() for k, p in m.named_parameters()}
    ga, gb = grads_of(xa, la), grads_of(xb, lb)
    m.load_state_dict(sd, strict=True)
    for p in m.parameters():
        p.grad = None
    crit(m(xa), la).backward()
    crit(m(xb), lb).backward()                                   # no zero_grad in between
    for k, p in m.named_parameters():
        assert rel_err(p.grad, ga[k] + gb[k]) <= 1e-6, k
    held = {k: p.grad for k, p in m.named_parameters()}
    for p in m.parameters():                                     # zero_grad(set_to_none=False)
        p.grad.zero_()
    crit(m(xa), la).backward()
    for k, p in m.named_parameters():
        assert p.grad is held[k] and rel_err(p.grad, ga[k]) <= 1e-6, k
    # frozen backbone
    m.load_state_dict(sd, strict=True)
    for p in m.parameters():
        p.grad = None
    for p in m.backbone.parameters():
        p.requires_grad_(False)
    crit(m(xa), la).backward()
    for k, p in m.named_parameters():
        if k.startswith("backbone."):
            assert p.grad is None, k
        else:
            assert torch.equal(p.grad, ga[k]), k
    for p in m.backbone.parameters():
        p.requires_grad_(True)


def test_num_classes_21_and_batch_one():
    """a 21-class head (the reference constructors' default num_classes, network/modeling.py:75) -- classifier padded to 24
    channels, loss over 21 classes -- vs the oracle; eval-mode batch 1; training batch 1 raises like torch (the ASPP
    image-pooling BatchNorm sees one value per channel, network/_deeplab.py:130-141)."""
    from iswm_amd.network import modeling
    from iswm_amd.utils.loss import CrossEntropyLoss
    from oracle import loss as oloss
    from oracle.deeplab import OracleDeepLab
    from oracle.synth import ArchCfg, synth_images, synth_state_dict
    cfg = ArchCfg("deeplabv3plus", "resnet50", 21, 16)
    sd = synth_state_dict(cfg)
    m = modeling.deeplabv3plus_resnet50(num_classes=21, output_stride=16, pretrained_backbone=False)
    assert list(m.state_dict().keys()) == list(sd.keys())
    m.load_state_dict(sd, strict=True)
    m.classifier.aspp.project[3].p = 0.0
    m = m.to(dev()).train()
    x = synth_images(4, 65, 65, seed=91)
    g = torch.Generator().manual_seed(92)
    lab = torch.randint(0, 21, (4, 65, 65), generator=g)
    lab[torch.rand(4, 65, 65, generator=g) < 0.05] = 255
    w = torch.linspace(0.5, 2.5, 21)
    with record_masks(m, "") as rec:
        lg = m(x.to(dev()))
    o = OracleDeepLab(cfg, sd, dropout_p=0.0).train()
    rec.apply_to(o)
    lgo = o(x)
    assert lg.shape == (4, 21, 65, 65) and rel_err(lg, lgo.detach()) <= RTOL
    loss = CrossEntropyLoss(weight=w, ignore_index=255)(lg, lab.to(dev()))
    lo = oloss.weighted_ce(lgo, lab, w, 255)
    assert rel_err(loss, lo.detach()) <= RTOL
    for p in m.parameters():
        p.grad = None
    up = upstream(lg.shape, 16)
    lg.backward(up.to(dev()))
    lgo.backward(up)
    params = dict(m.named_parameters())
    for k in ("classifier.classifier.6.weight", "classifier.classifier.6.bias", "classifier.classifier.3.weight"):
        assert rel_err(params[k].grad, o.sd[k].grad) <= 3 * RTOL, k
    m.load_state_dict(sd, strict=True)                           # (the training forward moved the running statistics)
    m.eval()
    with torch.no_grad():
        one = m(x[:1].to(dev()))
        assert rel_err(one, OracleDeepLab(cfg, sd, dropout_p=0.0).eval()(x[:1])) <= RTOL
    m.train()
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m(x[:1].to(dev()))
