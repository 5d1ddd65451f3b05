"""deeplabv3plus_xception / deeplabv3_xception on the GPU against the float64 stock-torch restatement of tests/xception_ref.py
(which tests/test_xception_cpu.py holds to features recorded from the reference's own Xception class).

Method and bounds of tests/test_mobilenet_gpu.py: logits / loss within RTOL (1e-3 of the tensor's scale); running statistics
within 1e-5; every parameter gradient within 3 * RTOL with the restatement following this path's recorded ReLU patterns
(every BatchNorm ReLU and every block's leading ReLU, which rectifies on load inside the depthwise kernel) and max-pool
window choices; the disagreements are asserted to BE near-ties (within RTOL of the site's scale) and rare (at most
max(3, 1e-4 of the elements)).

Plus the convolutions no other model uses: the stem's 3x3 with padding 0 (3 -> 32 stride 2, 32 -> 64) and the 728-channel
pointwise conv at its 768-wide input pitch, each with the entry point and kernel asserted, at the bounds of
tests/conv_ref.py (4 x torch's own fp32 error against float64, measured here on the same operands)."""
import functools
import os

import pytest
import torch

from tests import conv_ref as C
from tests import xception_ref as R
from tests.util import RTOL, rel_err

pytestmark = pytest.mark.gpu

WEIGHT = torch.tensor([1.0, 3.0])
# (arch, output stride, N, H, W): 131 x 115 gives conv4 a 4 x 2 output at output stride 8 (tests/test_xception_cpu.py)
CASES = [("deeplabv3plus", 16, 2, 131, 99), ("deeplabv3", 16, 2, 131, 99), ("deeplabv3plus", 8, 2, 131, 115)]
IDS = ["%s_os%d" % c[:2] for c in CASES]


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def _inputs(n, h, w):
    return R.synth_images(n, h, w, 5), R.synth_labels(n, h, w, 5)


def _hip_model(arch, os_, sd=None):
    from iswm_amd.network import _hip, modeling
    m = getattr(modeling, arch + "_xception")(num_classes=2, output_stride=os_)
    m.load_state_dict(sd if sd is not None else R.synth_state(arch, 2, os_), strict=True)
    for mod in m.modules():
        if isinstance(mod, _hip.Dropout):
            mod.p = 0.0
    return m.to(dev())


class spy_calls(object):
    """records the name of every libiswm_hip.so entry point called through ops.call inside the block"""

    def __enter__(self):
        from iswm_amd import ops
        self.ops, self.real, self.names = ops, ops.call, []

        def call(name, *a):
            self.names.append(name)
            return self.real(name, *a)
        ops.call = call
        return self

    def __exit__(self, *exc):
        self.ops.call = self.real
        return False


@functools.lru_cache(maxsize=None)
def _ref_eval(arch, os_, n, h, w):
    x, _ = _inputs(n, h, w)
    ref = R.build(arch, 2, os_, R.synth_state(arch, 2, os_)).eval()
    with torch.no_grad():
        return ref(x.double())


@pytest.mark.parametrize("arch,os_,n,h,w", CASES, ids=IDS)
def test_eval_logits(arch, os_, n, h, w):
    x, _ = _inputs(n, h, w)
    lg64 = _ref_eval(arch, os_, n, h, w)
    m = _hip_model(arch, os_).eval()
    with spy_calls() as spy, torch.no_grad():
        lg = m(x.to(dev()))
    err = rel_err(lg, lg64)
    print("eval logits rel err %.2e" % err)
    assert lg.shape == (n, 2, h, w) and err <= RTOL
    assert spy.names.count("iswm_dwconv3x3_pre_fwd") == 34 and "iswm_dwconv2d_fwd" not in spy.names
    margin = (lg64[:, 0] - lg64[:, 1]).abs()
    sure = margin > 2 * RTOL * float(lg64.abs().max())
    assert float(sure.double().mean()) > 0.9
    assert bool((lg.argmax(1).cpu()[sure] == lg64.argmax(1)[sure]).all())


def _near_ties(ref, masks, pools):
    """every site where the imposed decision differs from the restatement's own is a near-tie; returns (differing, total)"""
    total = bad = 0
    for site, mk in masks.items():
        z = ref.ctl.preact[site]
        mism = (z > 0) != mk
        total += mk.numel()
        bad += int(mism.sum())
        if mism.any():
            assert float(z[mism].abs().max()) <= RTOL * float(z.abs().max()), site
    for site, idx in pools.items():
        win = ref.ctl.preact[site]                                   # [N, C, 9, Ho, Wo], -inf outside the map
        own = win.argmax(2)
        mism = own != idx.long()
        total += idx.numel()
        bad += int(mism.sum())
        if mism.any():
            gap = win.max(2).values - win.gather(2, idx.long().unsqueeze(2)).squeeze(2)
            assert float(gap[mism].max()) <= RTOL * float(win[win > float("-inf")].abs().max()), site
    assert bad <= max(3, 1e-4 * total), (bad, total)
    return bad, total


def _grad_scale(key, ref_grads):
    """tests/test_mobilenet_gpu.py::_grad_scale: a BatchNorm bias whose gradient is nothing but rounding (its output only enters
    convolutions followed by train-mode BatchNorms) is measured against its weight gradient's scale"""
    own = float(ref_grads[key].abs().max())
    sibling = key[:-len("bias")] + "weight"
    if key.endswith(".bias") and sibling in ref_grads and ref_grads[sibling].dim() == 1:
        pair = float(ref_grads[sibling].abs().max())
        if own <= 1e-9 * pair:
            return pair
    return own


@pytest.mark.parametrize("arch,os_,n,h,w", CASES, ids=IDS)
def test_train_step(arch, os_, n, h, w):
    """one training step: logits, weighted-CE loss, every parameter gradient, running statistics, and which kernels ran"""
    from iswm_amd.network import _hip
    from iswm_amd.utils.loss import CrossEntropyLoss
    x, lab = _inputs(n, h, w)
    sd = R.synth_state(arch, 2, os_)
    m = _hip_model(arch, os_, sd).train()
    rec, pools = {}, {}
    with spy_calls() as spy:
        _hip.MASK_RECORDER, _hip.POOL_RECORDER = rec, pools
        try:
            lg = m(x.to(dev()))
        finally:
            _hip.MASK_RECORDER = _hip.POOL_RECORDER = None
        loss = CrossEntropyLoss(weight=WEIGHT, ignore_index=255)(lg, lab.to(dev()))
        loss.backward()
        torch.cuda.synchronize()
    assert spy.names.count("iswm_dwconv3x3_pre_fwd") == 34 and spy.names.count("iswm_dwconv3x3_pre_bwd") == 34
    for old in ("iswm_dwconv2d_fwd", "iswm_dwconv2d_dgrad", "iswm_dwconv2d_wgrad", "iswm_dwconv3x3_fwd_stats", "iswm_dwconv3x3_bwd"):
        assert old not in spy.names, old
    npool = 3 if os_ == 16 else 2
    assert spy.names.count("iswm_maxpool3x3s2_fwd_pl") == npool == spy.names.count("iswm_maxpool3x3s2_bwd") == len(pools)

    ref = R.build(arch, 2, os_, sd).train()
    ref.ctl.preact = {}
    with torch.no_grad():
        lg64 = ref(x.double())
        loss64 = R.weighted_ce(lg64, lab, WEIGHT)
    e_lg, e_loss = rel_err(lg, lg64), abs(float(loss.detach()) - float(loss64)) / abs(float(loss64))
    print("train logits rel err %.2e  loss rel err %.2e" % (e_lg, e_loss))
    assert e_lg <= RTOL and e_loss <= RTOL
    rsd = ref.state_dict()
    worst = 0.0
    for k, v in m.state_dict().items():
        if k.endswith("running_mean") or k.endswith("running_var"):
            worst = max(worst, rel_err(v, rsd[k]))
        elif k.endswith("num_batches_tracked"):
            assert int(v) == 1, k
    print("running statistics worst rel err %.2e" % worst)
    assert worst <= 1e-5

    # gradients: the restatement follows this path's recorded ReLU patterns and pool windows
    names = {mod: nm for nm, mod in m.named_modules()}
    masks = {names[k]: v.permute(0, 3, 1, 2).cpu() for k, v in rec.items()}
    pidx = {names[k]: v.permute(0, 3, 1, 2).cpu() for k, v in pools.items()}
    ref = R.build(arch, 2, os_, sd).train()
    assert set(masks) == set(ref.tops) and set(pidx) == set(ref.pool_sites)
    ref.ctl.preact, ref.ctl.masks, ref.ctl.pools = {}, masks, pidx
    R.weighted_ce(ref(x.double()), lab, WEIGHT).backward()
    bad, total = _near_ties(ref, masks, pidx)
    grads = dict(m.named_parameters())
    ref_grads = {k: p.grad for k, p in ref.named_parameters()}
    assert set(grads) == set(ref_grads) and all(p.grad is not None for p in grads.values())
    errs = {k: float((grads[k].grad.detach().cpu().double() - g).abs().max()) / _grad_scale(k, ref_grads) for k, g in ref_grads.items()}
    kmax = max(errs, key=errs.get)
    print("patterns / windows: %d of %d differ;  worst parameter-gradient rel err %.2e (%s)" % (bad, total, errs[kmax], kmax))
    assert errs[kmax] <= 3 * RTOL, (kmax, errs[kmax])


def damped(sd):
    """the synthetic state with the residual branches damped (the last BatchNorm of every block's rep, gamma x 0.3), as the
    three-step tests of the other models damp theirs"""
    last = {}
    for k in sd:
        parts = k.split(".")
        if len(parts) == 5 and parts[1].startswith("block") and parts[2] == "rep" and parts[4] == "weight" and sd[k].dim() == 1:
            last[parts[1]] = max(last.get(parts[1], -1), int(parts[3]))
    return {k: (v * 0.3 if (k.split(".")[1] in last and k.endswith("rep.%d.weight" % last[k.split(".")[1]])) else v)
            for k, v in sd.items()}


def test_three_optimizer_steps_track_the_restatement():
    """three SGD-nesterov steps from one damped state at lr 1e-4, each side with its own activation patterns: every step's loss"""
    from iswm_amd.optim import FusedSGD
    from iswm_amd.utils.loss import CrossEntropyLoss
    arch, os_, n, h, w = CASES[0]
    x, lab = _inputs(n, h, w)
    sd = damped(R.synth_state(arch, 2, os_))
    m = _hip_model(arch, os_, sd).train()
    ref = R.build(arch, 2, os_, sd).train()
    hyper = dict(lr=1e-4, momentum=0.9, weight_decay=1e-4, nesterov=True)
    opt, ropt = FusedSGD(m.parameters(), **hyper), torch.optim.SGD(ref.parameters(), **hyper)
    crit = CrossEntropyLoss(weight=WEIGHT, ignore_index=255)
    xd, labd = x.to(dev()), lab.to(dev())
    for step in range(3):
        opt.zero_grad()
        loss = crit(m(xd), labd)
        loss.backward()
        opt.step()
        ropt.zero_grad()
        rloss = R.weighted_ce(ref(x.double()), lab, WEIGHT)
        rloss.backward()
        ropt.step()
        err = abs(float(loss.detach()) - float(rloss.detach())) / abs(float(rloss.detach()))
        print("step %d: loss %.6f restatement %.6f rel %.2e" % (step, float(loss.detach()), float(rloss.detach()), err))
        assert err <= RTOL, step


# ---- the convolutions only this model uses ------------------------------------------------------------------------------------------
ROUTES = [C._r("stem_xc1_%dx%d" % (h, w), "x6", (n, h, w, 4, 32, 3, 2, 0, 1), "k_conv_fwd<64>", "k_conv_x6<64, 64, true, true, 3>",
               "k_conv_wgrad<64, 64, 0, true, 3>") for n, h, w in ((1, 37, 41), (2, 13, 11))] + \
         [C._r("xc_stem2_37x41", "x6", (1, 37, 41, 32, 64, 3, 1, 0, 1), "k_conv_x6_patch<false, 3>", "k_conv_x6_patch<true, 3>",
               "k_conv_wgrad<64, 64, 0, true, 3>"),
          C._r("xc_stem2_13x11", "x6", (2, 13, 11, 32, 64, 3, 1, 0, 1), "k_conv_x6<64, 64, false, true, 3>",
               "k_conv_x6<64, 64, true, true, 3>", "k_conv_wgrad<64, 64, 0, true, 3>")] + \
         [C._r("xc_pw728_%dx%d" % (h, w), "pl", (n, h, w, 768, 728, 1, 1, 0, 1), "k_conv_pl2<8, 1, 3, false>", "k_conv_dgrad<64>",
               "k_wgrad_pls<3>") for n, h, w in ((1, 37, 41), (2, 13, 11))]


@pytest.mark.parametrize("rt", ROUTES, ids=[r.id for r in ROUTES])
def test_stem_and_pointwise_convs(rt, monkeypatch):
    """forward, data gradient (plain and accumulating) and weight gradient of one geometry: the planner takes the named entry
    point and kernel, the results are within 4 x torch's own fp32 error of float64"""
    from iswm_amd import _lib, ops
    n, h, w, cin, cout, k, stride, pad, dil = rt.geom
    o = C.operands(rt, "dense")
    if cin == 768:                                   # the padding columns 728..767 of the operand buffer hold zeros
        o["x"][..., 728:] = 0
    ref = C.restate(rt, o)
    floor = C.floor(rt, o, ref)
    plan = C.planned(rt)
    calls, lib, real = [], _lib.load(), ops.call

    def spy(name, *a):
        if name in C.KIND:
            calls.append((name, C.kernel_name(lib, a[0]._obj, C.KIND[name])))
        return real(name, *a)
    monkeypatch.setattr(ops, "call", spy)
    with C.conv_math(rt):
        xd = o["x"].to(dev())
        if C.planes_operand(rt, cin):
            xd = ops.split_planes(xd)
        g = ops.ConvGeom(xd, cout, k, k, stride, pad, dil)
        got = {"y": ops.conv2d_fwd(xd, o["w_f"].to(dev()), g)[0].cpu()}
        dyd, wd = o["dy"].to(dev()), o["w_d"].to(dev())
        got["dx"] = ops.conv2d_dgrad(dyd, wd, g, (n, h, w, cin)).cpu()
        acc = o["base"].to(dev())
        ops.conv2d_dgrad(dyd, wd, g, (n, h, w, cin), dx=acc, accumulate=True)
        got["dx_acc"] = acc.cpu()
        got["dw"] = ops.conv2d_wgrad(xd, o["dy_w"].to(dev()), g).cpu()
    assert calls == [plan["fwd"], plan["dgrad"], plan["dgrad"], plan["wgrad"]], calls
    assert [c[1] for c in calls] == [rt.names["fwd"], rt.names["dgrad"], rt.names["dgrad"], rt.names["wgrad"]]
    out = C.unscale(rt, o, got)
    missed = []
    for q in out:
        err = rel_err(out[q], ref[q])
        print("conv %-18s %-7s err %.3e  bound %.3e" % (rt.id, q, err, 4 * floor[q]))
        if err > 4 * floor[q]:
            missed.append((q, err, 4 * floor[q]))
    assert not missed, missed


def test_predict_on_an_xception_checkpoint_and_quant_refusal(tmp_path, capsys):
    import numpy as np
    from PIL import Image
    from iswm_amd import predict, quant
    from iswm_amd.network import modeling
    m = modeling.deeplabv3plus_xception(num_classes=2, output_stride=16)
    m.load_state_dict(R.synth_state("deeplabv3plus", 2, 16), strict=True)
    ck = str(tmp_path / "xc.pth")
    torch.save({"model_state": m.state_dict()}, ck)
    inp = str(tmp_path / "in")
    os.makedirs(os.path.join(inp, "seq"))
    rng = np.random.default_rng(0)
    for name in ("a.png", "b.png"):
        Image.fromarray(rng.integers(0, 256, (13, 11, 3), dtype=np.uint8)).resize((99, 131), Image.BILINEAR).save(
            os.path.join(inp, "seq", name))
    res = str(tmp_path / "out")
    n = predict.main(["--input", inp, "--ckpt", ck, "--model", "deeplabv3plus_xception", "--save_val_results_to", res])
    assert n == 2 and sorted(os.listdir(os.path.join(res, "seq"))) == ["a_predict.png", "b_predict.png"]
    assert np.asarray(Image.open(os.path.join(res, "seq", "a_predict.png"))).ndim >= 2
    assert "Model loaded from" in capsys.readouterr().out
    m = m.to(dev()).eval()
    with pytest.raises(NotImplementedError, match="depthwise"):
        quant.calibrate(m, [])
    with pytest.raises(NotImplementedError, match="depthwise"):
        quant.quantize_model(m, {})
    with pytest.raises(ValueError, match="no output"):                  # 65 x 65: conv4 would have nothing to read
        with torch.no_grad():
            m(torch.zeros(1, 3, 65, 65, device=dev()))
