"""The layer between the HIP kernels and torch.autograd: what happens when forward and backward calls do not come strictly in
turn.  The modules keep what a forward saves on themselves (one slot each), so the contract ("Autograd
contract") is: a backward runs over the state its own forward saved, or raises RuntimeError before it launches a kernel or
touches a .grad -- never a wrong gradient, a TypeError or an AttributeError -- and the module is usable again afterwards.  The
criteria: the one-pass ones (CE, focal) serve one backward and refuse a second, the two-pass ones recompute and give the same
bits every time; every hand-written backward is once differentiable.

Every pair of interleaved inputs has the same shape.  Bit equality everywhere except against float64, where the bounds are the
existing 4 x FLOOR of tests/streaming_ref.py, overlap_loss_ref.py, ohem_ref.py, lovasz_ref.py and conv_ref.py.  The bookkeeping
alone: tests/test_autograd_contract_cpu.py."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_ref, lovasz_ref, ohem_ref, overlap_loss_ref, streaming_ref
from tests.util import rel_err

pytestmark = pytest.mark.gpu


def dev():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU path")
    return torch.device("cuda:0")


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def same(a, b):
    return tuple(a.shape) == tuple(b.shape) and torch.equal(bits(a), bits(b))


# ======================================================================================================================
# models and bridges
# ======================================================================================================================
class Net(object):
    """one model in train mode with its state dict, a criterion, two same-shape batches and the gradients of the isolated run
    "forward a / b, CE, backward" (computed once; tests compare bits against them and leave them alone)"""

    def __init__(self, m, sd, seeds=(91, 92)):
        from iswm_amd.utils.loss import CrossEntropyLoss
        from oracle.synth import synth_images, synth_labels
        self.m, self.sd = m.train(), sd
        self.crit = CrossEntropyLoss(weight=torch.tensor([1.0, 3.0])).to(dev())
        self.xa, self.xb = (synth_images(2, 65, 65, seed=s).to(dev()) for s in seeds)
        self.la, self.lb = (synth_labels(2, 65, 65, seed=s).to(dev()) for s in seeds)
        self.ga, self.gb = self.isolated(self.xa, self.la), self.isolated(self.xb, self.lb)

    def reset(self):
        self.m.load_state_dict(self.sd, strict=True)
        self.m.train()
        for p in self.m.parameters():
            p.grad = None

    def grads(self):
        return {k: p.grad.clone() for k, p in self.m.named_parameters()}

    def isolated(self, x, lab):
        self.reset()
        self.crit(self.m(x), lab).backward()
        return self.grads()

    def no_grads(self):
        return all(p.grad is None for p in self.m.parameters())

    def retired(self):
        """no conv holds live pre-packed weights (the model's WeightPacker ended)"""
        return not any(e["live"] for _, e in self.m._packer().entries)

    def recovers(self):
        """after a refused backward: the isolated run gives the bits it always gives"""
        assert self.retired()
        g = self.isolated(self.xa, self.la)
        assert all(same(g[k], self.ga[k]) for k in g)


def _build(backbone, os_, num_classes=2):
    from iswm_amd.network import modeling
    from oracle.synth import ArchCfg, synth_state_dict
    cfg = ArchCfg("deeplabv3plus", backbone, num_classes, os_)
    m = modeling._segm_resnet("deeplabv3plus", backbone, num_classes, os_, False)
    sd = synth_state_dict(cfg)
    m.load_state_dict(sd, strict=True)
    m.classifier.aspp.project[3].p = 0.0
    return m.to(dev()), sd


@pytest.fixture(scope="module")
def net():
    return Net(*_build("resnet50", 16))


@pytest.fixture(scope="module")
def net2():
    """a second instance from the same state dict"""
    return Net(*_build("resnet50", 16))


@pytest.fixture(scope="module")
def mobile():
    from iswm_amd.network import _hip, modeling
    from tests import mobilenet_ref
    m = modeling.deeplabv3_mobilenet(num_classes=2, output_stride=16)
    sd = mobilenet_ref.synth_state("deeplabv3", 2, 16)
    m.load_state_dict(sd, strict=True)
    for mod in m.modules():
        if isinstance(mod, _hip.Dropout):
            mod.p = 0.0
    return Net(m.to(dev()), sd)


def test_isolated_run_is_repeatable(net):
    """forward a, CE, backward, twice from the same state: bit-equal gradients for every parameter.  Every later bit comparison
    rests on this."""
    g = net.isolated(net.xa, net.la)
    diff = [k for k in g if not same(g[k], net.ga[k])]
    assert not diff, diff[:5]
    assert len(g) > 150 and all(bool(torch.isfinite(v).all()) for v in g.values())
    assert not all(same(net.ga[k], net.gb[k]) for k in g)                    # the two batches do differ


def test_backward_of_an_overwritten_call_is_refused(net):
    net.reset()
    ya = net.m(net.xa)
    yb = net.m(net.xb)
    with pytest.raises(RuntimeError, match="DeepLabV3.*replaced the state saved for this backward"):
        net.crit(ya, net.la).backward()
    assert net.no_grads()
    # the refusal dropped what the model held: the later call's own backward is refused too, not run over nothing
    with pytest.raises(RuntimeError, match="replaced"):
        net.crit(yb, net.lb).backward()
    assert net.no_grads()
    net.recovers()


def test_later_call_may_still_run_its_own_backward(net):
    """ya = m(xa); yb = m(xb); backward of b: the state is b's own, so b's gradient is its isolated one; a is refused after it"""
    net.reset()
    ya = net.m(net.xa)
    yb = net.m(net.xb)
    net.crit(yb, net.lb).backward()
    g = net.grads()
    assert all(same(g[k], net.gb[k]) for k in g)
    with pytest.raises(RuntimeError, match="replaced"):
        net.crit(ya, net.la).backward()
    g2 = net.grads()
    assert all(same(g2[k], g[k]) for k in g)
    net.recovers()


def test_combined_loss_of_two_calls_is_refused(net):
    net.reset()
    total = net.crit(net.m(net.xa), net.la) + net.crit(net.m(net.xb), net.lb)
    with pytest.raises(RuntimeError, match="replaced"):
        total.backward()
    net.recovers()


@pytest.mark.parametrize("mode", ["train", "eval_then_train"])
def test_no_grad_forward_in_between_is_refused(net, mode):
    net.reset()
    ya = net.m(net.xa)
    if mode != "train":
        net.m.eval()
    with torch.no_grad():
        net.m(net.xb)
    net.m.train()
    with pytest.raises(RuntimeError, match="DeepLabV3.*replaced"):
        net.crit(ya, net.la).backward()
    assert net.no_grads()
    net.recovers()


def test_second_backward_is_refused(net):
    """through the criterion (whose own backward refuses first) and through the bridge alone (an upstream tensor on the
    logits); the gradients of the first backward stay as they are"""
    net.reset()
    loss = net.crit(net.m(net.xa), net.la)
    loss.backward(retain_graph=True)
    g = net.grads()
    assert all(same(g[k], net.ga[k]) for k in g)
    with pytest.raises(RuntimeError, match="already consumed"):
        loss.backward()
    assert all(same(p.grad, net.ga[k]) for k, p in net.m.named_parameters())
    net.recovers()

    net.reset()
    y = net.m(net.xa)
    up = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(dev())
    y.backward(up, retain_graph=True)
    g = net.grads()
    with pytest.raises(RuntimeError, match="DeepLabV3.*already consumed .*retain_graph"):
        y.backward(up)
    assert all(same(p.grad, g[k]) for k, p in net.m.named_parameters())
    net.recovers()


def test_two_instances_do_not_disturb_each_other(net, net2):
    """m1(xa) and m2(xb) with grad, then an eval-mode no_grad forward of m2, then both backwards.  m1's gradient is its
    isolated one.  m2's own pending call was replaced by m2's no_grad forward, so by the rule of
    test_no_grad_forward_in_between_is_refused its backward is refused; with that forward moved behind m2's backward both
    gradient sets are the isolated ones."""
    assert net.m is not net2.m
    net.reset()
    net2.reset()
    l1 = net.crit(net.m(net.xa), net.la)
    l2 = net2.crit(net2.m(net2.xb), net2.lb)
    with torch.no_grad():
        net2.m.eval()(net2.xa)
    net2.m.train()
    l1.backward()
    assert all(same(p.grad, net.ga[k]) for k, p in net.m.named_parameters())
    with pytest.raises(RuntimeError, match="replaced"):
        l2.backward()
    assert net2.no_grads()
    net2.recovers()

    net.reset()
    net2.reset()
    l1 = net.crit(net.m(net.xa), net.la)
    l2 = net2.crit(net2.m(net2.xb), net2.lb)
    l2.backward()
    with torch.no_grad():
        net2.m.eval()(net2.xa)                                               # m1's call is still pending
    net2.m.train()
    l1.backward()
    assert all(same(p.grad, net.ga[k]) for k, p in net.m.named_parameters())
    assert all(same(p.grad, net2.gb[k]) for k, p in net2.m.named_parameters())
    assert all(same(net.gb[k], net2.gb[k]) for k in net.gb)                  # (two instances, one state dict: the same bits)


@pytest.mark.parametrize("grad_on", [True, False], ids=["with_grad", "no_grad"])
def test_child_run_on_its_own_in_between_is_refused(net, grad_on):
    net.reset()
    ya = net.m(net.xa)
    t = torch.randn(2, 64, 17, 17, device=dev(), requires_grad=True)
    with torch.set_grad_enabled(grad_on):
        net.m.backbone["layer1"](t)
    with pytest.raises(RuntimeError, match="DeepLabV3 .*Bottleneck.*replaced"):
        net.crit(ya, net.la).backward()
    assert net.no_grads() and t.grad is None
    net.recovers()


def test_child_call_replaced_by_the_model(net):
    """the other way round: a child's own call, then the whole model's forward, then the child's backward"""
    net.reset()
    t = torch.randn(2, 64, 17, 17, device=dev(), requires_grad=True)
    yc = net.m.backbone["layer1"](t)
    net.m(net.xa)
    with pytest.raises(RuntimeError, match="_Layer .*replaced"):
        yc.sum().backward()
    assert net.no_grads() and t.grad is None
    g = net.isolated(net.xa, net.la)             # (the model's own packed weights end with its next backward, here)
    assert all(same(g[k], net.ga[k]) for k in g) and net.retired()


def test_leaf_conv_bridge():
    """a bare Conv2d through _Bridge: its isolated dw / dx against float64, then the overwritten call, the second backward and
    the recovery.  The bound is conv_ref's rule applied to this geometry (no route of conv_ref.ROUTES has it: fp32 operands,
    2 x 9 x 9, 64 -> 64, 3 x 3 runs k_conv_x6 both ways and k_conv_wgrad<64, 64, 1>, a mix of the x6_s2 and x6_patch rows):
    4 x the error of torch's own fp32 CPU operator, on one thread, against the same float64 result on the same inputs."""
    from iswm_amd import _lib
    from iswm_amd.network import _hip
    d = dev()
    here = conv_ref.ROUTE["x6_patch"]._replace(geom=(2, 9, 9, 64, 64, 3, 1, 1, 1))
    assert _lib.load().iswm_get_conv_math() == conv_ref.MATH[here.mode]
    assert [v[1] for v in conv_ref.planned(here).values()] == ["k_conv_x6<64, 64, false, true, 3>", "k_conv_x6<64, 64, true, true, 3>",
                                                               "k_conv_wgrad<64, 64, 1, true, 3>"]
    g = torch.Generator().manual_seed(17)
    conv = _hip.Conv2d(64, 64, 3, padding=1, bias=False)
    with torch.no_grad():
        conv.weight.copy_(torch.randn(64, 64, 3, 3, generator=g) / 24.0)
    conv = conv.to(d)
    xa, xb = (torch.randn(2, 64, 9, 9, generator=g) for _ in range(2))
    up = torch.randn(2, 64, 9, 9, generator=g)

    def isolated(x0):
        conv.weight.grad = None
        x = x0.to(d).requires_grad_(True)
        conv(x).backward(up.to(d))
        return conv.weight.grad.clone(), x.grad.clone()
    dw, dx = isolated(xa)
    dw2, dx2 = isolated(xa)
    assert same(dw, dw2) and same(dx, dx2)
    x64, w64 = xa.double().requires_grad_(True), conv.weight.detach().cpu().double().requires_grad_(True)
    F.conv2d(x64, w64, padding=1).backward(up.double())
    x32, w32 = xa.clone().requires_grad_(True), conv.weight.detach().cpu().contiguous().requires_grad_(True)
    with conv_ref.one_thread():
        F.conv2d(x32, w32, padding=1).backward(up)
    for key, got, low, want in (("dw", dw, w32.grad, w64.grad), ("dx", dx, x32.grad, x64.grad)):
        floor, err = rel_err(low, want), rel_err(got, want)
        print("leaf conv %s  floor %.1e  bound %.1e  measured %.2e" % (key, floor, 4 * floor, err))
        assert 0 < floor < 1e-6 and err <= 4 * floor, (key, floor, err)

    conv.weight.grad = None
    a, b = xa.to(d).requires_grad_(True), xb.to(d).requires_grad_(True)
    ya = conv(a)
    conv(b)
    with pytest.raises(RuntimeError, match="Conv2d: .*replaced"):
        ya.backward(up.to(d))
    assert conv.weight.grad is None and a.grad is None
    assert all(same(p, q) for p, q in zip(isolated(xa), (dw, dx)))

    conv.weight.grad = None
    a = xa.to(d).requires_grad_(True)
    ya = conv(a)
    ya.backward(up.to(d), retain_graph=True)
    assert same(conv.weight.grad, dw) and same(a.grad, dx)
    with pytest.raises(RuntimeError, match="Conv2d: .*already consumed"):
        ya.backward(up.to(d))
    assert same(conv.weight.grad, dw) and same(a.grad, dx)
    assert all(same(p, q) for p, q in zip(isolated(xa), (dw, dx)))


def test_mobilenet_overwritten_call_and_recovery(mobile):
    g = mobile.isolated(mobile.xa, mobile.la)
    assert all(same(g[k], mobile.ga[k]) for k in g)
    mobile.reset()
    ya = mobile.m(mobile.xa)
    mobile.m(mobile.xb)
    with pytest.raises(RuntimeError, match="DeepLabV3.*replaced"):
        mobile.crit(ya, mobile.la).backward()
    assert mobile.no_grads()
    mobile.recovers()
    mobile.reset()
    ya = mobile.m(mobile.xa)
    with torch.no_grad():
        mobile.m.backbone["high_level_features"](torch.randn(2, 24, 17, 17, device=dev()))
    with pytest.raises(RuntimeError, match="DeepLabV3 .at its HipSequential.: .*replaced"):      # the child that ran, itself
        mobile.crit(ya, mobile.la).backward()
    assert mobile.no_grads()
    mobile.recovers()


def test_create_graph_through_the_model_is_refused(net):
    net.reset()
    x = net.xa.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once_differentiable.*_SegBridge"):
        torch.autograd.grad(net.m(x).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        torch.autograd.grad(net.crit(net.m(x), net.la), x, create_graph=True)
    t = torch.randn(2, 64, 17, 17, device=dev(), requires_grad=True)
    with pytest.raises(RuntimeError, match="once_differentiable.*_Bridge"):
        torch.autograd.grad(net.m.backbone["layer1"](t).sum(), t, create_graph=True)
    assert net.no_grads()
    g = net.isolated(net.xa, net.la)
    assert all(same(g[k], net.ga[k]) for k in g)


# ======================================================================================================================
# criteria
# ======================================================================================================================
def _case(name):
    """(make(weight on `device` or the CPU) -> criterion, logits, labels, class weights or None, one_pass, float64 reference of
    (loss, gradient at upstream 1) or None, FLOOR of the loss, FLOOR of the gradient) on the *_ref.py inputs"""
    from iswm_amd.utils import loss as L
    S, O, H, V = streaming_ref, overlap_loss_ref, ohem_ref, lovasz_ref
    if name in ("ce", "focal_mean", "focal_sum"):
        logits, labels, weight = S.loss_inputs(3, "i64", S.LOSS_SHAPES["small"])
        mode, alpha, gamma, wt = {"ce": (0, 1.0, 0.0, weight), "focal_mean": (1, 0.25, 2.0, weight), "focal_sum": (2, 1.0, 0.5, None)}[name]
        if mode == 0:
            make = lambda w: L.CrossEntropyLoss(weight=w, ignore_index=S.IGNORE)
        else:
            make = lambda w: L.FocalLoss(alpha=alpha, gamma=gamma, size_average=mode == 1, ignore_index=S.IGNORE, weight=w)
        v, _, g = S.loss_ref(logits, labels, wt, S.IGNORE, alpha, gamma, mode)
        return make, logits, labels, wt, True, (v, g), S.FLOOR["loss.value.m%d" % mode], S.FLOOR["loss.grad.m%d" % mode]
    if name in ("tversky", "dice"):
        logits, labels, weight = O.inputs("rag1", "i64", 1.0)
        if name == "tversky":
            wt, args = weight, (1.0, 2.0, 0.3, 0.7, 0.75, 1.0, "foreground")
            make = lambda w: L.TverskyLoss(alpha=0.3, beta=0.7, gamma=0.75, ce_weight=1.0, overlap_weight=2.0, weight=w)
        else:
            wt, args = None, (0.0, 1.0, 0.5, 0.5, 1.0, 1.0, "all")
            make = lambda w: L.DiceLoss(classes="all", weight=w)
        ref = O.overlap_ref(logits, labels, wt, O.IGNORE, *args)
        return make, logits, labels, wt, False, (ref["loss"], ref["grad"]), O.FLOOR["loss.rag1_s1"], O.FLOOR["grad.rag1_s1"]
    if name == "ohem":
        tag, logits, labels, wt, ig, th, k, _ = next(c for c in H.group_cases("r2b_s1") if c[0] == "i64_k10_t0.7_w")
        make = lambda w: L.OhemCrossEntropyLoss(thresh=th, min_kept=k, weight=w, ignore_index=ig)
        return make, logits, labels, wt, False, None, H.FLOOR["loss.r2b_s1"], H.FLOOR["grad.r2b_s1"]
    assert name == "lovasz"
    tag, logits, labels, wt, ig, classes, lce, llv, _ = next(c for c in V.group_cases("c3") if c[0] == "i64_w_ce1_all")
    make = lambda w: L.LovaszSoftmaxLoss(classes=classes, ce_weight=lce, lovasz_weight=llv, weight=w, ignore_index=ig)
    return make, logits, labels, wt, False, None, V.FLOOR["loss.c3"], V.FLOOR["grad.c3"]


ONE_PASS = ["ce", "focal_mean", "focal_sum"]
TWO_PASS = ["tversky", "dice", "ohem", "lovasz"]
CRITERIA = ONE_PASS + TWO_PASS


class Crit(object):
    def __init__(self, name):
        self.name = name
        self.make, logits, labels, wt, self.one_pass, self.ref, self.floor_loss, self.floor_grad = _case(name)
        d = dev()
        self.wt_cpu = wt
        self.crit = self.make(None if wt is None else wt.to(d))
        self.logits, self.labels = logits.to(d), labels.to(d)
        assert self.labels.dtype == torch.int64 and self.logits.is_contiguous()
        self.loss, self.grad = self.run(self.logits, self.labels)            # the contiguous call at upstream 1

    def run(self, logits, labels, crit=None):
        z = logits.detach().clone().requires_grad_(True)
        loss = (crit or self.crit)(z, labels)
        loss.backward()
        return loss.detach().clone(), z.grad.clone()

    def extras(self, crit=None):
        c = crit or self.crit
        return [float(getattr(c, a)) for a in ("last_kept", "last_nu", "last_present") if hasattr(c, a)]


@pytest.fixture(scope="module", params=CRITERIA)
def cr(request):
    return Crit(request.param)


def test_criterion_isolated_call(cr):
    """the base every later comparison uses: repeatable bits, and within the existing bounds of float64 where the reference
    needs nothing from the kernels (CE, focal, Tversky, Dice)"""
    loss, grad = cr.run(cr.logits, cr.labels)
    assert same(loss, cr.loss) and same(grad, cr.grad)
    assert cr.loss.shape == () and bool(torch.isfinite(cr.grad).all()) and bool(cr.grad.any())
    if cr.ref is not None:
        assert rel_err(cr.loss, cr.ref[0]) <= 4 * cr.floor_loss
        assert rel_err(cr.grad, cr.ref[1]) <= 4 * cr.floor_grad


def test_criterion_backward_twice_under_retain_graph(cr):
    z = cr.logits.clone().requires_grad_(True)
    loss = cr.crit(z, cr.labels)
    loss.backward(retain_graph=True)
    first = z.grad.clone()
    assert same(first, cr.grad)
    if cr.one_pass:
        with pytest.raises(RuntimeError, match="(CrossEntropyLoss|FocalLoss): .*already consumed .*retain_graph"):
            loss.backward()
        assert same(z.grad, first)                                           # not rescaled a second time, not accumulated into
        assert rel_err(z.grad, cr.ref[1]) <= 4 * cr.floor_grad
    else:
        z.grad = None
        loss.backward()
        assert same(z.grad, first)


def test_criterion_upstream_arithmetic(cr):
    z = cr.logits.clone().requires_grad_(True)
    loss = cr.crit(z, cr.labels)
    (2 * loss + 3 * loss).backward()
    assert rel_err(z.grad, 5.0 * cr.grad.double()) <= 4 * cr.floor_grad
    if cr.ref is not None:
        assert rel_err(z.grad, 5.0 * cr.ref[1]) <= 4 * cr.floor_grad


@pytest.mark.parametrize("form", ["channel_slice", "channels_last"])
def test_criterion_strided_logits(cr, form):
    b, c, h, w = cr.logits.shape
    if form == "channel_slice":
        leaf = torch.randn(b, c + 2, h, w, generator=torch.Generator().manual_seed(3)).to(dev())
        leaf[:, 1:1 + c] = cr.logits
        leaf.requires_grad_(True)
        z = leaf[:, 1:1 + c]
    else:
        leaf = cr.logits.clone().contiguous(memory_format=torch.channels_last).requires_grad_(True)
        z = leaf
    assert not z.is_contiguous()
    loss = cr.crit(z, cr.labels)
    assert same(loss, cr.loss)
    loss.backward()
    if form == "channel_slice":
        assert same(leaf.grad[:, 1:1 + c], cr.grad)
        rest = torch.cat([leaf.grad[:, :1], leaf.grad[:, 1 + c:]], 1)
        assert torch.equal(bits(rest), torch.zeros_like(bits(rest)))
    else:
        assert same(leaf.grad, cr.grad)


def test_criterion_label_forms(cr):
    """int32 labels, labels on the CPU, class weights left on the CPU: the bits of the int64 device call"""
    l32 = cr.labels.to(torch.int32)
    assert all(same(a, b) for a, b in zip(cr.run(cr.logits, l32), (cr.loss, cr.grad)))
    assert all(same(a, b) for a, b in zip(cr.run(cr.logits, cr.labels.cpu()), (cr.loss, cr.grad)))
    if cr.wt_cpu is not None:
        on_cpu = cr.make(cr.wt_cpu.clone())
        assert not (on_cpu.weight.is_cuda)
        assert all(same(a, b) for a, b in zip(cr.run(cr.logits, cr.labels.cpu(), on_cpu), (cr.loss, cr.grad)))


def test_criterion_without_grad(cr):
    with torch.no_grad():
        v = cr.crit(cr.logits.clone().requires_grad_(True), cr.labels)
    assert same(v, cr.loss) and not v.requires_grad
    v = cr.crit(cr.logits.clone(), cr.labels)
    assert same(v, cr.loss) and not v.requires_grad


def test_criterion_reused_for_two_calls(cr):
    """la = crit(za, a); lb = crit(zb, b); la.backward(); lb.backward(): the criteria keep per-call state in the autograd
    context, so each gradient is its isolated one; last_kept / last_nu / last_present describe call b"""
    zb0, b = (cr.logits.flip(3) * 0.75).contiguous(), cr.labels.flip(2).contiguous()
    loss_b, grad_b = cr.run(zb0, b)
    extras_b = cr.extras()
    assert not same(grad_b, cr.grad)
    za, zb = cr.logits.clone().requires_grad_(True), zb0.clone().requires_grad_(True)
    la_ = cr.crit(za, cr.labels)
    lb_ = cr.crit(zb, b)
    la_.backward()
    lb_.backward()
    assert same(la_, cr.loss) and same(lb_, loss_b)
    assert same(za.grad, cr.grad) and same(zb.grad, grad_b)
    assert cr.extras() == extras_b and len(extras_b) == {"ohem": 2, "lovasz": 1}.get(cr.name, 0)


def test_criterion_logits_edited_in_place_before_backward(cr):
    z = cr.logits.clone().requires_grad_(True)
    z2 = z * 1
    loss = cr.crit(z2, cr.labels)
    z2.add_(1)
    if cr.one_pass:                                                          # the gradient was formed in the forward
        loss.backward()
        assert same(z.grad, cr.grad)
        assert rel_err(z.grad, cr.ref[1]) <= 4 * cr.floor_grad
    else:                                                                    # the backward would read the edited logits
        with pytest.raises(RuntimeError, match="modified by an inplace operation"):
            loss.backward()
        assert z.grad is None


@pytest.mark.parametrize("name", ["ce", "focal_mean", "tversky", "ohem", "lovasz"])
def test_create_graph_through_a_criterion_is_refused(name):
    c = Crit(name)
    z = c.logits.clone().requires_grad_(True)
    with pytest.raises(RuntimeError, match="once_differentiable.*_(Loss|OverlapLoss|OhemLoss|LovaszLoss)Fn"):
        torch.autograd.grad(c.crit(z, c.labels), z, create_graph=True)
    (g,) = torch.autograd.grad(c.crit(z, c.labels), z)                      # the plain call is untouched
    assert same(g, c.grad) and not g.requires_grad
