"""INT8 post-training quantized inference (counterpart of the reference's evaluate_quantization.py model side).

    amax = calibrate(model, batches)            # MinMax: max |x| per tensor over all batches, on the device
    qm = quantize_model(model, amax)            # BatchNorm folded, int8 weights, fixed scales
    qm.forward_lowres(x)                        # same contract as _SimpleSegmentationModel.forward_lowres
    qm.save_int8(path); load_int8(path)

The scheme is fixed so that tests/quant_ref.py restates it bit for bit:
  * weights: BatchNorm (running statistics) folded in fp64, a = gamma / sqrt(var + eps), w' = w a, b' = beta - mean a;
    symmetric per-output-channel int8, s_w = max |w'| / 127 (1 for an all-zero channel), q = clamp(rint(w' / s_w), +-127);
  * activations: one symmetric scale per tensor, s = amax / 127 (1 when amax is 0); ReLU outputs in [0, 127], the
    residual branch's downsample output in [-127, 127]; the five ASPP branches share the ASPP concat's scale, the
    decoder's projection and upsample share the decoder concat's;
  * every convolution: csrc/qconv.hip with the fp64 epilogue v = acc * (s_in s_w[c]) + b'[c] (+ r s_r) (ReLU), then
    q = clamp(rint(v / s_out)) -- the classifier writes fp32 logits instead;
  * the stem (conv1 + bn1 + ReLU, max-pool) stays on the fp32-grade kernels; its output is quantized after the pool.
Inference only: autograd, CPU tensors and --separable_conv models are refused.
"""
import contextlib

import numpy as np
import torch
import torch.nn as nn

from . import ops
from .network import _hip
from .network._deeplab import ASPP, AtrousSeparableConvolution, DeepLabHead, DeepLabHeadV3Plus

FORMAT = "iswm_amd.int8.v1"
BN_EPS = ops.BN_EPS


# ---- host-side rules (fp64 numpy) ------------------------------------------------------------------------------------
def fold_bn(w, bn=None, bias=None):
    """conv weight [Cout, Cin, KH, KW] (+ its BatchNorm in eval form, or its own bias) -> (w', b') in fp64"""
    w = w.detach().cpu().double().numpy()
    if bn is None:
        b = np.zeros(w.shape[0]) if bias is None else bias.detach().cpu().double().numpy()
        return w, b
    g = bn.weight.detach().cpu().double().numpy()
    beta = bn.bias.detach().cpu().double().numpy()
    mean = bn.running_mean.detach().cpu().double().numpy()
    var = bn.running_var.detach().cpu().double().numpy()
    a = g / np.sqrt(var + float(bn.eps))
    return w * a[:, None, None, None], beta - mean * a


def quantize_weight(wf):
    """fp64 [Cout, Cin, KH, KW] -> (int8 [Cout, Cin, KH, KW], s_w fp64 [Cout]), symmetric per output channel"""
    m = np.abs(wf).reshape(wf.shape[0], -1).max(axis=1)
    s = np.where(m > 0, m / 127.0, 1.0)
    q = np.clip(np.rint(wf / s[:, None, None, None]), -127, 127).astype(np.int8)
    return q, s


def act_scale(amax):
    amax = float(amax)
    return amax / 127.0 if amax > 0 else 1.0


# ---- calibration -------------------------------------------------------------------------------------------------------
class AmaxRecorder(object):
    """max |x| per recorded tensor, kept on the device (one fp32 per key, max-accumulated by csrc/quant.hip)"""

    def __init__(self, model):
        self.names = {m: n for n, m in model.named_modules()}
        self.amax = {}
        self._slab = None

    def record(self, module, t, c=None):
        name = self.names[module]
        if isinstance(module, ASPP) or isinstance(module, DeepLabHeadV3Plus):
            name += ".cat"
        a = self.amax.get(name)
        if a is None:
            a = self.amax[name] = torch.zeros((1,), dtype=torch.float32, device=t.device)
        if c is None and isinstance(module, nn.Conv2d):
            c = module.out_channels
        c = t.shape[3] if c is None else min(c, t.shape[3])
        px, n, h, w, _, _, _ = ops.xgeom(t)
        need = ops._lib.load().iswm_absmax_workspace(n * h * w, c)
        if self._slab is None or self._slab.numel() * 4 < need:
            self._slab = torch.empty((max(1, need // 4),), dtype=torch.float32, device=t.device)
        ops.absmax(t, a, c, self._slab)

    def result(self):
        return {k: float(v.item()) for k, v in sorted(self.amax.items())}


@contextlib.contextmanager
def calibrating(model, recorder):
    """route the FP32 eval forward's range recording to `recorder` for the duration of the block"""
    if _hip.CALIB_RECORDER is not None:
        raise RuntimeError("a calibration is already running")
    _hip.CALIB_RECORDER = recorder
    try:
        yield recorder
    finally:
        _hip.CALIB_RECORDER = None


def _check_supported(model):
    for m in model.modules():
        if isinstance(m, (AtrousSeparableConvolution, _hip.DepthwiseConv2d)):
            raise NotImplementedError("INT8 inference does not cover --separable_conv models (depthwise convolutions)")
    if not isinstance(model.classifier, (DeepLabHeadV3Plus, DeepLabHead)):
        raise NotImplementedError("INT8 inference covers the DeepLabV3 / V3+ heads")


def calibrate(model, batches):
    """MinMax calibration: {tensor name: max |x| over every batch} from the FP32 eval forward (batches: NCHW fp32 CUDA)"""
    _check_supported(model)
    was = model.training
    model.eval()
    rec = AmaxRecorder(model)
    try:
        with torch.no_grad(), calibrating(model, rec):
            for x in batches:
                model.forward_lowres(x)
    finally:
        model.train(was)
    return rec.result()


# ---- the quantized model -----------------------------------------------------------------------------------------------
def _arch(model):
    bb = model.backbone
    nblocks = [len(bb[n]) for n in ("layer1", "layer2", "layer3", "layer4")]
    depth = {6: "resnet50", 23: "resnet101", 36: "resnet152"}[nblocks[2]]
    v3p = isinstance(model.classifier, DeepLabHeadV3Plus)
    aspp = model.classifier.aspp if v3p else model.classifier.classifier[0]
    os_ = 16 if aspp.convs[1][0].dilation[0] == 6 else 8
    return {"model": ("deeplabv3plus_" if v3p else "deeplabv3_") + depth, "num_classes": model.classifier.num_classes,
            "output_stride": os_, "in_channels": bb["conv1"].in_channels, "blocks": nblocks}


def _walk(arch):
    """the int8 network as (conv name, input key, output key, relu, residual key) in execution order, plus the tensor
    names the head needs; keys name activation scales"""
    v3p = arch["model"].startswith("deeplabv3plus")
    convs = []
    x = "backbone.maxpool"
    for li, nb in enumerate(arch["blocks"]):
        for b in range(nb):
            p = "backbone.layer%d.%d" % (li + 1, b)
            convs.append((p + ".conv1", x, p + ".conv1", True, None))
            convs.append((p + ".conv2", p + ".conv1", p + ".conv2", True, None))
            res = x
            if b == 0:
                convs.append((p + ".downsample.0", x, p + ".downsample.0", False, None))
                res = p + ".downsample.0"
            convs.append((p + ".conv3", p + ".conv2", p + ".conv3", True, res))
            x = p + ".conv3"
    low = "backbone.layer1.%d.conv3" % (arch["blocks"][0] - 1)
    if v3p:
        a, cls = "classifier.aspp", "classifier.classifier"
        tail = [(cls + ".0", "classifier.cat", cls + ".0", True, None), (cls + ".3", cls + ".0", cls + ".3", True, None),
                (cls + ".6", cls + ".3", None, False, None)]
    else:
        a, cls = "classifier.classifier.0", "classifier.classifier"
        tail = [(cls + ".1", a + ".project.0", cls + ".1", True, None), (cls + ".4", cls + ".1", None, False, None)]
    head = [(a + ".convs.%d.0" % i, x, a + ".cat", True, None) for i in range(4)]
    head.append((a + ".convs.4.1", x, a + ".cat", True, None))                  # on the pooled map, then broadcast
    head.append((a + ".project.0", a + ".cat", a + ".project.0", True, None))
    if v3p:
        head.append(("classifier.project.0", low, "classifier.cat", True, None))
    return convs + head + tail, {"aspp": a, "low": low, "v3p": v3p, "x": x}


def _bn_of(model, name):
    """the BatchNorm that follows conv `name` (the next child of its Sequential / the matching bnK of a Bottleneck)"""
    parent, _, last = name.rpartition(".")
    pm = model.get_submodule(parent)
    if last.startswith("conv") and hasattr(pm, "bn" + last[4:]):
        return getattr(pm, "bn" + last[4:])
    nxt = pm[int(last) + 1] if last.isdigit() and int(last) + 1 < len(pm) else None
    return nxt if isinstance(nxt, nn.BatchNorm2d) else None


def _ceil(v, m):
    return (v + m - 1) // m * m


class _QConv(object):
    """one int8 convolution with its fixed epilogue constants on the device"""

    def __init__(self, rec, s_in, s_out, s_res, relu, lo, dev):
        q = rec["w"]                                      # int8 [Cout, Cin, KH, KW]
        self.cout, cin, self.k, _ = q.shape
        self.stride, self.pad, self.dil = rec["geom"]
        cin_p, cout_p = _ceil(cin, 64), _ceil(self.cout, 16)
        wp = torch.zeros((cout_p, self.k, self.k, cin_p), dtype=torch.int8)
        wp[:self.cout, :, :, :cin] = torch.as_tensor(q).permute(0, 2, 3, 1)
        self.w = wp.reshape(cout_p, -1).contiguous().to(dev)
        s_w = np.asarray(rec["s_w"], dtype=np.float64)
        mul = np.zeros(cout_p)
        add = np.zeros(cout_p)
        mul[:self.cout] = s_in * s_w
        add[:self.cout] = np.asarray(rec["b"], dtype=np.float64)
        self.mul = torch.from_numpy(mul).to(dev)
        self.add = torch.from_numpy(add).to(dev)
        self.inv_s_out = 1.0 / s_out if s_out is not None else 1.0
        self.s_res = s_res or 0.0
        self.relu, self.lo = relu, lo

    def __call__(self, x, out=None, res=None, out_f32=False, cstore=None):
        return ops.qconv_fwd(x, self.w, self.mul, self.add, self.k, self.stride, self.pad, self.dil, self.relu, self.lo,
                             self.inv_s_out, out=out, res=res, s_res=self.s_res, out_f32=out_f32,
                             cstore=self.cout if cstore is None else cstore)


class QuantizedSegmentationModel(nn.Module):
    """The INT8 counterpart of a DeepLabV3 / V3+ _SimpleSegmentationModel (inference only)."""

    def __init__(self, arch, convs, act, stem_sd, device):
        super(QuantizedSegmentationModel, self).__init__()
        self.arch, self.convs, self.act = dict(arch), convs, dict(act)
        self.num_classes = arch["num_classes"]
        # the stem on the fp32-grade kernels (conv1 + bn1 + ReLU, max-pool)
        self.conv1 = _hip.Conv2d(arch["in_channels"], 64, kernel_size=7, stride=2, padding=3, bias=False)
        self.bn1 = _hip.BatchNorm2d(64)
        self.load_state_dict(stem_sd, strict=True)
        self.to(device).eval()
        for p in self.parameters():
            p.requires_grad_(False)
        self.plan, self.info = _walk(arch)
        s = self.act
        self.q = {}
        for name, kin, kout, relu, kres in self.plan:
            self.q[name] = _QConv(convs[name], s[kin], None if kout is None else s[kout], s[kres] if kres else None,
                                  relu, 0 if relu else -127, device)

    # ---- the two halves ----
    def _check_input(self, x):
        if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4):
            raise ValueError("the INT8 model takes a 4-D fp32 CUDA NCHW tensor (there is no CPU fallback)")
        if torch.is_grad_enabled() and x.requires_grad:
            raise RuntimeError("the INT8 model is inference only: call it under torch.no_grad()")

    def stem(self, x):
        """NCHW fp32 image -> int8 NHWC [N, H/4, W/4, 64], the max-pool output quantized with its scale"""
        self._check_input(x)
        with torch.no_grad():
            xh = ops.nchw_to_nhwc(x)
            y, _ = _hip.cba_fwd(self.conv1, self.bn1, True, xh, False, out_fmt="f32")
            p, _ = ops.maxpool_fwd(y, planes=False)
            return ops.quantize_i8(p, 1.0 / self.act["backbone.maxpool"], 0, ldy=64)

    def body(self, q):
        """int8 stem output -> the classifier's fp32 NHWC logits [N, hl, wl, pad4(num_classes)]"""
        if not (torch.is_tensor(q) and q.is_cuda and q.dtype == torch.int8 and q.dim() == 4):
            raise ValueError("body() takes the int8 NHWC CUDA tensor stem() returns")
        Q, info = self.q, self.info
        t = {"backbone.maxpool": q}
        for name, kin, kout, relu, kres in self.plan:
            if not name.startswith("backbone."):
                break
            t[kout] = Q[name](t[kin], res=t[kres] if kres else None)
        x = t[info["x"]]
        n, h, w, _ = x.shape
        a = info["aspp"]
        cat = torch.empty((n, h, w, 1280), dtype=torch.int8, device=x.device)
        for i in range(4):
            Q[a + ".convs.%d.0" % i](x, out=cat[..., 256 * i:256 * (i + 1)])
        sx = self.act[info["x"]]
        pooled = ops.qgap(x, sx, 1.0 / sx)
        v = Q[a + ".convs.4.1"](pooled)
        ops.qbcast(v, cat[..., 1024:1280])
        aspp = Q[a + ".project.0"](cat)                   # Dropout: identity in eval
        nc4 = _hip.pad4(self.num_classes)
        if info["v3p"]:
            low = t[info["low"]]
            _, hl, wl, _ = low.shape
            dec = torch.zeros((n, hl, wl, 320), dtype=torch.int8, device=x.device)
            Q["classifier.project.0"](low, out=dec[..., :48])
            ops.qbilinear(aspp, self.act[a + ".project.0"], 1.0 / self.act["classifier.cat"], dec[..., 48:304])
            c = "classifier.classifier"
            y = Q[c + ".3"](Q[c + ".0"](dec))
            return Q[c + ".6"](y, out_f32=True, cstore=nc4)
        c = "classifier.classifier"
        return Q[c + ".4"](Q[c + ".1"](aspp), out_f32=True, cstore=nc4)

    def forward_lowres(self, x):
        """x NCHW fp32 -> fp32 NHWC logits [B, hl, wl, pad4(num_classes)] (channels past num_classes are padding)"""
        self._check_input(x)
        with torch.no_grad():
            return self.body(self.stem(x))

    def forward(self, x):
        """NCHW logits at the input size"""
        yl = self.forward_lowres(x)
        return ops.bilinear_to_nchw_fwd(yl, self.num_classes, x.shape[2], x.shape[3])

    # ---- persistence ----
    def state_int8(self):
        return {"format": FORMAT, "arch": dict(self.arch), "act": dict(self.act),
                "convs": {k: {"w": torch.as_tensor(v["w"]), "s_w": torch.as_tensor(v["s_w"]),
                              "b": torch.as_tensor(v["b"]), "geom": tuple(v["geom"])} for k, v in self.convs.items()},
                "stem": {k: v.detach().cpu() for k, v in self.state_dict().items()}}

    def save_int8(self, path):
        torch.save(self.state_int8(), path)


def quantize_model(model, amax):
    """fp32 model (eval statistics) + calibrated amaxes -> QuantizedSegmentationModel on the model's device"""
    _check_supported(model)
    arch = _arch(model)
    plan, info = _walk(arch)
    act = {}
    for k, v in amax.items():
        act[k] = act_scale(v)
    # shared scales: the ASPP branches write the ASPP concat, the decoder projection the decoder concat
    need = {kin for _, kin, _, _, _ in plan} | {kout for _, _, kout, _, _ in plan if kout} | \
        {kres for *_, kres in plan if kres}
    missing = sorted(need - set(act))
    if missing:
        raise ValueError("calibration has no range for %s" % missing[:4])
    convs = {}
    for name, _, _, _, _ in plan:
        conv = model.get_submodule(name)
        bn = _bn_of(model, name)
        wf, b = fold_bn(conv.weight, bn, conv.bias)
        q, s_w = quantize_weight(wf)
        convs[name] = {"w": q, "s_w": s_w, "b": b,
                       "geom": (conv.stride[0], conv.padding[0], conv.dilation[0])}
    bb = model.backbone
    stem = {"conv1.weight": bb["conv1"].weight.detach().cpu().contiguous()}
    stem.update({"bn1." + k: v.detach().cpu() for k, v in bb["bn1"].state_dict().items()})
    return QuantizedSegmentationModel(arch, convs, {k: act[k] for k in sorted(need)}, stem,
                                      next(model.parameters()).device)


def is_int8_checkpoint(obj):
    return isinstance(obj, dict) and obj.get("format") == FORMAT


def read_checkpoint(path):
    """(INT8 checkpoint dict or None, the file's contents): the file is read once with train.load_checkpoint, the
    weights-only loader that also admits the numpy scalars of FP32 checkpoints' score dictionaries"""
    from .train import load_checkpoint
    d = load_checkpoint(path)
    return (d if is_int8_checkpoint(d) else None), d


def load_int8(path_or_dict, device=None):
    if isinstance(path_or_dict, dict):
        d = path_or_dict
    else:
        from .train import load_checkpoint
        d = load_checkpoint(path_or_dict)
    if not is_int8_checkpoint(d):
        raise ValueError("not an iswm_amd INT8 checkpoint (format tag %r)" % (d.get("format") if isinstance(d, dict)
                                                                               else type(d).__name__,))
    convs = {k: {"w": v["w"].numpy(), "s_w": v["s_w"].numpy(), "b": v["b"].numpy(), "geom": tuple(v["geom"])}
             for k, v in d["convs"].items()}
    stem = dict(d["stem"])
    return QuantizedSegmentationModel(d["arch"], convs, d["act"], stem, device or torch.device("cuda"))
