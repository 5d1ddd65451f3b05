"""numpy restatement of the INT8 inference path (iswm_amd/quant.py, csrc/qconv.hip, csrc/quant.hip) -- its parity pin.

Every rule of DESIGN.md section 10 is written out again here with numpy only: the BatchNorm fold and weight
quantization, the exact integer convolution (int64), each fp64 epilogue, the average pool, the broadcast, the
bilinear resize and the shared concat scales.  numpy float64 arithmetic does not contract a * b + c, and the kernels
are compiled with contraction off, so the int8 tensors and the fp32 logits must match bit for bit.
"""
import numpy as np


# ---- host rules ----
def fold_bn(w, gamma, beta, mean, var, eps):
    """w [Cout, Cin, KH, KW]; BatchNorm in eval form folded in fp64 -> (w', b')"""
    w = np.asarray(w, np.float64)
    a = np.asarray(gamma, np.float64) / np.sqrt(np.asarray(var, np.float64) + eps)
    return w * a[:, None, None, None], np.asarray(beta, np.float64) - np.asarray(mean, np.float64) * a


def quantize_weight(wf):
    wf = np.asarray(wf, np.float64)
    q = np.empty(wf.shape, np.int8)
    s = np.empty(wf.shape[0])
    for c in range(wf.shape[0]):
        m = np.abs(wf[c]).max()
        s[c] = m / 127.0 if m > 0 else 1.0
        q[c] = np.clip(np.rint(wf[c] / s[c]), -127, 127)
    return q, s


def act_scale(amax):
    return float(amax) / 127.0 if amax > 0 else 1.0


def quantize(x, inv_s, lo):
    return np.clip(np.rint(np.asarray(x, np.float64) * inv_s), lo, 127).astype(np.int8)


# ---- kernels ----
def absmax(x, c=None, amax0=0.0):
    """max(amax0, max |x[..., :c]|) as the fp32 the device holds"""
    x = np.asarray(x, np.float32)
    return np.float32(max(np.float32(amax0), np.abs(x[..., :c]).max()))


def conv_int(x, w, stride, pad, dil):
    """x int8 [N, H, W, Cin], w int8 [Cout, Cin, KH, KW] -> exact int64 [N, Ho, Wo, Cout] (zero padding)"""
    n, h, wd, cin = x.shape
    cout, cin2, kh, kw = w.shape
    assert cin2 <= cin
    ho = (h + 2 * pad - dil * (kh - 1) - 1) // stride + 1
    wo = (wd + 2 * pad - dil * (kw - 1) - 1) // stride + 1
    xp = np.zeros((n, h + 2 * pad, wd + 2 * pad, cin2), np.float64)
    xp[:, pad:pad + h, pad:pad + wd] = x[..., :cin2]
    acc = np.zeros((n, ho, wo, cout), np.float64)        # |partial sums| < 2^31 (the kernel's int32): exact in fp64
    wt = np.asarray(w, np.float64)
    for i in range(kh):
        for j in range(kw):
            r0, c0 = i * dil, j * dil
            patch = xp[:, r0:r0 + stride * (ho - 1) + 1:stride, c0:c0 + stride * (wo - 1) + 1:stride]
            acc += patch @ wt[:, :, i, j].T
    return acc.astype(np.int64)


def epilogue(acc, mul, add, relu, inv_s_out=None, lo=0, res=None, s_res=0.0):
    """v = acc * mul + add (+ res * s_res) (ReLU) -> int8 (inv_s_out given) or fp32"""
    v = acc.astype(np.float64) * mul + add
    if res is not None:
        v = v + res.astype(np.float64) * s_res
    if relu:
        v = np.maximum(v, 0.0)
    if inv_s_out is None:
        return v.astype(np.float32)
    return quantize(v, inv_s_out, lo)


def qgap(x, s_in):
    n, h, w, c = x.shape
    s = x.astype(np.int64).sum(axis=(1, 2))
    v = s.astype(np.float64) * s_in / float(h * w)
    return quantize(v, 1.0 / s_in, -127)[:, None, None, :]


def _src(scale, dst, n_in):
    s = np.float32(scale) * (np.float32(dst) + np.float32(0.5)) - np.float32(0.5)
    s = max(s, np.float32(0.0))
    i0 = min(int(s), n_in - 1)
    i1 = i0 + (1 if i0 < n_in - 1 else 0)
    l1 = np.float32(s - np.float32(i0))
    return i0, i1, np.float32(np.float32(1.0) - l1), l1


def qbilinear(x, s_in, ho, wo, inv_s_out):
    n, hi, wi, c = x.shape
    sh, sw = np.float32(hi) / np.float32(ho), np.float32(wi) / np.float32(wo)
    xd = x.astype(np.float64) * s_in
    out = np.empty((n, ho, wo, c), np.int8)
    cols = [_src(sw, j, wi) for j in range(wo)]
    j0 = np.array([t[0] for t in cols])
    j1 = np.array([t[1] for t in cols])
    w0 = np.array([t[2] for t in cols], np.float64)[None, :, None]
    w1 = np.array([t[3] for t in cols], np.float64)[None, :, None]
    for i in range(ho):
        i0, i1, h0, h1 = _src(sh, i, hi)
        a, b = xd[:, i0, j0], xd[:, i0, j1]
        d, e = xd[:, i1, j0], xd[:, i1, j1]
        v = float(h0) * (w0 * a + w1 * b) + float(h1) * (w0 * d + w1 * e)
        out[:, i] = quantize(v, inv_s_out, -127)
    return out


# ---- the whole network from the int8 stem output ----
def conv(st, name, x, s_in, s_out, relu, lo=0, res=None, s_res=0.0):
    r = st["convs"][name]
    w = np.asarray(r["w"])
    stride, pad, dil = r["geom"]
    acc = conv_int(x, w, stride, pad, dil)
    mul = s_in * np.asarray(r["s_w"], np.float64)
    return epilogue(acc, mul, np.asarray(r["b"], np.float64), relu, None if s_out is None else 1.0 / s_out, lo, res,
                    s_res)


def forward_body(st, q):
    """st: a QuantizedSegmentationModel.state_int8() dict; q: int8 [N, h, w, 64] stem output -> fp32 logits
    [N, hl, wl, num_classes]"""
    arch, s = st["arch"], st["act"]
    q = np.asarray(q)
    t = {"backbone.maxpool": q}
    x = "backbone.maxpool"
    for li, nb in enumerate(arch["blocks"]):
        for b in range(nb):
            p = "backbone.layer%d.%d" % (li + 1, b)
            o1 = conv(st, p + ".conv1", t[x], s[x], s[p + ".conv1"], True)
            o2 = conv(st, p + ".conv2", o1, s[p + ".conv1"], s[p + ".conv2"], True)
            if b == 0:
                rk = p + ".downsample.0"
                t[rk] = conv(st, rk, t[x], s[x], s[rk], False, lo=-127)
            else:
                rk = x
            t[p + ".conv3"] = conv(st, p + ".conv3", o2, s[p + ".conv2"], s[p + ".conv3"], True, res=t[rk], s_res=s[rk])
            x = p + ".conv3"
    v3p = arch["model"].startswith("deeplabv3plus")
    a = "classifier.aspp" if v3p else "classifier.classifier.0"
    hi = t[x]
    sc = s[a + ".cat"]
    br = [conv(st, a + ".convs.%d.0" % i, hi, s[x], sc, True) for i in range(4)]
    pooled = qgap(hi, s[x])
    pv = conv(st, a + ".convs.4.1", pooled, s[x], sc, True)
    br.append(np.broadcast_to(pv, br[0].shape[:3] + (pv.shape[3],)))
    cat = np.concatenate(br, axis=3)
    ao = conv(st, a + ".project.0", cat, sc, s[a + ".project.0"], True)
    c = "classifier.classifier"
    if v3p:
        low = t["backbone.layer1.%d.conv3" % (arch["blocks"][0] - 1)]
        sd = s["classifier.cat"]
        proj = conv(st, "classifier.project.0", low, s["backbone.layer1.%d.conv3" % (arch["blocks"][0] - 1)], sd, True)
        up = qbilinear(ao, s[a + ".project.0"], low.shape[1], low.shape[2], 1.0 / sd)
        dec = np.concatenate([proj, up, np.zeros(up.shape[:3] + (16,), np.int8)], axis=3)
        y0 = conv(st, c + ".0", dec, sd, s[c + ".0"], True)
        y3 = conv(st, c + ".3", y0, s[c + ".0"], s[c + ".3"], True)
        return conv(st, c + ".6", y3, s[c + ".3"], None, False)
    y1 = conv(st, c + ".1", ao, s[a + ".project.0"], s[c + ".1"], True)
    return conv(st, c + ".4", y1, s[c + ".1"], None, False)
