"""float64 restatement of the per-image Lovasz-Softmax criterion of csrc/lovasz.hip, with the seeded
inputs, case lists and fp32 floors that tests/test_lovasz_cpu.py (no GPU), tests/test_lovasz_gpu.py and
tests/helpers/lovasz_ddp_worker.py (the kernels) share.

Nothing here calls the product: torch and numpy on the CPU only.  The definition, written out again, per image b and class c:

    V_b   = pixels of image b with y != ignore_index and 0 <= y < C;  p = softmax(z);  g_ic = [y_i == c]
    S     = {c >= 1} ('foreground') or every class ('all')
    e_ic  = |g_ic - p_ic| clamped to [0, 1] over V_b;   G_bc = sum g_ic;   (b, c) is PRESENT iff c in S and G_bc > 0
    order = descending e; among equal e, g = 1 before g = 0; then ascending pixel index (valid pixels only)
    at sorted position j (0-based): cg_j = #{g = 1 at positions <= j}, U_j = G + (j + 1 - cg_j), I_j = G - cg_j
    w_j   = 1 / U_j if g_(j) = 1, else I_j / ((U_j - 1) U_j)
    L_bc  = sum_j e_(j) w_j;   N = number of present segments
    L     = l_ce sum_V w_y nll / sum_V w_y + l_lv (sum_present L_bc) / N       (a term whose normaliser is 0 is 0)
    dL/dz_ik = upstream [ l_ce w_y (p_ik - g_ik) / sum w + (l_lv / N) sum_{c present} m_ic (1 - 2 g_ic) p_ic (d_ck - p_ik) ]
    m_ic  = the w of pixel i's position in segment (b, c); the gradient is exactly 0 at invalid pixels

FLOOR holds, per check and group, the error of THIS formula evaluated in float32 with stock torch ops on the CPU against the
float64 evaluation (both on the float64 order, so one order), the largest over the group's cases, rounded up to two digits and
never below 2^-24.  Checks: e (absolute: e <= 1), omega (per element, relative, over the valid pixels of present segments with
omega > 0), loss (relative) and grad (max |a - e| / max |e|).  The GPU tests bound every float comparison by 4 x FLOOR;
test_lovasz_cpu.py measures every floor again and fails if a recorded figure is above 1.25 x or below half of what it measures."""
import functools
import math

import numpy as np
import torch

IGNORE = 255
FLOOR_MIN = 2.0 ** -24
CLASSES = ("foreground", "all")
UPSTREAM = 0.37

# name -> ((B, C, H, W), foreground fraction or None for uniform labels)
SHAPES = {
    "p1": ((1, 2, 1, 1), None),          # one pixel
    "odd": ((1, 2, 31, 43), None),       # 1333 pixels: no multiple of 4, 64 or 256
    "img": ((3, 2, 65, 65), 0.2),        # image boundaries inside a thread's four pixels; image 1 has no foreground: absent
    "c3": ((2, 3, 17, 23), None),
    "c8": ((2, 8, 9, 7), None),          # the register-path limit: 14 foreground segments
    "big": ((1, 2, 513, 513), 0.05),     # 263 169 pixels, 5 % foreground: 65 tiles, the cancellation of the difference form
}
BIG = ("big",)
MUTANTS = ["diff_form", "ascending", "invalid_positions", "absent_counted", "sign_dropped", "u_prev", "batch_order"]
CHECKS = ("e", "omega", "loss", "grad")


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs(name, kind, ignore_index=IGNORE):
    """(logits fp32 [B,C,H,W], labels [B,H,W] uint8 or int64, class weights fp32 [C]); about 5 % of the labels are ignore_index;
    with 8 pixels or more, int64 labels also carry -1 and C + 1 and uint8 labels values in [C, 254], all invalid.  Shared and
    cached: callers must not write into the result."""
    (b, c, h, w), fg = SHAPES[name]
    g = gen(4100 + 17 * c + h * w)
    logits = torch.randn(b, c, h, w, generator=g)
    if fg is None:
        labels = torch.randint(0, c, (b, h, w), generator=g)
    else:
        labels = (torch.rand(b, h, w, generator=g) < fg).long()
        logits[:, 1] += 2.0 * labels.float() - 1.0              # a model that is partly right: errors spread over (0, 1)
    n = labels.numel()
    if n > 1:
        labels[torch.rand(b, h, w, generator=g) < 0.05] = ignore_index
    if name == "img":
        labels[1][labels[1] == 1] = 0
    flat = labels.view(-1)
    if n >= 8:
        bad = (-1, -1, c + 1, c + 1) if kind == "i64" else (c, 254, min(c + 17, 254), c)
        for pos, v in zip((1, n // 3, n // 2, n - 1), bad):
            flat[pos] = v
    if kind == "u8":
        labels = labels.to(torch.uint8)
    weight = torch.rand(c, generator=g) * 2 + 0.5
    return logits, labels, weight


def valid_mask(labels, c, ignore_index=IGNORE):
    y = labels.long()
    return (y != ignore_index) & (y >= 0) & (y < c)


def first_class(classes):
    assert classes in CLASSES
    return 0 if classes == "all" else 1


def pixel_terms(logits, labels, ignore_index, dtype=torch.float64):
    """log-probabilities [B, HW, C], clamped labels [B, HW], validity [B, HW] in `dtype`"""
    b, c = logits.shape[:2]
    z = logits.to(dtype).reshape(b, c, -1).permute(0, 2, 1)
    y = labels.reshape(b, -1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    logp = torch.log_softmax(z, 2) if dtype == torch.float32 else z - torch.logsumexp(z, 2, keepdim=True)
    return logp, yc, valid


def segment_order(e, g, valid):
    """[.., P] -> positions -> pixel index: descending e, g = 1 before g = 0 among equal e, then ascending index; the invalid
    pixels behind all valid ones (in index order)"""
    first = torch.sort(g.to(torch.int8), dim=-1, descending=True, stable=True).indices
    key = torch.where(valid, e, torch.full_like(e, -1.0)).gather(-1, first)
    return first.gather(-1, torch.sort(key, dim=-1, descending=True, stable=True).indices)


def jaccard_weights(gs, vs, G, dtype, mutant=None):
    """sorted g bits and validity [.., P], G [.., 1] -> omega [.., P] by the closed form (0 at invalid positions)"""
    cg = torch.cumsum((gs & vs).long(), -1)
    j1 = torch.arange(1, gs.shape[-1] + 1).expand_as(cg)
    if mutant == "u_prev":
        j1 = j1 - 1
    U, I = G + (j1 - cg), G - cg
    if mutant == "diff_form":                           # what every public implementation does, in float32
        Jf = 1.0 - I.float() / U.float()
        om = Jf.clone()
        om[..., 1:] = Jf[..., 1:] - Jf[..., :-1]
        om = om.to(dtype)
    else:
        den = ((U - 1) * U).clamp(min=1)
        om = torch.where(gs, 1.0 / U.clamp(min=1).to(dtype), I.to(dtype) / den.to(dtype))
    return torch.where(vs, om, torch.zeros_like(om))


def lovasz_ref(logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, dtype=torch.float64, upstream=1.0,
               perm=None, mutant=None):
    """dict(e, g, valid, G, present, perm, omega (sorted order), m (pixel order), Lbc, N, sums = [sum w nll, sum w, sum L_bc, N],
    loss, grad [B,C,H,W]) of the module docstring's definition in `dtype`; e, g, perm, omega and m are [B, |S|, HW].
    perm: an order [B, |S|, HW] to use instead of the one this function finds (the kernel's: one order, no circular check).
    `mutant` (test_lovasz_cpu.py only) plants one of MUTANTS."""
    b, c, h, w = logits.shape
    hw = h * w
    first = first_class(classes)
    logp, yc, valid = pixel_terms(logits, labels, ignore_index, dtype)
    p = torch.exp(logp)
    onehot = torch.nn.functional.one_hot(yc, c).bool() & valid[..., None]
    wy = weight.to(dtype)[yc] if weight is not None else torch.ones(yc.shape, dtype=dtype)
    vm = valid.to(dtype)
    nll = -logp.gather(2, yc[..., None])[..., 0]
    s1, s2 = (wy * nll * vm).sum(), (wy * vm).sum()

    ps = p[..., first:].permute(0, 2, 1)                                    # [B, |S|, HW]
    gsel = onehot[..., first:].permute(0, 2, 1)
    vsel = valid[:, None, :].expand_as(gsel)
    if mutant == "invalid_positions":                                       # every pixel is ranked (g = 0 at an invalid one)
        vsel = torch.ones_like(vsel)
    if mutant == "batch_order":                                             # one order per class over the whole batch
        ps, gsel, vsel = (t.permute(1, 0, 2).reshape(1, c - first, b * hw) for t in (ps, gsel, vsel))
    e = (gsel.to(dtype) - ps).abs().clamp(0.0, 1.0)
    G = (gsel & vsel).sum(-1, keepdim=True)
    present = G[..., 0] > 0
    if perm is None:
        perm = segment_order(-e if mutant == "ascending" else e, gsel, vsel)
    else:
        perm = perm.long()
    gs, vs, es = gsel.gather(-1, perm), vsel.gather(-1, perm), e.gather(-1, perm)
    omega = jaccard_weights(gs, vs, G, dtype, mutant)
    omega = torch.where(present[..., None], omega, torch.zeros_like(omega))
    if mutant == "invalid_positions":                                       # ranked, but no term of their own
        omega = torch.where(valid[:, None, :].expand_as(vsel).gather(-1, perm), omega, torch.zeros_like(omega))
    Lbc = (es * omega).sum(-1)
    n = present.numel() if mutant == "absent_counted" else int(present.sum())
    lv = Lbc[present].sum()
    m = torch.zeros_like(omega).scatter_(-1, perm, omega)
    if mutant == "batch_order":
        m = m.reshape(c - first, b, hw).permute(1, 0, 2)
        gsel = gsel.reshape(c - first, b, hw).permute(1, 0, 2)
        ps = ps.reshape(c - first, b, hw).permute(1, 0, 2)

    ce_on, lv_on = ce_weight != 0 and float(s2) > 0, lovasz_weight != 0 and n > 0
    zero = torch.zeros((), dtype=dtype)
    loss = (ce_weight * s1 / s2 if ce_on else zero) + (lovasz_weight * lv / n if lv_on else zero)
    sign = torch.ones_like(ps) if mutant == "sign_dropped" else 1.0 - 2.0 * gsel.to(dtype)
    q = torch.zeros_like(p)
    q[..., first:] = (m * sign * ps).permute(0, 2, 1)
    grad = torch.zeros_like(p)
    if ce_on:
        grad = grad + (ce_weight / s2) * wy[..., None] * (p - onehot.to(dtype))
    if lv_on:
        grad = grad + (lovasz_weight / n) * (q - p * q.sum(-1, keepdim=True))
    grad = upstream * torch.where(valid[..., None], grad, torch.zeros_like(grad))
    return dict(e=e, g=gsel, valid=valid, G=G[..., 0], present=present, perm=perm, omega=omega, m=m, Lbc=Lbc, N=n,
                sums=torch.stack([s1, s2, lv.to(dtype), torch.tensor(float(n), dtype=dtype)]), loss=loss,
                grad=grad.permute(0, 2, 1).reshape(b, c, h, w).contiguous())


def rel_err(a, e):
    """max |a - e| / max |e| (absolute where e is all zero)"""
    a, e = a.detach().cpu().double().reshape(-1), e.detach().cpu().double().reshape(-1)
    if a.numel() == 0:
        return 0.0
    scale = float(e.abs().max())
    return float((a - e).abs().max()) / (scale if scale > 0 else 1.0)


def abs_err(a, e):
    a, e = a.detach().cpu().double().reshape(-1), e.detach().cpu().double().reshape(-1)
    return float((a - e).abs().max()) if a.numel() else 0.0


def elem_rel_err(a, e):
    """the largest |a - e| / e over the elements with e > 0; where e is 0, a must be 0 too (inf otherwise)"""
    a, e = a.detach().cpu().double().reshape(-1), e.detach().cpu().double().reshape(-1)
    if bool((a[e == 0] != 0).any()):
        return math.inf
    on = e > 0
    return float(((a[on] - e[on]).abs() / e[on]).max()) if bool(on.any()) else 0.0


def floors_of(logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, upstream=1.0):
    """{check: error of the fp32 stock-torch evaluation against float64}, both on the float64 order -- what FLOOR records"""
    ref = lovasz_ref(logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, upstream=upstream)
    low = lovasz_ref(logits, labels, weight, ignore_index, classes, ce_weight, lovasz_weight, dtype=torch.float32,
                     upstream=upstream, perm=ref["perm"])
    v = ref["valid"][:, None, :].expand_as(ref["e"])
    return {"e": abs_err(low["e"][v], ref["e"][v]), "omega": elem_rel_err(low["omega"], ref["omega"]),
            "loss": rel_err(low["loss"], ref["loss"]), "grad": rel_err(low["grad"], ref["grad"])}


@functools.lru_cache(maxsize=None)
def group_cases(group):
    """every case a FLOOR group covers: (tag, logits, labels, weight or None, ignore_index, classes, ce_weight, lovasz_weight,
    upstream).  Both label widths, class weights on and off, l_ce in {0, 1}, both class sets; the big shape keeps two cases."""
    out = []
    for kind in ("u8", "i64"):
        logits, labels, weight = inputs(group, kind)
        for wt in (False, True):
            for lce in (0.0, 1.0):
                for classes in CLASSES:
                    if group in BIG and (wt, lce, classes) != ((kind == "u8"), (1.0 if kind == "u8" else 0.0), "foreground"):
                        continue
                    tag = "%s_%s_ce%g_%s" % (kind, "w" if wt else "now", lce, classes)
                    out.append((tag, logits, labels, weight if wt else None, IGNORE, classes, lce, 0.8, UPSTREAM))
    return out


@functools.lru_cache(maxsize=None)
def group_reference(group, index):
    _, logits, labels, wt, ig, classes, lce, llv, up = group_cases(group)[index]
    return lovasz_ref(logits, labels, wt, ig, classes, lce, llv, upstream=up)


IG2_SHAPE, IG2_IGNORE = (2, 3, 13, 11), 2            # an ignore_index INSIDE [0, C)


@functools.lru_cache(maxsize=None)
def ig2_inputs():
    b, c, h, w = IG2_SHAPE
    g = gen(77)
    return torch.randn(b, c, h, w, generator=g), torch.randint(0, c, (b, h, w), generator=g).to(torch.uint8)


# ---- inputs for the sort -----------------------------------------------------------------------------------------------------------
def make_keys(e, g, valid):
    """the key of the kernels from fp32 errors, g bits and validity: ((bits(e) << 1) | g) + 1, 0 where invalid -> int64"""
    bits = e.float().contiguous().view(torch.int32).long()
    return torch.where(valid, ((bits << 1) | g.long()) + 1, torch.zeros_like(bits))


def span_keys(n, seed=57):
    """keys made by hand (int64 values of uint32 keys): log-uniform errors from 1e-30 to 1 plus zeros, denormals, exactly 1.0
    and a run of 2 000 equal keys, both g bits, 5 % invalid -- every bit of every digit takes both values"""
    g = gen(seed)
    v = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * (0.0 - math.log(1e-30)) + math.log(1e-30)).float()
    if n >= 64:
        v[:5] = 0.0
        v[5:10] = 1e-42
        v[10:13] = 1.0
    if n >= 4200:
        v[100:2100] = v[100]
    gbit = torch.rand(n, generator=g) < 0.3
    if n >= 4200:
        gbit[100:2100] = True
    keys = make_keys(v, gbit, torch.rand(n, generator=g) >= 0.05)
    return keys[torch.randperm(n, generator=g)].contiguous()


def tie_inputs(pattern):
    """four: logits drawn from four values, so the errors take a handful of values and every rank falls inside a tie group of
    thousands; same: all pixels identical; one: a single valid pixel; none: no valid pixel"""
    b, c, h, w = 2, 2, 129, 129
    g = gen(55)
    if pattern == "four":
        vals = torch.tensor([-1.5, 0.0, 0.25, 2.0])
        logits = vals[torch.randint(0, 4, (b, c, h, w), generator=g)]
    else:
        logits = torch.zeros(b, c, h, w)
        logits[:, 1] = 0.75
    labels = torch.randint(0, c, (b, h, w), generator=g)
    if pattern == "same":
        labels = torch.ones_like(labels)
    labels[torch.rand(b, h, w, generator=g) < 0.05] = IGNORE
    if pattern in ("one", "none"):
        labels[:] = IGNORE
    if pattern == "one":
        labels[1, 17, 29] = 1
    return logits, labels.to(torch.uint8)


def sort_reference(keys):
    """numpy's stable descending argsort of uint32 keys [nseg, P] (given as int64 or int32 bit patterns) -> (sorted, perm) int64"""
    k = np.asarray(keys, dtype=np.int64) & 0xFFFFFFFF
    perm = np.argsort(-k, axis=-1, kind="stable")
    return np.take_along_axis(k, perm, -1), perm


def floor_key(check, group):
    return "%s.%s" % (check, group)


# fp32 floors (see the module docstring); measured by tests/test_lovasz_cpu.py over group_cases(group)
FLOOR = {
    "e.big": 9.1e-08,
    "e.c3": 1.1e-07,
    "e.c8": 9.1e-08,
    "e.img": 9.3e-08,
    "e.odd": 8.0e-08,
    "e.p1": 6.0e-08,
    "grad.big": 1.3e-06,
    "grad.c3": 4.8e-07,
    "grad.c8": 1.7e-07,
    "grad.img": 7.2e-07,
    "grad.odd": 4.9e-07,
    "grad.p1": 8.8e-08,
    "loss.big": 6.0e-08,
    "loss.c3": 6.0e-08,
    "loss.c8": 1.2e-07,
    "loss.img": 1.4e-07,
    "loss.odd": 6.0e-08,
    "loss.p1": 8.3e-08,
    "omega.big": 1.1e-07,
    "omega.c3": 6.0e-08,
    "omega.c8": 6.0e-08,
    "omega.img": 6.0e-08,
    "omega.odd": 6.0e-08,
    "omega.p1": 6.0e-08,
}
