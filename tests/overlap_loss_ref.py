"""float64 restatement of the region-overlap criteria (soft Dice / Tversky / focal-Tversky next to the weighted CE) of
csrc/loss.hip, with the seeded inputs and case lists that tests/test_overlap_loss_cpu.py (no GPU: ties the restatement to
float64 autograd, states the degenerate values, measures the fp32 floors, shows that the bounds see six mutants) and
tests/test_overlap_loss_gpu.py / tests/helpers/overlap_ddp_worker.py (the kernels) share.

Nothing here calls the product: torch on the CPU only.  The definition, written out again:

    V = pixels with y != ignore_index and 0 <= y < C;  p = softmax(z);  g_ic = [y_i == c]
    I_c = sum_V p_ic g_ic    P_c = sum_V p_ic    G_c = sum_V g_ic
    D_c = I_c + alpha (P_c - I_c) + beta (G_c - I_c) + s       T_c = (I_c + s) / D_c       l_c = max(1 - T_c, 0)^gamma
    L   = lce * sum_V w_y nll / sum_V w_y  +  lov * mean_{c in S} l_c          S = {c >= 1} ('foreground') or every class ('all')
    u_c = [c in S] / |S| * l'_c * (D_c - (I_c + s)(1 - alpha - beta)) / D_c^2         l'_c = -gamma (1 - T_c)^(gamma - 1),
    v_c = [c in S] / |S| * l'_c * (-alpha (I_c + s)) / D_c^2                                 0 where 1 - T_c <= 0
    q_ic = u_c g_ic + v_c
    dL/dz_ik = lce * w_y (p_ik - g_ik) / sum w  +  lov * p_ik (q_ik - sum_c p_ic q_ic)   on V,   exactly 0 elsewhere
lce == 0 leaves the CE term out altogether (so a batch without a valid pixel, where sum w == 0, has the finite value lov * L_ov).

FLOOR holds, per check, the error of THIS formula evaluated in float32 with stock torch ops on the CPU (dtype=torch.float32:
torch's fp32 log_softmax, fp32 sums, fp32 coefficients) against the float64 evaluation on the same inputs, the largest over
the check's cases, rounded up to two digits, and never below 2^-24 (each result is a stored fp32 value).  The GPU tests bound
every float comparison by 4 x FLOOR (the rule of tests/test_streaming_kernels_gpu.py); test_overlap_loss_cpu.py measures every
floor again and fails if a recorded figure is above 1.25 x or below half of what it measures.
"""
import functools

import torch
import torch.nn.functional as F

IGNORE = 255
FLOOR_MIN = 2.0 ** -24

# B, C, H, W
SHAPES = {
    "p1": (1, 2, 1, 1),              # one pixel
    "rag1": (2, 2, 13, 11),          # one ragged block
    "rag2": (1, 2, 33, 37),          # a second ragged block (1221 pixels)
    "img": (3, 2, 65, 65),           # image boundaries inside a thread's four pixels
    "c3": (1, 3, 7, 9),
    "c8": (2, 8, 9, 7),              # the register-path limit
}
CAP_SHAPE = (1, 2, 2897, 2897)       # 8 392 609 pixels > 8192 blocks x 1024: a second, ragged trip through the grid-stride loop
FIN_SHAPE = (4, 2, 515, 515)         # 1037 blocks: the finalize kernel's 16-deep load batch once (every lane), then its tail (13 lanes)
BIG = {"cap": CAP_SHAPE, "fin": FIN_SHAPE}          # uint8 labels, logits of order 1, CAP_COMBOS only
SCALES = {"s1": 1.0, "s30": 30.0}    # logits of order 1; |m| on both sides of the kernel's log-softmax split at 8
INPUT_CASES = [(sh, kind, sc) for sh in SHAPES for kind in ("u8", "i64") for sc in SCALES]
INPUT_IDS = ["%s_%s_%s" % c for c in INPUT_CASES]

# (alpha, beta, gamma)
PARAMS = {"dice": (0.5, 0.5, 1.0), "tversky": (0.3, 0.7, 1.0), "focal": (0.3, 0.7, 0.75), "focal2": (0.7, 0.3, 2.0)}
SMOOTH = 1.0
LOV = {0.0: 1.0, 1.0: 2.0}           # the overlap term's factor that goes with each CE factor (2: a lost factor shows)
# (class weights?, lce, parameter set, classes)
COMBOS = [(wt, lce, ps, cl) for wt in (False, True) for lce in (0.0, 1.0) for ps in PARAMS for cl in ("foreground", "all")]
CAP_COMBOS = [(True, 1.0, "tversky", "foreground"), (False, 0.0, "focal", "all")]
DEGENERATE = ["all_ignored", "no_foreground", "all_foreground"]
DEGEN_SHAPE = (2, 2, 13, 11)
# the inputs the mutants are shown on (and one more kernel case): three classes, ignore_index 2 -- a label value INSIDE [0, C), so
# "ignored pixels counted in G" is a different number -- class weights, CE + Tversky over the foreground
IG2_SHAPE, IG2_IGNORE, IG2_COMBO = (2, 3, 13, 11), 2, (True, 1.0, "tversky", "foreground")
MUTANTS = ["swap_alpha_beta", "ignored_in_P", "ignored_in_G", "no_pq_term", "no_s_in_numerator", "all_classes"]


def resolve(shape):
    """(B, C, H, W) of a key of SHAPES or BIG (or the tuple itself)"""
    return SHAPES.get(shape, BIG.get(shape, shape)) if isinstance(shape, str) else shape


def gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, scale, ignore_index=IGNORE, seed=0):
    """(logits fp32 [B,C,H,W] = randn * scale, labels [B,H,W], class weights fp32 [C]): about 10 % of the labels are
    ignore_index; with 8 pixels or more, int64 labels also carry -1 and C + 1 and uint8 labels values in [C, 254], all of
    which are invalid.  `shape`: a key of SHAPES / BIG or (B, C, H, W).  Shared and cached: callers must not write into the result."""
    b, c, h, w = shape = resolve(shape)
    g = gen(4000 + 31 * c + h * w + seed)
    logits = torch.randn(b, c, h, w, generator=g) * scale
    labels = torch.randint(0, c, (b, h, w), generator=g)
    r = torch.rand(b, h, w, generator=g)
    n = labels.numel()
    if n > 1:
        labels[r < 0.10] = ignore_index
    flat = labels.view(-1)
    if n >= 8:
        bad = (-1, -1, c + 1, c + 1) if kind == "i64" else (c, 254, min(c + 17, 254), c)
        for pos, v in zip((1, n // 3, n // 2, n - 1), bad):
            flat[pos] = v
    if kind == "u8":
        labels = labels.to(torch.uint8)
    weight = torch.rand(c, generator=g) * 2 + 0.5
    return logits, labels, weight


@functools.lru_cache(maxsize=None)
def degenerate_inputs(pattern, kind="u8"):
    logits, labels, weight = inputs(DEGEN_SHAPE, kind, 1.0, seed=5)
    fill = {"all_ignored": IGNORE, "no_foreground": 0, "all_foreground": 1}[pattern]
    return logits, torch.full_like(labels, fill), weight


@functools.lru_cache(maxsize=None)
def saturated_inputs(shape, kind):
    """logits +-40 by a seeded hard mask (class k = the pixel's predicted class gets +40, the others -40): every p is 0 or 1 to
    within 1e-34, so I_c, P_c, G_c are the integer true-positive, predicted and labelled counts over the valid pixels"""
    b, c, h, w = shape = resolve(shape)
    _, labels, _ = inputs(shape, kind, 1.0)
    pred = torch.randint(0, c, (b, h, w), generator=gen(77 + c + h))
    logits = torch.full((b, c, h, w), -40.0).scatter_(1, pred[:, None], 40.0)
    y = labels.long()
    ok = valid_mask(labels, c)
    counts = torch.zeros(3, c, dtype=torch.float64)
    for k in range(c):
        counts[0, k] = int((ok & (y == k) & (pred == k)).sum())
        counts[1, k] = int((ok & (pred == k)).sum())
        counts[2, k] = int((ok & (y == k)).sum())
    return logits, labels, counts.reshape(-1)


def valid_mask(labels, c, ignore_index=IGNORE):
    y = labels.long()
    return (y != ignore_index) & (y >= 0) & (y < c)


def overlap_ref(logits, labels, weight, ignore_index, lce, lov, alpha, beta, gamma, smooth, classes, dtype=torch.float64,
                mutant=None):
    """dict(sums = [sum w nll, sum w, I[C], P[C], G[C]], loss, grad [B,C,H,W]) of the module docstring's definition, in `dtype`.
    `mutant` (test_overlap_loss_cpu.py only) plants one of MUTANTS: a wrong formula the bounds must see."""
    b, c, h, w = logits.shape
    z = logits.to(dtype).permute(0, 2, 3, 1).reshape(-1, c)
    y = labels.reshape(-1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    logp = torch.log_softmax(z, 1) if dtype == torch.float32 else z - torch.logsumexp(z, 1, keepdim=True)
    p = torch.exp(logp)
    vm = valid[:, None].to(dtype)
    g = F.one_hot(yc, c).to(dtype) * vm
    wy = (weight.to(dtype)[yc] if weight is not None else torch.ones(z.shape[0], dtype=dtype)) * vm[:, 0]
    s1, s2 = (wy * -(logp * g).sum(1)).sum(), wy.sum()
    big_i, big_p, big_g = (p * g).sum(0), (p * vm).sum(0), g.sum(0)
    if mutant == "ignored_in_P":
        big_p = p.sum(0)
    if mutant == "ignored_in_G":
        inrange = (y >= 0) & (y < c)
        big_g = (F.one_hot(torch.where(inrange, y, torch.zeros_like(y)), c).to(dtype) * inrange[:, None].to(dtype)).sum(0)
    sums = torch.cat([torch.stack([s1, s2]), big_i, big_p, big_g])
    if mutant == "swap_alpha_beta":
        alpha, beta = beta, alpha
    num = big_i + (0.0 if mutant == "no_s_in_numerator" else smooth)
    den = big_i + alpha * (big_p - big_i) + beta * (big_g - big_i) + smooth
    om = 1.0 - num / den
    pos = om > 0
    oms = torch.where(pos, om, torch.ones_like(om))
    ell = torch.where(pos, oms ** gamma, torch.zeros_like(om))
    dell = torch.where(pos, -gamma * oms ** (gamma - 1.0), torch.zeros_like(om))
    sel = torch.ones(c, dtype=dtype)
    if classes == "foreground" and mutant != "all_classes":
        sel[0] = 0.0
    else:
        assert classes in ("foreground", "all")
    nsel = sel.sum()
    assert nsel > 0 and smooth > 0
    loss = lov * (sel * ell).sum() / nsel
    k = sel / nsel * dell / den ** 2
    u, v = k * (den - num * (1.0 - alpha - beta)), k * (-alpha * num)
    q = u[None] * g + v[None]
    dot = torch.zeros_like(p[:, :1]) if mutant == "no_pq_term" else (p * q).sum(1, keepdim=True)
    grad = lov * p * (q - dot)
    if lce != 0:
        loss = loss + lce * s1 / s2
        grad = grad + lce * wy[:, None] * (p - g) / s2
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    return dict(sums=sums, loss=loss, grad=grad.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous())


def combo_args(combo, weight):
    """(weight or None, (lce, lov, alpha, beta, gamma, smooth, classes)) of one COMBOS entry"""
    wt, lce, ps, cl = combo
    return (weight if wt else None), (lce, LOV[lce]) + PARAMS[ps] + (SMOOTH, cl)


def combo_id(combo):
    return "%s_ce%g_%s_%s" % ("w" if combo[0] else "now", combo[1], combo[2], combo[3])


@functools.lru_cache(maxsize=None)
def reference(shape, kind, scale, combo, ignore_index=IGNORE):
    logits, labels, weight = inputs(shape, kind, scale, ignore_index)
    wt, args = combo_args(combo, weight)
    return overlap_ref(logits, labels, wt, ignore_index, *args)


@functools.lru_cache(maxsize=None)
def degenerate_reference(pattern, combo, kind="u8"):
    logits, labels, weight = degenerate_inputs(pattern, kind)
    wt, args = combo_args(combo, weight)
    return overlap_ref(logits, labels, wt, IGNORE, *args)


def degenerate_combos(pattern):
    """every combination, except that without a valid pixel the CE term is 0 / 0 (as nn.CrossEntropyLoss has it): overlap only"""
    return [cb for cb in COMBOS if not (pattern == "all_ignored" and cb[1] != 0.0)]


def rel_err(a, e):
    """max |a - e| / max |e| (absolute where e is all zero)"""
    a, e = a.detach().double().reshape(-1), e.detach().double().reshape(-1)
    scale = float(e.abs().max())
    return float((a - e).abs().max()) / (scale if scale > 0 else 1.0)


def floor_key(check, group):
    return "%s.%s" % (check, group)


def group(shape, scale):
    """the floor group of an INPUT_CASES entry: one per shape and logit scale, over both label widths and every COMBOS entry"""
    return "%s_%s" % (shape, scale)


# fp32 floors (see the module docstring); measured by tests/test_overlap_loss_cpu.py.  Groups: <shape>_<scale> = the INPUT_CASES of that
# shape and logit scale, both label widths, every COMBOS entry; cap, fin = BIG; degen = no_foreground and all_foreground (all_ignored is exact: 0); ig2 = the
# mutants' inputs.
FLOOR = {
    "grad.c3_s1": 3.1e-07,
    "grad.c3_s30": 3.4e-07,
    "grad.c8_s1": 1.8e-07,
    "grad.c8_s30": 1.2e-06,
    "grad.cap": 5.1e-07,
    "grad.degen": 4.5e-07,
    "grad.fin": 4.7e-07,
    "grad.ig2": 1.7e-07,
    "grad.img_s1": 4.9e-07,
    "grad.img_s30": 5.7e-07,
    "grad.p1_s1": 2.8e-06,           # one pixel, overlap term only: 1 - T cancels to 1e-2 of its operands
    "grad.p1_s30": 6.0e-08,
    "grad.rag1_s1": 3.9e-07,
    "grad.rag1_s30": 4.4e-07,
    "grad.rag2_s1": 4.3e-07,
    "grad.rag2_s30": 4.5e-07,
    "loss.c3_s1": 1.1e-07,
    "loss.c3_s30": 1.7e-07,
    "loss.c8_s1": 7.6e-08,
    "loss.c8_s30": 1.5e-07,
    "loss.cap": 1.1e-07,
    "loss.degen": 2.2e-07,
    "loss.fin": 7.7e-08,
    "loss.ig2": 6.0e-08,
    "loss.img_s1": 1.7e-07,
    "loss.img_s30": 1.8e-07,
    "loss.p1_s1": 4.9e-06,           # the same cancellation
    "loss.p1_s30": 6.0e-08,
    "loss.rag1_s1": 1.2e-07,
    "loss.rag1_s30": 1.6e-07,
    "loss.rag2_s1": 7.2e-08,
    "loss.rag2_s30": 1.2e-07,
    "sums.c3_s1": 6.0e-08,
    "sums.c3_s30": 7.8e-08,
    "sums.c8_s1": 6.0e-08,
    "sums.c8_s30": 1.2e-07,
    "sums.cap": 7.4e-08,
    "sums.degen": 1.4e-07,
    "sums.fin": 6.0e-08,
    "sums.ig2": 6.0e-08,
    "sums.img_s1": 6.0e-08,
    "sums.img_s30": 1.0e-07,
    "sums.p1_s1": 6.0e-08,
    "sums.p1_s30": 6.0e-08,
    "sums.rag1_s1": 1.5e-07,
    "sums.rag1_s30": 7.4e-08,
    "sums.rag2_s1": 6.0e-08,
    "sums.rag2_s30": 9.1e-08,
}
