"""float64 restatement of the hard-pixel mining criterion (OHEM / bootstrapped cross-entropy) of csrc/loss.hip, with the seeded
inputs, case lists and fp32 floors that tests/test_ohem_cpu.py (no GPU: ties the restatement to float64 stock torch, states the
degenerate values, measures the floors, shows that the bounds see six mutants), tests/test_ohem_gpu.py and
tests/helpers/ohem_ddp_worker.py (the kernels) share.

Nothing here calls the product: torch on the CPU only.  The definition, written out again:

    V    = pixels with y != ignore_index and 0 <= y < C;   nll_i = -log_softmax(z_i)[y_i];   w = class weights (1 without)
    k    = min(min_kept, |V|)
    nu_k = the k-th largest nll over V (+inf if k == 0);   nu_0 = float32(-ln thresh), thresh in (0, 1];   nu = min(nu_0, nu_k)
    K    = {i in V : nll_i >= nu}                           every tie at nu is kept, so |K| >= k
    L    = sum_K w_y nll / sum_K w_y                        0 (and a zero gradient) if K is empty or sum_K w_y == 0
    dL/dz_ic = upstream * w_y (p_ic - [y_i == c]) / sum_K w_y   on K,   exactly 0 elsewhere

Where a kept set is compared, it is pinned: the kernels' keys and nu decide K on the GPU, a float64 nll decides it here, and the
two may differ only at pixels whose nll lies within the fp32 rounding of nu -- the band |nll64 - nu| <= BAND * max(1, nu), which may
hold at most BAND_MAX pixels.  Loss and gradient are then compared on ONE mask (`kept=` below), so no check is circular.

FLOOR holds, per check and group, the error of THIS formula evaluated in float32 with stock torch ops on the CPU (fp32
log_softmax, fp32 sums) on the float64 kept set, against the float64 evaluation, the largest over the group's cases, rounded up to
two digits and never below 2^-24 (each result is a stored fp32 value).  The GPU tests bound every float comparison by 4 x FLOOR;
test_ohem_cpu.py measures every floor again and fails if a recorded figure is above 1.25 x or below half of what it measures.
Errors are max |a - e| / max |e| (rel_err)."""
import functools
import math

import torch
import torch.nn.functional as F

IGNORE = 255
FLOOR_MIN = 2.0 ** -24
BAND = 4 * 2.0 ** -21
BAND_MAX = 4
SENTINEL = -1                        # the key of an invalid pixel

# random inputs: name -> ((B, C, H, W), logit scale); 5 % of the labels ignored
RANDOM = {
    "r2_s1": ((2, 2, 65, 65), 1.0),
    "r2_s30": ((2, 2, 65, 65), 30.0),
    "r3_s1": ((4, 3, 33, 47), 1.0),
    "r8_s30": ((2, 8, 65, 65), 30.0),
    "r2b_s1": ((3, 2, 17, 23), 1.0),
}
RANKS = {"k1": lambda nv: 1, "k10": lambda nv: nv // 10, "k3": lambda nv: nv // 3}
THRESH = (0.7, 1.0)
RANDOM_CASES = [(name, kind) for name in RANDOM for kind in ("u8", "i64")]

# edge shapes (logits of order 1), each with both label widths
SHAPES = {
    "p1": (1, 2, 1, 1),              # one pixel
    "odd": (1, 2, 31, 43),           # 1333 pixels: no multiple of 4, 256 or 1024; two ragged blocks
    "rag2": (1, 2, 33, 37),          # 1221 pixels: a second ragged block
    "img": (3, 2, 65, 65),           # image boundaries inside a thread's four pixels (4225 pixels per image)
    "c3": (1, 3, 7, 9),
    "c8": (2, 8, 9, 7),              # the register-path limit
    "fin": (4, 2, 515, 515),         # 1037 blocks: the finalize kernel's 16-deep load batch in every lane, then its tail
    "cap": (1, 2, 2897, 2897),       # 8 392 609 pixels > 8192 blocks x 1024: a second, ragged trip through the grid-stride loop
}
SHAPE_CASES = [(name, kind) for name in SHAPES for kind in ("u8", "i64")]
IG2_SHAPE, IG2_IGNORE = (2, 3, 13, 11), 2            # an ignore_index INSIDE [0, C)
MUTANTS = ["gt_at_tie", "k_plus_one", "ignored_in_k", "count_normaliser", "max_of_thresholds", "grad_on_dropped"]


def gen(seed):
    return torch.Generator().manual_seed(seed)


def nu0_of(thresh):
    """float32(-ln thresh); thresh = 1 gives +0"""
    assert 0.0 < thresh <= 1.0
    return float(torch.tensor(-math.log(thresh) + 0.0, dtype=torch.float32))


@functools.lru_cache(maxsize=None)
def inputs(shape, kind, scale, ignore_index=IGNORE, seed=0):
    """(logits fp32 [B,C,H,W] = randn * scale, labels [B,H,W], class weights fp32 [C]): about 5 % of the labels are ignore_index;
    with 8 pixels or more, int64 labels also carry -1 and C + 1 and uint8 labels values in [C, 254], all invalid.  Shared and
    cached: callers must not write into the result."""
    b, c, h, w = shape
    g = gen(9000 + 31 * c + h * w + seed)
    logits = torch.randn(b, c, h, w, generator=g) * scale
    labels = torch.randint(0, c, (b, h, w), generator=g)
    r = torch.rand(b, h, w, generator=g)
    n = labels.numel()
    if n > 1:
        labels[r < 0.05] = ignore_index
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


def pixel_terms(logits, labels, ignore_index, dtype=torch.float64):
    """flattened (pixel-major) log-probabilities [N, C], clamped labels, validity and nll [N] in `dtype`"""
    c = logits.shape[1]
    z = logits.to(dtype).permute(0, 2, 3, 1).reshape(-1, c)
    y = labels.reshape(-1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    logp = torch.log_softmax(z, 1) if dtype == torch.float32 else z - torch.logsumexp(z, 1, keepdim=True)
    nll = -logp.gather(1, yc[:, None])[:, 0]
    return logp, yc, valid, nll


def ohem_ref(logits, labels, weight, ignore_index, thresh, min_kept, dtype=torch.float64, upstream=1.0, kept=None, mutant=None,
             terms=None):
    """dict(nll [B,H,W], valid, k, nu, kept [B,H,W], sums = [sum_K w nll, sum_K w, |K|], loss, grad [B,C,H,W]) of the module
    docstring's definition in `dtype`.  kept: a mask [B,H,W] to use instead of the one this function selects (the pinned set).
    `mutant` (test_ohem_cpu.py only) plants one of MUTANTS: a wrong formula the checks must see.  terms: pixel_terms' result
    for these inputs and dtype, if the caller has it already."""
    b, c, h, w = logits.shape
    logp, yc, valid, nll = terms if terms is not None else pixel_terms(logits, labels, ignore_index, dtype)
    nv = int(valid.sum())
    in_k = valid
    if mutant == "ignored_in_k":                        # every in-range label takes part in the selection
        y = labels.reshape(-1).long()
        in_k = (y >= 0) & (y < c)
    k = min(int(min_kept), int(in_k.sum()))
    if mutant == "k_plus_one":
        k = min(k + 1, nv)
    nu_k = float(torch.sort(nll[in_k], descending=True).values[k - 1]) if k > 0 else math.inf
    nu0 = nu0_of(thresh)
    nu = max(nu0, nu_k) if mutant == "max_of_thresholds" else min(nu0, nu_k)
    if kept is None:
        kept = valid & ((nll > nu) if mutant == "gt_at_tie" else (nll >= nu))
    else:
        kept = kept.reshape(-1) & valid
    wy = weight.to(dtype)[yc] if weight is not None else torch.ones(nll.shape[0], dtype=dtype)
    km = kept.to(dtype)
    s1, s2, n = (wy * nll * km).sum(), (wy * km).sum(), int(kept.sum())
    norm = torch.tensor(float(n), dtype=dtype) if mutant == "count_normaliser" else s2
    any_kept = n > 0 and float(norm) > 0
    loss = s1 / norm if any_kept else torch.zeros((), dtype=dtype)
    g = F.one_hot(yc, c).to(dtype)
    on = valid if mutant == "grad_on_dropped" else kept
    grad = upstream * wy[:, None] * (torch.exp(logp) - g) / (norm if any_kept else 1.0)
    grad = torch.where(on[:, None] & torch.tensor(any_kept), grad, torch.zeros_like(grad))
    return dict(nll=nll.reshape(b, h, w), valid=valid.reshape(b, h, w), k=k, nu=nu, kept=kept.reshape(b, h, w),
                sums=torch.stack([s1, s2, torch.tensor(float(n), dtype=dtype)]), loss=loss,
                grad=grad.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous())


def rel_err(a, e):
    """max |a - e| / max |e| (absolute where e is all zero)"""
    a, e = a.detach().double().reshape(-1), e.detach().double().reshape(-1)
    if a.numel() == 0:
        return 0.0
    scale = float(e.abs().max())
    return float((a - e).abs().max()) / (scale if scale > 0 else 1.0)


def band_count(nll64, valid, nu):
    """valid pixels whose float64 nll lies within the fp32 rounding of nu: the only ones two correct selections may disagree on"""
    if not math.isfinite(nu) or nu == 0.0:             # nu = 0 keeps every valid pixel in any arithmetic (nll >= 0): no band
        return torch.zeros_like(valid)
    return valid & ((nll64 - nu).abs() <= BAND * max(1.0, nu))


def floors_of(logits, labels, weight, ignore_index, thresh, min_kept, upstream=1.0):
    """{check: error of the fp32 stock-torch evaluation against float64} on the float64 kept set -- what FLOOR records"""
    ref = ohem_ref(logits, labels, weight, ignore_index, thresh, min_kept, upstream=upstream)
    low = ohem_ref(logits, labels, weight, ignore_index, thresh, min_kept, dtype=torch.float32, upstream=upstream, kept=ref["kept"])
    v = ref["valid"]
    return {"keys": rel_err(low["nll"][v], ref["nll"][v]), "sums": rel_err(low["sums"][:2], ref["sums"][:2]),
            "loss": rel_err(low["loss"], ref["loss"]), "grad": rel_err(low["grad"], ref["grad"])}


def cases_of(nv):
    """the (k, thresh) grid of the random inputs"""
    return [(name, RANKS[name](nv), th) for name in RANKS for th in THRESH]


# ---- gap inputs: a hard population with nll in [1, 3] and an easy one with nll <= 0.1; nothing in between ------------------------
GAP_SHAPE = (2, 2, 37, 41)
GAP3_SHAPE = (1, 3, 29, 31)
GAP_NU0_THRESH = math.exp(-0.5)      # nu_0 = 0.5, inside the gap: nu_0 decides
GAP_NUK_THRESH = math.exp(-5.0)      # nu_0 = 5 > every nll: the k-th largest (the smallest hard nll) decides


@functools.lru_cache(maxsize=None)
def gap_inputs(shape, kind):
    """the true class's logit leads the others (all 0) by g: hard pixels (a third) have g in [-2.9, -0.6] at C = 2 (nll in
    [1.05, 2.95]; a little more at C = 3), easy ones g in [3, 6] (nll <= 0.1); 5 % ignored.  -> logits, labels, weights, #hard"""
    b, c, h, w = shape
    g = gen(700 + c + h)
    labels = torch.randint(0, c, (b, h, w), generator=g)
    hard = torch.rand(b, h, w, generator=g) < 1.0 / 3
    u = torch.rand(b, h, w, generator=g)
    lead = torch.where(hard, -2.9 + 2.3 * u, 3.0 + 3.0 * u)
    logits = torch.zeros(b, c, h, w).scatter_(1, labels[:, None], lead[:, None])
    labels[torch.rand(b, h, w, generator=g) < 0.05] = IGNORE
    nhard = int((hard & (labels != IGNORE)).sum())
    if kind == "u8":
        labels = labels.to(torch.uint8)
    return logits, labels, torch.tensor([0.7, 2.1, 1.3][:c]), nhard


GAP_CASES = [(sh, kind, wt, th) for sh in ("gap", "gap3") for kind in ("u8", "i64") for wt in (False, True)
             for th in ("nu0", "nuk")]
GAP_UPSTREAM = 0.37


def gap_case(case):
    sh, kind, wt, th = case
    logits, labels, weight, nhard = gap_inputs(GAP_SHAPE if sh == "gap" else GAP3_SHAPE, kind)
    return logits, labels, (weight if wt else None), nhard, (GAP_NU0_THRESH if th == "nu0" else GAP_NUK_THRESH)


# ---- inputs for the exact selection ----------------------------------------------------------------------------------------------
def tie_inputs(pattern):
    """four: logits drawn from four values, so the nll take a handful of values and every rank falls inside a tie group of
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
        labels = torch.zeros_like(labels)
    labels[torch.rand(b, h, w, generator=g) < 0.05] = IGNORE
    if pattern in ("one", "none"):
        labels[:] = IGNORE
    if pattern == "one":
        labels[1, 17, 29] = 1
    return logits, labels.to(torch.uint8)


def span_inputs():
    """the true class leads or trails by a gap spread evenly over [-80, 69]: the float64 nll runs from 1e-30 to 80.  (In fp32 the
    sum of exponentials rounds to 1 once the lead passes 17, so the kernel's own keys are 0 there: span_keys covers the rest.)"""
    b, c, h, w = 1, 2, 97, 89
    g = gen(56)
    labels = torch.randint(0, c, (b, h, w), generator=g)
    lead = torch.rand(b, h, w, generator=g) * 149.0 - 80.0
    logits = torch.zeros(b, c, h, w).scatter_(1, labels[:, None], lead[:, None])
    labels[torch.rand(b, h, w, generator=g) < 0.05] = IGNORE
    return logits, labels.to(torch.uint8)


def span_keys():
    """keys made by hand (int32 bit patterns of non-negative floats, -1 = invalid): log-uniform from 1e-30 to 80 plus zeros,
    denormals, +inf and runs of equal values -- every bit of every digit takes both values"""
    g = gen(57)
    n = 40000
    v = torch.exp(torch.rand(n, generator=g, dtype=torch.float64) * (math.log(80.0) - math.log(1e-30)) + math.log(1e-30)).float()
    v[:50] = 0.0
    v[50:60] = 1e-42
    v[60:63] = float("inf")
    v[100:2100] = v[100]
    keys = v.view(torch.int32).clone()
    keys[torch.rand(n, generator=g) < 0.05] = SENTINEL
    return keys[torch.randperm(n, generator=g)].contiguous()


BIG = ("fin", "cap")                 # one case per label width; their band may hold more than BAND_MAX pixels (8e6 x 4e-6 x density)
GROUPS = list(RANDOM) + list(SHAPES) + ["ig2", "gap"]


@functools.lru_cache(maxsize=None)
def group_cases(group):
    """every case a FLOOR group covers: (tag, logits, labels, weight or None, ignore_index, thresh, min_kept, upstream)"""
    out = []
    if group in RANDOM:
        shape, scale = RANDOM[group]
        for kind in ("u8", "i64"):
            logits, labels, weight = inputs(shape, kind, scale)
            nv = int(valid_mask(labels, shape[1]).sum())
            for name, k, th in cases_of(nv):
                for wt in (None, weight):
                    tag = "%s_%s_t%g_%s" % (kind, name, th, "now" if wt is None else "w")
                    out.append((tag, logits, labels, wt, IGNORE, th, k, 1.0))
    elif group in SHAPES or group == "ig2":
        shape, ig = (IG2_SHAPE, IG2_IGNORE) if group == "ig2" else (SHAPES[group], IGNORE)
        for kind in ("u8", "i64"):
            logits, labels, weight = inputs(shape, kind, 1.0, ig)
            nv = int(valid_mask(labels, shape[1], ig).sum())
            ths = ((0.7,) if kind == "u8" else (1.0,)) if group in BIG else (0.7, 1.0)
            for th in ths:
                out.append(("%s_k%d_t%g" % (kind, nv // 3, th), logits, labels, weight, ig, th, nv // 3, 1.0))
    elif group == "gap":
        for case in GAP_CASES:
            logits, labels, wt, nhard, th = gap_case(case)
            out.append(("%s_%s_%s_%s" % (case[0], case[1], "w" if case[2] else "now", case[3]), logits, labels, wt, IGNORE, th,
                        nhard, GAP_UPSTREAM))
    else:
        raise KeyError(group)
    return out


@functools.lru_cache(maxsize=None)
def group_reference(group, index):
    _, logits, labels, wt, ig, th, k, up = group_cases(group)[index]
    return ohem_ref(logits, labels, wt, ig, th, k, upstream=up)


def floor_key(check, group):
    return "%s.%s" % (check, group)


# fp32 floors (see the module docstring); measured by tests/test_ohem_cpu.py.  Groups: the RANDOM names (both label widths, every
# cases_of entry, with and without class weights), the SHAPES names and ig2 (both label widths, k = |V| / 3 at thresh 0.7 and
# thresh 1, with class weights), gap (every GAP_CASES entry, upstream GAP_UPSTREAM).
FLOOR = {
    "grad.c3": 1.9e-07,
    "grad.c8": 9.6e-08,
    "grad.cap": 2.1e-07,
    "grad.fin": 2.3e-07,
    "grad.gap": 2.0e-07,
    "grad.ig2": 1.6e-07,
    "grad.img": 2.1e-07,
    "grad.odd": 1.4e-07,
    "grad.p1": 6.3e-08,
    "grad.r2_s1": 1.8e-07,
    "grad.r2_s30": 1.9e-07,
    "grad.r2b_s1": 1.7e-07,
    "grad.r3_s1": 1.9e-07,
    "grad.r8_s30": 2.5e-07,
    "grad.rag2": 2.1e-07,
    "keys.c3": 6.0e-08,
    "keys.c8": 6.5e-08,
    "keys.cap": 7.1e-08,
    "keys.fin": 7.8e-08,
    "keys.gap": 6.0e-08,
    "keys.ig2": 6.0e-08,
    "keys.img": 7.4e-08,
    "keys.odd": 7.8e-08,
    "keys.p1": 6.0e-08,
    "keys.r2_s1": 6.9e-08,
    "keys.r2_s30": 6.0e-08,
    "keys.r2b_s1": 6.0e-08,
    "keys.r3_s1": 8.1e-08,
    "keys.r8_s30": 6.0e-08,
    "keys.rag2": 6.0e-08,
    "loss.c3": 1.5e-07,
    "loss.c8": 1.3e-07,
    "loss.cap": 1.3e-07,
    "loss.fin": 1.9e-07,
    "loss.gap": 1.2e-07,
    "loss.ig2": 1.1e-07,
    "loss.img": 6.0e-08,
    "loss.odd": 6.0e-08,
    "loss.p1": 6.0e-08,
    "loss.r2_s1": 6.9e-08,
    "loss.r2_s30": 6.0e-08,
    "loss.r2b_s1": 1.3e-07,
    "loss.r3_s1": 7.7e-08,
    "loss.r8_s30": 6.0e-08,
    "loss.rag2": 1.1e-07,
    "sums.c3": 7.4e-08,
    "sums.c8": 7.2e-08,
    "sums.cap": 7.9e-08,
    "sums.fin": 1.1e-07,
    "sums.gap": 9.5e-08,
    "sums.ig2": 7.0e-08,
    "sums.img": 6.5e-08,
    "sums.odd": 6.0e-08,
    "sums.p1": 6.0e-08,
    "sums.r2_s1": 6.7e-08,
    "sums.r2_s30": 9.9e-08,
    "sums.r2b_s1": 1.6e-07,
    "sums.r3_s1": 8.3e-08,
    "sums.r8_s30": 7.0e-08,
    "sums.rag2": 9.5e-08,
}
