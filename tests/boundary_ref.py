"""Restatement of the signed squared Euclidean distance map and of the boundary (distance-map) criterion of csrc/boundary.hip,
with the label generators, seeded inputs and case lists that tests/test_boundary_cpu.py (no GPU: brute force against scipy, the
restatement against float64 autograd, the fp32 floors, eight mutants) and tests/test_boundary_gpu.py /
tests/helpers/boundary_ddp_worker.py (the kernels) share.  Logits, seeds, shapes, the validity rule and the error measure are
tests/overlap_loss_ref.py's, imported.

Nothing here calls the product: numpy, scipy and torch on the CPU only.  The definition, written out again:

    K = {1 .. C-1} ('foreground') or {0 .. C-1} ('all');  valid: y != ignore_index and 0 <= y < C;  per image n and class c of K
    F = {p : y_p == c and valid}     G = {p : valid and y_p != c}     (invalid pixels in neither)
    d2(p, S) = min over q in S of (px-qx)^2 + (py-qy)^2
    sd2(p) = +d2(p, F) on G,  -d2(p, G) on F,  0 at invalid pixels,  0 over the whole plane when F or G is empty
    phi = sqrt(sd2) where sd2 > 0,  -(sqrt(-sd2) - 1) where sd2 < 0,  0 elsewhere;  clamped to [-D, D] when clip D > 0
    V = valid pixels, N = |V|, p = softmax(z), g_ic = [y_i == c]
    L = lce * sum_V w_y nll / sum_V w_y  +  lbd * sum_V sum_{c in K} p_ic phi_ic / (N |K|)
    dL/dz_ik = lce * w_y (p_ik - g_ik) / sum_V w + lbd / (N |K|) * p_ik ([k in K] phi_ik - sum_{c in K} p_ic phi_ic) on V, else 0
lce == 0 leaves the CE term out altogether (finite without a valid pixel); N == 0 makes the boundary term and its gradient 0.

The map has two restatements: edt_brute (numpy integers, every pixel against every pixel of the other set, planes up to
BRUTE_MAX pixels) and edt_scipy (scipy.ndimage.distance_transform_edt of the array whose zeros are F, and of the one whose zeros
are G, squared and rounded: a squared Euclidean distance between grid points is an integer, and the float64 distance of
scipy is within 1e-9 of its root at these sizes).  test_boundary_cpu.py shows them equal on every small case.

Labels have structure (PATTERNS): independent random labels put every pixel within two pixels of the other set, |phi| <= 2, and a
wrong distance would hide in the rounding of the loss.  The band pattern at 65 x 65 reaches |phi| > 30.  On top of the
pattern, label_case() sprinkles 5 % ignore_index and the four invalid values of overlap_loss_ref.inputs.

FLOOR holds, per check, the error of THIS formula evaluated in float32 with stock torch ops on the CPU (phi from
sd2.float().sqrt(), torch's fp32 log_softmax, fp32 sums and coefficients) against the float64 evaluation on the same inputs and the
same exact map, the largest over the check's cases, rounded up to two digits, and never below 2^-24.  The GPU tests bound every
float comparison by 4 x FLOOR; test_boundary_cpu.py measures every floor again and fails if a recorded figure is above 1.25 x
or below half of what it measures.  The boundary sum's error is taken relative to sum_V sum_K |p phi| (key "abs_bd" of the
reference): the term's signs cancel, so its own value is the wrong scale.  N is compared exactly and has no floor.
"""
import functools

import numpy as np
import torch

from tests.overlap_loss_ref import BIG, FLOOR_MIN, IG2_IGNORE, IGNORE, SCALES, SHAPES, gen, inputs, rel_err, resolve, valid_mask

BRUTE_MAX = 5000                                  # pixels of a plane the O(n^2) map is run on
PATTERNS = ("blobs", "bands", "corner_fg", "one_bg", "full_row", "checker", "ignore_frame", "out_of_range")
CLASSES = ("foreground", "all")
CLIPS = (0.0, 8.0)
# (class weights?, lce, lbd, clip): CE + boundary with a factor a lost weight shows in, and the boundary term alone
COMBOS = [(wt, lce, lbd, clip) for wt in (False, True) for lce, lbd in ((1.0, 2.0), (0.0, 1.0)) for clip in CLIPS]
INPUT_CASES = [(sh, kind, sc) for sh in SHAPES for kind in ("u8", "i64") for sc in SCALES]
INPUT_IDS = ["%s_%s_%s" % c for c in INPUT_CASES]
SHAPE_PATTERN = {"p1": ("corner_fg",), "rag1": ("bands", "blobs"), "rag2": ("blobs",), "img": ("bands", "blobs", "ignore_frame"),
                 "c3": ("blobs",), "c8": ("blobs", "bands"), "cap": ("bands",), "fin": ("bands", "blobs", "ignore_frame", "checker")}
BIG_COMBO = (True, 1.0, 2.0, 8.0)                 # cap and fin: uint8 labels, logits of order 1, the map from scipy
DEGENERATE = ["all_ignored", "no_foreground", "all_foreground"]
DEGEN_SHAPE = (2, 2, 13, 11)
# the mutants' inputs: three classes with ignore_index 2 (IG2_IGNORE), a label value INSIDE [0, C): an image that is foreground
# but for one pixel (inside distances up to 28, beyond the clamp at 8) and a band whose right half is labelled 2 (invalid)
IG2_SHAPE = (2, 3, 33, 35)
IG2_COMBOS = [(True, 1.0, 2.0, 0.0), (True, 1.0, 2.0, 8.0)]
IG2_PATTERNS = ("one_bg", "bands")
CHECKS = ("s_nll", "s_w", "s_bd", "loss", "grad")
MAP_MUTANTS = ["cityblock", "column_only", "invalid_as_background"]
FORMULA_MUTANTS = ["sign_flipped_inside", "no_minus_one", "mean_over_all_pixels", "no_K", "clamp_before_minus_one"]

# the planes the map kernels are run on: name -> (B, C, H, W, patterns of the images in turn (None: every pattern, one per run))
MAP_SHAPES = {
    "1x1": (1, 2, 1, 1, None), "1x9": (1, 2, 1, 9, None), "9x1": (1, 2, 9, 1, None), "2x2": (1, 2, 2, 2, None),
    "5x255": (1, 2, 5, 255, None), "5x256": (1, 2, 5, 256, None), "5x257": (1, 2, 5, 257, None),   # the row block's thread stride
    "b3_65": (3, 2, 65, 65, ("bands", "blobs", "ignore_frame")),                  # leaks across images
    "b3_65r": (3, 2, 65, 65, ("one_bg", "checker", "corner_fg")),
    "33x300": (2, 2, 33, 300, None),
    "3x2897": (1, 2, 3, 2897, ("bands",)), "2897x3": (1, 2, 2897, 3, ("bands",)),  # longer than any chunk of rows or columns
    "3xfull": (1, 2, 3, 2897, ("full_row",)), "fullx3": (1, 2, 2897, 3, ("corner_fg",)),
    "c3": (2, 3, 19, 23, None),                                                    # leaks across class planes
}


def selected(c, classes):
    assert classes in CLASSES
    return list(range(1 if classes == "foreground" else 0, c))


def pattern(name, h, w, c=2, seed=0, ignore_index=IGNORE):
    """int64 [h, w] labels of one of PATTERNS (classes 1 .. c-1 in turn where the pattern has more than one piece)"""
    rng = np.random.default_rng(1000 + 7 * seed + h * w)
    yy, xx = np.mgrid[0:h, 0:w]
    lab = np.zeros((h, w), np.int64)
    fg = lambda k: 1 + k % max(c - 1, 1) if c > 1 else 0
    if name in ("blobs", "out_of_range"):
        for k in range(3 + seed % 2):
            cy, cx, r = rng.uniform(0, h), rng.uniform(0, w), rng.uniform(0.08, 0.22) * max(h, w)
            lab[(yy - cy) ** 2 + (xx - cx) ** 2 <= r * r] = fg(k)
        if name == "out_of_range":
            lab[(yy + 2 * xx) % 11 == 3] = c + (seed % 3)          # a lattice of values that are no class index
    elif name == "bands":
        mid = 0.10 * h + 0.05 * h * np.sin(xx * 6.2832 / max(w, 2) + seed)        # a thin wavy band near the top: the bottom is far
        lab[np.abs(yy - mid) <= 1.0] = 1
        if c > 2:
            lab[(lab == 1) & (xx > w // 2)] = 2
        if w == 1 or h <= 3:                                        # a plane too thin for a band along x: a few pixels of it
            lab[:] = 0
            lab[h // 7, :max(1, w // 9)] = 1
    elif name == "corner_fg":
        lab[0, 0] = fg(seed)
    elif name == "one_bg":
        lab[:] = fg(seed)
        lab[h // 2, w // 3] = 0
    elif name == "full_row":
        lab[h // 2, :] = fg(seed)
    elif name == "checker":
        lab = (yy + xx) % max(c, 2) if c > 1 else lab
    elif name == "ignore_frame":
        f = max(1, min(h, w) // 8)                                  # the frame a padded crop leaves, the mask touching it
        lab[f:max(f + 1, h // 2), f:max(f + 1, (2 * w) // 3)] = fg(seed)
        frame = (yy < f) | (yy >= h - f) | (xx < f) | (xx >= w - f)
        lab[frame] = ignore_index
    else:
        raise KeyError(name)
    return lab


@functools.lru_cache(maxsize=None)
def map_labels(shape_name, pat, kind, ignore_index=IGNORE):
    """labels [B,H,W] of a MAP_SHAPES entry: its own pattern list, or `pat` in every image with another seed"""
    b, c, h, w, pats = MAP_SHAPES[shape_name]
    planes = [pattern((pats[i % len(pats)] if pats else pat), h, w, c, seed=i, ignore_index=ignore_index) for i in range(b)]
    lab = torch.from_numpy(np.stack(planes))
    if kind == "i64":
        flat = lab.view(-1)
        if flat.numel() >= 8:
            flat[flat.numel() // 3] = -1                            # an int64 label below the class range
    return lab.to(torch.uint8) if kind == "u8" else lab


def map_runs(shape_name):
    return MAP_SHAPES[shape_name][4] and ("own",) or PATTERNS


@functools.lru_cache(maxsize=None)
def label_case(shape, kind, ignore_index=IGNORE, patterns=None, seed=0):
    """structured labels [B,H,W] for a criterion case: SHAPE_PATTERN's patterns over the images, then 5 % ignore_index and,
    with 8 pixels or more, the four invalid values overlap_loss_ref.inputs plants.  Shared and cached: do not write into it."""
    name = shape if isinstance(shape, str) else None
    b, c, h, w = resolve(shape)
    pats = patterns or SHAPE_PATTERN.get(name, ("bands", "blobs"))
    lab = torch.from_numpy(np.stack([pattern(pats[i % len(pats)], h, w, c, seed=i + seed, ignore_index=ignore_index)
                                     for i in range(b)]))
    n = lab.numel()
    if n > 1:
        lab[torch.rand(b, h, w, generator=gen(900 + h * w + seed)) < 0.05] = ignore_index
    flat = lab.view(-1)
    if n >= 8:
        bad = (-1, -1, c + 1, c + 1) if kind == "i64" else (c, 254, min(c + 17, 254), c)
        for pos, v in zip((1, n // 3, n // 2, n - 1), bad):
            flat[pos] = v
    return lab.to(torch.uint8) if kind == "u8" else lab


def _sets(lab, c, cls, ignore_index, mutant=None):
    """(F, G) of one image (numpy int64 [H,W]) and class"""
    valid = (lab != ignore_index) & (lab >= 0) & (lab < c)
    f = valid & (lab == cls)
    g = valid & (lab != cls)
    if mutant == "invalid_as_background":
        g = ~f
    return f, g


def _d2_brute(h, w, member, mutant=None):
    """int64 [H,W]: min over q in `member` of the squared distance (a large number where member is empty)"""
    qy, qx = np.nonzero(member)
    out = np.full((h, w), 1 << 40, np.int64)
    if qy.size == 0:
        return out
    py, px = np.mgrid[0:h, 0:w]
    py, px = py.reshape(-1), px.reshape(-1)
    res = np.empty(py.size, np.int64)
    step = max(1, (1 << 22) // qy.size)
    for s in range(0, py.size, step):
        dy, dx = np.abs(py[s:s + step, None] - qy[None]), np.abs(px[s:s + step, None] - qx[None])
        if mutant == "cityblock":
            d = (dy + dx) ** 2
        elif mutant == "column_only":
            d = np.where(dx == 0, dy * dy, 1 << 40)
        else:
            d = dy * dy + dx * dx
        res[s:s + step] = d.min(1)
    return res.reshape(h, w)


def _d2_scipy(h, w, member):
    from scipy.ndimage import distance_transform_edt
    if not member.any():
        return np.full((h, w), 1 << 40, np.int64)
    d = distance_transform_edt(~member)
    return np.rint(d * d).astype(np.int64)


def signed_edt_ref(labels, c, classes="foreground", ignore_index=IGNORE, how="auto", mutant=None):
    """int32 tensor [B, |K|, H, W] of the module docstring's definition.  how: 'brute', 'scipy' or 'auto' (brute up to BRUTE_MAX
    pixels a plane).  `mutant` (test_boundary_cpu.py only, brute force) plants one of MAP_MUTANTS."""
    lab = labels.long().numpy()
    b, h, w = lab.shape
    ks = selected(c, classes)
    if how == "auto":
        how = "brute" if h * w <= BRUTE_MAX else "scipy"
    assert mutant is None or how == "brute"
    d2 = (lambda m: _d2_brute(h, w, m, mutant)) if how == "brute" else (lambda m: _d2_scipy(h, w, m))
    out = np.zeros((b, len(ks), h, w), np.int64)
    for n in range(b):
        for j, cls in enumerate(ks):
            f, g = _sets(lab[n], c, cls, ignore_index, mutant)
            if mutant == "column_only":                                 # (a column without the other set keeps 0)
                df, dg = d2(f), d2(g)
                df[df >= 1 << 40], dg[dg >= 1 << 40] = 0, 0
                out[n, j] = np.where(g, df, 0) - np.where(f, dg, 0)
                continue
            if not f.any() or not g.any():
                continue
            out[n, j] = np.where(g, d2(f), 0) - np.where(f, d2(g), 0)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return torch.from_numpy(out.astype(np.int32))


def phi_of(sd2, clip, dtype=torch.float64, mutant=None):
    """the signed distance the probabilities are weighted by, from the integer map"""
    s = sd2.to(dtype)
    root = s.abs().sqrt()
    inside = -(root - 1.0)
    if mutant == "sign_flipped_inside":
        inside = root - 1.0
    if mutant == "no_minus_one":
        inside = -root
    if mutant == "clamp_before_minus_one" and clip > 0:
        inside = -(root.clamp(max=clip) - 1.0)
    phi = torch.where(sd2 > 0, root, torch.where(sd2 < 0, inside, torch.zeros_like(s)))
    return phi.clamp(-clip, clip) if clip > 0 else phi


def boundary_ref(logits, labels, sd2, weight, ignore_index, lce, lbd, clip, classes, dtype=torch.float64, mutant=None):
    """dict(sums = [sum w nll, sum w, sum p phi, N] (float64), abs_bd = sum |p phi|, loss, ce, bd, grad [B,C,H,W]) of the module
    docstring's definition, in `dtype`, on the integer map sd2 [B,|K|,H,W].  `mutant` plants one of FORMULA_MUTANTS."""
    b, c, h, w = logits.shape
    ks = selected(c, classes)
    assert tuple(sd2.shape) == (b, len(ks), h, w)
    z = logits.to(dtype).permute(0, 2, 3, 1).reshape(-1, c)
    y = labels.reshape(-1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    logp = torch.log_softmax(z, 1) if dtype == torch.float32 else z - torch.logsumexp(z, 1, keepdim=True)
    p = torch.exp(logp)
    vm = valid[:, None].to(dtype)
    g = torch.nn.functional.one_hot(yc, c).to(dtype) * vm
    wy = (weight.to(dtype)[yc] if weight is not None else torch.ones(z.shape[0], dtype=dtype)) * vm[:, 0]
    s1, s2 = (wy * -(logp * g).sum(1)).sum(), wy.sum()
    phi = torch.zeros(z.shape[0], c, dtype=dtype)
    phi[:, ks] = phi_of(sd2, clip, dtype, mutant).permute(0, 2, 3, 1).reshape(-1, len(ks))
    pphi = p * phi * vm
    sbd, abs_bd = pphi.sum(), pphi.abs().sum()
    n = int(valid.sum())
    den = float(y.numel() if mutant == "mean_over_all_pixels" else n) * (1 if mutant == "no_K" else len(ks))
    zero = torch.zeros((), dtype=dtype)
    bd = lbd * sbd / den if n > 0 else zero
    gfac = lbd / den if n > 0 else 0.0
    grad = gfac * p * (phi - (p * phi).sum(1, keepdim=True))
    ce = zero
    if lce != 0:
        ce = lce * s1 / s2
        grad = grad + lce * wy[:, None] * (p - g) / s2
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    sums = torch.stack([s1.double(), s2.double(), sbd.double(), torch.tensor(float(n), dtype=torch.float64)])
    return dict(sums=sums, abs_bd=float(abs_bd), loss=ce + bd, ce=ce, bd=bd,
                grad=grad.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous())


def combo_args(combo, weight):
    """(weight or None, lce, lbd, clip) of one COMBOS entry"""
    wt, lce, lbd, clip = combo
    return (weight if wt else None), lce, lbd, clip


def combo_id(combo):
    return "%s_ce%g_bd%g_clip%g" % ("w" if combo[0] else "now", combo[1], combo[2], combo[3])


def case_classes(shape):
    """two-class shapes run over the foreground plane; c3 over every class, c8 over the foreground classes"""
    return "all" if shape == "c3" else "foreground"


@functools.lru_cache(maxsize=None)
def case(shape, kind, scale, ignore_index=IGNORE, patterns=None):
    """(logits, labels, class weights, exact map, classes) of a criterion case; shared and cached: do not write into them"""
    logits, _, weight = inputs(shape, kind, scale, ignore_index)
    labels = label_case(shape, kind, ignore_index, patterns)
    classes = case_classes(shape)
    return logits, labels, weight, signed_edt_ref(labels, logits.shape[1], classes, ignore_index), classes


@functools.lru_cache(maxsize=None)
def reference(shape, kind, scale, combo, ignore_index=IGNORE, patterns=None):
    logits, labels, weight, sd2, classes = case(shape, kind, scale, ignore_index, patterns)
    wt, lce, lbd, clip = combo_args(combo, weight)
    return boundary_ref(logits, labels, sd2, wt, ignore_index, lce, lbd, clip, classes)


@functools.lru_cache(maxsize=None)
def degenerate_case(pattern_name, kind="u8"):
    logits, labels, weight = inputs(DEGEN_SHAPE, kind, 1.0, seed=5)
    fill = {"all_ignored": IGNORE, "no_foreground": 0, "all_foreground": 1}[pattern_name]
    labels = torch.full_like(labels, fill)
    return logits, labels, weight, signed_edt_ref(labels, 2, "foreground", IGNORE), "foreground"


@functools.lru_cache(maxsize=None)
def degenerate_reference(pattern_name, combo, kind="u8"):
    logits, labels, weight, sd2, classes = degenerate_case(pattern_name, kind)
    wt, lce, lbd, clip = combo_args(combo, weight)
    return boundary_ref(logits, labels, sd2, wt, IGNORE, lce, lbd, clip, classes)


def degenerate_combos(pattern_name):
    """every combination, except that without a valid pixel the CE term is 0 / 0 (as nn.CrossEntropyLoss has it): boundary only"""
    return [cb for cb in COMBOS if not (pattern_name == "all_ignored" and cb[1] != 0.0)]


def errors(got_sums, got_loss, got_grad, ref):
    """{check: error} of CHECKS: the CE sums by their own scale, the boundary sum by sum |p phi|, the loss, the gradient by the
    largest float64 gradient entry"""
    gs = got_sums.detach().double().cpu().reshape(-1)
    e = {"s_nll": rel_err(gs[0], ref["sums"][0]), "s_w": rel_err(gs[1], ref["sums"][1])}
    e["s_bd"] = abs(float(gs[2]) - float(ref["sums"][2])) / (ref["abs_bd"] if ref["abs_bd"] > 0 else 1.0)
    e["loss"] = rel_err(got_loss.reshape(()), ref["loss"])
    e["grad"] = rel_err(got_grad, ref["grad"])
    return e


def floor_key(check, group):
    return "%s.%s" % (check, group)


def group(shape, scale):
    """the floor group of an INPUT_CASES entry: one per shape and logit scale, over both label widths and every COMBOS entry"""
    return "%s_%s" % (shape, scale)


@functools.lru_cache(maxsize=None)
def ddp_inputs():
    """the batch of 4 of tests/helpers/boundary_ddp_worker.py: (logits, labels, weight, exact map); the first half (rank 0's) is
    all ignored, so a per-rank N or sum w would differ from the global batch's"""
    g = gen(29)
    logits = torch.randn(4, 2, 65, 65, generator=g)
    labels = label_case((4, 2, 65, 65), "u8", IGNORE, ("bands", "blobs", "ignore_frame", "blobs"), seed=3).clone()
    labels[:2] = IGNORE
    return logits, labels, torch.tensor([1.0, 3.0]), signed_edt_ref(labels, 2, "foreground", IGNORE)


DDP_COMBO = (True, 1.0, 2.0, 8.0)


@functools.lru_cache(maxsize=None)
def ddp_reference():
    logits, labels, weight, sd2 = ddp_inputs()
    return boundary_ref(logits, labels, sd2, weight, IGNORE, DDP_COMBO[1], DDP_COMBO[2], DDP_COMBO[3], "foreground")


# fp32 floors (see the module docstring); measured by tests/test_boundary_cpu.py.  Groups: <shape>_<scale> = the INPUT_CASES of that
# shape and logit scale, both label widths, every COMBOS entry; cap, fin = BIG with BIG_COMBO; degen = no_foreground and
# all_foreground (all_ignored is exact: 0); ig2 = the mutants' inputs with IG2_COMBOS; ddp = the inputs of
# tests/helpers/boundary_ddp_worker.py.
FLOOR = {
    "grad.c3_s1": 1.2e-07,
    "grad.c3_s30": 3.1e-07,
    "grad.c8_s1": 1.4e-07,
    "grad.c8_s30": 3.3e-07,
    "grad.cap": 3.5e-07,
    "grad.ddp": 2.5e-07,
    "grad.degen": 2.6e-07,
    "grad.fin": 3.7e-07,
    "grad.ig2": 1.7e-07,
    "grad.img_s1": 3.4e-07,
    "grad.img_s30": 3.8e-07,
    "grad.p1_s1": 6.0e-08,
    "grad.p1_s30": 6.0e-08,
    "grad.rag1_s1": 2.7e-07,
    "grad.rag1_s30": 4.7e-07,
    "grad.rag2_s1": 2.5e-07,
    "grad.rag2_s30": 3.3e-07,
    "loss.c3_s1": 9.7e-08,
    "loss.c3_s30": 1.1e-07,
    "loss.c8_s1": 9.8e-08,
    "loss.c8_s30": 6.0e-08,
    "loss.cap": 6.0e-08,
    "loss.ddp": 9.1e-08,
    "loss.degen": 2.2e-07,
    "loss.fin": 9.6e-08,
    "loss.ig2": 8.8e-08,
    "loss.img_s1": 6.1e-08,
    "loss.img_s30": 2.5e-07,
    "loss.p1_s1": 9.3e-08,
    "loss.p1_s30": 6.0e-08,
    "loss.rag1_s1": 6.0e-08,
    "loss.rag1_s30": 2.6e-07,
    "loss.rag2_s1": 1.3e-07,
    "loss.rag2_s30": 9.3e-08,
    "s_bd.c3_s1": 6.9e-08,
    "s_bd.c3_s30": 7.4e-08,
    "s_bd.c8_s1": 6.0e-08,
    "s_bd.c8_s30": 6.0e-08,
    "s_bd.cap": 6.0e-08,
    "s_bd.ddp": 6.0e-08,
    "s_bd.degen": 6.0e-08,
    "s_bd.fin": 6.0e-08,
    "s_bd.ig2": 6.0e-08,
    "s_bd.img_s1": 6.0e-08,
    "s_bd.img_s30": 6.0e-08,
    "s_bd.p1_s1": 6.0e-08,
    "s_bd.p1_s30": 6.0e-08,
    "s_bd.rag1_s1": 8.5e-08,
    "s_bd.rag1_s30": 6.0e-08,
    "s_bd.rag2_s1": 7.8e-08,
    "s_bd.rag2_s30": 6.0e-08,
    "s_nll.c3_s1": 6.0e-08,
    "s_nll.c3_s30": 6.0e-08,
    "s_nll.c8_s1": 9.4e-08,
    "s_nll.c8_s30": 6.0e-08,
    "s_nll.cap": 6.0e-08,
    "s_nll.ddp": 1.2e-07,
    "s_nll.degen": 9.5e-08,
    "s_nll.fin": 6.0e-08,
    "s_nll.ig2": 6.0e-08,
    "s_nll.img_s1": 8.6e-08,
    "s_nll.img_s30": 1.1e-07,
    "s_nll.p1_s1": 9.3e-08,
    "s_nll.p1_s30": 6.0e-08,
    "s_nll.rag1_s1": 6.0e-08,
    "s_nll.rag1_s30": 6.9e-08,
    "s_nll.rag2_s1": 7.9e-08,
    "s_nll.rag2_s30": 6.0e-08,
    "s_w.c3_s1": 6.0e-08,
    "s_w.c3_s30": 6.0e-08,
    "s_w.c8_s1": 6.0e-08,
    "s_w.c8_s30": 6.0e-08,
    "s_w.cap": 1.5e-07,
    "s_w.ddp": 6.0e-08,
    "s_w.degen": 1.4e-07,
    "s_w.fin": 1.8e-07,
    "s_w.ig2": 6.0e-08,
    "s_w.img_s1": 2.2e-07,
    "s_w.img_s30": 2.2e-07,
    "s_w.p1_s1": 6.0e-08,
    "s_w.p1_s30": 6.0e-08,
    "s_w.rag1_s1": 1.4e-07,
    "s_w.rag1_s30": 1.4e-07,
    "s_w.rag2_s1": 6.0e-08,
    "s_w.rag2_s30": 6.0e-08,
}
