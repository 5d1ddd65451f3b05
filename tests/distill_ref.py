"""float64 restatement of the teacher-student distillation criterion of csrc/distill.hip (weighted CE + tau^2 KL(teacher ||
student) at temperature tau), with the seeded inputs and case lists that tests/test_distill_cpu.py (no GPU: ties the restatement
to float64 autograd, measures the fp32 floors, shows that the bounds see seven mutants) and tests/test_distill_gpu.py /
tests/helpers/distill_ddp_worker.py (the kernels) share.  Shapes, seeded inputs, the validity rule and the error measure are
tests/overlap_loss_ref.py's, imported.

Nothing here calls the product: torch on the CPU only.  The definition, written out again:

    V = pixels with y != ignore_index and 0 <= y < C;  s = student logits, t = teacher logits, tau > 0
    p = softmax(s)     ptau = softmax(s / tau)     q = softmax(t / tau)     g_ic = [y_i == c]
    KL_i = sum_c q_ic (log q_ic - log ptau_ic)
    N = |V|     A = #{i in V : argmax_c s_ic == argmax_c t_ic}   (lowest class index among equal maxima)
    L = lce * sum_V w_y nll / sum_V w_y  +  lkd * tau^2 * sum_V KL_i / N
    dL/ds_ik = lce * w_y (p_ik - g_ik) / sum_V w  +  lkd * tau * (ptau_ik - q_ik) / N      on V,   exactly 0 elsewhere
lce == 0 leaves the CE term out altogether (finite without a valid pixel); N == 0 makes the distillation term and its gradient 0.

Student logits = inputs(shape, kind, scale)[0], teacher logits = inputs(shape, kind, scale, seed=1)[0]: independent draws, so
sum KL is of order N and about half the pixels agree (with two classes).

FLOOR holds, per check, the error of THIS formula evaluated in float32 with stock torch ops on the CPU (dtype=torch.float32:
the scaled logits formed as z * float32(1 / tau), as the kernel forms them, torch's fp32 log_softmax, fp32 sums and
coefficients) against the float64 evaluation on the same inputs, the largest over the check's cases, rounded up to two digits,
and never below 2^-24.  The GPU tests bound every float comparison by 4 x FLOOR; test_distill_cpu.py measures every floor again
and fails if a recorded figure is above 1.25 x or below half of what it measures.  The three float sums are checked one by one,
each by its own scale (s_nll, s_w, s_kl): a vector-wide relative error would let the largest component hide the others.  N and
A are compared exactly and have no floor.

The single-pixel shape p1 runs at logit scale 1 only: at scale 30 its one saturated pixel has a loss and a gradient of about 0,
and the fp32 floor of a RELATIVE error there is 1.0, which bounds nothing.  At scale 1 its floors are those of one pixel without
any averaging: a KL of 0.01 to 0.2 formed from log-probabilities of order 1 (5e-6 of it at tau = 3) and a gradient whose two
entries cancel to 1e-3 of a probability at tau = 0.5 (3.6e-5).  They stand in the groups <check>.p1_s1, which like every group
span the four temperatures, and lend their figures to no other shape.
"""
import functools

import torch

from tests.overlap_loss_ref import (BIG, FLOOR_MIN, IG2_IGNORE, IG2_SHAPE, IGNORE, SCALES, SHAPES, gen, inputs, rel_err, resolve,
                                    valid_mask)

TEMPS = {"t1": 1.0, "t2": 2.0, "t3": 3.0, "t05": 0.5}          # 3.0: its reciprocal is inexact; 0.5: sharpened
# (class weights?, lce, lkd): CE + distillation with a factor a lost weight shows in, and distillation alone
COMBOS = [(wt, lce, lkd) for wt in (False, True) for lce, lkd in ((1.0, 2.0), (0.0, 1.0))]
INPUT_CASES = [(sh, kind, sc) for sh in SHAPES for kind in ("u8", "i64") for sc in SCALES if not (sh == "p1" and sc != "s1")]
INPUT_IDS = ["%s_%s_%s" % c for c in INPUT_CASES]
BIG_TEMP, BIG_COMBO = "t2", (True, 1.0, 2.0)                     # cap and fin: uint8 labels, logits of order 1
DEGENERATE = ["all_ignored", "no_foreground", "all_foreground"]
DEGEN_SHAPE, DEGEN_TEMP = (2, 2, 13, 11), "t2"
IG2_TEMPS, IG2_COMBO = ("t2", "t3"), (True, 1.0, 2.0)           # three classes, ignore_index 2: the mutants' inputs
SAME_CASE, SAME_TEMPS = ("img", "u8", "s1"), ("t1", "t3")       # teacher == student, bit for bit
CHECKS = ("s_nll", "s_w", "s_kl", "loss", "grad")
MUTANTS = ["tau_not_squared", "grad_tau_squared", "kl_reversed", "teacher_unscaled", "ignored_in_N", "mean_over_all_pixels",
           "agreement_counts_invalid"]


def pair(shape, kind, scale, ignore_index=IGNORE):
    """(student logits, teacher logits, labels, class weights) of an INPUT_CASES entry; shared and cached: do not write into them"""
    student, labels, weight = inputs(shape, kind, scale, ignore_index)
    teacher = inputs(shape, kind, scale, ignore_index, seed=1)[0]
    return student, teacher, labels, weight


@functools.lru_cache(maxsize=None)
def degenerate_inputs(pattern, kind="u8"):
    student, labels, weight = inputs(DEGEN_SHAPE, kind, 1.0, seed=5)
    teacher = inputs(DEGEN_SHAPE, kind, 1.0, seed=6)[0]
    fill = {"all_ignored": IGNORE, "no_foreground": 0, "all_foreground": 1}[pattern]
    return student, teacher, torch.full_like(labels, fill), weight


@functools.lru_cache(maxsize=None)
def saturated_pair(shape, kind):
    """student and teacher logits +-40 by two different seeded hard masks -> (student, teacher, labels, N, A): N the valid
    pixels, A the valid pixels where the two masks coincide, both integers"""
    b, c, h, w = shape = resolve(shape)
    _, labels, _ = inputs(shape, kind, 1.0)
    ps = torch.randint(0, c, (b, h, w), generator=gen(77 + c + h))
    pt = torch.randint(0, c, (b, h, w), generator=gen(177 + c + h))
    student = torch.full((b, c, h, w), -40.0).scatter_(1, ps[:, None], 40.0)
    teacher = torch.full((b, c, h, w), -40.0).scatter_(1, pt[:, None], 40.0)
    ok = valid_mask(labels, c)
    return student, teacher, labels, int(ok.sum()), int((ok & (ps == pt)).sum())


def first_argmax(z):
    """the lowest index among the largest entries of each row"""
    c = z.shape[1]
    idx = torch.arange(c).expand_as(z)
    return torch.where(z == z.max(1, keepdim=True).values, idx, torch.full_like(idx, c)).min(1).values


def distill_ref(student, teacher, labels, weight, ignore_index, tau, lce, lkd, dtype=torch.float64, mutant=None):
    """dict(sums = [sum w nll, sum w, sum KL, N, A] (float64), loss, ce, kd, grad [B,C,H,W]) of the module docstring's
    definition, in `dtype`.  `mutant` (test_distill_cpu.py only) plants one of MUTANTS: a wrong formula the bounds must see."""
    b, c, h, w = student.shape
    flat = lambda t: t.to(dtype).permute(0, 2, 3, 1).reshape(-1, c)
    z, zt = flat(student), flat(teacher)
    y = labels.reshape(-1).long()
    valid = (y != ignore_index) & (y >= 0) & (y < c)
    yc = torch.where(valid, y, torch.zeros_like(y))
    if dtype == torch.float32:
        inv = torch.tensor(1.0 / tau, dtype=torch.float32)              # float32(1 / tau), as the host passes it
        lsm = lambda v: torch.log_softmax(v, 1)
        zs, zq = z * inv, zt * inv
    else:
        lsm = lambda v: v - torch.logsumexp(v, 1, keepdim=True)
        zs, zq = z / tau, zt / tau
    if mutant == "teacher_unscaled":
        zq = zt
    logp, logpt, logq = lsm(z), lsm(zs), lsm(zq)
    p, pt, q = torch.exp(logp), torch.exp(logpt), torch.exp(logq)
    vm = valid[:, None].to(dtype)
    g = torch.nn.functional.one_hot(yc, c).to(dtype) * vm
    wy = (weight.to(dtype)[yc] if weight is not None else torch.ones(z.shape[0], dtype=dtype)) * vm[:, 0]
    s1, s2 = (wy * -(logp * g).sum(1)).sum(), wy.sum()
    kl = (q * (logq - logpt)).sum(1) if mutant != "kl_reversed" else (pt * (logpt - logq)).sum(1)
    skl = (kl * vm[:, 0]).sum()
    counted = valid
    if mutant == "ignored_in_N":
        counted = (y >= 0) & (y < c)
    n = int(counted.sum())
    if mutant == "mean_over_all_pixels":
        n = y.numel()
    agree = first_argmax(z) == first_argmax(zt)
    a = int((agree & valid).sum()) if mutant != "agreement_counts_invalid" else int(agree.sum())
    tau_d = torch.tensor(tau, dtype=dtype)
    zero = torch.zeros((), dtype=dtype)
    kd = lkd * (tau_d if mutant == "tau_not_squared" else tau_d * tau_d) * skl / n if n > 0 else zero
    gfac = lkd * (tau_d * tau_d if mutant == "grad_tau_squared" else tau_d) / n if n > 0 else zero
    grad = gfac * (pt - q)
    ce = zero
    if lce != 0:
        ce = lce * s1 / s2
        grad = grad + lce * wy[:, None] * (p - g) / s2
    grad = torch.where(valid[:, None], grad, torch.zeros_like(grad))
    sums = torch.stack([s1.double(), s2.double(), skl.double(), torch.tensor(float(n), dtype=torch.float64),
                        torch.tensor(float(a), dtype=torch.float64)])
    return dict(sums=sums, loss=ce + kd, ce=ce, kd=kd, grad=grad.reshape(b, h, w, c).permute(0, 3, 1, 2).contiguous())


def combo_args(combo, weight):
    """(weight or None, lce, lkd) of one COMBOS entry"""
    wt, lce, lkd = combo
    return (weight if wt else None), lce, lkd


def combo_id(combo):
    return "%s_ce%g_kd%g" % ("w" if combo[0] else "now", combo[1], combo[2])


@functools.lru_cache(maxsize=None)
def reference(shape, kind, scale, temp, combo, ignore_index=IGNORE):
    student, teacher, labels, weight = pair(shape, kind, scale, ignore_index)
    wt, lce, lkd = combo_args(combo, weight)
    return distill_ref(student, teacher, labels, wt, ignore_index, TEMPS[temp], lce, lkd)


@functools.lru_cache(maxsize=None)
def degenerate_reference(pattern, combo, kind="u8"):
    student, teacher, labels, weight = degenerate_inputs(pattern, kind)
    wt, lce, lkd = combo_args(combo, weight)
    return distill_ref(student, teacher, labels, wt, IGNORE, TEMPS[DEGEN_TEMP], lce, lkd)


@functools.lru_cache(maxsize=None)
def same_reference(temp):
    """teacher == student with lce = 1, class weights: the distillation term is 0, what is left is the CE's loss and gradient"""
    student, _, labels, weight = pair(SAME_CASE[0], SAME_CASE[1], SCALES[SAME_CASE[2]])
    return distill_ref(student, student, labels, weight, IGNORE, TEMPS[temp], 1.0, 2.0)


def degenerate_combos(pattern):
    """every combination, except that without a valid pixel the CE term is 0 / 0 (as nn.CrossEntropyLoss has it): distillation only"""
    return [cb for cb in COMBOS if not (pattern == "all_ignored" and cb[1] != 0.0)]


def errors(got_sums, got_loss, got_grad, ref):
    """{check: error} of CHECKS: each float sum by its own scale, the loss, the gradient by the largest float64 gradient entry"""
    gs = got_sums.detach().double().cpu().reshape(-1)
    e = {"s_nll": rel_err(gs[0], ref["sums"][0]), "s_w": rel_err(gs[1], ref["sums"][1]), "s_kl": rel_err(gs[2], ref["sums"][2])}
    e["loss"] = rel_err(got_loss.reshape(()), ref["loss"])
    e["grad"] = rel_err(got_grad, ref["grad"])
    return e


def floor_key(check, group):
    return "%s.%s" % (check, group)


def group(shape, scale):
    """the floor group of an INPUT_CASES entry: one per shape and logit scale, over both label widths, the four temperatures and
    every COMBOS entry"""
    return "%s_%s" % (shape, scale)


# fp32 floors (see the module docstring); measured by tests/test_distill_cpu.py.  Groups: <shape>_<scale> = the INPUT_CASES of that
# shape and logit scale, both label widths, four temperatures, every COMBOS entry (p1: scale 1 only); cap, fin = BIG
# at BIG_TEMP with BIG_COMBO; degen = no_foreground and all_foreground at DEGEN_TEMP (all_ignored is exact: 0); ig2 = the mutants'
# inputs at IG2_TEMPS; same = teacher == student at SAME_TEMPS; ddp = the inputs of tests/helpers/distill_ddp_worker.py.
FLOOR = {
    "grad.c3_s1": 2.5e-07,
    "grad.c3_s30": 2.6e-07,
    "grad.c8_s1": 2.5e-07,
    "grad.c8_s30": 3.2e-07,
    "grad.cap": 2.2e-07,
    "grad.ddp": 1.4e-07,
    "grad.degen": 1.6e-07,
    "grad.fin": 1.7e-07,
    "grad.ig2": 2.2e-07,
    "grad.img_s1": 1.9e-07,
    "grad.img_s30": 3.4e-07,
    "grad.p1_s1": 3.7e-05,
    "grad.rag1_s1": 3.0e-07,
    "grad.rag1_s30": 1.9e-07,
    "grad.rag2_s1": 1.6e-07,
    "grad.rag2_s30": 2.2e-07,
    "grad.same": 1.6e-07,
    "loss.c3_s1": 1.3e-07,
    "loss.c3_s30": 1.7e-07,
    "loss.c8_s1": 2.2e-07,
    "loss.c8_s30": 1.1e-07,
    "loss.cap": 6.0e-08,
    "loss.ddp": 6.0e-08,
    "loss.degen": 1.1e-07,
    "loss.fin": 6.0e-08,
    "loss.ig2": 6.7e-08,
    "loss.img_s1": 9.2e-08,
    "loss.img_s30": 7.5e-08,
    "loss.p1_s1": 5.3e-06,
    "loss.rag1_s1": 1.9e-07,
    "loss.rag1_s30": 1.2e-07,
    "loss.rag2_s1": 1.4e-07,
    "loss.rag2_s30": 7.7e-08,
    "loss.same": 6.0e-08,
    "s_kl.c3_s1": 8.6e-08,
    "s_kl.c3_s30": 1.2e-07,
    "s_kl.c8_s1": 1.9e-07,
    "s_kl.c8_s30": 7.0e-08,
    "s_kl.cap": 6.0e-08,
    "s_kl.ddp": 6.6e-08,
    "s_kl.degen": 6.0e-08,
    "s_kl.fin": 6.0e-08,
    "s_kl.ig2": 9.2e-08,
    "s_kl.img_s1": 1.6e-07,
    "s_kl.img_s30": 6.0e-08,
    "s_kl.p1_s1": 5.3e-06,
    "s_kl.rag1_s1": 1.1e-07,
    "s_kl.rag1_s30": 9.0e-08,
    "s_kl.rag2_s1": 1.7e-07,
    "s_kl.rag2_s30": 6.0e-08,
    "s_kl.same": 6.0e-08,
    "s_nll.c3_s1": 6.0e-08,
    "s_nll.c3_s30": 7.8e-08,
    "s_nll.c8_s1": 6.0e-08,
    "s_nll.c8_s30": 1.2e-07,
    "s_nll.cap": 6.0e-08,
    "s_nll.ddp": 6.0e-08,
    "s_nll.degen": 9.5e-08,
    "s_nll.fin": 6.0e-08,
    "s_nll.ig2": 6.0e-08,
    "s_nll.img_s1": 6.0e-08,
    "s_nll.img_s30": 1.0e-07,
    "s_nll.p1_s1": 9.3e-08,
    "s_nll.rag1_s1": 6.0e-08,
    "s_nll.rag1_s30": 7.4e-08,
    "s_nll.rag2_s1": 6.0e-08,
    "s_nll.rag2_s30": 9.1e-08,
    "s_nll.same": 6.0e-08,
    "s_w.c3_s1": 7.1e-08,
    "s_w.c3_s30": 7.1e-08,
    "s_w.c8_s1": 6.0e-08,
    "s_w.c8_s30": 6.0e-08,
    "s_w.cap": 7.4e-08,
    "s_w.ddp": 6.0e-08,
    "s_w.degen": 1.4e-07,
    "s_w.fin": 6.0e-08,
    "s_w.ig2": 6.3e-08,
    "s_w.img_s1": 6.0e-08,
    "s_w.img_s30": 6.0e-08,
    "s_w.p1_s1": 6.0e-08,
    "s_w.rag1_s1": 1.5e-07,
    "s_w.rag1_s30": 1.5e-07,
    "s_w.rag2_s1": 6.0e-08,
    "s_w.rag2_s30": 6.0e-08,
    "s_w.same": 6.0e-08,
}


@functools.lru_cache(maxsize=None)
def ddp_inputs():
    """the batch of 4 of tests/helpers/distill_ddp_worker.py: (student, teacher, labels, weight); the first half (rank 0's) is
    all ignored, so a per-rank N or sum w would differ from the global batch's"""
    g = gen(23)
    student = torch.randn(4, 2, 65, 65, generator=g)
    teacher = torch.randn(4, 2, 65, 65, generator=g)
    labels = (torch.rand(4, 65, 65, generator=g) < 0.2).to(torch.uint8)
    labels[torch.rand(4, 65, 65, generator=g) < 0.1] = IGNORE
    labels[:2] = IGNORE
    return student, teacher, labels, torch.tensor([1.0, 3.0])


DDP_TEMP, DDP_COMBO = 2.0, (True, 1.0, 2.0)


@functools.lru_cache(maxsize=None)
def ddp_reference():
    student, teacher, labels, weight = ddp_inputs()
    return distill_ref(student, teacher, labels, weight, IGNORE, DDP_TEMP, DDP_COMBO[1], DDP_COMBO[2])
