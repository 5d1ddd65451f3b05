"""numpy restatement of the local dense-CRF refinement of csrc/crf.hip (include/iswm_hip_cr.h), with the seeded
inputs and the case list that tests/test_crf_cpu.py and tests/test_crf_gpu.py share.

`refine` takes the dtype of every floating-point operation as an argument: float64 is the reference, float32 the same statement in
the kernel's number format, and the distance between the two (E32) is the unit the GPU bound is written in.  It is built from
shifted slices -- one pass over the (2R+1)^2 - 1 offsets, row-major, each adding its overlap of the plane -- so the sums run in the
order the definition gives and a 70 x 90 case takes well under a second."""
import numpy as np

DEFAULTS = dict(radius=5, step=2, w_bilateral=10.0, w_spatial=3.0, theta_alpha=80.0, theta_beta=13.0, theta_gamma=3.0)
TINY = 1e-20

# (N, H, W): smaller than any halo, a single row, sizes that are no multiple of the 32-pixel tile, several tiles on each axis, two
# images (the batch stride)
SHAPES = ((1, 1, 1), (1, 1, 40), (1, 5, 7), (2, 37, 53), (1, 70, 45), (1, 33, 130))
# (R, D, T, w_b, w_s, theta_alpha, theta_beta, theta_gamma): the radius and step extremes, odd and even T, all with w_b + w_s <= 2
# (the update is then no expansion, so an error of one iteration is not amplified by the next)
PARAMS = ((3, 1, 3, 1.2, 0.6, 4.0, 20.0, 2.0), (7, 4, 2, 1.0, 1.0, 30.0, 25.0, 10.0), (1, 3, 1, 0.5, 1.5, 2.0, 8.0, 1.5))
CASES = tuple((s, p) for s in SHAPES for p in PARAMS)


def clamp(p, dtype=np.float64):
    return np.clip(np.asarray(p).astype(dtype), dtype(1e-6), dtype(1 - 1e-6))


def _offsets(H, W, R, D):
    """the neighbours of the definition, row-major over the window: (dy, dx, slices of i, slices of j) for the offsets whose
    overlap with the plane is not empty"""
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if dy == 0 and dx == 0:
                continue
            oy, ox = dy * D, dx * D
            i0, i1 = max(0, -oy), min(H, H - oy)
            j0, j1 = max(0, -ox), min(W, W - ox)
            if i0 >= i1 or j0 >= j1:
                continue
            yield dy, dx, (slice(i0, i1), slice(j0, j1)), (slice(i0 + oy, i1 + oy), slice(j0 + ox, j1 + ox))


def kernels(img, R, D, theta_alpha, theta_beta, theta_gamma, dtype=np.float64):
    """[(slices of i, slices of j, kb over the overlap, ks)] for one frame uint8 [H, W, 3], and the norms Nb, Ns"""
    H, W, _ = img.shape
    I = img.astype(np.int64)
    two = dtype(2)
    ta2, tb2, tg2 = (two * dtype(t) * dtype(t) for t in (theta_alpha, theta_beta, theta_gamma))
    out = []
    Nb, Ns = np.zeros((H, W), dtype), np.zeros((H, W), dtype)
    for dy, dx, si, sj in _offsets(H, W, R, D):
        d2 = dtype((dy * dy + dx * dx) * D * D)
        dI2 = ((I[si] - I[sj]) ** 2).sum(-1)                   # exact integers
        assert dI2.max() <= 195075
        kb = np.exp(-(d2 / ta2) - dI2.astype(dtype) / tb2).astype(dtype)
        ks = dtype(np.exp(-(d2 / tg2)))
        Nb[si] += kb
        Ns[si] += ks
        out.append((si, sj, kb, ks))
    return out, Nb, Ns


def step(q, u, kern, Nb, Ns, w_b, w_s, dtype=np.float64):
    """one mean-field update -> (q', z, m_b, m_s)"""
    s = dtype(2) * q - dtype(1)
    Sb, Ss = np.zeros_like(q), np.zeros_like(q)
    for si, sj, kb, ks in kern:
        Sb[si] += kb * s[sj]
        Ss[si] += ks * s[sj]
    with np.errstate(divide="ignore", invalid="ignore"):
        m_b = np.where(Nb < dtype(TINY), dtype(0), Sb / Nb).astype(dtype)
        m_s = np.where(Ns < dtype(TINY), dtype(0), Ss / Ns).astype(dtype)
    z = u + dtype(w_b) * m_b + dtype(w_s) * m_s
    return (dtype(1) / (dtype(1) + np.exp(-z))).astype(dtype), z, m_b, m_s


def refine(prob, img, iters, radius=5, step_=2, w_bilateral=10.0, w_spatial=3.0, theta_alpha=80.0, theta_beta=13.0,
           theta_gamma=3.0, dtype=np.float64, trace=None):
    """prob [N, H, W] (or [H, W]) and img uint8 [N, H, W, 3] (or [H, W, 3]) -> q^T in `dtype`.  `trace`, a list, receives per image
    and iteration (u, z, m_b, m_s)."""
    prob, img = np.asarray(prob), np.asarray(img)
    single = prob.ndim == 2
    if single:
        prob, img = prob[None], img[None]
    assert img.dtype == np.uint8 and img.shape == prob.shape + (3,)
    out = np.empty(prob.shape, dtype)
    for n in range(prob.shape[0]):
        pc = clamp(prob[n], dtype)
        u = (np.log(pc) - np.log(dtype(1) - pc)).astype(dtype)
        kern, Nb, Ns = kernels(img[n], radius, step_, theta_alpha, theta_beta, theta_gamma, dtype)
        q = pc
        for _ in range(iters):
            q, z, m_b, m_s = step(q, u, kern, Nb, Ns, w_bilateral, w_spatial, dtype)
            if trace is not None:
                trace.append((u, z, m_b, m_s))
        out[n] = q
    return out[0] if single else out


def refine_case(prob, img, params, dtype=np.float64, trace=None):
    R, D, T, w_b, w_s, ta, tb, tg = params
    return refine(prob, img, T, R, D, w_b, w_s, ta, tb, tg, dtype=dtype, trace=trace)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------

def block_frames(n, h, w, seed, block=6):
    """uint8 [n, h, w, 3]: blocks of one random colour plus noise of 0..11 per channel, so every pixel has neighbours of a similar
    colour (its bilateral norm stays far from the 1e-20 cut) and neighbours of a very different one"""
    rng = np.random.RandomState(seed)
    by, bx = (h + block - 1) // block, (w + block - 1) // block
    base = rng.randint(0, 244, size=(n, by, bx, 3))
    full = np.repeat(np.repeat(base, block, axis=1), block, axis=2)[:, :h, :w]
    return (full + rng.randint(0, 12, size=(n, h, w, 3))).astype(np.uint8)


def uniform_prob(n, h, w, seed):
    """fp32 [n, h, w] uniform in [0.05, 0.95]"""
    return np.random.RandomState(seed).uniform(0.05, 0.95, size=(n, h, w)).astype(np.float32)


def case_inputs(shape, k):
    """the inputs of case (shape, PARAMS[k]): a seed of its own per pair.  The base was chosen among 1000..1011 so that the float64
    result of every case stays inside (0.015, 0.99): no case saturates, so none hides an error (test_crf_cpu asserts it)"""
    n, h, w = shape
    seed = 1002 + 17 * (n * 131 + h * 7 + w) + k
    return uniform_prob(n, h, w, seed), block_frames(n, h, w, seed + 1)


def wavy_edge(h=70, w=90, seed=7):
    """(truth bool [h, w], frame uint8 [h, w, 3], prob fp32 [h, w]): two noisy flat regions split by a wavy edge; the probability
    is the true mask shifted 3 px along both axes, blurred 9 x 9, squeezed to [0.1, 0.9] and given N(0, 0.05) noise"""
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    truth = xx > 0.5 * w + 8.0 * np.sin(yy / 7.0)
    flat = np.where(truth[..., None], np.array([170, 120, 60]), np.array([40, 80, 150]))
    frame = np.clip(flat + rng.normal(0.0, 6.0, size=(h, w, 3)), 0, 255).astype(np.uint8)
    shifted = np.zeros((h, w))
    shifted[3:, 3:] = truth[:-3, :-3]
    shifted[:3, :] = shifted[3:4, :]
    shifted[:, :3] = shifted[:, 3:4]
    pad = np.pad(shifted, 4, mode="edge")
    blur = np.zeros((h, w))
    for dy in range(9):
        for dx in range(9):
            blur += pad[dy:dy + h, dx:dx + w]
    blur /= 81.0
    prob = np.clip(0.1 + 0.8 * blur + rng.normal(0.0, 0.05, size=(h, w)), 0.0, 1.0).astype(np.float32)
    return truth, frame, prob


def misclassified(q, truth, thr=0.5):
    return int(((np.asarray(q) > thr) != truth).sum())
