// Fused class-weighted cross-entropy / focal loss over per-pixel NCHW logits, forward and
// backward in ONE pass over the logits (HBM-bound: per pixel C*4 B logits + 1|8 B label read,
// C*4 B gradient written; 24 B/pixel at C = 2 with int64 labels).
//
//   mode 0  nn.CrossEntropyLoss(weight=w, ignore_index, 'mean')     train.py:454-459
//           L = sum_i w[y_i] nll_i / sum_i w[y_i]      over y_i != ignore_index
//   mode 1  FocalLoss(size_average=True)                            utils/loss.py:23-35
//           ce_i = w[y_i] nll_i (0 if ignored), pt = exp(-ce), f = alpha (1-pt)^gamma ce,
//           L = mean over ALL pixels (ignored ones included in the denominator)
//   mode 2  FocalLoss(size_average=False):  L = sum_i f_i
//
// The kernel writes the gradient UNNORMALISED (dL_i/dz without the 1/sum_w or 1/npix
// factor) plus per-block partial sums; iswm_loss_finalize reduces those in a fixed order
// (double precision, bit-reproducible) and iswm_loss_bwd_scale applies upstream/normaliser.
// Under data parallelism the host all-reduces sums[2] between the two so that the
// normaliser is the GLOBAL sum of weights, as the reference's gathered-logits loss has it.
#include "loss_common.h"      // log_softmax, loss_pixel, gather_pixels, block_reduce, by_label_and_classes, refuse_pixel_args

namespace iswm {

// CT > 0: class count known at compile time (2: the binary internal-wave masks), logits held in registers.
template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_loss_fwd(const float* __restrict__ logits,
                                                  const LabelT* __restrict__ labels, int Crt, int64_t HW,
                                                  int64_t npix, const float* __restrict__ cw, int ignore_index,
                                                  float alpha, float gamma, int mode,
                                                  float* __restrict__ grad, float* __restrict__ partials,
                                                  int nblocks) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : 8;
    const int C = CT > 0 ? CT : Crt;
    __shared__ float red[2][4];
    float s1 = 0.f, s2 = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        if (CT > 0 || C <= CMAX) {
            float z[UNR][CMAX];
            long long y[UNR];
            int64_t off[UNR];
            bool in[UNR];
            gather_pixels(logits, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, off, in);
#pragma unroll
            for (int u = 0; u < UNR; ++u) {
                if (off[u] < 0) continue;
                float coef, m, lg;
                bool valid;
                loss_pixel(z[u], C, y[u], cw, ignore_index, alpha, gamma, mode, s1, s2, coef, m, lg, valid);
#pragma unroll
                for (int c = 0; c < CMAX; ++c)
                    if (c < C) {
                        const float pc = expf(log_softmax(z[u][c], m, lg));
                        grad[off[u] + c * HW] = valid ? coef * (pc - (c == (int)y[u] ? 1.f : 0.f)) : 0.f;
                    }
            }
        } else {                                    // many classes: stream the class axis from memory
            for (int u = 0; u < UNR; ++u) {
                const int64_t i = i0 + u * stride;
                if (i >= npix) break;
                const int64_t b = i / HW, p = i - b * HW;
                const float* zp = logits + b * C * HW + p;
                float m = zp[0];
                for (int c = 1; c < C; ++c) m = fmaxf(m, zp[c * HW]);
                float se = 0.f;
                for (int c = 0; c < C; ++c) se += expf(zp[c * HW] - m);
                const float lg = logf(se);
                const long long yy = (long long)labels[i];
                const bool valid = valid_label(yy, C, ignore_index);
                float coef = 0.f;
                if (valid) loss_terms(-log_softmax(zp[yy * HW], m, lg), cw ? cw[yy] : 1.f, alpha, gamma, mode, s1, s2, coef);
                float* g = grad + b * C * HW + p;
                for (int c = 0; c < C; ++c) {
                    const float pc = expf(log_softmax(zp[c * HW], m, lg));
                    g[c * HW] = valid ? coef * (pc - (c == (int)yy ? 1.f : 0.f)) : 0.f;
                }
            }
        }
    }
    float s[2] = {s1, s2};
    block_reduce(s, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = block_total(red[0]);
        partials[nblocks + blockIdx.x] = block_total(red[1]);
    }
}

// one wave: lane l sums partials l, l + 64, ... in double (fixed order), then a shuffle tree -- the single-thread loop over
// the partials took longer than the loss pass itself
__global__ __launch_bounds__(64) void k_loss_finalize(const float* __restrict__ partials, int blocks, int mode, double npix,
                                                      float* sums, float* loss) {
    const int lane = threadIdx.x;
    double a = 0.0, b = 0.0;
    for (int i = lane; i < blocks; i += 64) {
        a += (double)partials[i];
        b += (double)partials[blocks + i];
    }
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_down(a, o);
        b += __shfl_down(b, o);
    }
    if (lane == 0) {
        sums[0] = (float)a;
        sums[1] = (float)b;
        if (loss) loss[0] = mode == 0 ? (float)(a / b) : (mode == 1 ? (float)(a / npix) : (float)a);
    }
}

__global__ __launch_bounds__(256) void k_loss_bwd_scale(float* __restrict__ grad, int64_t n,
                                                        const float* __restrict__ sums,
                                                        const float* __restrict__ upstream, int mode,
                                                        float inv_npix) {
    float f = upstream ? upstream[0] : 1.f;
    f *= mode == 0 ? 1.f / sums[1] : (mode == 1 ? inv_npix : 1.f);
    const int64_t n4 = n >> 2;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<float4*>(grad)[i];
        reinterpret_cast<float4*>(grad)[i] = make_float4(v.x * f, v.y * f, v.z * f, v.w * f);
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) grad[n4 * 4 + threadIdx.x] *= f;
}

__global__ __launch_bounds__(256) void k_argmax_nchw(const float* __restrict__ logits, int C, int64_t HW,
                                                     int64_t npix, int64_t* __restrict__ out) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < npix; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, p = i - b * HW;
        const float* z = logits + b * C * HW + p;
        float best = z[0];
        int bi = 0;
        for (int c = 1; c < C; ++c) {
            float v = z[c * HW];
            if (v > best) {  // strict: ties keep the lowest class index (torch.max semantics)
                best = v;
                bi = c;
            }
        }
        out[i] = bi;
    }
}

// ---- region-overlap losses (soft Dice / Tversky / focal-Tversky) next to the weighted CE: two passes -------------------------
//   V = valid pixels (valid_label), p = softmax(z), g = one-hot(y)
//   I_c = sum_V p_ic g_ic,  P_c = sum_V p_ic,  G_c = sum_V g_ic (an exact count)
//   D_c = I_c + alpha (P_c - I_c) + beta (G_c - I_c) + s,  T_c = (I_c + s) / D_c,  l_c = max(1 - T_c, 0)^gamma
//   L   = lambda_ce sum(w nll) / sum(w) + lambda_ov mean_{c in S} l_c
// CE's gradient needs one global scalar, so k_loss_fwd writes it in the pass that forms the sums.  A Tversky gradient needs
// per-class coefficients that exist only after the global reduction:
//   k_overlap_sums      reads logits + labels, writes per-block partials of {sum w nll, sum w, I_c, P_c, G_c}  (no per-pixel store)
//   k_overlap_finalize  one wave per value: partials -> sums[2 + 3C] in double, fixed order
//   k_overlap_coeffs    sums -> loss (fp32) and coef = {lambda_ce / sum w, lambda_ov u_c, lambda_ov v_c}, in double, on the device
//   k_overlap_bwd       reads logits + labels again, recomputes the softmax, writes the finished gradient once
// Under data parallelism the host all-reduces sums between finalize and coeffs: T_c is then the global batch's.
// Per pixel at C = 2, uint8 labels: 9 B read + (9 B read + 8 B written) = 26 B; the CE path moves 17 + 16 = 33 B.

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_overlap_sums(const float* __restrict__ logits, const LabelT* __restrict__ labels,
                                                      int Crt, int64_t HW, int64_t npix, const float* __restrict__ cw,
                                                      int ignore_index, float* __restrict__ partials, int nblocks) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    __shared__ float red[2 + 3 * CMAX][4];
    float s1 = 0.f, s2 = 0.f, si[CMAX], sp[CMAX], sg[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) si[c] = sp[c] = sg[c] = 0.f;
    // gather_pixels, loss_pixel and block_reduce as in k_loss_fwd: the two CE partials are iswm_loss_fwd's bit for bit
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX];
        long long y[UNR];
        bool in[UNR];
        gather_pixels(logits, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, no_offsets(), in);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (!in[u]) continue;
            float coef, m, lg;
            bool valid;
            loss_pixel(z[u], C, y[u], cw, ignore_index, 1.f, 0.f, 0, s1, s2, coef, m, lg, valid);
            if (!valid) continue;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float pc = expf(log_softmax(z[u][c], m, lg));
                    const bool hit = c == (int)y[u];
                    sp[c] += pc;
                    si[c] += hit ? pc : 0.f;
                    sg[c] += hit ? 1.f : 0.f;
                }
        }
    }
    float s[2 + 3 * CMAX] = {s1, s2};          // {s1, s2, I[CMAX], P[CMAX], G[CMAX]}
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        s[2 + c] = si[c];
        s[2 + CMAX + c] = sp[c];
        s[2 + 2 * CMAX + c] = sg[c];
    }
    block_reduce(s, red);
    const int v = threadIdx.x;                  // value index in the [2 + 3C] layout {s1, s2, I[C], P[C], G[C]}
    if (v < 2 + 3 * C) {
        const int k = v < 2 ? v : 2 + ((v - 2) / C) * CMAX + (v - 2) % C;
        partials[(int64_t)v * nblocks + blockIdx.x] = block_total(red[k]);
    }
}

// block v, one wave: the lane loop and shuffle tree of k_loss_finalize over the partials of value v -- the same additions in the
// same order (the CE sums come out bit for bit), but the loads are issued 16 at a time: one load per addition is a chain of
// memory latencies (4112 partials: 65 of them per lane, 17 us in the kernel trace)
__global__ __launch_bounds__(64) void k_overlap_finalize(const float* __restrict__ partials, int blocks, double* __restrict__ sums) {
    constexpr int DEPTH = 16;
    const int lane = threadIdx.x;
    const float* p = partials + (int64_t)blockIdx.x * blocks;
    double a = 0.0;
    int i = lane;
    for (; i + (DEPTH - 1) * 64 < blocks; i += DEPTH * 64) {
        float v[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) v[k] = p[i + k * 64];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) a += (double)v[k];
    }
    for (; i < blocks; i += 64) a += (double)p[i];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    if (lane == 0) sums[blockIdx.x] = a;
}

// one wave, double: the loss value and the coefficients of the backward pass.  coef = {lambda_ce / sum w, lambda_ov u_c [C],
// lambda_ov v_c [C]} with u_c = dL_ov/dI_c, v_c = dL_ov/dP_c; l'_c is taken as 0 where 1 - T_c <= 0 (the definition: autograd's
// 0 * inf there is nan for gamma < 1).  lambda_ce == 0 leaves the CE term out altogether, so an all-ignored batch (sum w == 0) is
// finite when only the overlap term is asked for.
__global__ __launch_bounds__(64) void k_overlap_coeffs(const double* __restrict__ sums, int C, double lce, double lov, double alpha,
                                                       double beta, double gamma, double s, int all, float* __restrict__ loss,
                                                       float* __restrict__ coef) {
    const int c = threadIdx.x;                  // lane c: class c (one pow per class, the classes side by side)
    const int first = all ? 0 : 1;
    const double inv = 1.0 / (double)(C - first);
    double l = 0.0;
    if (c < C) {
        const double I = sums[2 + c], P = sums[2 + C + c], G = sums[2 + 2 * C + c];
        const double num = I + s, D = I + alpha * (P - I) + beta * (G - I) + s;
        const double om = 1.0 - num / D;
        double dl = 0.0;
        if (om > 0.0) {
            l = gamma == 1.0 ? om : pow(om, gamma);
            dl = -gamma * (l / om);             // -gamma om^(gamma - 1)
        }
        const double k = c >= first ? lov * inv * dl / (D * D) : 0.0;
        l = c >= first ? l : 0.0;
        coef[1 + c] = (float)(k * (D - num * (1.0 - alpha - beta)));
        coef[1 + C + c] = (float)(k * (-alpha * num));
    }
    double acc = 0.0;
    for (int k = 0; k < C; ++k) acc += __shfl(l, k);        // fixed order
    if (c == 0) {
        coef[0] = lce != 0.0 ? (float)(lce / sums[1]) : 0.f;
        loss[0] = (float)((lce != 0.0 ? lce * (sums[0] / sums[1]) : 0.0) + lov * acc * inv);
    }
}

// for valid i:  dL/dz_ik = upstream [ coef[0] w_y (p_ik - g_ik) + p_ik (q_ik - sum_c p_ic q_ic) ],  q_ic = u_c g_ic + v_c;  else 0
template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_overlap_bwd(const float* __restrict__ logits, const LabelT* __restrict__ labels, int Crt,
                                                     int64_t HW, int64_t npix, const float* __restrict__ cw, int ignore_index,
                                                     const float* __restrict__ coef, const float* __restrict__ upstream,
                                                     float* __restrict__ grad) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const float up = upstream ? upstream[0] : 1.f;
    const float a = coef[0];
    float uc[CMAX], vc[CMAX];
#pragma unroll
    for (int c = 0; c < CMAX; ++c) {
        uc[c] = c < C ? coef[1 + c] : 0.f;
        vc[c] = c < C ? coef[1 + C + c] : 0.f;
    }
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX];
        long long y[UNR];
        int64_t off[UNR];
        bool in[UNR];
        gather_pixels(logits, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, off, in);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (off[u] < 0) continue;
            const long long yy = y[u];
            const bool valid = valid_label(yy, C, ignore_index);
            // softmax_stats, unrolled by hand: on the shared loops this kernel takes 75 VGPRs at runtime C (6 waves per SIMD,
            // not 7); same operations in the same order
            float m = z[u][0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c) m = c < C ? fmaxf(m, z[u][c]) : m;
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) se += c < C ? expf(z[u][c] - m) : 0.f;
            const float lg = logf(se);
            const float aw = valid ? a * (cw ? cw[yy] : 1.f) : 0.f;
            float pc[CMAX], q[CMAX], dot = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                pc[c] = c < C ? expf(log_softmax(z[u][c], m, lg)) : 0.f;
                q[c] = (c == (int)yy ? uc[c] : 0.f) + vc[c];
                dot += pc[c] * q[c];
            }
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float g = c == (int)yy ? 1.f : 0.f;
                    grad[off[u] + c * HW] = valid ? up * (aw * (pc[c] - g) + pc[c] * (q[c] - dot)) : 0.f;
                }
        }
    }
}

// ---- hard-pixel mining (OHEM / bootstrapped CE): the weighted CE over the pixels the model still gets wrong ---------------------
//   V = valid pixels (valid_label), nll_i as loss_pixel forms it, k = min(min_kept, |V|)
//   nu = min(float32(-ln thresh), k-th largest nll over V)   (+inf for the second term if k == 0)
//   K = {i in V : nll_i >= nu},  L = sum_K w nll / sum_K w,  dL/dz = upstream w (p - g) / sum_K w on K, exactly 0 elsewhere
// The gradient hangs on a global order statistic, so nothing can be written in the pass that forms the sums:
//   k_ohem_keys   logits + labels -> one int32 key per pixel (the bit pattern of nll, -1 for an invalid pixel) and |V|
//   k_ohem_hist   keys -> the histogram of one digit of the keys that carry the prefix selected so far (LDS bins, integer atomics)
//   k_ohem_scan   one workgroup: the bin that holds rank r -> prefix and remaining rank for the next digit; after the last
//                 digit nu as a device scalar.  Three digits of 11 + 10 + 10 bits from the top of the 31 significant bits.
//   k_ohem_sums   keys + labels -> per-block partials {sum_K w nll, sum_K w, |K|} in gather_pixels' order, then k_overlap_finalize
//   k_ohem_loss   sums -> {loss, 1 / sum_K w}
//   k_ohem_bwd    logits + labels + keys + nu -> the finished gradient, once
// Key order: nll >= 0 always (log se >= 0 because the largest class contributes exp(0) = 1; both forms of log_softmax are then
// <= 0), except that -log_softmax(..) of +0 is -0.0, whose bit pattern would sort above everything: the key is
// nll > 0 ? nll : +0 (a NaN becomes 0 as well).  Non-negative floats order as their bit patterns, read as int32; the invalid
// pixels' -1 lies below every valid key and below every nu >= 0, so it is never counted, selected or kept.
// The kept decision is key >= bits(nu) on the STORED keys in the sums and the backward pass alike -- never on an nll formed again.
// Integer counts are order-independent, the float sums run in k_loss_fwd's fixed order: every result is bit-reproducible, and with
// thresh = 1 (nu = 0) the first two sums are iswm_loss_fwd's mode-0 sums bit for bit (0 + w * -0.0 and 0 + w * 0.0 are both +0).
// Under data parallelism the host all-reduces |V|, every histogram and the three sums between the kernels.
// Per pixel at C = 2, uint8 labels: keys 9 B read + 4 written, 3 x 4 B histogram reads, sums 5 B read, backward 5 B read +
// (8 B read only where a pixel is kept) + 8 written: 43 B + 8 B per kept pixel; the CE path moves 33 B.
constexpr int OHEM_DIGITS = 3, OHEM_BINS = 2048, OHEM_HIST_UNR = 8;
__host__ __device__ constexpr int ohem_shift(int d) { return d == 0 ? 20 : (d == 1 ? 10 : 0); }
__host__ __device__ constexpr int ohem_width(int d) { return d == 0 ? 11 : 10; }
// the kept decision of the sums and the backward pass: the STORED key against the bits of nu (the label guards the weight lookup)
__device__ __forceinline__ bool ohem_kept(int key, int nu_bits, long long y, int C) {
    return key >= 0 && key >= nu_bits && y >= 0 && y < C;
}

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_ohem_keys(const float* __restrict__ logits, const LabelT* __restrict__ labels, int Crt,
                                                   int64_t HW, int64_t npix, int ignore_index, int* __restrict__ keys,
                                                   int* __restrict__ counts) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    __shared__ int red[1][4];
    int cnt = 0;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX];
        long long y[UNR];
        bool in[UNR];
        gather_pixels(logits, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, no_offsets(), in);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (!in[u]) continue;
            float s1 = 0.f, s2 = 0.f, coef, m, lg;      // s1 = 0 + 1 * nll: loss_pixel's own nll
            bool valid;
            loss_pixel(z[u], C, y[u], nullptr, ignore_index, 1.f, 0.f, 0, s1, s2, coef, m, lg, valid);
            keys[i0 + u * stride] = valid ? __float_as_int(s1 > 0.f ? s1 : 0.f) : -1;
            cnt += valid ? 1 : 0;
        }
    }
    int s[1] = {cnt};
    block_reduce(s, red);
    if (threadIdx.x == 0) counts[blockIdx.x] = block_total(red[0]);
}

// |V| = the sum of the blocks' counts.  One workgroup: 4112 atomics on one address from k_ohem_keys itself took longer (35 us
// in the kernel trace) than the pass.
__global__ __launch_bounds__(256) void k_ohem_count(const int* __restrict__ counts, int blocks, unsigned long long* __restrict__ nvalid) {
    __shared__ unsigned long long red[1][4];
    unsigned long long n = 0;
    for (int i = threadIdx.x; i < blocks; i += 256) n += (unsigned long long)counts[i];
    unsigned long long s[1] = {n};
    block_reduce(s, red);
    if (threadIdx.x == 0) nvalid[0] = block_total(red[0]);
}

// Few, long-lived workgroups (two per compute unit, 8 keys in flight per thread): every workgroup flushes its non-empty bins with
// one global atomic each, and the keys of a batch crowd into a few dozen bins of the top digit -- 2048 workgroups meant 2048
// atomics on each of those addresses and 48 us for the digit-0 pass in the kernel trace.  hist is ADDED to (the caller zeroes it).
// state = {prefix, rank, k, -}: digit 0 counts every valid key, a later digit the keys that agree with prefix above its own bits
// (an arithmetic shift keeps the invalid pixels' -1 apart from every prefix, which is never negative)
__global__ __launch_bounds__(256) void k_ohem_hist(const int* __restrict__ keys, int64_t npix, const long long* __restrict__ state,
                                                   int digit, unsigned long long* __restrict__ hist) {
    __shared__ unsigned int bins[OHEM_BINS];
    const int shift = ohem_shift(digit), width = ohem_width(digit), nb = 1 << width;
    for (int j = threadIdx.x; j < nb; j += blockDim.x) bins[j] = 0u;
    __syncthreads();
    const int top = shift + width;                                      // 31 at digit 0: key >> 31 is 0 (valid) or -1
    const int want = digit == 0 ? 0 : (int)(state[0] >> top);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += OHEM_HIST_UNR * stride) {
        int k[OHEM_HIST_UNR];
#pragma unroll
        for (int u = 0; u < OHEM_HIST_UNR; ++u) k[u] = i0 + u * stride < npix ? keys[i0 + u * stride] : -1;
#pragma unroll
        for (int u = 0; u < OHEM_HIST_UNR; ++u)
            if ((k[u] >> top) == want) atomicAdd(&bins[(k[u] >> shift) & (nb - 1)], 1u);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < nb; j += blockDim.x)
        if (bins[j]) atomicAdd(&hist[j], (unsigned long long)bins[j]);
}

// one workgroup.  Thread t owns the bins nb-1 - t*per .. nb-1 - (t+1)*per + 1 (descending: rank 1 is the largest key); an
// inclusive scan of the threads' totals finds the one thread whose run holds rank r, which walks its bins.  r == 0 (k == 0:
// nothing is asked for) selects nothing.  r never exceeds the histogram's total: at digit 0 that is |V| >= k, later it is the
// count of the bin chosen before.
__global__ __launch_bounds__(256) void k_ohem_scan(const unsigned long long* __restrict__ hist,
                                                   const unsigned long long* __restrict__ nvalid, int digit, long long min_kept,
                                                   float nu0, long long* __restrict__ state, float* __restrict__ nu) {
    __shared__ unsigned long long tot[2][256];
    const int shift = ohem_shift(digit), width = ohem_width(digit), nb = 1 << width, per = nb / 256;
    const int t = threadIdx.x;
    long long prefix = 0, k, r;
    if (digit == 0) {
        const long long nv = (long long)nvalid[0];
        k = min_kept < nv ? min_kept : nv;
        r = k;
    } else {
        prefix = state[0];
        r = state[1];
        k = state[2];
    }
    unsigned long long h[8], mine = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        h[j] = j < per ? hist[nb - 1 - (t * per + j)] : 0ull;
        mine += h[j];
    }
    __syncthreads();                                    // every thread has read state before anyone writes it
    tot[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {                 // inclusive scan, integers: exact
        tot[cur ^ 1][t] = tot[cur][t] + (t >= o ? tot[cur][t - o] : 0ull);
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long incl = tot[cur][t], excl = incl - mine, rr = (unsigned long long)r;
    if (r > 0 && excl < rr && rr <= incl) {
        unsigned long long above = excl;
        int bin = 0;
        bool found = false;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (j < per && !found) {
                if (rr <= above + h[j]) {
                    bin = nb - 1 - (t * per + j);
                    found = true;
                } else {
                    above += h[j];
                }
            }
        }
        prefix |= (long long)bin << shift;
        r = (long long)(rr - above);
        state[0] = prefix;
        state[1] = r;
        state[2] = k;
        if (digit == OHEM_DIGITS - 1) nu[0] = fminf(nu0, __int_as_float((int)prefix));
    } else if (t == 0 && r <= 0) {
        state[0] = 0;
        state[1] = 0;
        state[2] = k;
        if (digit == OHEM_DIGITS - 1) nu[0] = nu0;      // min(nu0, +inf)
    }
}

// gather_pixels' per-thread pixel order (keys instead of logits) and block_reduce over the kept pixels; the count rides along
// as a float (exact: a block sees fewer than 2^24 pixels, the launcher checks it)
template <typename LabelT>
__global__ __launch_bounds__(256) void k_ohem_sums(const int* __restrict__ keys, const LabelT* __restrict__ labels, int C,
                                                   int64_t npix, const float* __restrict__ cw, const int* __restrict__ nu_bits,
                                                   float* __restrict__ partials, int nblocks) {
    constexpr int UNR = LOSS_UNR;
    __shared__ float red[3][4];
    const int nb = nu_bits[0];
    float s1 = 0.f, s2 = 0.f, s3 = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        int k[UNR];
        long long y[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t i = i0 + u * stride;
            const bool in = i < npix;
            k[u] = in ? keys[i] : -1;
            y[u] = in ? (long long)labels[i] : -1;
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (ohem_kept(k[u], nb, y[u], C)) {
                const float w = cw ? cw[y[u]] : 1.f;
                s1 = fmaf(w, __int_as_float(k[u]), s1);     // loss_terms' fused add: thresh = 1 gives iswm_loss_fwd's bits
                s2 += w;
                s3 += 1.f;
            }
        }
    }
    float s[3] = {s1, s2, s3};
    block_reduce(s, red);
    const int v = threadIdx.x;
    if (v < 3) partials[(int64_t)v * nblocks + blockIdx.x] = block_total(red[v]);
}

// out = {loss, 1 / sum_K w}; both 0 when nothing is kept (or the kept pixels' weights sum to 0)
__global__ void k_ohem_loss(const double* __restrict__ sums, float* __restrict__ out) {
    const bool any = sums[2] > 0.0 && sums[1] > 0.0;
    out[0] = any ? (float)(sums[0] / sums[1]) : 0.f;
    out[1] = any ? (float)(1.0 / sums[1]) : 0.f;
}

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_ohem_bwd(const float* __restrict__ logits, const LabelT* __restrict__ labels, int Crt,
                                                  int64_t HW, int64_t npix, const float* __restrict__ cw,
                                                  const int* __restrict__ keys, const int* __restrict__ nu_bits,
                                                  const float* __restrict__ lossinv, const float* __restrict__ upstream,
                                                  float* __restrict__ grad) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const int nb = nu_bits[0];
    const float f = upstream[0] * lossinv[1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX];
        long long y[UNR];
        int64_t off[UNR];
        bool in[UNR];
        bool kept[UNR] = {};
        const auto keep = [&](int u, int64_t i, long long yy) { return kept[u] = ohem_kept(keys[i], nb, yy, C); };
        gather_pixels(logits, labels, C, HW, npix, i0, stride, -1, keep, z, y, off, in);      // dropped: logits not read
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (off[u] < 0) continue;
            float m, lg;
            softmax_stats(z[u], C, m, lg);
            const float wf = kept[u] ? (cw ? cw[y[u]] : 1.f) * f : 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float pc = expf(log_softmax(z[u][c], m, lg));
                    grad[off[u] + c * HW] = kept[u] ? wf * (pc - (c == (int)y[u] ? 1.f : 0.f)) : 0.f;
                }
        }
    }
}

}  // namespace iswm

using namespace iswm;

static const char* const OVERLAP_TAKES = "the overlap losses take";
static const char* const OHEM_TAKES = "hard-pixel mining takes";

extern "C" int iswm_loss_blocks(int64_t npix) {
    int64_t b = (npix + 1023) / 1024;      // 4 pixels per thread and iteration
    if (b > 8192) b = 8192;
    if (b < 1) b = 1;
    return (int)b;
}

extern "C" int iswm_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                             const float* class_weight, int ignore_index, float alpha, float gamma, int mode,
                             float* grad_unnorm, float* partials, iswm_stream_t stream) {
    if (refuse_pixel_args("loss_fwd", logits && labels && grad_unnorm && partials,
                          B > 0 && C > 0 && HW > 0, C, nullptr, label_bytes)) return 1;
    ISWM_REQUIRE(mode >= 0 && mode <= 2, "loss_fwd: bad mode");
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_loss_fwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C,
                           HW, npix, class_weight, ignore_index, alpha, gamma, mode, grad_unnorm, partials, blocks);
    });
    return check_launch("loss_fwd");
}

extern "C" int iswm_loss_finalize(const float* partials, int blocks, int mode, int64_t npix, float* sums,
                                  float* loss, iswm_stream_t stream) {
    ISWM_REQUIRE(partials && sums && blocks > 0, "loss_finalize: bad argument");
    hipLaunchKernelGGL(k_loss_finalize, dim3(1), dim3(64), 0, (hipStream_t)stream, partials, blocks, mode,
                       (double)npix, sums, loss);
    return check_launch("loss_finalize");
}

extern "C" int iswm_loss_bwd_scale(float* grad, int64_t n, const float* sums, const float* upstream, int mode,
                                   int64_t npix, iswm_stream_t stream) {
    ISWM_REQUIRE(grad && sums && n > 0 && aligned16(grad), "loss_bwd_scale: bad argument");
    hipLaunchKernelGGL(k_loss_bwd_scale, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, grad,
                       n, sums, upstream, mode, 1.f / (float)npix);
    return check_launch("loss_bwd_scale");
}

extern "C" int iswm_argmax_nchw(const float* logits, int B, int C, int64_t HW, int64_t* out, iswm_stream_t stream) {
    ISWM_REQUIRE(logits && out && B > 0 && C > 0 && HW > 0, "argmax: bad argument");
    const int64_t npix = (int64_t)B * HW;
    hipLaunchKernelGGL(k_argmax_nchw, dim3(stream_grid(npix, 256)), dim3(256), 0, (hipStream_t)stream, logits, C,
                       HW, npix, out);
    return check_launch("argmax");
}

extern "C" int iswm_overlap_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                                     const float* class_weight, int ignore_index, float* partials, double* sums,
                                     iswm_stream_t stream) {
    if (refuse_pixel_args("overlap_loss_fwd", logits && labels && partials && sums,
                          B > 0 && HW > 0, C, OVERLAP_TAKES, label_bytes)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_overlap_sums<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C,
                           HW, npix, class_weight, ignore_index, partials, blocks);
    });
    hipLaunchKernelGGL(k_overlap_finalize, dim3(2 + 3 * C), dim3(64), 0, s, partials, blocks, sums);
    return check_launch("overlap_loss_fwd");
}

extern "C" int iswm_overlap_loss_coeffs(const double* sums, int C, double ce_weight, double overlap_weight, double alpha,
                                        double beta, double gamma, double smooth, int classes, float* loss, float* coef,
                                        iswm_stream_t stream) {
    ISWM_REQUIRE(sums && loss && coef, "overlap_loss_coeffs: null pointer");
    ISWM_REQUIRE(C >= 1 && C <= OVL_CMAX, "overlap_loss_coeffs: %d classes (the overlap losses take 1 to %d)", C, OVL_CMAX);
    ISWM_REQUIRE(smooth > 0.0 && smooth < INFINITY, "overlap_loss_coeffs: smooth must be positive");
    ISWM_REQUIRE(alpha >= 0.0 && beta >= 0.0 && alpha < INFINITY && beta < INFINITY,
                 "overlap_loss_coeffs: alpha and beta must not be negative");
    ISWM_REQUIRE(gamma > 0.0 && gamma < INFINITY, "overlap_loss_coeffs: gamma must be positive");
    ISWM_REQUIRE(ce_weight >= 0.0 && overlap_weight >= 0.0 && ce_weight < INFINITY && overlap_weight < INFINITY,
                 "overlap_loss_coeffs: the term weights must not be negative");
    ISWM_REQUIRE(classes == 0 || classes == 1, "overlap_loss_coeffs: classes is 0 (foreground) or 1 (all)");
    ISWM_REQUIRE(classes == 1 || C >= 2, "overlap_loss_coeffs: no foreground class among %d (empty class set)", C);
    hipLaunchKernelGGL(k_overlap_coeffs, dim3(1), dim3(64), 0, (hipStream_t)stream, sums, C, ce_weight, overlap_weight,
                       alpha, beta, gamma, smooth, classes, loss, coef);
    return check_launch("overlap_loss_coeffs");
}

extern "C" int iswm_overlap_loss_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                                     const float* class_weight, int ignore_index, const float* coef, const float* upstream,
                                     float* grad, iswm_stream_t stream) {
    if (refuse_pixel_args("overlap_loss_bwd", logits && labels && coef && upstream && grad,
                          B > 0 && HW > 0, C, OVERLAP_TAKES, label_bytes)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_overlap_bwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C,
                           HW, npix, class_weight, ignore_index, coef, upstream, grad);
    });
    return check_launch("overlap_loss_bwd");
}

extern "C" int iswm_ohem_keys(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                              int ignore_index, int32_t* keys, int32_t* counts, int64_t* nvalid, iswm_stream_t stream) {
    if (refuse_pixel_args("ohem_keys", logits && labels && keys && counts && nvalid,
                          B > 0 && HW > 0, C, OHEM_TAKES, label_bytes)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_ohem_keys<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C,
                           HW, npix, ignore_index, keys, counts);
    });
    hipLaunchKernelGGL(k_ohem_count, dim3(1), dim3(256), 0, s, counts, blocks, (unsigned long long*)nvalid);
    return check_launch("ohem_keys");
}

extern "C" int iswm_ohem_digits(void) { return OHEM_DIGITS; }
extern "C" int iswm_ohem_bins(void) { return OHEM_BINS; }

extern "C" int iswm_ohem_hist(const int32_t* keys, int64_t npix, const int64_t* state, int digit, int64_t* hist,
                              iswm_stream_t stream) {
    ISWM_REQUIRE(keys && state && hist && npix > 0, "ohem_hist: bad argument");
    ISWM_REQUIRE(digit >= 0 && digit < OHEM_DIGITS, "ohem_hist: digit %d (there are %d)", digit, OHEM_DIGITS);
    int64_t blocks = (npix + 256 * OHEM_HIST_UNR - 1) / (256 * OHEM_HIST_UNR);
    if (blocks > 2 * device_cus()) blocks = 2 * device_cus();
    hipLaunchKernelGGL(k_ohem_hist, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, keys, npix,
                       (const long long*)state, digit, (unsigned long long*)hist);
    return check_launch("ohem_hist");
}

extern "C" int iswm_ohem_scan(const int64_t* hist, const int64_t* nvalid, int digit, int64_t min_kept, float nu0,
                              int64_t* state, float* nu, iswm_stream_t stream) {
    ISWM_REQUIRE(hist && nvalid && state && nu, "ohem_scan: null pointer");
    ISWM_REQUIRE(digit >= 0 && digit < OHEM_DIGITS, "ohem_scan: digit %d (there are %d)", digit, OHEM_DIGITS);
    ISWM_REQUIRE(min_kept >= 0, "ohem_scan: min_kept must not be negative");
    ISWM_REQUIRE(nu0 >= 0.f && nu0 < INFINITY, "ohem_scan: nu0 = -ln(thresh) must be finite and not negative (thresh in (0, 1])");
    hipLaunchKernelGGL(k_ohem_scan, dim3(1), dim3(256), 0, (hipStream_t)stream, (const unsigned long long*)hist,
                       (const unsigned long long*)nvalid, digit, (long long)min_kept, nu0 + 0.f, (long long*)state, nu);
    return check_launch("ohem_scan");
}

extern "C" int iswm_ohem_sums(const int32_t* keys, const void* labels, int label_bytes, int64_t npix, int C,
                              const float* class_weight, const float* nu, float* partials, double* sums,
                              iswm_stream_t stream) {
    if (refuse_pixel_args("ohem_sums", keys && labels && nu && partials && sums,
                          npix > 0 && npix <= ((int64_t)1 << 36), C, OHEM_TAKES, label_bytes)) return 1;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    if (label_bytes == 1)
        hipLaunchKernelGGL((k_ohem_sums<uint8_t>), dim3(blocks), dim3(256), 0, s, keys, (const uint8_t*)labels, C, npix,
                           class_weight, (const int*)nu, partials, blocks);
    else
        hipLaunchKernelGGL((k_ohem_sums<int64_t>), dim3(blocks), dim3(256), 0, s, keys, (const int64_t*)labels, C, npix,
                           class_weight, (const int*)nu, partials, blocks);
    hipLaunchKernelGGL(k_overlap_finalize, dim3(3), dim3(64), 0, s, partials, blocks, sums);
    return check_launch("ohem_sums");
}

extern "C" int iswm_ohem_loss(const double* sums, float* out, iswm_stream_t stream) {
    ISWM_REQUIRE(sums && out, "ohem_loss: null pointer");
    hipLaunchKernelGGL(k_ohem_loss, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, out);
    return check_launch("ohem_loss");
}

extern "C" int iswm_ohem_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                             const float* class_weight, const int32_t* keys, const float* nu, const float* lossinv,
                             const float* upstream, float* grad, iswm_stream_t stream) {
    if (refuse_pixel_args("ohem_bwd", logits && labels && keys && nu && lossinv && upstream && grad,
                          B > 0 && HW > 0, C, OHEM_TAKES, label_bytes)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_ohem_bwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C,
                           HW, npix, class_weight, keys, (const int*)nu, lossinv, upstream, grad);
    });
    return check_launch("ohem_bwd");
}
