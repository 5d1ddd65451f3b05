// Teacher-student distillation next to the weighted CE (include/iswm_hip_kd.h): two passes over TWO logit tensors and the labels,
// nothing stored per pixel.
//   V = valid pixels (valid_label), s = student logits, t = teacher logits, tau > 0, inv_tau = float(1 / tau) from the host
//   p = softmax(s), ptau = softmax(s * inv_tau), q = softmax(t * inv_tau), g = one-hot(y)
//   KL_i = sum_c q_ic (log q_ic - log ptau_ic),  N = |V|,  A = #{i in V : argmax s_i == argmax t_i} (lowest index among equal maxima)
//   L = lce sum_V w nll / sum_V w + lkd tau^2 sum_V KL_i / N
//   dL/ds_ik = lce w_y (p_ik - g_ik) / sum_V w + lkd tau (ptau_ik - q_ik) / N  on V, exactly 0 elsewhere
//   k_distill_sums      reads s, t and the labels, writes per-block partials of {sum w nll, sum w, sum KL, N, A}
//   k_overlap_finalize  loss.hip's, one wave per value: partials -> sums[5] in double, fixed order
//   k_distill_coeffs    sums -> out = {L, CE term, KD term} (fp32) and coef = {lce / sum w, lkd tau / N}, in double, on the device
//   k_distill_bwd       reads s, t and the labels again, recomputes the softmaxes, writes the finished gradient once
// Under data parallelism the host all-reduces sums between finalize and coeffs: sum w and N are then the global batch's.
// Per pixel at C = 2, uint8 labels: 17 B read + (17 B read + 8 B written) = 42 B.
//
// The CE partials: gather_pixels, loss_pixel and block_reduce as in k_loss_fwd, so sums[0..1] are iswm_loss_fwd's mode-0 sums bit
// for bit.
// The scaled logits are z * inv_tau formed with contraction off (scale_logits): a rounded product that the compiler may not fuse
// into the subtraction of the maximum behind it, for the student and the teacher alike, and both go through softmax_stats and
// log_softmax.  A teacher equal to the student bit for bit therefore has log q - log ptau == 0 in every class: sum KL is 0.0
// and ptau - q is 0.  With inv_tau == 1 the product is exact and ptau is p: the student's statistics are formed once.
// N and A ride along as floats and are exact: a block counts at most 256 * ceil(npix / (256 * blocks)) pixels, which with the
// 8192-block cap of iswm_loss_blocks stays below 2^24 up to npix = 2^36 (the launcher refuses more); a thread's running count, a
// wave's and a block's are then integers below 2^24, exact in fp32, and the finalize step adds the blocks' counts in double
// (exact below 2^53).
#include "loss_common.h"      // log_softmax, softmax_stats, loss_pixel, gather_pixels, block_reduce, by_label_and_classes, refuse_pixel_args
#include "../../include/iswm_hip_kd.h"

namespace iswm {

constexpr int KD_SUMS = 5;

// the pixel's logits times inv_tau, rounded once (see the header of this file).  Contraction is off for these products: as
// `z * inv_tau` under hipcc's default contraction (__fmul_rn is the same plain product in the HIP headers) the compiler fused
// the student's into fma(z, inv_tau, -m) and left the teacher's alone, and equal tensors gave sum KL = -3.6e-6 at tau = 3.
template <int CMAX>
__device__ __forceinline__ void scale_logits(const float (&z)[CMAX], float inv_tau, float (&zs)[CMAX]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int c = 0; c < CMAX; ++c) zs[c] = z[c] * inv_tau;
}

// the lowest index among the largest of the pixel's C logits (k_argmax_nchw's strict comparison)
template <int CMAX>
__device__ __forceinline__ int first_argmax(const float (&z)[CMAX], int C) {
    float best = z[0];
    int bi = 0;
#pragma unroll
    for (int c = 1; c < CMAX; ++c)
        if (c < C && z[c] > best) {
            best = z[c];
            bi = c;
        }
    return bi;
}

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_distill_sums(const float* __restrict__ student, const float* __restrict__ teacher,
                                                      const LabelT* __restrict__ labels, int Crt, int64_t HW, int64_t npix,
                                                      const float* __restrict__ cw, int ignore_index, float inv_tau,
                                                      float* __restrict__ partials, int nblocks) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const bool unit = inv_tau == 1.f;
    __shared__ float red[KD_SUMS][4];
    float s1 = 0.f, s2 = 0.f, skl = 0.f, sn = 0.f, sa = 0.f;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX], zt[UNR][CMAX];
        long long y[UNR], yt[UNR];
        bool in[UNR], int_[UNR];
        gather_pixels(student, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, no_offsets(), in);
        gather_pixels(teacher, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), zt, yt, no_offsets(), int_);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (!in[u]) continue;
            float coef, m, lg;
            bool valid;
            loss_pixel(z[u], C, y[u], cw, ignore_index, 1.f, 0.f, 0, s1, s2, coef, m, lg, valid);
            if (!valid) continue;
            sn += 1.f;
            sa += first_argmax(z[u], C) == first_argmax(zt[u], C) ? 1.f : 0.f;
            float zs[CMAX], zq[CMAX], ms = m, lgs = lg, mq, lgq;
            scale_logits(z[u], inv_tau, zs);
            scale_logits(zt[u], inv_tau, zq);
            if (!unit) softmax_stats(zs, C, ms, lgs);
            softmax_stats(zq, C, mq, lgq);
            float kl = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float lq = log_softmax(zq[c], mq, lgq), lp = log_softmax(zs[c], ms, lgs);
                    kl += expf(lq) * (lq - lp);
                }
            skl += kl;
        }
    }
    float s[KD_SUMS] = {s1, s2, skl, sn, sa};
    block_reduce(s, red);
    const int v = threadIdx.x;
    if (v < KD_SUMS) partials[(int64_t)v * nblocks + blockIdx.x] = block_total(red[v]);
}

// loss.hip's: block v, one wave, adds the partials of value v in double in k_loss_finalize's order (the two CE sums come out as
// iswm_loss_fwd forms them); launched from here on the host, defined there
__global__ __launch_bounds__(64) void k_overlap_finalize(const float* __restrict__ partials, int blocks, double* __restrict__ sums);

// one thread, double.  lce == 0 leaves the CE term out altogether (finite without a valid pixel); N == 0 makes the
// distillation term and its coefficient exactly 0.
__global__ void k_distill_coeffs(const double* __restrict__ sums, double lce, double lkd, double tau, float* __restrict__ out,
                                 float* __restrict__ coef) {
    const double n = sums[3];
    const double ce = lce != 0.0 ? lce * (sums[0] / sums[1]) : 0.0;
    const double kd = n > 0.0 ? lkd * tau * tau * sums[2] / n : 0.0;
    out[0] = (float)(ce + kd);
    out[1] = (float)ce;
    out[2] = (float)kd;
    coef[0] = lce != 0.0 ? (float)(lce / sums[1]) : 0.f;
    coef[1] = n > 0.0 ? (float)(lkd * tau / n) : 0.f;
}

// for valid i:  dL/ds_ik = upstream [ coef[0] w_y (p_ik - g_ik) + coef[1] (ptau_ik - q_ik) ];  else 0
template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_distill_bwd(const float* __restrict__ student, const float* __restrict__ teacher,
                                                     const LabelT* __restrict__ labels, int Crt, int64_t HW, int64_t npix,
                                                     const float* __restrict__ cw, int ignore_index, float inv_tau,
                                                     const float* __restrict__ coef, const float* __restrict__ upstream,
                                                     float* __restrict__ grad) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const bool unit = inv_tau == 1.f;
    const float up = upstream[0], a = coef[0], bk = coef[1];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i0 < npix; i0 += UNR * stride) {
        float z[UNR][CMAX], zt[UNR][CMAX];
        long long y[UNR], yt[UNR];
        int64_t off[UNR];
        bool in[UNR], int_[UNR];
        gather_pixels(student, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), z, y, off, in);
        gather_pixels(teacher, labels, C, HW, npix, i0, stride, (long long)ignore_index, every_pixel(), zt, yt, no_offsets(), int_);
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            if (off[u] < 0) continue;
            const long long yy = y[u];
            const bool valid = valid_label(yy, C, ignore_index);
            float m, lg;
            softmax_stats(z[u], C, m, lg);
            float zs[CMAX], zq[CMAX], ms = m, lgs = lg, mq, lgq;
            scale_logits(z[u], inv_tau, zs);
            scale_logits(zt[u], inv_tau, zq);
            if (!unit) softmax_stats(zs, C, ms, lgs);
            softmax_stats(zq, C, mq, lgq);
            const float aw = valid ? a * (cw ? cw[yy] : 1.f) : 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float pc = expf(log_softmax(z[u][c], m, lg));
                    const float pt = unit ? pc : expf(log_softmax(zs[c], ms, lgs));
                    const float qc = expf(log_softmax(zq[c], mq, lgq));
                    const float g = c == (int)yy ? 1.f : 0.f;
                    grad[off[u] + c * HW] = valid ? up * (aw * (pc - g) + bk * (pt - qc)) : 0.f;
                }
        }
    }
}

}  // namespace iswm

using namespace iswm;

static const char* const DISTILL_TAKES = "the distillation loss takes";

static bool distill_shape(int B, int64_t HW) { return B > 0 && HW > 0 && (int64_t)B * HW <= ((int64_t)1 << 36); }

extern "C" int64_t iswm_distill_loss_partials(int64_t npix) { return (int64_t)KD_SUMS * iswm_loss_blocks(npix); }

extern "C" int iswm_distill_loss_fwd(const float* student, const float* teacher, const void* labels, int label_bytes, int B, int C,
                                     int64_t HW, const float* class_weight, int ignore_index, float inv_tau, float* partials,
                                     double* sums, iswm_stream_t stream) {
    if (refuse_pixel_args("distill_loss_fwd", student && labels && partials && sums, distill_shape(B, HW), C, DISTILL_TAKES,
                          label_bytes)) return 1;
    ISWM_REQUIRE(teacher, "distill_loss_fwd: teacher pointer null");
    ISWM_REQUIRE(inv_tau > 0.f && inv_tau < INFINITY, "distill_loss_fwd: 1 / temperature must be positive and finite");
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_distill_sums<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, student, teacher,
                           (const T*)labels, C, HW, npix, class_weight, ignore_index, inv_tau, partials, blocks);
    });
    hipLaunchKernelGGL(k_overlap_finalize, dim3(KD_SUMS), dim3(64), 0, s, partials, blocks, sums);
    return check_launch("distill_loss_fwd");
}

extern "C" int iswm_distill_loss_coeffs(const double* sums, double ce_weight, double distill_weight, double temperature,
                                        float* out, float* coef, iswm_stream_t stream) {
    ISWM_REQUIRE(sums && out && coef, "distill_loss_coeffs: null pointer");
    ISWM_REQUIRE(temperature > 0.0 && temperature < INFINITY, "distill_loss_coeffs: the temperature must be positive and finite");
    ISWM_REQUIRE(ce_weight >= 0.0 && distill_weight >= 0.0 && ce_weight < INFINITY && distill_weight < INFINITY,
                 "distill_loss_coeffs: the term weights must be finite and not negative");
    hipLaunchKernelGGL(k_distill_coeffs, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, ce_weight, distill_weight, temperature,
                       out, coef);
    return check_launch("distill_loss_coeffs");
}

extern "C" int iswm_distill_loss_bwd(const float* student, const float* teacher, const void* labels, int label_bytes, int B, int C,
                                     int64_t HW, const float* class_weight, int ignore_index, float inv_tau, const float* coef,
                                     const float* upstream, float* grad, iswm_stream_t stream) {
    if (refuse_pixel_args("distill_loss_bwd", student && labels && coef && upstream && grad, distill_shape(B, HW), C,
                          DISTILL_TAKES, label_bytes)) return 1;
    ISWM_REQUIRE(teacher, "distill_loss_bwd: teacher pointer null");
    ISWM_REQUIRE(inv_tau > 0.f && inv_tau < INFINITY, "distill_loss_bwd: 1 / temperature must be positive and finite");
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_distill_bwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, student, teacher,
                           (const T*)labels, C, HW, npix, class_weight, ignore_index, inv_tau, coef, upstream, grad);
    });
    return check_launch("distill_loss_bwd");
}
