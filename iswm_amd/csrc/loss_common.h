// What the per-pixel criteria share (loss.hip, lovasz.hip): the two forms of log softmax, the validity rule, one pixel's value
// terms, the pixel walk, the fixed-order block sums, the kernel instantiation by label width and class count and the refusals of
// the per-pixel entry points.  Kernels that use these add their pixels in the same per-thread order, which is what makes their
// CE sums agree bit for bit.
#pragma once
#include <type_traits>

#include "common.h"

namespace iswm {

// log softmax of one class, in one of two forms chosen per pixel by |m| (m = the pixel's largest logit):
//   |m| <  LSE_SPLIT   z - (m + log(se)), what this kernel has always evaluated.  The sum lse = m + log(se) is rounded to an ulp of
//                      |lse| < 8 + log C < 16, at most 2^-21 = 4.8e-7 of a probability: at torch's own fp32 floor (3e-7).
//   |m| >= LSE_SPLIT   (z - m) - log(se): the maximum comes off first, so nothing is rounded at the scale of |m| (the first form
//                      costs 4e-6 on every probability at logits of magnitude 30-80).
// Why not the second form everywhere: it differs from the first in the last bit of about half the probabilities, and a training
// run amplifies that (ReLU and max-pool ties) to 2e-3 of the loss within 25 steps -- every recorded loss curve, golden vector and
// parent-vs-child comparison of a training run would move for no gain in accuracy where logits are of order 1.  Both forms are
// the same function to rounding, so the loss steps by at most one rounding (1e-6 relative) where |m| crosses the split; the
// branch is per pixel (m is shared by the pixel's classes) in an HBM-bound kernel.
constexpr float LSE_SPLIT = 8.f;
__device__ __forceinline__ float log_softmax(float z, float m, float lg) {
    return fabsf(m) < LSE_SPLIT ? z - (m + lg) : (z - m) - lg;
}

// the pixels every criterion counts: a label that is ignore_index or no class index adds no term and has a gradient of exactly 0
__device__ __forceinline__ bool valid_label(long long y, int C, int ignore_index) {
    return (y != (long long)ignore_index) && y >= 0 && y < C;
}

// m = the largest of the pixel's C logits (a register array) and lg = log sum exp(z - m), both in the order c = 0 .. C-1
__device__ __forceinline__ void softmax_stats(const float* z, int C, float& m, float& lg) {
    m = z[0];
    for (int c = 1; c < C; ++c) m = fmaxf(m, z[c]);
    float se = 0.f;
    for (int c = 0; c < C; ++c) se += expf(z[c] - m);
    lg = logf(se);
}

// one valid pixel of weight w: its value terms, and coef = dL_i/dce_i * w (the gradient is coef * (p - onehot), unnormalised)
__device__ __forceinline__ void loss_terms(float nll, float w, float alpha, float gamma, int mode, float& s1, float& s2, float& coef) {
    if (mode == 0) {
        s1 = fmaf(w, nll, s1);      // spelt out: the focal branch's w * nll must not draw this product out of the fused add
        s2 += w;
        coef = w;
    } else {
        const float ce = w * nll;
        float f, dfdce;
        if (gamma == 0.f) {
            f = alpha * ce;
            dfdce = alpha;
        } else {
            const float pt = expf(-ce);
            const float om = 1.f - pt;
            const float pw = powf(om, gamma);
            f = alpha * pw * ce;
            dfdce = (ce > 0.f && om > 0.f) ? alpha * (pw + gamma * powf(om, gamma - 1.f) * pt * ce) : 0.f;
        }
        s1 += f;
        s2 += w;
        coef = dfdce * w;
    }
}

// one pixel with its logits in registers: value terms and the unnormalised gradient coefficient (0 at an invalid pixel)
__device__ __forceinline__ void loss_pixel(const float* zc, int C, long long y, const float* __restrict__ cw,
                                           int ignore_index, float alpha, float gamma, int mode, float& s1, float& s2,
                                           float& coef, float& m, float& lg, bool& valid) {
    softmax_stats(zc, C, m, lg);
    valid = valid_label(y, C, ignore_index);
    coef = 0.f;
    if (valid) {
        float zy = zc[0];
        for (int c = 1; c < C; ++c) zy = (c == (int)y) ? zc[c] : zy;
        loss_terms(-log_softmax(zy, m, lg), cw ? cw[y] : 1.f, alpha, gamma, mode, s1, s2, coef);
    }
}

// The pixel walk of every kernel that reads logits: thread t of the grid takes the pixels i0 + u * stride, u < LOSS_UNR, of one
// iteration of `for (i0 = global thread index; i0 < npix; i0 += LOSS_UNR * stride)`, stride = the grid's thread count.
// LOSS_UNR independent pixels per thread and iteration (consecutive threads take consecutive pixels: every load and store of
// a wave is one contiguous 256-B run): 4x the bytes in flight of the one-pixel loop, which ran at 1.7 TB/s.  Kernels on this
// walk add their pixels in the same per-thread order, which is what makes their sums agree bit for bit.
// -> per pixel u: z[u] (the C logits, 0 beyond C), y[u] (the label; ypad past the end), off[u] (the offset of class 0 in
// logits / grad; -1 past the end) and in[u] (i < npix).  A kernel that writes no gradient passes no_offsets() for off and
// tests in[u]: an offset that is formed and then dropped still costs it two scalar registers.
// read(u, i, y) says whether pixel i's logits are wanted: where it is false they are not loaded (z[u] = 0) -- the backward
// pass of the hard-pixel loss reads 8 B only where a pixel is kept.
constexpr int LOSS_UNR = 4;
struct every_pixel {
    __device__ bool operator()(int, int64_t, long long) const { return true; }
};
struct no_offsets {
    struct sink {
        __device__ void operator=(int64_t) const {}
    };
    __device__ sink operator[](int) const { return sink(); }
};
template <int CMAX, typename LabelT, typename Read, typename Off>
__device__ __forceinline__ void gather_pixels(const float* logits, const LabelT* labels, int C, int64_t HW, int64_t npix, int64_t i0,
                                              int64_t stride, long long ypad, Read read, float (&z)[LOSS_UNR][CMAX],
                                              long long (&y)[LOSS_UNR], Off&& off, bool (&in)[LOSS_UNR]) {
#pragma unroll
    for (int u = 0; u < LOSS_UNR; ++u) {
        const int64_t i = i0 + u * stride;
        in[u] = i < npix;
        const int64_t ii = in[u] ? i : 0;
        const int64_t b = ii / HW, p = ii - b * HW;
        off[u] = in[u] ? b * C * HW + p : -1;
        y[u] = in[u] ? (long long)labels[ii] : ypad;
        const bool rd = in[u] && read(u, ii, y[u]);
#pragma unroll
        for (int c = 0; c < CMAX; ++c) z[u][c] = (rd && c < C) ? logits[b * C * HW + c * HW + p] : 0.f;
    }
}

// Block sums of N values per thread in a fixed order, no atomics: shuffle tree within each of the 4 waves, lane 0 -> red[k][wave],
// barrier.  block_total(red[k]) is then value k's sum over the 256 threads, (wave 0 + wave 1) + (wave 2 + wave 3).
// Callers accumulate in scalars and pack them into v right before the call: as one array across the pixel loop the sums of
// k_overlap_sums reached registers late and the kernel went from 81 to 320 VGPRs.
template <typename T, int N>
__device__ __forceinline__ void block_reduce(T (&v)[N], T (&red)[N][4]) {
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += __shfl_down(v[k], o);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
}
template <typename T>
__device__ __forceinline__ T block_total(const T (&r)[4]) {
    return (r[0] + r[1]) + (r[2] + r[3]);
}

// the criteria that hold a pixel's classes in registers take at most this many
constexpr int OVL_CMAX = 8;

}  // namespace iswm

// the kernel instantiation of a call: f(label type, CT) with CT = 2 (the binary masks: class count at compile time) or 0 (C at run time)
template <typename F>
static void by_label_and_classes(int label_bytes, int C, F&& f) {
    if (label_bytes == 1) {
        if (C == 2) f(uint8_t(), std::integral_constant<int, 2>());
        else f(uint8_t(), std::integral_constant<int, 0>());
    } else {
        if (C == 2) f(int64_t(), std::integral_constant<int, 2>());
        else f(int64_t(), std::integral_constant<int, 0>());
    }
}

// the refusals the per-pixel entry points share, in this order; `takes` names the criterion whose kernels hold the classes in
// registers (null: any C > 0 passes, the weighted CE streams the class axis beyond 8)
static int refuse_pixel_args(const char* fn, bool pointers, bool shape, int C, const char* takes, int label_bytes) {
    ISWM_REQUIRE(pointers, "%s: null pointer", fn);
    ISWM_REQUIRE(shape, "%s: bad shape", fn);
    ISWM_REQUIRE(!takes || (C >= 1 && C <= iswm::OVL_CMAX), "%s: %d classes (%s 1 to %d)", fn, C, takes, iswm::OVL_CMAX);
    ISWM_REQUIRE(label_bytes == 1 || label_bytes == 8, "%s: labels must be uint8 or int64", fn);
    return 0;
}
