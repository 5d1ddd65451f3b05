// The tail every maps kernel shares once it holds a pixel's foreground probability p (DESIGN.md sections 9 and 25): the
// pred / conf / band bytes of a 16-pixel chunk, its stores, the running statistics, the workgroup sum in a fixed order and the
// launch geometry.  k_predict_maps (predict.hip) takes p from the logits, k_prob_maps (crf.hip) from an fp32 map; fed the same
// p they write the same bytes, statistics included, because the chunks, their owners and every order of summation are these.
#pragma once
#include "common.h"

namespace iswm {

constexpr int PM_BLOCK = 256;
constexpr int PM_PIX = 16;           // consecutive raster pixels per thread: one 16-B store per uint8 map

struct PredictPartial {              // one workgroup's share of one image (32 B)
    double sum;
    float mn, mx;
    long long n_low, n_pred;
};

// The shared code is macro text, not functions: k_predict_maps's device assembly is held instruction for instruction (DESIGN.md
// section 13), and helper functions, __forceinline__ included, changed its register allocation both times they were tried (sections
// 13 and 25).  Macro text gives the compiler the statements it had.  The names are fixed: sum, mn, mx, n_low, n_pred, wp, wc, wb, pv.

// a thread's running statistics
#define ISWM_MAP_STATS_DECL                  \
    double sum = 0.0;                        \
    float mn = INFINITY, mx = -INFINITY;     \
    long long n_low = 0, n_pred = 0

// the bytes of one chunk, four pixels to a word, and its probabilities
#define ISWM_MAP_CHUNK_DECL \
    unsigned int wp[4] = {0u, 0u, 0u, 0u}, wc[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u}; \
    float pv[PM_PIX]

// pixel j of the chunk: pred = p > thr in fp32, conf truncates, band compares conf with the host's integer bounds
#define ISWM_MAP_PIXEL(j, p, thr, lo, hi)                                           \
    do {                                                                            \
        pv[j] = p;                                                                  \
        const unsigned int vp = p > thr ? 255u : 0u;                                \
        const unsigned int vc = (unsigned int)(p * 255.0f);                         \
        const unsigned int vb = ((int)vc >= lo && (int)vc <= hi) ? 255u : 0u;       \
        wp[j >> 2] |= vp << (8 * (j & 3));                                          \
        wc[j >> 2] |= vc << (8 * (j & 3));                                          \
        wb[j >> 2] |= vb << (8 * (j & 3));                                          \
        sum += (double)p;                                                           \
        mn = fminf(mn, p);                                                          \
        mx = fmaxf(mx, p);                                                          \
        n_low += p < thr ? 1 : 0;                                                   \
        n_pred += vp ? 1 : 0;                                                       \
    } while (0)

// the chunk at raster pixel q0 of which the pixels [j0, j1) belong to the caller: a whole chunk is one 16-B store per uint8 map,
// a shared or short one goes byte by byte
#define ISWM_MAP_STORE(q0, j0, j1, pred, conf, band, prob)                                                                \
    do {                                                                                                                  \
        if (j0 == 0 && j1 == PM_PIX) {                                                                                    \
            *reinterpret_cast<uint4*>(pred + q0) = make_uint4(wp[0], wp[1], wp[2], wp[3]);                                \
            *reinterpret_cast<uint4*>(conf + q0) = make_uint4(wc[0], wc[1], wc[2], wc[3]);                                \
            *reinterpret_cast<uint4*>(band + q0) = make_uint4(wb[0], wb[1], wb[2], wb[3]);                                \
            if (prob) {                                                                                                   \
                _Pragma("unroll") for (int j = 0; j < PM_PIX; j += 4)                                                     \
                    *reinterpret_cast<float4*>(prob + q0 + j) = make_float4(pv[j], pv[j + 1], pv[j + 2], pv[j + 3]);      \
            }                                                                                                             \
        } else {                                                                                                          \
            _Pragma("unroll") for (int j = 0; j < PM_PIX; ++j) {                                                          \
                if (j < j0 || j >= j1) continue;                                                                          \
                const int sh8 = 8 * (j & 3);                                                                              \
                pred[q0 + j] = (unsigned char)(wp[j >> 2] >> sh8);                                                        \
                conf[q0 + j] = (unsigned char)(wc[j >> 2] >> sh8);                                                        \
                band[q0 + j] = (unsigned char)(wb[j >> 2] >> sh8);                                                        \
                if (prob) prob[q0 + j] = pv[j];                                                                           \
            }                                                                                                             \
        }                                                                                                                 \
    } while (0)

// workgroup reduction in a fixed order: wave shuffles, then thread 0 over the four wave results, into partials[slot]
#define ISWM_MAP_BLOCK_SUM(partials, slot)                                                  \
    __shared__ PredictPartial red[PM_BLOCK / 64];                                           \
    _Pragma("unroll") for (int off = 32; off > 0; off >>= 1) {                              \
        sum += __shfl_down(sum, off, 64);                                                   \
        mn = fminf(mn, __shfl_down(mn, off, 64));                                           \
        mx = fmaxf(mx, __shfl_down(mx, off, 64));                                           \
        n_low += __shfl_down(n_low, off, 64);                                               \
        n_pred += __shfl_down(n_pred, off, 64);                                             \
    }                                                                                       \
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;                             \
    if (lane == 0) red[wave] = PredictPartial{sum, mn, mx, n_low, n_pred};                  \
    __syncthreads();                                                                        \
    if (threadIdx.x == 0) {                                                                 \
        PredictPartial r = red[0];                                                          \
        for (int w = 1; w < PM_BLOCK / 64; ++w) {                                           \
            r.sum += red[w].sum;                                                            \
            r.mn = fminf(r.mn, red[w].mn);                                                  \
            r.mx = fmaxf(r.mx, red[w].mx);                                                  \
            r.n_low += red[w].n_low;                                                        \
            r.n_pred += red[w].n_pred;                                                      \
        }                                                                                   \
        partials[slot] = r;                                                                 \
    }

// workgroups per image: about one chunk per thread, at most ~2048 workgroups in all
inline int predict_blocks_per_image(int N, int H, int W) {
    const int64_t chunks = ((int64_t)H * W + PM_PIX - 1) / PM_PIX + 1;
    int64_t b = (chunks + PM_BLOCK - 1) / PM_BLOCK;
    const int64_t cap = N >= 2048 ? 1 : 2048 / N;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

// stats[n] = the partials of image n summed in a fixed order (k_predict_stats, predict.hip), on the caller's stream
int launch_predict_stats(const PredictPartial* partials, int blocks, int N, double* stats, hipStream_t stream);

}  // namespace iswm
