// Inference outputs on the device: the reference's predict.py per-image chain
//   ToTensor -> Normalize (predict.py:93-97), model, softmax, prob[:, 1], `> threshold`, `* 255 -> uint8`,
//   binarize_confidence_map (predict.py:214-290)
// as two kernels around the model:
//   * k_predict_normalize: uint8 HWC RGB -> normalised fp32 NCHW, (v / 255.0f - m) / s in IEEE fp32 as torch does
//     on the CPU (the expression k_augment uses);
//   * k_predict_maps: the classifier's low-resolution NHWC logits -> bilinear sample (the index and weight arithmetic
//     of k_bilinear_to_nchw_fwd, bilinear.h) -> softmax over C classes -> p = prob[fg] -> pred / conf / band uint8
//     maps (+ optional fp32 p) and per-workgroup statistics in a slab, summed by k_predict_stats in a fixed order.
// and, for frames larger than the training crops, predicted in overlapping windows:
//   * k_scene_tiles_normalize: the windows of a resident uint8 scene -> normalised fp32 NCHW, the same arithmetic;
//   * k_scene_maps: the logits of all windows -> per scene pixel the ramp-weighted blend of the covering windows' p
//     (a gather in a fixed order) -> the same maps and statistics.
// and, for test-time augmentation, the probability averaged over resampled and mirrored views:
//   * k_predict_view_normalize: resident uint8 frames -> one view (bilinear resample, mirror) as normalised fp32 NCHW;
//   * k_predict_views_maps: the logits of all views -> per frame pixel the mean of the views' p (a gather in list
//     order) -> the same maps and statistics.
// Exactness: the threshold compare is fp32 (torch compares a float32 tensor with a Python float
// in float32); conf truncates (numpy astype(uint8)); the band compares conf with integer bounds the host derived
// from the reference's fp64 expression conf / 255.0 >= min_prob, <= max_prob; no float atomics anywhere.
#include "bilinear.h"
#include "predict_tail.h"            // PM_BLOCK, PM_PIX, PredictPartial, the map tail and the workgroup sum
#include "rowmap.h"

namespace iswm {

constexpr int PM_MAX_GROUPS = 4;     // logits kept in registers for C <= 16; larger C re-samples in a second pass

__global__ __launch_bounds__(256) void k_predict_normalize(const unsigned char* __restrict__ img, int N, int64_t HW,
                                                           float m0, float m1, float m2, float s0, float s1, float s2,
                                                           float* __restrict__ out) {
    const int64_t M = (int64_t)N * HW;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / HW, p = i - n * HW;
        const unsigned char* s = img + i * 3;
        float* o = out + n * 3 * HW + p;
        o[0] = __fdiv_rn(__fdiv_rn((float)s[0], 255.0f) - m0, s0);
        o[HW] = __fdiv_rn(__fdiv_rn((float)s[1], 255.0f) - m1, s1);
        o[2 * HW] = __fdiv_rn(__fdiv_rn((float)s[2], 255.0f) - m2, s2);
    }
}

// the four source taps of one output pixel, same expression as k_bilinear_to_nchw_fwd
__device__ __forceinline__ float4 bilerp4(const float* pa, const float* pb, const float* pd, const float* pe,
                                          const Lerp& lh, const Lerp& lw, int c0) {
    float4 a = ld4(pa + c0), b = ld4(pb + c0), d = ld4(pd + c0), e = ld4(pe + c0);
    float4 o;
    o.x = lh.l0 * (lw.l0 * a.x + lw.l1 * b.x) + lh.l1 * (lw.l0 * d.x + lw.l1 * e.x);
    o.y = lh.l0 * (lw.l0 * a.y + lw.l1 * b.y) + lh.l1 * (lw.l0 * d.y + lw.l1 * e.y);
    o.z = lh.l0 * (lw.l0 * a.z + lw.l1 * b.z) + lh.l1 * (lw.l0 * d.z + lw.l1 * e.z);
    o.w = lh.l0 * (lw.l0 * a.w + lw.l1 * b.w) + lh.l1 * (lw.l0 * d.w + lw.l1 * e.w);
    return o;
}

__device__ __forceinline__ float comp(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// p = softmax(l)[fg] with m = max_c l_c, e_c = expf(l_c - m), s summed in class order
template <int G>
__device__ __forceinline__ float fg_prob(const float* pa, const float* pb, const float* pd, const float* pe,
                                         const Lerp& lh, const Lerp& lw, int C, int fg) {
    if constexpr (G > 0) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = bilerp4(pa, pb, pd, pe, lh, lw, 4 * g);
        float m = v[0].x;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < C) m = fmaxf(m, comp(v[g], k));
        float s = 0.f, ef = 0.f;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < C) {
                    const float e = expf(comp(v[g], k) - m);
                    s += e;
                    if (4 * g + k == fg) ef = e;
                }
        return __fdiv_rn(ef, s);
    } else {                     // C > 16: sample twice (the same arithmetic gives the same logits)
        float m = -INFINITY;
        for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 v = bilerp4(pa, pb, pd, pe, lh, lw, c0);
            for (int k = 0; k < 4 && c0 + k < C; ++k) m = fmaxf(m, comp(v, k));
        }
        float s = 0.f, ef = 0.f;
        for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 v = bilerp4(pa, pb, pd, pe, lh, lw, c0);
            for (int k = 0; k < 4 && c0 + k < C; ++k) {
                const float e = expf(comp(v, k) - m);
                s += e;
                if (c0 + k == fg) ef = e;
            }
        }
        return __fdiv_rn(ef, s);
    }
}

// grid (blocks_per_image, N).  Image n owns the raster pixels [n*H*W, (n+1)*H*W) of the [N, H, W] outputs; a thread
// takes the 16-pixel chunks k of the whole tensor (pixels [16k, 16k+16)) that overlap its image and produces the
// pixels of the chunk inside it.  A chunk wholly inside the image is stored as one 16-B store per uint8 map; a chunk
// shared by two images (at most one per image boundary) is written byte by byte by both.
template <int G>
__global__ __launch_bounds__(PM_BLOCK) void k_predict_maps(const float* __restrict__ yl, int Hi, int Wi, int ldx, int C,
                                                           int fg, int Ho, int Wo, float sh, float sw, float thr, int lo,
                                                           int hi, unsigned char* __restrict__ pred,
                                                           unsigned char* __restrict__ conf,
                                                           unsigned char* __restrict__ band, float* __restrict__ prob,
                                                           PredictPartial* __restrict__ partials) {
    const int n = blockIdx.y;
    const int64_t HW = (int64_t)Ho * Wo;
    const int64_t p_begin = (int64_t)n * HW, p_end = p_begin + HW;
    const int64_t k_begin = p_begin / PM_PIX, k_end = (p_end + PM_PIX - 1) / PM_PIX;
    const float* base = yl + (size_t)n * Hi * Wi * ldx;

    ISWM_MAP_STATS_DECL;
    for (int64_t k = k_begin + (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x; k < k_end;
         k += (int64_t)gridDim.x * PM_BLOCK) {
        const int64_t q0 = k * PM_PIX;
        const int j0 = q0 < p_begin ? (int)(p_begin - q0) : 0;
        const int j1 = q0 + PM_PIX > p_end ? (int)(p_end - q0) : PM_PIX;
        int rem = (int)(q0 + j0 - p_begin);
        int oh = rem / Wo, ow = rem - oh * Wo;
        Lerp lh = src_index(sh, oh, Hi);
        ISWM_MAP_CHUNK_DECL;
#pragma unroll
        for (int j = 0; j < PM_PIX; ++j) {
            pv[j] = 0.f;
            if (j < j0 || j >= j1) continue;
            const Lerp lw = src_index(sw, ow, Wi);
            const float* pa = base + ((size_t)lh.i0 * Wi + lw.i0) * ldx;
            const float* pb = base + ((size_t)lh.i0 * Wi + lw.i1) * ldx;
            const float* pd = base + ((size_t)lh.i1 * Wi + lw.i0) * ldx;
            const float* pe = base + ((size_t)lh.i1 * Wi + lw.i1) * ldx;
            const float p = fg_prob<G>(pa, pb, pd, pe, lh, lw, C, fg);
            ISWM_MAP_PIXEL(j, p, thr, lo, hi);
            if (++ow == Wo) {
                ow = 0;
                lh = src_index(sh, ++oh, Hi);
            }
        }
        ISWM_MAP_STORE(q0, j0, j1, pred, conf, band, prob);
    }
    ISWM_MAP_BLOCK_SUM(partials, (size_t)n * gridDim.x + blockIdx.x)
}

// stats[n] = {min p, max p, sum p, count(p < thr), count(pred)}: one wave per image; lane l takes the partials
// l, l + 64, ... in order, then a shuffle tree -- a fixed order, so the result is bit-reproducible
__global__ __launch_bounds__(64) void k_predict_stats(const PredictPartial* __restrict__ partials, int blocks,
                                                      double* __restrict__ stats) {
    const int n = blockIdx.x, lane = threadIdx.x;
    const PredictPartial* p = partials + (size_t)n * blocks;
    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long n_low = 0, n_pred = 0;
    for (int b = lane; b < blocks; b += 64) {
        sum += p[b].sum;
        mn = fminf(mn, p[b].mn);
        mx = fmaxf(mx, p[b].mx);
        n_low += p[b].n_low;
        n_pred += p[b].n_pred;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        mn = fminf(mn, __shfl_down(mn, off, 64));
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        n_low += __shfl_down(n_low, off, 64);
        n_pred += __shfl_down(n_pred, off, 64);
    }
    if (lane == 0) {
        double* s = stats + (size_t)n * 5;
        s[0] = (double)mn;
        s[1] = (double)mx;
        s[2] = sum;
        s[3] = (double)n_low;
        s[4] = (double)n_pred;
    }
}

// ---- sliding-window prediction of whole scenes -------------------------------------------
// A scene of H x W is cut into nty x ntx windows of th x tw (iswm_scene_plan): window k of an axis starts at
// min(k * s, L - t), so the last one is pulled back inside the scene.  Both kernels derive the origins from the plan.

__host__ __device__ __forceinline__ int scene_origin(int k, int s, int L, int t) {
    const int o = k * s;
    return o < L - t ? o : L - t;
}

// blending weight along one axis: a ramp of R steps from each edge of the window
__device__ __forceinline__ int scene_w1d(int i, int len, int R) {
    const int e = i + 1 < len - i ? i + 1 : len - i;
    return e < R ? e : R;
}

// the windows of one axis that cover coordinate c, in ascending order: the regular ones k0 .. k0 + nreg - 1 (origin
// k * s), then the pulled-back last one when n > nreg; wsum = the sum of their ramp weights at c (>= 1: every
// coordinate of a valid plan is covered)
struct SceneCover {
    int k0, nreg, n, wsum;
};

__device__ __forceinline__ int scene_cover_tile(const SceneCover& cv, int i, int nt) {
    return i < cv.nreg ? cv.k0 + i : nt - 1;
}

__device__ __forceinline__ SceneCover scene_cover(int c, int L, int t, int s, int nt, int R) {
    SceneCover cv;
    const int lo = (c - t + s) / s, hi = c / s;           // ceil((c - t + 1) / s) where that is positive
    cv.k0 = lo > 0 ? lo : 0;
    const int k1 = hi < nt - 2 ? hi : nt - 2;
    cv.nreg = k1 >= cv.k0 ? k1 - cv.k0 + 1 : 0;
    cv.n = cv.nreg + (c >= L - t ? 1 : 0);
    cv.wsum = 0;
    for (int i = 0; i < cv.n; ++i)
        cv.wsum += scene_w1d(c - scene_origin(scene_cover_tile(cv, i, nt), s, L, t), t, R);
    return cv;
}

// uint8 HWC scene -> the windows first_tile .. first_tile + B - 1 as fp32 NCHW [B][3][th][tw], k_predict_normalize's
// arithmetic; one thread per output pixel, consecutive threads along a window row
__global__ __launch_bounds__(256) void k_scene_tiles_normalize(const unsigned char* __restrict__ scene,
                                                               iswm_scene_plan pl, int k0, int B, float m0, float m1,
                                                               float m2, float s0, float s1, float s2,
                                                               float* __restrict__ out) {
    const int64_t thw = (int64_t)pl.th * pl.tw, M = (int64_t)B * thw;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t b = i / thw, p = i - b * thw;
        const int y = (int)(p / pl.tw), x = (int)(p - (int64_t)y * pl.tw);
        const int k = k0 + (int)b, ty = k / pl.ntx, tx = k - ty * pl.ntx;
        const int oy = scene_origin(ty, pl.sy, pl.H, pl.th), ox = scene_origin(tx, pl.sx, pl.W, pl.tw);
        const unsigned char* s = scene + ((int64_t)(oy + y) * pl.W + (ox + x)) * 3;
        float* o = out + b * 3 * thw + p;
        o[0] = __fdiv_rn(__fdiv_rn((float)s[0], 255.0f) - m0, s0);
        o[thw] = __fdiv_rn(__fdiv_rn((float)s[1], 255.0f) - m1, s1);
        o[2 * thw] = __fdiv_rn(__fdiv_rn((float)s[2], 255.0f) - m2, s2);
    }
}

// p of scene pixel (y, x): the windows that cover it, ascending ty then tx, each sampled as k_predict_maps samples
// its image (fg_prob at the in-window coordinate) and blended with weight w_t / W, w_t = w1d(y) * w1d(x) and
// W = sum w_t = cy.wsum * cx.wsum (the covering set is a product set); integers below 2^24, so exact in fp32.
// A pixel under one window has w_t / W = 1 and fmaf(1, p_t, 0) = p_t.
template <int G>
__device__ __forceinline__ float scene_prob(const float* __restrict__ yl, size_t tile_stride,
                                            const iswm_scene_plan& pl, int Hi, int Wi, int ldx, int C, int fg,
                                            float sh, float sw, const SceneCover& cy, int y, int x) {
    const SceneCover cx = scene_cover(x, pl.W, pl.tw, pl.sx, pl.ntx, pl.ramp);
    const float wsum = (float)(cy.wsum * cx.wsum);
    float p = 0.f;
    for (int a = 0; a < cy.n; ++a) {
        const int ty = scene_cover_tile(cy, a, pl.nty);
        const int iy = y - scene_origin(ty, pl.sy, pl.H, pl.th);
        const int wy = scene_w1d(iy, pl.th, pl.ramp);
        const Lerp lh = src_index(sh, iy, Hi);
        for (int b = 0; b < cx.n; ++b) {
            const int tx = scene_cover_tile(cx, b, pl.ntx);
            const int ix = x - scene_origin(tx, pl.sx, pl.W, pl.tw);
            const Lerp lw = src_index(sw, ix, Wi);
            const float* base = yl + ((size_t)ty * pl.ntx + tx) * tile_stride;
            const float* pa = base + ((size_t)lh.i0 * Wi + lw.i0) * ldx;
            const float* pb = base + ((size_t)lh.i0 * Wi + lw.i1) * ldx;
            const float* pd = base + ((size_t)lh.i1 * Wi + lw.i0) * ldx;
            const float* pe = base + ((size_t)lh.i1 * Wi + lw.i1) * ldx;
            const float pt = fg_prob<G>(pa, pb, pd, pe, lh, lw, C, fg);
            const float wn = __fdiv_rn((float)(wy * scene_w1d(ix, pl.tw, pl.ramp)), wsum);
            p = fmaf(wn, pt, p);
        }
    }
    return fminf(p, 1.0f);
}

// grid (blocks).  One scene per launch: a thread takes 16-pixel chunks k (raster pixels [16k, 16k + 16)) of the
// [H, W] outputs, which start at 0, so only the last chunk can be short.  A gather: every output pixel visits the
// windows that cover it, so nothing is accumulated in memory and every byte is written once.  The maps, the
// statistics and their order of reduction are k_predict_maps's.
template <int G>
__global__ __launch_bounds__(PM_BLOCK) void k_scene_maps(const float* __restrict__ yl, iswm_scene_plan pl, int Hi,
                                                         int Wi, int ldx, int C, int fg, float sh, float sw, float thr,
                                                         int lo, int hi, unsigned char* __restrict__ pred,
                                                         unsigned char* __restrict__ conf,
                                                         unsigned char* __restrict__ band, float* __restrict__ prob,
                                                         PredictPartial* __restrict__ partials) {
    const int64_t HW = (int64_t)pl.H * pl.W;
    const int64_t k_end = (HW + PM_PIX - 1) / PM_PIX;
    const size_t tile_stride = (size_t)Hi * Wi * ldx;

    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long n_low = 0, n_pred = 0;
    for (int64_t k = (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x; k < k_end; k += (int64_t)gridDim.x * PM_BLOCK) {
        const int64_t q0 = k * PM_PIX;
        const int j1 = q0 + PM_PIX > HW ? (int)(HW - q0) : PM_PIX;
        int oh = (int)(q0 / pl.W), ow = (int)(q0 - (int64_t)oh * pl.W);
        SceneCover cy = scene_cover(oh, pl.H, pl.th, pl.sy, pl.nty, pl.ramp);
        unsigned int wp[4] = {0u, 0u, 0u, 0u}, wc[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
        float pv[PM_PIX];
#pragma unroll
        for (int j = 0; j < PM_PIX; ++j) {
            pv[j] = 0.f;
            if (j >= j1) continue;
            const float p = scene_prob<G>(yl, tile_stride, pl, Hi, Wi, ldx, C, fg, sh, sw, cy, oh, ow);
            pv[j] = p;
            const unsigned int vp = p > thr ? 255u : 0u;
            const unsigned int vc = (unsigned int)(p * 255.0f);
            const unsigned int vb = ((int)vc >= lo && (int)vc <= hi) ? 255u : 0u;
            wp[j >> 2] |= vp << (8 * (j & 3));
            wc[j >> 2] |= vc << (8 * (j & 3));
            wb[j >> 2] |= vb << (8 * (j & 3));
            sum += (double)p;
            mn = fminf(mn, p);
            mx = fmaxf(mx, p);
            n_low += p < thr ? 1 : 0;
            n_pred += vp ? 1 : 0;
            if (++ow == pl.W) {
                ow = 0;
                ++oh;
                if (oh < pl.H) cy = scene_cover(oh, pl.H, pl.th, pl.sy, pl.nty, pl.ramp);
            }
        }
        if (j1 == PM_PIX) {
            *reinterpret_cast<uint4*>(pred + q0) = make_uint4(wp[0], wp[1], wp[2], wp[3]);
            *reinterpret_cast<uint4*>(conf + q0) = make_uint4(wc[0], wc[1], wc[2], wc[3]);
            *reinterpret_cast<uint4*>(band + q0) = make_uint4(wb[0], wb[1], wb[2], wb[3]);
            if (prob) {
#pragma unroll
                for (int j = 0; j < PM_PIX; j += 4)
                    *reinterpret_cast<float4*>(prob + q0 + j) = make_float4(pv[j], pv[j + 1], pv[j + 2], pv[j + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PM_PIX; ++j) {
                if (j >= j1) continue;
                const int sh8 = 8 * (j & 3);
                pred[q0 + j] = (unsigned char)(wp[j >> 2] >> sh8);
                conf[q0 + j] = (unsigned char)(wc[j >> 2] >> sh8);
                band[q0 + j] = (unsigned char)(wb[j >> 2] >> sh8);
                if (prob) prob[q0 + j] = pv[j];
            }
        }
    }

    // k_predict_maps's workgroup reduction, in its order (kept apart: that kernel's code is pinned, section 13)
    __shared__ PredictPartial red[PM_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        mn = fminf(mn, __shfl_down(mn, off, 64));
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        n_low += __shfl_down(n_low, off, 64);
        n_pred += __shfl_down(n_pred, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = PredictPartial{sum, mn, mx, n_low, n_pred};
    __syncthreads();
    if (threadIdx.x == 0) {
        PredictPartial r = red[0];
        for (int w = 1; w < PM_BLOCK / 64; ++w) {
            r.sum += red[w].sum;
            r.mn = fminf(r.mn, red[w].mn);
            r.mx = fmaxf(r.mx, red[w].mx);
            r.n_low += red[w].n_low;
            r.n_pred += red[w].n_pred;
        }
        partials[blockIdx.x] = r;
    }
}

// ---- flip and multi-scale test-time augmentation -----------------------------------------
// The probability of a frame is the mean over views of it: the frame resampled to Hv x Wv and, for a flipped view,
// mirrored left to right.  k_predict_view_normalize makes one view's network input from the resident uint8 frames;
// k_predict_views_maps gathers every view's low-resolution logits into the frame's maps.

// uint8 NHWC frames -> one view as fp32 NCHW [N][3][Hv][Wv]: F.interpolate(bilinear, align_corners=False) of the
// frame, then .flip(-1), then k_predict_normalize's arithmetic.  One thread per output pixel, consecutive threads
// along an output row.  With Hv = H the scale is 1.0f, the source coordinate the integer itself, l1 = 0 and l0 = 1:
// 1 * (1 * a + 0 * b) + 0 * (...) = a with or without contraction, so the identity view is k_predict_normalize's bits.
__global__ __launch_bounds__(256) void k_predict_view_normalize(const unsigned char* __restrict__ img, int N, int H,
                                                                int W, int Hv, int Wv, int flip, float sh, float sw,
                                                                float m0, float m1, float m2, float s0, float s1,
                                                                float s2, float* __restrict__ out) {
    const int64_t HWv = (int64_t)Hv * Wv, M = (int64_t)N * HWv;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < M; i += (int64_t)gridDim.x * 256) {
        const int64_t n = i / HWv, p = i - n * HWv;
        const int y = (int)(p / Wv), x = (int)(p - (int64_t)y * Wv);
        const Lerp lh = src_index(sh, y, H);
        const Lerp lw = src_index(sw, flip ? Wv - 1 - x : x, W);
        const unsigned char* f = img + n * ((int64_t)H * W * 3);
        const unsigned char* pa = f + ((int64_t)lh.i0 * W + lw.i0) * 3;
        const unsigned char* pb = f + ((int64_t)lh.i0 * W + lw.i1) * 3;
        const unsigned char* pd = f + ((int64_t)lh.i1 * W + lw.i0) * 3;
        const unsigned char* pe = f + ((int64_t)lh.i1 * W + lw.i1) * 3;
        const float v0 = lh.l0 * (lw.l0 * (float)pa[0] + lw.l1 * (float)pb[0]) +
                         lh.l1 * (lw.l0 * (float)pd[0] + lw.l1 * (float)pe[0]);
        const float v1 = lh.l0 * (lw.l0 * (float)pa[1] + lw.l1 * (float)pb[1]) +
                         lh.l1 * (lw.l0 * (float)pd[1] + lw.l1 * (float)pe[1]);
        const float v2 = lh.l0 * (lw.l0 * (float)pa[2] + lw.l1 * (float)pb[2]) +
                         lh.l1 * (lw.l0 * (float)pd[2] + lw.l1 * (float)pe[2]);
        float* o = out + n * 3 * HWv + p;
        o[0] = __fdiv_rn(__fdiv_rn(v0, 255.0f) - m0, s0);
        o[HWv] = __fdiv_rn(__fdiv_rn(v1, 255.0f) - m1, s1);
        o[2 * HWv] = __fdiv_rn(__fdiv_rn(v2, 255.0f) - m2, s2);
    }
}

// the views of one launch, passed by value: iswm_predict_view plus the two scales the host derived from it
struct PredictViewArg {
    const float* yl;
    int Hi, Wi, flip;
    float sh, sw;                    // (float)Hi / (float)Ho, (float)Wi / (float)Wo
};
struct PredictViewList {
    PredictViewArg v[ISWM_PREDICT_MAX_VIEWS];
};

// p of frame pixel (oh, ow) of image n: every view sampled as k_predict_maps samples its image, one bilinear step from
// the view's logits to the frame, a flipped view at the mirrored column; summed in list order and divided once.  No
// clamp: every p_v <= 1, so the exact partial sum of k of them is <= k, k is representable, and round-to-nearest is
// monotone: the fp32 partial sum stays <= k and acc / V <= 1.
template <int G>
__device__ __forceinline__ float views_prob(const PredictViewList& vl, int V, int n, int ldx, int C, int fg, int Wo,
                                            int oh, int ow) {
    float acc = 0.f;
    for (int v = 0; v < V; ++v) {
        const PredictViewArg& a = vl.v[v];
        const Lerp lh = src_index(a.sh, oh, a.Hi);
        const Lerp lw = src_index(a.sw, a.flip ? Wo - 1 - ow : ow, a.Wi);
        const float* base = a.yl + (size_t)n * a.Hi * a.Wi * ldx;
        const float* pa = base + ((size_t)lh.i0 * a.Wi + lw.i0) * ldx;
        const float* pb = base + ((size_t)lh.i0 * a.Wi + lw.i1) * ldx;
        const float* pd = base + ((size_t)lh.i1 * a.Wi + lw.i0) * ldx;
        const float* pe = base + ((size_t)lh.i1 * a.Wi + lw.i1) * ldx;
        acc += fg_prob<G>(pa, pb, pd, pe, lh, lw, C, fg);
    }
    return __fdiv_rn(acc, (float)V);
}

// grid (blocks_per_image, N): k_predict_maps's chunks, maps, statistics and order of reduction, with views_prob for p.
// A gather: nothing is accumulated in memory and every output byte is written once.
template <int G>
__global__ __launch_bounds__(PM_BLOCK) void k_predict_views_maps(PredictViewList vl, int V, int ldx, int C, int fg,
                                                                 int Ho, int Wo, float thr, int lo, int hi,
                                                                 unsigned char* __restrict__ pred,
                                                                 unsigned char* __restrict__ conf,
                                                                 unsigned char* __restrict__ band,
                                                                 float* __restrict__ prob,
                                                                 PredictPartial* __restrict__ partials) {
    const int n = blockIdx.y;
    const int64_t HW = (int64_t)Ho * Wo;
    const int64_t p_begin = (int64_t)n * HW, p_end = p_begin + HW;
    const int64_t k_begin = p_begin / PM_PIX, k_end = (p_end + PM_PIX - 1) / PM_PIX;

    double sum = 0.0;
    float mn = INFINITY, mx = -INFINITY;
    long long n_low = 0, n_pred = 0;
    for (int64_t k = k_begin + (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x; k < k_end;
         k += (int64_t)gridDim.x * PM_BLOCK) {
        const int64_t q0 = k * PM_PIX;
        const int j0 = q0 < p_begin ? (int)(p_begin - q0) : 0;
        const int j1 = q0 + PM_PIX > p_end ? (int)(p_end - q0) : PM_PIX;
        int rem = (int)(q0 + j0 - p_begin);
        int oh = rem / Wo, ow = rem - oh * Wo;
        unsigned int wp[4] = {0u, 0u, 0u, 0u}, wc[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
        float pv[PM_PIX];
#pragma unroll
        for (int j = 0; j < PM_PIX; ++j) {
            pv[j] = 0.f;
            if (j < j0 || j >= j1) continue;
            const float p = views_prob<G>(vl, V, n, ldx, C, fg, Wo, oh, ow);
            pv[j] = p;
            const unsigned int vp = p > thr ? 255u : 0u;
            const unsigned int vc = (unsigned int)(p * 255.0f);
            const unsigned int vb = ((int)vc >= lo && (int)vc <= hi) ? 255u : 0u;
            wp[j >> 2] |= vp << (8 * (j & 3));
            wc[j >> 2] |= vc << (8 * (j & 3));
            wb[j >> 2] |= vb << (8 * (j & 3));
            sum += (double)p;
            mn = fminf(mn, p);
            mx = fmaxf(mx, p);
            n_low += p < thr ? 1 : 0;
            n_pred += vp ? 1 : 0;
            if (++ow == Wo) {
                ow = 0;
                ++oh;
            }
        }
        if (j0 == 0 && j1 == PM_PIX) {
            *reinterpret_cast<uint4*>(pred + q0) = make_uint4(wp[0], wp[1], wp[2], wp[3]);
            *reinterpret_cast<uint4*>(conf + q0) = make_uint4(wc[0], wc[1], wc[2], wc[3]);
            *reinterpret_cast<uint4*>(band + q0) = make_uint4(wb[0], wb[1], wb[2], wb[3]);
            if (prob) {
#pragma unroll
                for (int j = 0; j < PM_PIX; j += 4)
                    *reinterpret_cast<float4*>(prob + q0 + j) = make_float4(pv[j], pv[j + 1], pv[j + 2], pv[j + 3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < PM_PIX; ++j) {
                if (j < j0 || j >= j1) continue;
                const int sh8 = 8 * (j & 3);
                pred[q0 + j] = (unsigned char)(wp[j >> 2] >> sh8);
                conf[q0 + j] = (unsigned char)(wc[j >> 2] >> sh8);
                band[q0 + j] = (unsigned char)(wb[j >> 2] >> sh8);
                if (prob) prob[q0 + j] = pv[j];
            }
        }
    }

    // k_predict_maps's workgroup reduction, in its order (kept apart: that kernel's code is pinned, section 13)
    __shared__ PredictPartial red[PM_BLOCK / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        sum += __shfl_down(sum, off, 64);
        mn = fminf(mn, __shfl_down(mn, off, 64));
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
        n_low += __shfl_down(n_low, off, 64);
        n_pred += __shfl_down(n_pred, off, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = PredictPartial{sum, mn, mx, n_low, n_pred};
    __syncthreads();
    if (threadIdx.x == 0) {
        PredictPartial r = red[0];
        for (int w = 1; w < PM_BLOCK / 64; ++w) {
            r.sum += red[w].sum;
            r.mn = fminf(r.mn, red[w].mn);
            r.mx = fmaxf(r.mx, red[w].mx);
            r.n_low += red[w].n_low;
            r.n_pred += red[w].n_pred;
        }
        partials[(size_t)n * gridDim.x + blockIdx.x] = r;
    }
}

// one axis of the plan: t = min(T, L); one window when it spans the axis, else windows every s = t - O with the last
// pulled back.  false: the overlap exceeds half a window.
static bool scene_plan_axis(int L, int T, int O, int* t, int* s, int* n) {
    *t = T < L ? T : L;
    if (L <= *t) {
        *s = *t;
        *n = 1;
        return true;
    }
    if (O > *t / 2) return false;
    *s = *t - O;
    *n = (L - *t + *s - 1) / *s + 1;
    return true;
}

// what the kernels rely on: every coordinate is covered, every window lies inside the scene, the weights stay
// below 2^24 / 9
static bool scene_axis_ok(int L, int t, int s, int n) {
    if (L < 1 || t < 1 || t > L || s < 1 || n < 1) return false;
    if (n == 1) return t == L;
    return s <= t && t - s <= t / 2 && (int64_t)(n - 2) * s < L - t && (int64_t)(n - 1) * s >= L - t;
}

static bool scene_plan_ok(const iswm_scene_plan& p) {
    return scene_axis_ok(p.H, p.th, p.sy, p.nty) && scene_axis_ok(p.W, p.tw, p.sx, p.ntx) && p.ramp >= 1 &&
           p.ramp <= 1024 && (int64_t)p.nty * p.ntx <= 0x7fffffff;
}

int launch_predict_stats(const PredictPartial* partials, int blocks, int N, double* stats, hipStream_t stream) {
    hipLaunchKernelGGL(k_predict_stats, dim3(N), dim3(64), 0, stream, partials, blocks, stats);
    return check_launch("predict_stats");
}

}  // namespace iswm

using namespace iswm;

extern "C" int iswm_predict_normalize(const unsigned char* img, int N, int H, int W, const float* mean3,
                                      const float* std3, float* out_nchw, iswm_stream_t stream) {
    ISWM_REQUIRE(img && mean3 && std3 && out_nchw, "predict_normalize: null pointer");
    ISWM_REQUIRE(N > 0 && H > 0 && W > 0, "predict_normalize: bad size");
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(k_predict_normalize, dim3(stream_grid((int64_t)N * HW, 256)), dim3(256), 0,
                       (hipStream_t)stream, img, N, HW, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2],
                       out_nchw);
    return check_launch("predict_normalize");
}

extern "C" size_t iswm_predict_maps_workspace(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)N * predict_blocks_per_image(N, H, W) * sizeof(PredictPartial);
}

extern "C" int iswm_predict_maps(const float* yl, int N, int Hi, int Wi, int ldx, int C, int fg, int Ho, int Wo,
                                 float thr, int band_lo, int band_hi, unsigned char* pred, unsigned char* conf,
                                 unsigned char* band, float* prob, double* stats, void* workspace,
                                 size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(yl && pred && conf && band && stats && workspace, "predict_maps: null pointer");
    ISWM_REQUIRE(N > 0 && N <= 65535 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0, "predict_maps: bad size");
    ISWM_REQUIRE(C > 0 && ldx % 4 == 0 && ldx >= ((C + 3) / 4) * 4, "predict_maps: need ldx %% 4 == 0, ldx >= pad4(C)");
    ISWM_REQUIRE(fg >= 0 && fg < C, "predict_maps: foreground class %d outside [0, %d)", fg, C);
    ISWM_REQUIRE(aligned16(yl) && aligned16(pred) && aligned16(conf) && aligned16(band) && (!prob || aligned16(prob)),
                 "predict_maps: pointers must be 16-byte aligned");
    const int blocks = predict_blocks_per_image(N, Ho, Wo);
    ISWM_REQUIRE(workspace_bytes >= (size_t)N * blocks * sizeof(PredictPartial),
                 "predict_maps: workspace too small (see iswm_predict_maps_workspace)");
    const dim3 grid(blocks, N);
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
    PredictPartial* part = (PredictPartial*)workspace;
    const int groups = (C + 3) / 4;
#define ISWM_PM(G)                                                                                                   \
    hipLaunchKernelGGL(k_predict_maps<G>, grid, dim3(PM_BLOCK), 0, (hipStream_t)stream, yl, Hi, Wi, ldx, C, fg, Ho, \
                       Wo, sh, sw, thr, band_lo, band_hi, pred, conf, band, prob, part)
    switch (groups > PM_MAX_GROUPS ? 0 : groups) {
        case 1: ISWM_PM(1); break;
        case 2: ISWM_PM(2); break;
        case 3: ISWM_PM(3); break;
        case 4: ISWM_PM(4); break;
        default: ISWM_PM(0); break;
    }
#undef ISWM_PM
    int rc = check_launch("predict_maps");
    if (rc) return rc;
    return launch_predict_stats(part, blocks, N, stats, (hipStream_t)stream);
}

extern "C" int iswm_scene_plan_make(int H, int W, int tile, int overlap, iswm_scene_plan* out) {
    ISWM_REQUIRE(out, "scene_plan_make: null pointer");
    ISWM_REQUIRE(H >= 1 && W >= 1, "scene_plan_make: bad scene size %d x %d", H, W);
    ISWM_REQUIRE(tile >= 1, "scene_plan_make: tile %d (overlap %d) must be at least 1", tile, overlap);
    ISWM_REQUIRE(overlap >= 0 && overlap <= 1024, "scene_plan_make: overlap %d (tile %d) outside [0, 1024]", overlap,
                 tile);
    iswm_scene_plan p;
    p.H = H;
    p.W = W;
    ISWM_REQUIRE(scene_plan_axis(H, tile, overlap, &p.th, &p.sy, &p.nty),
                 "scene_plan_make: overlap %d exceeds half of the %d-pixel window (height %d)", overlap, p.th, H);
    ISWM_REQUIRE(scene_plan_axis(W, tile, overlap, &p.tw, &p.sx, &p.ntx),
                 "scene_plan_make: overlap %d exceeds half of the %d-pixel window (width %d)", overlap, p.tw, W);
    ISWM_REQUIRE((int64_t)p.nty * p.ntx <= 0x7fffffff, "scene_plan_make: %d x %d windows are too many", p.nty, p.ntx);
    p.ramp = overlap > 1 ? overlap : 1;
    *out = p;
    return 0;
}

extern "C" int iswm_scene_tiles_normalize(const unsigned char* scene, const iswm_scene_plan* plan, int first_tile,
                                          int count, const float* mean3, const float* std3, float* out_nchw,
                                          iswm_stream_t stream) {
    ISWM_REQUIRE(scene && plan && mean3 && std3 && out_nchw, "scene_tiles_normalize: null pointer");
    ISWM_REQUIRE(scene_plan_ok(*plan), "scene_tiles_normalize: inconsistent plan (see iswm_scene_plan_make)");
    ISWM_REQUIRE(first_tile >= 0 && count >= 1 && (int64_t)first_tile + count <= (int64_t)plan->nty * plan->ntx,
                 "scene_tiles_normalize: tiles [%d, %d + %d) outside the plan's %d x %d", first_tile, first_tile, count,
                 plan->nty, plan->ntx);
    const int64_t M = (int64_t)count * plan->th * plan->tw;
    hipLaunchKernelGGL(k_scene_tiles_normalize, dim3(stream_grid(M, 256)), dim3(256), 0, (hipStream_t)stream, scene,
                       *plan, first_tile, count, mean3[0], mean3[1], mean3[2], std3[0], std3[1], std3[2], out_nchw);
    return check_launch("scene_tiles_normalize");
}

extern "C" size_t iswm_scene_maps_workspace(int H, int W) { return iswm_predict_maps_workspace(1, H, W); }

extern "C" int iswm_scene_maps(const float* yl, const iswm_scene_plan* plan, int Hi, int Wi, int ldx, int C, int fg,
                               float thr, int band_lo, int band_hi, unsigned char* pred, unsigned char* conf,
                               unsigned char* band, float* prob, double* stats, void* workspace,
                               size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(yl && plan && pred && conf && band && stats && workspace, "scene_maps: null pointer");
    ISWM_REQUIRE(scene_plan_ok(*plan), "scene_maps: inconsistent plan (see iswm_scene_plan_make)");
    ISWM_REQUIRE(Hi > 0 && Wi > 0, "scene_maps: bad size");
    ISWM_REQUIRE(C > 0 && ldx % 4 == 0 && ldx >= ((C + 3) / 4) * 4, "scene_maps: need ldx %% 4 == 0, ldx >= pad4(C)");
    ISWM_REQUIRE(fg >= 0 && fg < C, "scene_maps: foreground class %d outside [0, %d)", fg, C);
    ISWM_REQUIRE(aligned16(yl) && aligned16(pred) && aligned16(conf) && aligned16(band) && (!prob || aligned16(prob)),
                 "scene_maps: pointers must be 16-byte aligned");
    const int blocks = predict_blocks_per_image(1, plan->H, plan->W);
    ISWM_REQUIRE(workspace_bytes >= (size_t)blocks * sizeof(PredictPartial),
                 "scene_maps: workspace too small (see iswm_scene_maps_workspace)");
    // a scene of one window is predict_maps itself: run that kernel, so the bytes are its own for every class count
    // (k_scene_maps samples with the same source, but the compiler contracts bilerp4's a * b + c * d per inlining
    // site, and for 5 <= C <= 16 the two kernels differ in the last bits of p)
    if (plan->nty == 1 && plan->ntx == 1)
        return iswm_predict_maps(yl, 1, Hi, Wi, ldx, C, fg, plan->H, plan->W, thr, band_lo, band_hi, pred, conf, band,
                                 prob, stats, workspace, workspace_bytes, stream);
    const float sh = (float)Hi / (float)plan->th, sw = (float)Wi / (float)plan->tw;
    PredictPartial* part = (PredictPartial*)workspace;
    const int groups = (C + 3) / 4;
#define ISWM_SM(G)                                                                                                   \
    hipLaunchKernelGGL(k_scene_maps<G>, dim3(blocks), dim3(PM_BLOCK), 0, (hipStream_t)stream, yl, *plan, Hi, Wi, ldx, \
                       C, fg, sh, sw, thr, band_lo, band_hi, pred, conf, band, prob, part)
    switch (groups > PM_MAX_GROUPS ? 0 : groups) {
        case 1: ISWM_SM(1); break;
        case 2: ISWM_SM(2); break;
        case 3: ISWM_SM(3); break;
        case 4: ISWM_SM(4); break;
        default: ISWM_SM(0); break;
    }
#undef ISWM_SM
    int rc = check_launch("scene_maps");
    if (rc) return rc;
    return launch_predict_stats(part, blocks, 1, stats, (hipStream_t)stream);
}

extern "C" int iswm_predict_view_normalize(const unsigned char* img, int N, int H, int W, int Hv, int Wv, int flip,
                                           const float* mean3, const float* std3, float* out_nchw,
                                           iswm_stream_t stream) {
    ISWM_REQUIRE(img && mean3 && std3 && out_nchw, "predict_view_normalize: null pointer");
    ISWM_REQUIRE(N > 0 && H > 0 && W > 0, "predict_view_normalize: bad size");
    ISWM_REQUIRE(Hv > 0 && Wv > 0, "predict_view_normalize: bad view size %d x %d", Hv, Wv);
    ISWM_REQUIRE(flip == 0 || flip == 1, "predict_view_normalize: flip %d is neither 0 nor 1", flip);
    const float sh = (float)H / (float)Hv, sw = (float)W / (float)Wv;
    hipLaunchKernelGGL(k_predict_view_normalize, dim3(stream_grid((int64_t)N * Hv * Wv, 256)), dim3(256), 0,
                       (hipStream_t)stream, img, N, H, W, Hv, Wv, flip, sh, sw, mean3[0], mean3[1], mean3[2], std3[0],
                       std3[1], std3[2], out_nchw);
    return check_launch("predict_view_normalize");
}

extern "C" size_t iswm_predict_views_maps_workspace(int N, int H, int W) {
    return iswm_predict_maps_workspace(N, H, W);
}

extern "C" int iswm_predict_views_maps(const iswm_predict_view* views, int nviews, int N, int ldx, int C, int fg,
                                       int Ho, int Wo, float thr, int band_lo, int band_hi, unsigned char* pred,
                                       unsigned char* conf, unsigned char* band, float* prob, double* stats,
                                       void* workspace, size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(views && pred && conf && band && stats && workspace, "predict_views_maps: null pointer");
    ISWM_REQUIRE(nviews >= 1 && nviews <= ISWM_PREDICT_MAX_VIEWS, "predict_views_maps: %d views outside [1, %d]",
                 nviews, ISWM_PREDICT_MAX_VIEWS);
    ISWM_REQUIRE(N > 0 && N <= 65535 && Ho > 0 && Wo > 0, "predict_views_maps: bad size");
    ISWM_REQUIRE(C > 0 && ldx % 4 == 0 && ldx >= ((C + 3) / 4) * 4,
                 "predict_views_maps: need ldx %% 4 == 0, ldx >= pad4(C)");
    ISWM_REQUIRE(fg >= 0 && fg < C, "predict_views_maps: foreground class %d outside [0, %d)", fg, C);
    ISWM_REQUIRE(aligned16(pred) && aligned16(conf) && aligned16(band) && (!prob || aligned16(prob)),
                 "predict_views_maps: pointers must be 16-byte aligned");
    PredictViewList vl = {};
    for (int v = 0; v < nviews; ++v) {
        ISWM_REQUIRE(views[v].yl, "predict_views_maps: view %d has no logits (null pointer)", v);
        ISWM_REQUIRE(aligned16(views[v].yl), "predict_views_maps: the logits of view %d must be 16-byte aligned", v);
        ISWM_REQUIRE(views[v].Hi > 0 && views[v].Wi > 0, "predict_views_maps: view %d has bad size %d x %d", v,
                     views[v].Hi, views[v].Wi);
        ISWM_REQUIRE(views[v].flip == 0 || views[v].flip == 1, "predict_views_maps: view %d has flip %d, neither 0 nor 1",
                     v, views[v].flip);
        vl.v[v] = PredictViewArg{views[v].yl, views[v].Hi, views[v].Wi, views[v].flip,
                                 (float)views[v].Hi / (float)Ho, (float)views[v].Wi / (float)Wo};
    }
    // one unflipped view is predict_maps itself: run that kernel, so the bytes are its own for every class count (the
    // compiler contracts bilerp4 per inlining site; iswm_scene_maps does the same for a one-window plan)
    if (nviews == 1 && !views[0].flip)
        return iswm_predict_maps(views[0].yl, N, views[0].Hi, views[0].Wi, ldx, C, fg, Ho, Wo, thr, band_lo, band_hi,
                                 pred, conf, band, prob, stats, workspace, workspace_bytes, stream);
    const int blocks = predict_blocks_per_image(N, Ho, Wo);
    ISWM_REQUIRE(workspace_bytes >= (size_t)N * blocks * sizeof(PredictPartial),
                 "predict_views_maps: workspace too small (see iswm_predict_views_maps_workspace)");
    const dim3 grid(blocks, N);
    PredictPartial* part = (PredictPartial*)workspace;
    const int groups = (C + 3) / 4;
#define ISWM_VM(G)                                                                                                  \
    hipLaunchKernelGGL(k_predict_views_maps<G>, grid, dim3(PM_BLOCK), 0, (hipStream_t)stream, vl, nviews, ldx, C, \
                       fg, Ho, Wo, thr, band_lo, band_hi, pred, conf, band, prob, part)
    switch (groups > PM_MAX_GROUPS ? 0 : groups) {
        case 1: ISWM_VM(1); break;
        case 2: ISWM_VM(2); break;
        case 3: ISWM_VM(3); break;
        case 4: ISWM_VM(4); break;
        default: ISWM_VM(0); break;
    }
#undef ISWM_VM
    int rc = check_launch("predict_views_maps");
    if (rc) return rc;
    return launch_predict_stats(part, blocks, N, stats, (hipStream_t)stream);
}
