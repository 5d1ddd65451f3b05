// Local dense-CRF refinement of the foreground probability on the frame itself (include/iswm_hip_cr.h): the
// mean-field update of a two-label Potts model over a dilated (2R+1)^2 window (ConvCRF), kernel weights recomputed on the fly.
//
//   k_crf_iter<FIRST>  one launch per iteration, one workgroup of 256 threads per 32 x 32 output tile of one image.  The tile plus
//                      a halo of R*D pixels is staged in LDS as 8-byte cells {s = 2q - 1 (fp32), colour (B << 16 | G << 8 | R)}: at
//                      R*D = 28 that is 88^2 x 8 B = 61 952 B.  A cell outside the image carries s = 0 and CRF_OUTSIDE in the byte
//                      above the colour, which no pixel has (a valid neighbour may be black, so no colour can say it), and gets
//                      weight 0 in both kernels.  A thread owns the four pixels (ty + 8k, tx) of the tile; a wave's 64 lanes read
//                      two rows of 32 consecutive cells with one ds_read_b64 each -- all 64 banks once per half wave, no conflict.
//                      Per neighbour: one cell read, dI^2 as an exact integer from two v_dot4_u32_u8 (|ci|^2 + |cj|^2 - 2 ci.cj;
//                      the marker byte only reaches |cj|^2 of a cell that is masked anyway), one v_exp_f32 for the colour factor,
//                      the two spatial factors from tables in the kernel arguments (the index is the same in every lane: scalar
//                      loads), and four accumulators per pixel.  The sums run row-major over the window in every thread, no
//                      atomics: the same bits every run.
//                      FIRST reads the probability itself (clamped to [1e-6, 1 - 1e-6]) and writes the unary plane
//                      u = log p - log(1 - p); the later iterations read q and u.
//                      The norms Nb, Ns are recomputed every iteration: kb has to be formed again anyway (its exponential is the
//                      cost), the norm is one more add per kernel value, and keeping them would cost 8 B per pixel of workspace
//                      and of traffic per iteration and a first iteration unlike the others.
//   k_prob_maps        an fp32 [N,H,W] probability -> pred / conf / band / stats with k_predict_maps's chunks, tail and workgroup
//                      sum (predict_tail.h) and k_predict_stats itself: fed the prob that iswm_predict_maps wrote, the bytes are
//                      that call's, statistics included.
#include <math.h>

#include "predict_tail.h"
#include "../../include/iswm_hip_cr.h"

namespace iswm {

constexpr int CRF_TILE = 32;
constexpr int CRF_ROWS = 4;                       // pixels per thread: rows ty, ty + 8, ty + 16, ty + 24 of the tile
constexpr int CRF_MAX_RADIUS = 7, CRF_MAX_STEP = 4, CRF_MAX_ITERS = 20, CRF_MAX_SIDE = 8192;
constexpr uint32_t CRF_OUTSIDE = 0xFF000000u;     // a cell outside the image
constexpr float CRF_TINY = 1e-20f;                // a message whose norm is below this is 0

struct CrfTables {                                // exp(-(dy^2 + dx^2) D^2 / (2 theta^2)) at [|dy| * 8 + |dx|]
    float b[64];                                  // theta_alpha: the bilateral kernel's spatial factor
    float s[64];                                  // theta_gamma: the spatial kernel
};

__device__ __forceinline__ float crf_clamp(float p) { return fminf(fmaxf(p, 1e-6f), (float)(1.0 - 1e-6)); }

template <bool FIRST>
__global__ __launch_bounds__(256) void k_crf_iter(const float* __restrict__ src, const unsigned char* __restrict__ img,
                                                  float* __restrict__ unary, float* __restrict__ dst, int H, int W, int R, int D,
                                                  float w_b, float w_s, float cb, CrfTables tab) {
    extern __shared__ uint2 cell[];               // .x = the bits of s, .y = the colour or CRF_OUTSIDE
    const int RD = R * D, WT = CRF_TILE + 2 * RD;
    const int x0 = blockIdx.x * CRF_TILE, y0 = blockIdx.y * CRF_TILE;
    const size_t plane = (size_t)blockIdx.z * H * W;

    for (int i = threadIdx.x; i < WT * WT; i += 256) {
        const int ly = i / WT, lx = i - ly * WT;
        const int gy = y0 - RD + ly, gx = x0 - RD + lx;
        uint2 c = make_uint2(0u, CRF_OUTSIDE);    // s = 0.0f
        if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
            const size_t g = plane + (size_t)gy * W + gx;
            float q = src[g];
            if (FIRST) q = crf_clamp(q);
            const unsigned char* px = img + g * 3;
            c.x = __float_as_uint(2.0f * q - 1.0f);
            c.y = (uint32_t)px[0] | ((uint32_t)px[1] << 8) | ((uint32_t)px[2] << 16);
        }
        cell[i] = c;
    }
    __syncthreads();

    const int tx = threadIdx.x & (CRF_TILE - 1), ty = threadIdx.x >> 5;
    int centre[CRF_ROWS];
    uint32_t ci[CRF_ROWS], nii[CRF_ROWS];
    float Sb[CRF_ROWS], Nb[CRF_ROWS], Ss[CRF_ROWS], Ns[CRF_ROWS];
#pragma unroll
    for (int k = 0; k < CRF_ROWS; ++k) {
        centre[k] = (ty + 8 * k + RD) * WT + tx + RD;
        ci[k] = cell[centre[k]].y & 0x00FFFFFFu;  // a pixel of the tile outside the image: computed, never stored
        nii[k] = __builtin_amdgcn_udot4(ci[k], ci[k], 0u, false);
        Sb[k] = Nb[k] = Ss[k] = Ns[k] = 0.f;
    }
    for (int dy = -R; dy <= R; ++dy) {
        for (int dx = -R; dx <= R; ++dx) {
            if (dy == 0 && dx == 0) continue;
            const int t = (dy < 0 ? -dy : dy) * 8 + (dx < 0 ? -dx : dx);
            const float tb = tab.b[t], ts = tab.s[t];
            const int off = dy * D * WT + dx * D;
            uint2 c4[CRF_ROWS];
#pragma unroll
            for (int k = 0; k < CRF_ROWS; ++k) c4[k] = cell[centre[k] + off];     // four reads in flight
#pragma unroll
            for (int k = 0; k < CRF_ROWS; ++k) {
                const uint2 c = c4[k];
                const bool inside = c.y < 0x01000000u;
                const uint32_t d2 = nii[k] + __builtin_amdgcn_udot4(c.y, c.y, 0u, false) -
                                    2u * __builtin_amdgcn_udot4(ci[k], c.y, 0u, false);
                // no branch: outside the image d2 is meaningless but the exponent stays <= 0, so the factor is finite and the
                // selected 0 makes the product 0
                const float kb = (inside ? tb : 0.f) * __builtin_amdgcn_exp2f((float)d2 * cb);
                const float ks = inside ? ts : 0.f;
                const float s = __uint_as_float(c.x);
                Sb[k] = fmaf(kb, s, Sb[k]);
                Nb[k] += kb;
                Ss[k] = fmaf(ks, s, Ss[k]);
                Ns[k] += ks;
            }
        }
    }

#pragma unroll
    for (int k = 0; k < CRF_ROWS; ++k) {
        const int y = y0 + ty + 8 * k, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const size_t g = plane + (size_t)y * W + x;
        float u;
        if (FIRST) {
            const float p = crf_clamp(src[g]);
            u = logf(p) - logf(1.0f - p);
            unary[g] = u;
        } else {
            u = unary[g];
        }
        const float m_b = Nb[k] < CRF_TINY ? 0.f : __fdiv_rn(Sb[k], Nb[k]);
        const float m_s = Ns[k] < CRF_TINY ? 0.f : __fdiv_rn(Ss[k], Ns[k]);
        const float z = u + w_b * m_b + w_s * m_s;
        dst[g] = __fdiv_rn(1.0f, 1.0f + expf(-z));
    }
}

// grid (blocks_per_image, N): k_predict_maps's walk over the 16-pixel chunks of the [N, H, W] tensor, with p read from the map
__global__ __launch_bounds__(PM_BLOCK) void k_prob_maps(const float* __restrict__ prob, int64_t HW, float thr, int lo, int hi,
                                                        unsigned char* __restrict__ pred, unsigned char* __restrict__ conf,
                                                        unsigned char* __restrict__ band,
                                                        PredictPartial* __restrict__ partials) {
    const int n = blockIdx.y;
    const int64_t p_begin = (int64_t)n * HW, p_end = p_begin + HW;
    const int64_t k_begin = p_begin / PM_PIX, k_end = (p_end + PM_PIX - 1) / PM_PIX;
    float* const no_prob = nullptr;               // the map is the input: nothing to write back

    ISWM_MAP_STATS_DECL;
    for (int64_t k = k_begin + (int64_t)blockIdx.x * PM_BLOCK + threadIdx.x; k < k_end;
         k += (int64_t)gridDim.x * PM_BLOCK) {
        const int64_t q0 = k * PM_PIX;
        const int j0 = q0 < p_begin ? (int)(p_begin - q0) : 0;
        const int j1 = q0 + PM_PIX > p_end ? (int)(p_end - q0) : PM_PIX;
        float in[PM_PIX];
        if (j0 == 0 && j1 == PM_PIX) {
#pragma unroll
            for (int j = 0; j < PM_PIX; j += 4) {
                const float4 v = *reinterpret_cast<const float4*>(prob + q0 + j);
                in[j] = v.x, in[j + 1] = v.y, in[j + 2] = v.z, in[j + 3] = v.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < PM_PIX; ++j) in[j] = (j < j0 || j >= j1) ? 0.f : prob[q0 + j];
        }
        ISWM_MAP_CHUNK_DECL;
#pragma unroll
        for (int j = 0; j < PM_PIX; ++j) {
            pv[j] = 0.f;
            if (j < j0 || j >= j1) continue;
            const float p = in[j];
            ISWM_MAP_PIXEL(j, p, thr, lo, hi);
        }
        ISWM_MAP_STORE(q0, j0, j1, pred, conf, band, no_prob);
    }
    ISWM_MAP_BLOCK_SUM(partials, (size_t)n * gridDim.x + blockIdx.x)
}

static bool crf_shape(int N, int H, int W) {
    return N >= 1 && N <= 65535 && H >= 1 && H <= CRF_MAX_SIDE && W >= 1 && W <= CRF_MAX_SIDE;
}

}  // namespace iswm

using namespace iswm;

extern "C" int64_t iswm_crf_refine_workspace(int N, int H, int W) {
    if (!crf_shape(N, H, W)) return -1;
    return 2 * (int64_t)N * H * W * (int64_t)sizeof(float);      // the unary plane and one plane of q
}

extern "C" int iswm_crf_refine(const float* prob, const unsigned char* img, int N, int H, int W, int radius, int step, int iters,
                               float w_bilateral, float w_spatial, float theta_alpha, float theta_beta, float theta_gamma,
                               float* out, void* workspace, int64_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(prob && img && out && workspace, "crf_refine: null pointer");
    ISWM_REQUIRE(crf_shape(N, H, W), "crf_refine: bad shape %d x %d x %d (1 <= N <= 65535, 1 <= H, W <= %d)", N, H, W,
                 CRF_MAX_SIDE);
    ISWM_REQUIRE(radius >= 1 && radius <= CRF_MAX_RADIUS, "crf_refine: radius %d outside [1, %d]", radius, CRF_MAX_RADIUS);
    ISWM_REQUIRE(step >= 1 && step <= CRF_MAX_STEP, "crf_refine: step %d outside [1, %d]", step, CRF_MAX_STEP);
    ISWM_REQUIRE(iters >= 1 && iters <= CRF_MAX_ITERS, "crf_refine: %d iterations outside [1, %d]", iters, CRF_MAX_ITERS);
    ISWM_REQUIRE(w_bilateral >= 0.f && w_spatial >= 0.f && isfinite(w_bilateral) && isfinite(w_spatial),
                 "crf_refine: the weights must be finite and not negative");
    ISWM_REQUIRE(theta_alpha > 0.f && theta_beta > 0.f && theta_gamma > 0.f && isfinite(theta_alpha) && isfinite(theta_beta) &&
                     isfinite(theta_gamma),
                 "crf_refine: theta_alpha, theta_beta and theta_gamma must be finite and positive");
    ISWM_REQUIRE(out != prob, "crf_refine: out may not alias prob");
    ISWM_REQUIRE(workspace_bytes >= iswm_crf_refine_workspace(N, H, W),
                 "crf_refine: workspace too small (see iswm_crf_refine_workspace)");

    CrfTables tab;
    for (int a = 0; a < 8; ++a)
        for (int b = 0; b < 8; ++b) {
            const double d2 = (double)(a * a + b * b) * step * step;
            tab.b[a * 8 + b] = (float)exp(-d2 / (2.0 * (double)theta_alpha * theta_alpha));
            tab.s[a * 8 + b] = (float)exp(-d2 / (2.0 * (double)theta_gamma * theta_gamma));
        }
    const float cb = (float)(-1.4426950408889634 / (2.0 * (double)theta_beta * theta_beta));     // exp(x) = exp2(x log2 e)

    const size_t npix = (size_t)N * H * W;
    float* unary = (float*)workspace;
    float* plane = unary + npix;
    const int side = CRF_TILE + 2 * radius * step;
    const size_t lds = (size_t)side * side * sizeof(uint2);
    const dim3 grid((W + CRF_TILE - 1) / CRF_TILE, (H + CRF_TILE - 1) / CRF_TILE, N);
    const float* src = prob;
    for (int i = 0; i < iters; ++i) {             // the last iteration writes out; the ones before alternate with the plane
        float* dst = (iters - 1 - i) % 2 == 0 ? out : plane;
        if (i == 0)
            hipLaunchKernelGGL(k_crf_iter<true>, grid, dim3(256), lds, (hipStream_t)stream, src, img, unary, dst, H, W, radius,
                               step, w_bilateral, w_spatial, cb, tab);
        else
            hipLaunchKernelGGL(k_crf_iter<false>, grid, dim3(256), lds, (hipStream_t)stream, src, img, unary, dst, H, W, radius,
                               step, w_bilateral, w_spatial, cb, tab);
        src = dst;
    }
    return check_launch("crf_refine");
}

extern "C" int64_t iswm_prob_maps_workspace(int N, int H, int W) {
    if (!crf_shape(N, H, W)) return -1;
    return (int64_t)N * predict_blocks_per_image(N, H, W) * (int64_t)sizeof(PredictPartial);
}

extern "C" int iswm_prob_maps(const float* prob, int N, int H, int W, float thr, int band_lo, int band_hi, unsigned char* pred,
                              unsigned char* conf, unsigned char* band, double* stats, void* workspace, int64_t workspace_bytes,
                              iswm_stream_t stream) {
    ISWM_REQUIRE(prob && pred && conf && band && stats && workspace, "prob_maps: null pointer");
    ISWM_REQUIRE(crf_shape(N, H, W), "prob_maps: bad shape %d x %d x %d (1 <= N <= 65535, 1 <= H, W <= %d)", N, H, W, CRF_MAX_SIDE);
    ISWM_REQUIRE(aligned16(prob) && aligned16(pred) && aligned16(conf) && aligned16(band),
                 "prob_maps: pointers must be 16-byte aligned");
    ISWM_REQUIRE(workspace_bytes >= iswm_prob_maps_workspace(N, H, W),
                 "prob_maps: workspace too small (see iswm_prob_maps_workspace)");
    const int blocks = predict_blocks_per_image(N, H, W);
    PredictPartial* part = (PredictPartial*)workspace;
    hipLaunchKernelGGL(k_prob_maps, dim3(blocks, N), dim3(PM_BLOCK), 0, (hipStream_t)stream, prob, (int64_t)H * W, thr, band_lo,
                       band_hi, pred, conf, band, part);
    int rc = check_launch("prob_maps");
    if (rc) return rc;
    return launch_predict_stats(part, blocks, N, stats, (hipStream_t)stream);
}
