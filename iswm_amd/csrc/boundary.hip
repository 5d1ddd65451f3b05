// The signed squared Euclidean distance map of a label tensor and the boundary (distance-map) criterion of Kervadec et al. on
// it, next to the weighted CE (include/iswm_hip_bd.h).
//
// ---- the map: exact in integers, two launches, 4 B of workspace per pixel and class plane
//   plane (n, c), c in K = {first .. C-1}:  F = {valid, y == c}   G = {valid, y != c}   invalid pixels in neither
//   k_edt_columns   one thread per (plane, column): a sweep down writes the vertical distance to the nearest F pixel and to the
//                   nearest G pixel at or above the row, a sweep up takes the minimum with the nearest at or below; two 16-bit
//                   fields of one word, EDT_NONE = nothing of that set in the column.  Rows go in batches of EDT_BATCH loads
//                   issued before they are used: the sweep is a chain of H dependent steps per thread and has few threads
//                   (B |K| W), so the loads of a batch are put in flight together.
//   k_edt_rows      one workgroup per (plane, row): both fields squared into LDS (8 B x W: 32 KiB at W = 4096), then each thread
//                   takes min over x' of (x - x')^2 + g^2(x') from the array OPPOSITE to its own membership, searching outward
//                   from x and stopping once dx^2 >= best (every later candidate is at least dx^2).  A pixel whose own field is
//                   0 is a member of that set; a pixel with neither field 0 is invalid -> 0.  No member of the opposite set in
//                   the whole plane leaves best at EDT_INF -> 0, which is the empty-F / empty-G rule.
//   (x - x')^2 + g^2 <= 2 * 4095^2 < 2^25 and EDT_INF + 4095^2 < 2^31: no overflow in 32 bits at sides up to 4096.
//
// ---- the criterion: two passes, nothing stored per pixel besides sd2
//   phi = sqrtf(sd2) (sd2 > 0), -(sqrtf(-sd2) - 1) (sd2 < 0), 0 elsewhere; clamped to [-clip, clip] if clip > 0
//   L = lce sum_V w nll / sum_V w + lbd sum_V sum_{c in K} p_ic phi_ic / (N |K|)
//   dL/dz_ik = lce w_y (p_ik - g_ik) / sum_V w + lbd / (N |K|) p_ik ([k in K] phi_ik - sum_{c in K} p_ic phi_ic) on V, else 0
//   k_boundary_sums     reads logits, labels and sd2, writes per-block partials of {sum w nll, sum w, sum p phi, N}
//   k_overlap_finalize  loss.hip's, one wave per value: partials -> sums[4] in double, fixed order
//   k_boundary_coeffs   sums -> out = {L, CE term, boundary term} (fp32) and coef = {lce / sum w, lbd / (N |K|)}, in double
//   k_boundary_bwd      reads logits, labels and sd2 again, recomputes the softmax, writes the finished gradient once
// Under data parallelism the host all-reduces sums between finalize and coeffs: sum w and N are then the global batch's.
// Per pixel at C = 2, uint8 labels, |K| = 1: 13 B read + (13 B read + 8 B written) = 34 B, plus the map's 4 B written once.
// The CE partials: gather_pixels, loss_pixel and block_reduce as in k_loss_fwd, so sums[0..1] are iswm_loss_fwd's mode-0 sums
// bit for bit.  N rides along as a float and is exact (the argument of distill.hip: B * HW <= 2^36).
#include "loss_common.h"      // log_softmax, softmax_stats, loss_pixel, gather_pixels, block_reduce, by_label_and_classes, refuse_pixel_args
#include "../../include/iswm_hip_bd.h"

namespace iswm {

constexpr int EDT_MAX_SIDE = 4096;
constexpr uint32_t EDT_NONE = 0xFFFFu;          // a 16-bit field: no pixel of the set in this column
constexpr uint32_t EDT_INF = 1u << 30;          // a squared field in LDS: the same
constexpr int EDT_BATCH = 8;

template <typename LabelT>
__global__ __launch_bounds__(256) void k_edt_columns(const LabelT* __restrict__ labels, int C, int H, int W, int K, int first,
                                                     int ignore_index, int64_t ncols, uint32_t* __restrict__ ws) {
    const int64_t col = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    const int64_t plane = col / W;
    const int x = (int)(col - plane * W);
    const int64_t b = plane / K;
    const int c = first + (int)(plane - b * K);
    const LabelT* lp = labels + b * H * W + x;
    uint32_t* wp = ws + plane * H * W + x;
    int lastF = -1, lastG = -1;
    for (int y0 = 0; y0 < H; y0 += EDT_BATCH) {
        long long yv[EDT_BATCH];
#pragma unroll
        for (int u = 0; u < EDT_BATCH; ++u) yv[u] = y0 + u < H ? (long long)lp[(int64_t)(y0 + u) * W] : (long long)ignore_index;
#pragma unroll
        for (int u = 0; u < EDT_BATCH; ++u) {
            const int y = y0 + u;
            if (y >= H) break;
            const bool valid = valid_label(yv[u], C, ignore_index);
            if (valid && yv[u] == c) lastF = y;
            if (valid && yv[u] != c) lastG = y;
            const uint32_t dF = lastF < 0 ? EDT_NONE : (uint32_t)(y - lastF), dG = lastG < 0 ? EDT_NONE : (uint32_t)(y - lastG);
            wp[(int64_t)y * W] = dF | (dG << 16);
        }
    }
    int nextF = -1, nextG = -1;
    for (int y0 = H - 1; y0 >= 0; y0 -= EDT_BATCH) {
        uint32_t v[EDT_BATCH];
#pragma unroll
        for (int u = 0; u < EDT_BATCH; ++u) v[u] = y0 - u >= 0 ? wp[(int64_t)(y0 - u) * W] : 0u;
#pragma unroll
        for (int u = 0; u < EDT_BATCH; ++u) {
            const int y = y0 - u;
            if (y < 0) break;
            uint32_t dF = v[u] & 0xFFFFu, dG = v[u] >> 16;
            if (dF == 0u) nextF = y;
            if (dG == 0u) nextG = y;
            const uint32_t uF = nextF < 0 ? EDT_NONE : (uint32_t)(nextF - y), uG = nextG < 0 ? EDT_NONE : (uint32_t)(nextG - y);
            dF = uF < dF ? uF : dF;
            dG = uG < dG ? uG : dG;
            wp[(int64_t)y * W] = dF | (dG << 16);
        }
    }
}

__global__ __launch_bounds__(256) void k_edt_rows(const uint32_t* __restrict__ ws, int W, int32_t* __restrict__ sd2) {
    extern __shared__ uint32_t sq[];            // [0, W): squared distance to F down the column, [W, 2W): to G
    const int64_t base = (int64_t)blockIdx.x * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const uint32_t v = ws[base + x], dF = v & 0xFFFFu, dG = v >> 16;
        sq[x] = dF == EDT_NONE ? EDT_INF : dF * dF;
        sq[W + x] = dG == EDT_NONE ? EDT_INF : dG * dG;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const bool inF = sq[x] == 0u, inG = sq[W + x] == 0u;
        int32_t out = 0;
        if (inF || inG) {
            const uint32_t* a = inF ? sq + W : sq;
            uint32_t best = a[x];
            const int far = x > W - 1 - x ? x : W - 1 - x;
            for (int d = 1; d <= far; ++d) {
                const uint32_t dd = (uint32_t)d * (uint32_t)d;
                if (dd >= best) break;
                if (x - d >= 0) {
                    const uint32_t t = dd + a[x - d];
                    best = t < best ? t : best;
                }
                if (x + d < W) {
                    const uint32_t t = dd + a[x + d];
                    best = t < best ? t : best;
                }
            }
            out = best >= EDT_INF ? 0 : (inF ? -(int32_t)best : (int32_t)best);
        }
        sd2[base + x] = out;
    }
}

// the distance a pixel's probability is weighted by, from its signed squared distance
__device__ __forceinline__ float boundary_phi(int32_t sd2, float clip) {
    float phi = 0.f;
    if (sd2 > 0) phi = sqrtf((float)sd2);
    if (sd2 < 0) phi = -(sqrtf((float)(-sd2)) - 1.f);
    if (clip > 0.f) phi = fminf(fmaxf(phi, -clip), clip);
    return phi;
}

constexpr int BD_SUMS = 4;

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_boundary_sums(const float* __restrict__ logits, const LabelT* __restrict__ labels,
                                                       const int32_t* __restrict__ sd2, int Crt, int first, int64_t HW,
                                                       int64_t npix, const float* __restrict__ cw, int ignore_index, float clip,
                                                       float* __restrict__ partials, int nblocks) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const int K = C - first;
    __shared__ float red[BD_SUMS][4];
    float s1 = 0.f, s2 = 0.f, sbd = 0.f, sn = 0.f;
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
            sn += 1.f;
            const int64_t i = i0 + u * stride, b = i / HW, p = i - b * HW;
            const int32_t* dp = sd2 + b * K * HW + p;
            float dot = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C && c >= first) dot += expf(log_softmax(z[u][c], m, lg)) * boundary_phi(dp[(int64_t)(c - first) * HW], clip);
            sbd += dot;
        }
    }
    float s[BD_SUMS] = {s1, s2, sbd, sn};
    block_reduce(s, red);
    const int v = threadIdx.x;
    if (v < BD_SUMS) partials[(int64_t)v * nblocks + blockIdx.x] = block_total(red[v]);
}

// loss.hip's: block v, one wave, adds the partials of value v in double in k_loss_finalize's order (the two CE sums come out as
// iswm_loss_fwd forms them); launched from here on the host, defined there
__global__ __launch_bounds__(64) void k_overlap_finalize(const float* __restrict__ partials, int blocks, double* __restrict__ sums);

// one thread, double.  lce == 0 leaves the CE term out altogether (finite without a valid pixel); N == 0 makes the boundary
// term and its coefficient exactly 0.
__global__ void k_boundary_coeffs(const double* __restrict__ sums, int nsel, double lce, double lbd, float* __restrict__ out,
                                  float* __restrict__ coef) {
    const double n = sums[3];
    const double ce = lce != 0.0 ? lce * (sums[0] / sums[1]) : 0.0;
    const double bd = n > 0.0 ? lbd * sums[2] / (n * nsel) : 0.0;
    out[0] = (float)(ce + bd);
    out[1] = (float)ce;
    out[2] = (float)bd;
    coef[0] = lce != 0.0 ? (float)(lce / sums[1]) : 0.f;
    coef[1] = n > 0.0 ? (float)(lbd / (n * nsel)) : 0.f;
}

// for valid i:  dL/dz_ik = upstream [ coef[0] w_y (p_ik - g_ik) + coef[1] p_ik ([k in K] phi_ik - sum_{c in K} p_ic phi_ic) ];  else 0
template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_boundary_bwd(const float* __restrict__ logits, const LabelT* __restrict__ labels,
                                                      const int32_t* __restrict__ sd2, int Crt, int first, int64_t HW,
                                                      int64_t npix, const float* __restrict__ cw, int ignore_index, float clip,
                                                      const float* __restrict__ coef, const float* __restrict__ upstream,
                                                      float* __restrict__ grad) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const int K = C - first;
    const float up = upstream[0], a = coef[0], bk = coef[1];
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
            float m, lg;
            softmax_stats(z[u], C, m, lg);
            const int64_t i = i0 + u * stride, b = i / HW, p = i - b * HW;
            const int32_t* dp = sd2 + b * K * HW + p;
            float pc[CMAX], phi[CMAX], dot = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                pc[c] = phi[c] = 0.f;
                if (c < C) {
                    pc[c] = expf(log_softmax(z[u][c], m, lg));
                    if (valid && c >= first) {
                        phi[c] = boundary_phi(dp[(int64_t)(c - first) * HW], clip);
                        dot += pc[c] * phi[c];
                    }
                }
            }
            const float aw = valid ? a * (cw ? cw[yy] : 1.f) : 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float g = c == (int)yy ? 1.f : 0.f;
                    const float t = c >= first ? phi[c] - dot : -dot;
                    grad[off[u] + c * HW] = valid ? up * (aw * (pc[c] - g) + bk * (pc[c] * t)) : 0.f;
                }
        }
    }
}

}  // namespace iswm

using namespace iswm;

static const char* const BOUNDARY_TAKES = "the boundary loss takes";

static bool boundary_shape(int B, int64_t HW) { return B > 0 && HW > 0 && (int64_t)B * HW <= ((int64_t)1 << 36); }

static bool edt_shape(int B, int C, int H, int W, int first_class) {
    return B > 0 && C > 0 && H > 0 && W > 0 && H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE && (first_class == 0 || first_class == 1) &&
           C - first_class >= 1 && (int64_t)B * (C - first_class) * H < ((int64_t)1 << 31) &&
           (int64_t)B * (C - first_class) * W < ((int64_t)1 << 31) * 256;
}

extern "C" int64_t iswm_signed_edt_workspace(int B, int C, int H, int W, int first_class) {
    if (!edt_shape(B, C, H, W, first_class)) return -1;
    return (int64_t)B * (C - first_class) * H * W * (int64_t)sizeof(uint32_t);
}

extern "C" int iswm_signed_edt(const void* labels, int label_bytes, int B, int C, int H, int W, int first_class, int ignore_index,
                               int32_t* sd2, void* workspace, int64_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(labels && sd2 && workspace, "signed_edt: null pointer");
    ISWM_REQUIRE(H <= EDT_MAX_SIDE && W <= EDT_MAX_SIDE, "signed_edt: a %d x %d plane (the distance map takes sides up to %d)", H, W,
                 EDT_MAX_SIDE);
    ISWM_REQUIRE(first_class == 0 || first_class == 1, "signed_edt: first_class is 0 (every class) or 1 (the foreground classes)");
    ISWM_REQUIRE(C - first_class >= 1, "signed_edt: %d classes from class %d on leave no class plane", C, first_class);
    ISWM_REQUIRE(edt_shape(B, C, H, W, first_class), "signed_edt: bad shape");
    ISWM_REQUIRE(label_bytes == 1 || label_bytes == 8, "signed_edt: labels must be uint8 or int64");
    ISWM_REQUIRE(workspace_bytes >= iswm_signed_edt_workspace(B, C, H, W, first_class), "signed_edt: workspace too small");
    const int K = C - first_class;
    const int64_t ncols = (int64_t)B * K * W, nrows = (int64_t)B * K * H;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* ws = (uint32_t*)workspace;
    if (label_bytes == 1)
        hipLaunchKernelGGL((k_edt_columns<uint8_t>), dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, (const uint8_t*)labels, C,
                           H, W, K, first_class, ignore_index, ncols, ws);
    else
        hipLaunchKernelGGL((k_edt_columns<int64_t>), dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, (const int64_t*)labels, C,
                           H, W, K, first_class, ignore_index, ncols, ws);
    hipLaunchKernelGGL(k_edt_rows, dim3((unsigned)nrows), dim3(256), 2 * W * sizeof(uint32_t), s, ws, W, sd2);
    return check_launch("signed_edt");
}

static int refuse_boundary_args(const char* fn, int C, int first_class, const void* sd2, float clip) {
    ISWM_REQUIRE(sd2, "%s: distance map pointer null", fn);
    ISWM_REQUIRE(first_class == 0 || first_class == 1, "%s: first_class is 0 (every class) or 1 (the foreground classes)", fn);
    ISWM_REQUIRE(C - first_class >= 1, "%s: %d classes from class %d on leave no class plane", fn, C, first_class);
    ISWM_REQUIRE(clip >= 0.f && clip < INFINITY, "%s: the clip distance must be finite and not negative (0: no clamp)", fn);
    return 0;
}

extern "C" int64_t iswm_boundary_loss_partials(int64_t npix) { return (int64_t)BD_SUMS * iswm_loss_blocks(npix); }

extern "C" int iswm_boundary_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                                      int first_class, const int32_t* sd2, const float* class_weight, int ignore_index, float clip,
                                      float* partials, double* sums, iswm_stream_t stream) {
    if (refuse_pixel_args("boundary_loss_fwd", logits && labels && partials && sums, boundary_shape(B, HW), C, BOUNDARY_TAKES,
                          label_bytes)) return 1;
    if (refuse_boundary_args("boundary_loss_fwd", C, first_class, sd2, clip)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_boundary_sums<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, sd2,
                           C, first_class, HW, npix, class_weight, ignore_index, clip, partials, blocks);
    });
    hipLaunchKernelGGL(k_overlap_finalize, dim3(BD_SUMS), dim3(64), 0, s, partials, blocks, sums);
    return check_launch("boundary_loss_fwd");
}

extern "C" int iswm_boundary_loss_coeffs(const double* sums, int nsel, double ce_weight, double boundary_weight, float* out,
                                         float* coef, iswm_stream_t stream) {
    ISWM_REQUIRE(sums && out && coef, "boundary_loss_coeffs: null pointer");
    ISWM_REQUIRE(nsel >= 1 && nsel <= OVL_CMAX, "boundary_loss_coeffs: %d selected classes (1 to %d)", nsel, OVL_CMAX);
    ISWM_REQUIRE(ce_weight >= 0.0 && boundary_weight >= 0.0 && ce_weight < INFINITY && boundary_weight < INFINITY,
                 "boundary_loss_coeffs: the term weights must be finite and not negative");
    hipLaunchKernelGGL(k_boundary_coeffs, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, nsel, ce_weight, boundary_weight, out,
                       coef);
    return check_launch("boundary_loss_coeffs");
}

extern "C" int iswm_boundary_loss_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                                      int first_class, const int32_t* sd2, const float* class_weight, int ignore_index, float clip,
                                      const float* coef, const float* upstream, float* grad, iswm_stream_t stream) {
    if (refuse_pixel_args("boundary_loss_bwd", logits && labels && coef && upstream && grad, boundary_shape(B, HW), C,
                          BOUNDARY_TAKES, label_bytes)) return 1;
    if (refuse_boundary_args("boundary_loss_bwd", C, first_class, sd2, clip)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_boundary_bwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, sd2,
                           C, first_class, HW, npix, class_weight, ignore_index, clip, coef, upstream, grad);
    });
    return check_launch("boundary_loss_bwd");
}
