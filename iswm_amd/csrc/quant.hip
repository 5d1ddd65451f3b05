// Memory-bound passes of the post-training quantized inference path (iswm_amd/quant.py):
//   * k_absmax + k_absmax_finalize: max |x| over the real channels of an fp32 NHWC or planes tensor (planes are
//     reconstructed with planes.h's own join); one partial per workgroup in a slab, then ONE workgroup folds the slab
//     into a device float with max (amax = max(amax, slab)), so calibration batches accumulate without a sync;
//   * k_quantize_i8: fp32 / planes -> int8 NHWC, q = clamp(rint(x * inv_s), lo, 127), padding channels 0;
//   * k_qgap: int8 global average pool, exact int32 sum, v = sum * s_in / HW, re-quantized with s_in;
//   * k_qbcast: int8 [N, C] broadcast into a channel slice of an [N, H, W, ld] buffer;
//   * k_qbilinear: int8 bilinear resize (bilinear.h's index and weight arithmetic) into a channel slice: the four
//     dequantized taps combined in fp64 in a fixed order, quantized with the destination scale.
// All fp64 arithmetic is uncontracted, so numpy float64 reproduces it bit for bit (tests/quant_ref.py).
#pragma clang fp contract(off)
#include "bilinear.h"
#include "planes.h"

namespace iswm {

constexpr int QB = 256;

__device__ __forceinline__ int q_round(double v, double inv_s, int lo) {
    double r = rint(v * inv_s);
    r = r < (double)lo ? (double)lo : r;
    r = r > 127.0 ? 127.0 : r;
    return (int)r;
}

__device__ __forceinline__ float block_max(float m) {
    __shared__ float red[QB / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) red[wave] = m;
    __syncthreads();
    float r = red[0];
#pragma unroll
    for (int w = 1; w < QB / 64; ++w) r = fmaxf(r, red[w]);
    return r;
}

__global__ __launch_bounds__(QB) void k_absmax(const void* __restrict__ x, int64_t ps, int64_t rows, int C, int ld,
                                               float* __restrict__ slab) {
    const int G = (C + 3) / 4;
    const int64_t total = rows * G;
    float m = 0.f;
    for (int64_t i = (int64_t)blockIdx.x * QB + threadIdx.x; i < total; i += (int64_t)gridDim.x * QB) {
        const int64_t r = i / G;
        const int g = (int)(i - r * G);
        const float4 v = ld4x(x, r * ld + 4 * g, ps);
        const int c = 4 * g;
        m = fmaxf(m, fabsf(v.x));
        if (c + 1 < C) m = fmaxf(m, fabsf(v.y));
        if (c + 2 < C) m = fmaxf(m, fabsf(v.z));
        if (c + 3 < C) m = fmaxf(m, fabsf(v.w));
    }
    m = block_max(m);
    if (threadIdx.x == 0) slab[blockIdx.x] = m;
}

__global__ __launch_bounds__(QB) void k_absmax_finalize(const float* __restrict__ slab, int n, float* __restrict__ amax) {
    float m = 0.f;
    for (int i = threadIdx.x; i < n; i += QB) m = fmaxf(m, slab[i]);
    m = block_max(m);
    if (threadIdx.x == 0) amax[0] = fmaxf(amax[0], m);
}

__global__ __launch_bounds__(QB) void k_quantize_i8(const void* __restrict__ x, int64_t ps, int64_t rows, int C, int ld,
                                                    double inv_s, int lo, int8_t* __restrict__ y, int ldy) {
    const int G = ldy / 4;
    const int64_t total = rows * G;
    for (int64_t i = (int64_t)blockIdx.x * QB + threadIdx.x; i < total; i += (int64_t)gridDim.x * QB) {
        const int64_t r = i / G;
        const int g = (int)(i - r * G), c = 4 * g;
        unsigned pk = 0;
        if (c < C) {
            const float4 v = ld4x(x, r * ld + c, ps);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (c + k < C) pk |= (unsigned)(q_round((double)e[k], inv_s, lo) & 0xFF) << (8 * k);
        }
        *reinterpret_cast<unsigned*>(y + r * ldy + c) = pk;
    }
}

// grid (ceil(C / 256), N): thread = channel; the pixels are summed in order (exact in int32: HW * 127 < 2^31)
__global__ __launch_bounds__(QB) void k_qgap(const int8_t* __restrict__ x, int HW, int C, int ldx, double s_in,
                                             double inv_s_in, int8_t* __restrict__ y, int ldy) {
    const int c = blockIdx.x * QB + threadIdx.x, n = blockIdx.y;
    if (c >= C) return;
    const int8_t* p = x + (size_t)n * HW * ldx + c;
    int s = 0;
    for (int i = 0; i < HW; ++i) s += p[(size_t)i * ldx];
    const double v = (double)s * s_in / (double)HW;
    y[(size_t)n * ldy + c] = (int8_t)q_round(v, inv_s_in, -127);
}

__global__ __launch_bounds__(QB) void k_qbcast(const int8_t* __restrict__ v, int N, int HW, int C, int ldv,
                                               int8_t* __restrict__ y, int ldy) {
    const int G = C / 4;
    const int64_t total = (int64_t)N * HW * G;
    for (int64_t i = (int64_t)blockIdx.x * QB + threadIdx.x; i < total; i += (int64_t)gridDim.x * QB) {
        const int64_t r = i / G;
        const int g = (int)(i - r * G);
        const int n = (int)(r / HW);
        *reinterpret_cast<unsigned*>(y + r * ldy + 4 * g) = *reinterpret_cast<const unsigned*>(v + (size_t)n * ldv + 4 * g);
    }
}

__global__ __launch_bounds__(QB) void k_qbilinear(const int8_t* __restrict__ x, int N, int Hi, int Wi, int C, int ldx,
                                                  double s_in, int Ho, int Wo, float sh, float sw, double inv_s_out,
                                                  int8_t* __restrict__ y, int ldy) {
    const int G = C / 4;
    const int64_t total = (int64_t)N * Ho * Wo * G;
    for (int64_t i = (int64_t)blockIdx.x * QB + threadIdx.x; i < total; i += (int64_t)gridDim.x * QB) {
        const int64_t r = i / G;
        const int g = (int)(i - r * G);
        const int n = (int)(r / ((int64_t)Ho * Wo));
        const int rem = (int)(r - (int64_t)n * Ho * Wo);
        const int oh = rem / Wo, ow = rem - oh * Wo;
        const Lerp lh = src_index(sh, oh, Hi), lw = src_index(sw, ow, Wi);
        const int8_t* base = x + (size_t)n * Hi * Wi * ldx + 4 * g;
        const unsigned ua = *reinterpret_cast<const unsigned*>(base + ((size_t)lh.i0 * Wi + lw.i0) * ldx);
        const unsigned ub = *reinterpret_cast<const unsigned*>(base + ((size_t)lh.i0 * Wi + lw.i1) * ldx);
        const unsigned ud = *reinterpret_cast<const unsigned*>(base + ((size_t)lh.i1 * Wi + lw.i0) * ldx);
        const unsigned ue = *reinterpret_cast<const unsigned*>(base + ((size_t)lh.i1 * Wi + lw.i1) * ldx);
        const double h0 = lh.l0, h1 = lh.l1, w0 = lw.l0, w1 = lw.l1;
        unsigned pk = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double a = (double)(int8_t)(ua >> (8 * k)) * s_in, b = (double)(int8_t)(ub >> (8 * k)) * s_in;
            const double dd = (double)(int8_t)(ud >> (8 * k)) * s_in, e = (double)(int8_t)(ue >> (8 * k)) * s_in;
            const double v = h0 * (w0 * a + w1 * b) + h1 * (w0 * dd + w1 * e);
            pk |= (unsigned)(q_round(v, inv_s_out, -127) & 0xFF) << (8 * k);
        }
        *reinterpret_cast<unsigned*>(y + r * ldy + 4 * g) = pk;
    }
}

static int absmax_blocks(int64_t rows, int C) { return stream_grid(rows * ((C + 3) / 4), QB); }

}  // namespace iswm

using namespace iswm;

static bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

extern "C" size_t iswm_absmax_workspace(int64_t rows, int C) {
    if (rows <= 0 || C <= 0) return 0;
    return (size_t)absmax_blocks(rows, C) * sizeof(float);
}

extern "C" int iswm_absmax(const void* x, int64_t ps, int64_t rows, int C, int ld, float* slab, size_t slab_bytes,
                           float* amax, iswm_stream_t stream) {
    ISWM_REQUIRE(x && slab && amax, "absmax: null pointer");
    ISWM_REQUIRE(rows > 0 && C > 0 && ld % 4 == 0 && ld >= (C + 3) / 4 * 4, "absmax: need rows, C > 0, ld %% 4 == 0, ld >= pad4(C)");
    const int nb = absmax_blocks(rows, C);
    ISWM_REQUIRE(slab_bytes >= (size_t)nb * sizeof(float), "absmax: slab too small (see iswm_absmax_workspace)");
    hipLaunchKernelGGL(k_absmax, dim3(nb), dim3(QB), 0, (hipStream_t)stream, x, ps, rows, C, ld, slab);
    if (int rc = check_launch("absmax")) return rc;
    hipLaunchKernelGGL(k_absmax_finalize, dim3(1), dim3(QB), 0, (hipStream_t)stream, slab, nb, amax);
    return check_launch("absmax_finalize");
}

extern "C" int iswm_quantize_i8(const void* x, int64_t ps, int64_t rows, int C, int ld, double inv_s, int lo,
                                signed char* y, int ldy, iswm_stream_t stream) {
    ISWM_REQUIRE(x && y, "quantize_i8: null pointer");
    ISWM_REQUIRE(rows > 0 && C > 0 && ld % 4 == 0 && ld >= (C + 3) / 4 * 4, "quantize_i8: need ld %% 4 == 0, ld >= pad4(C)");
    ISWM_REQUIRE(ldy % 4 == 0 && ldy >= C && aligned4(y), "quantize_i8: need ldy %% 4 == 0, ldy >= C, y 4-byte aligned");
    ISWM_REQUIRE(lo == 0 || lo == -127, "quantize_i8: lo is 0 or -127");
    hipLaunchKernelGGL(k_quantize_i8, dim3(stream_grid(rows * (ldy / 4), QB)), dim3(QB), 0, (hipStream_t)stream, x, ps,
                       rows, C, ld, inv_s, lo, reinterpret_cast<int8_t*>(y), ldy);
    return check_launch("quantize_i8");
}

extern "C" int iswm_qgap(const signed char* x, int N, int HW, int C, int ldx, double s_in, double inv_s_in,
                         signed char* y, int ldy, iswm_stream_t stream) {
    ISWM_REQUIRE(x && y, "qgap: null pointer");
    ISWM_REQUIRE(N > 0 && N <= 65535 && HW > 0 && HW < (1 << 24) && C > 0 && ldx >= C && ldy >= C, "qgap: bad size");
    hipLaunchKernelGGL(k_qgap, dim3((C + QB - 1) / QB, N), dim3(QB), 0, (hipStream_t)stream,
                       reinterpret_cast<const int8_t*>(x), HW, C, ldx, s_in, inv_s_in, reinterpret_cast<int8_t*>(y), ldy);
    return check_launch("qgap");
}

extern "C" int iswm_qbcast(const signed char* v, int N, int HW, int C, int ldv, signed char* y, int ldy,
                           iswm_stream_t stream) {
    ISWM_REQUIRE(v && y, "qbcast: null pointer");
    ISWM_REQUIRE(N > 0 && HW > 0 && C > 0 && C % 4 == 0 && ldv % 4 == 0 && ldy % 4 == 0 && ldv >= C && ldy >= C,
                 "qbcast: need C, ldv, ldy multiples of 4");
    ISWM_REQUIRE(aligned4(v) && aligned4(y), "qbcast: pointers must be 4-byte aligned");
    hipLaunchKernelGGL(k_qbcast, dim3(stream_grid((int64_t)N * HW * (C / 4), QB)), dim3(QB), 0, (hipStream_t)stream,
                       reinterpret_cast<const int8_t*>(v), N, HW, C, ldv, reinterpret_cast<int8_t*>(y), ldy);
    return check_launch("qbcast");
}

extern "C" int iswm_qbilinear(const signed char* x, int N, int Hi, int Wi, int C, int ldx, double s_in, int Ho, int Wo,
                              double inv_s_out, signed char* y, int ldy, iswm_stream_t stream) {
    ISWM_REQUIRE(x && y, "qbilinear: null pointer");
    ISWM_REQUIRE(N > 0 && Hi > 0 && Wi > 0 && Ho > 0 && Wo > 0 && C > 0 && C % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 &&
                     ldx >= C && ldy >= C,
                 "qbilinear: need C, ldx, ldy multiples of 4");
    ISWM_REQUIRE(aligned4(x) && aligned4(y), "qbilinear: pointers must be 4-byte aligned");
    const float sh = (float)Hi / (float)Ho, sw = (float)Wi / (float)Wo;
    hipLaunchKernelGGL(k_qbilinear, dim3(stream_grid((int64_t)N * Ho * Wo * (C / 4), QB)), dim3(QB), 0,
                       (hipStream_t)stream, reinterpret_cast<const int8_t*>(x), N, Hi, Wi, C, ldx, s_in, Ho, Wo, sh, sw,
                       inv_s_out, reinterpret_cast<int8_t*>(y), ldy);
    return check_launch("qbilinear");
}
