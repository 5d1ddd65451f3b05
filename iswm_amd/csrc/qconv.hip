// INT8 implicit-GEMM convolution, forward only: the convolutions of the post-training quantized inference path
// (iswm_amd/quant.py).
//
//   GEMM  D[cout][pixel] = sum_k W[cout][k] * X[k][pixel],   k = (tap, cin),  int8 x int8 -> exact int32
//
// on v_mfma_i32_16x16x64_i8.  The weights are the A (row) operand and the activations the B (column) operand, so a
// lane's four accumulators are four CONSECUTIVE output channels of one pixel (C/D map: col = lane & 15,
// row = 4 (lane >> 4) + r): the int8 epilogue stores one dword per pixel and row block, the fp32 one a float4.
// A and B lane maps: lane l holds 16 bytes, row / column l & 15, k = 16 (l >> 4) + j.  Both operands are loaded with
// the same k assignment, so the product is independent of the hardware's k order inside a lane group;
// tests/test_quant_gpu.py checks the row / column maps with exact asymmetric integer data.
//
// Tile: a wave computes (16 MB pixels) x (16 NB output channels); four waves of a workgroup stack along the pixels.
// Operands go global -> registers straight (16-B loads: 4 lanes cover one pixel's 64-channel chunk, 64 contiguous
// bytes), one K step (one tap, 64 input channels) ahead of the MFMAs that use them.  Padding taps and pixels past M
// load zeros.  Epilogue (fp64, no contraction; the restatement in tests/quant_ref.py does the same operations):
//   v = (double)acc * mul[c] + add[c];  v += (double)res * s_res;  v = max(v, 0);
//   int8:  q = clamp(rint(v * inv_s_out), lo, 127)      fp32:  (float)v
#pragma clang fp contract(off)
#include "common.h"

namespace iswm {

typedef int qv4i __attribute__((ext_vector_type(4)));

constexpr int QC_WAVES = 4;
constexpr int QC_MB = 4;

__device__ __forceinline__ int q_clamp(double v, double inv_s, int lo) {
    double r = rint(v * inv_s);
    r = r < (double)lo ? (double)lo : r;
    r = r > 127.0 ? 127.0 : r;
    return (int)r;
}

template <int MB, int NB>
__global__ __launch_bounds__(256) void k_qconv(const iswm_qconv_desc d, const int8_t* __restrict__ x,
                                               const int8_t* __restrict__ w, const double* __restrict__ mul,
                                               const double* __restrict__ add, const int8_t* __restrict__ res,
                                               double s_res, double inv_s_out, void* __restrict__ y) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int li = lane & 15, lh = lane >> 4;
    const int HoWo = d.Ho * d.Wo;
    const int64_t M = (int64_t)d.N * HoWo;
    const int64_t m0 = ((int64_t)blockIdx.x * QC_WAVES + wave) * (16 * MB);
    if (m0 >= M) return;                       // no barriers below: a wave past the last pixel simply leaves
    const int n0 = blockIdx.y * (16 * NB);
    const int K = d.KH * d.KW * d.Cin;

    int pn[MB], ph[MB], pw[MB];
    bool pv[MB];
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        const int64_t m = m0 + 16 * b + li;
        pv[b] = m < M;
        const int mm = pv[b] ? (int)m : 0;
        pn[b] = mm / HoWo;
        const int rem = mm - pn[b] * HoWo;
        const int oh = rem / d.Wo, ow = rem - oh * d.Wo;
        ph[b] = oh * d.stride - d.pad;
        pw[b] = ow * d.stride - d.pad;
    }
    const int8_t* wl[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j) wl[j] = w + (size_t)(n0 + 16 * j + li) * K + 16 * lh;

    qv4i acc[MB][NB];
#pragma unroll
    for (int b = 0; b < MB; ++b)
#pragma unroll
        for (int j = 0; j < NB; ++j) acc[b][j] = qv4i{0, 0, 0, 0};

    const qv4i zero = {0, 0, 0, 0};
    const int chunks = d.Cin >> 6;
    const int steps = d.KH * d.KW * chunks;
    // step s = (tap, chunk); xp[b] = this lane's source row of the step's tap (nullptr: padding / past M)
    const int8_t* xp[MB];
    auto tap_rows = [&](int tap) {
        const int kh = tap / d.KW, kw = tap - kh * d.KW;
#pragma unroll
        for (int b = 0; b < MB; ++b) {
            const int ih = ph[b] + kh * d.dil, iw = pw[b] + kw * d.dil;
            const bool ok = pv[b] && ih >= 0 && ih < d.H && iw >= 0 && iw < d.W;
            xp[b] = ok ? x + ((size_t)(pn[b] * d.H + ih) * d.W + iw) * d.ldx + 16 * lh : nullptr;
        }
    };
    tap_rows(0);
    qv4i a[MB], bw[NB];
#pragma unroll
    for (int b = 0; b < MB; ++b) a[b] = xp[b] ? *reinterpret_cast<const qv4i*>(xp[b]) : zero;
#pragma unroll
    for (int j = 0; j < NB; ++j) bw[j] = *reinterpret_cast<const qv4i*>(wl[j]);
    int tap = 0, c0 = 0;
    for (int s = 0; s < steps; ++s) {
        // fetch step s + 1 (nothing after the last one)
        qv4i an[MB], bn[NB];
        if (s + 1 < steps) {
            c0 += 64;
            if (c0 == d.Cin) {
                c0 = 0;
                tap_rows(++tap);
            }
            const int kk = tap * d.Cin + c0;
#pragma unroll
            for (int b = 0; b < MB; ++b) an[b] = xp[b] ? *reinterpret_cast<const qv4i*>(xp[b] + c0) : zero;
#pragma unroll
            for (int j = 0; j < NB; ++j) bn[j] = *reinterpret_cast<const qv4i*>(wl[j] + kk);
        }
#pragma unroll
        for (int b = 0; b < MB; ++b)
#pragma unroll
            for (int j = 0; j < NB; ++j) acc[b][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(bw[j], a[b], acc[b][j], 0, 0, 0);
        if (s + 1 < steps) {
#pragma unroll
            for (int b = 0; b < MB; ++b) a[b] = an[b];
#pragma unroll
            for (int j = 0; j < NB; ++j) bw[j] = bn[j];
        }
    }

    // epilogue: lane (li, lh) owns pixel m0 + 16 b + li, channels n0 + 16 j + 4 lh + r
#pragma unroll
    for (int b = 0; b < MB; ++b) {
        if (!pv[b]) continue;
        const int64_t m = m0 + 16 * b + li;
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int c = n0 + 16 * j + 4 * lh;
            if (c >= d.cstore) continue;
            int rq[4] = {0, 0, 0, 0};
            if (res) {
                const unsigned rw = *reinterpret_cast<const unsigned*>(res + (size_t)m * d.ldr + c);
#pragma unroll
                for (int r = 0; r < 4; ++r) rq[r] = (int)(int8_t)(rw >> (8 * r));
            }
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = (double)acc[b][j][r] * mul[c + r] + add[c + r];
                if (res) v[r] = v[r] + (double)rq[r] * s_res;
                if (d.relu) v[r] = v[r] > 0.0 ? v[r] : 0.0;
            }
            const bool full = c + 4 <= d.cstore;
            if (d.out_f32) {
                float* o = reinterpret_cast<float*>(y) + (size_t)m * d.ldy + c;
                if (full) {
                    *reinterpret_cast<float4*>(o) = make_float4((float)v[0], (float)v[1], (float)v[2], (float)v[3]);
                } else {
                    for (int r = 0; r < 4 && c + r < d.cstore; ++r) o[r] = (float)v[r];
                }
            } else {
                int8_t* o = reinterpret_cast<int8_t*>(y) + (size_t)m * d.ldy + c;
                unsigned pk = 0;
#pragma unroll
                for (int r = 0; r < 4; ++r) pk |= (unsigned)(q_clamp(v[r], inv_s_out, d.lo) & 0xFF) << (8 * r);
                if (full) {
                    *reinterpret_cast<unsigned*>(o) = pk;
                } else {
                    for (int r = 0; r < 4 && c + r < d.cstore; ++r) o[r] = (int8_t)(pk >> (8 * r));
                }
            }
        }
    }
}

}  // namespace iswm

using namespace iswm;

static int qconv_check(const iswm_qconv_desc* d) {
    ISWM_REQUIRE(d, "qconv: null descriptor");
    ISWM_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0 && d->Ho > 0 && d->Wo > 0, "qconv: bad map size");
    ISWM_REQUIRE(d->Cin > 0 && d->Cin % 64 == 0, "qconv: Cin %d must be a positive multiple of 64", d->Cin);
    ISWM_REQUIRE(d->Cout > 0 && d->Cout % 16 == 0, "qconv: Cout %d must be a positive multiple of 16", d->Cout);
    ISWM_REQUIRE(d->KH > 0 && d->KW > 0 && d->stride > 0 && d->dil > 0 && d->pad >= 0, "qconv: bad filter geometry");
    ISWM_REQUIRE((d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1 == d->Ho &&
                     (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1 == d->Wo,
                 "qconv: output size does not match the geometry");
    ISWM_REQUIRE(d->ldx >= d->Cin && d->ldx % 16 == 0, "qconv: need ldx >= Cin, ldx %% 16 == 0");
    ISWM_REQUIRE(d->cstore > 0 && d->cstore <= d->Cout && d->ldy >= d->cstore && d->ldy % 4 == 0,
                 "qconv: need 0 < cstore <= Cout, ldy >= cstore, ldy %% 4 == 0");
    ISWM_REQUIRE(d->out_f32 == 0 || d->out_f32 == 1, "qconv: out_f32 is 0 or 1");
    ISWM_REQUIRE(d->lo == 0 || d->lo == -127, "qconv: lo is 0 or -127");
    ISWM_REQUIRE((int64_t)d->N * d->Ho * d->Wo < (1LL << 31) && (int64_t)d->N * d->H * d->W < (1LL << 31),
                 "qconv: map too large");
    return 0;
}

extern "C" size_t iswm_qconv_weight_bytes(const iswm_qconv_desc* d) {
    if (!d || d->Cout <= 0 || d->Cout % 16 || d->Cin <= 0 || d->Cin % 64 || d->KH <= 0 || d->KW <= 0) return 0;
    return (size_t)d->Cout * d->KH * d->KW * d->Cin;
}

extern "C" int iswm_qconv_fwd(const iswm_qconv_desc* d, const signed char* x, const signed char* w, const double* mul,
                              const double* add, const signed char* res, double s_res, double inv_s_out, void* y,
                              iswm_stream_t stream) {
    if (int rc = qconv_check(d)) return rc;
    ISWM_REQUIRE(x && w && mul && add && y, "qconv: null pointer");
    ISWM_REQUIRE(aligned16(x) && aligned16(w), "qconv: x and w must be 16-byte aligned");
    ISWM_REQUIRE((reinterpret_cast<uintptr_t>(y) & (d->out_f32 ? 15 : 3)) == 0 && (!d->out_f32 || d->ldy % 4 == 0),
                 "qconv: y must be 4-byte (int8) / 16-byte (fp32) aligned");
    ISWM_REQUIRE(!res || ((reinterpret_cast<uintptr_t>(res) & 3) == 0 && d->ldr % 4 == 0 && d->ldr >= d->cstore),
                 "qconv: residual must be 4-byte aligned with ldr %% 4 == 0, ldr >= cstore");
    ISWM_REQUIRE(!res || !d->out_f32, "qconv: a residual needs int8 output");
    const int64_t M = (int64_t)d->N * d->Ho * d->Wo;
    const int64_t rows_per_wg = (int64_t)QC_WAVES * 16 * QC_MB;
    const bool wide = d->Cout % 64 == 0;
    const dim3 grid((unsigned)((M + rows_per_wg - 1) / rows_per_wg), (unsigned)(d->Cout / (wide ? 64 : 16)));
    ISWM_REQUIRE(grid.x < (1u << 31) && grid.y <= 65535, "qconv: grid too large");
    const int8_t* xi = reinterpret_cast<const int8_t*>(x);
    const int8_t* wi = reinterpret_cast<const int8_t*>(w);
    const int8_t* ri = reinterpret_cast<const int8_t*>(res);
    if (wide)
        hipLaunchKernelGGL((k_qconv<QC_MB, 4>), grid, dim3(256), 0, (hipStream_t)stream, *d, xi, wi, mul, add, ri, s_res,
                           inv_s_out, y);
    else
        hipLaunchKernelGGL((k_qconv<QC_MB, 1>), grid, dim3(256), 0, (hipStream_t)stream, *d, xi, wi, mul, add, ri, s_res,
                           inv_s_out, y);
    return check_launch("qconv");
}
