// Device-side pieces shared by the round-1 convolution kernels -- the fp32-operand kernels on the 32x32 MFMA C/D map:
// k_conv_fwd / k_conv_dgrad (conv_mfma.hip), k_conv_fwd_u / k_conv_dgrad_u (conv_mfma_u.hip) and k_conv_x6 (conv_mfma_x6.hip).
// One workgroup = 4 waves (2 x 2) on a BM x BN tile; wave (wm, wn) owns (BM/2) x (BN/2) as 32x32 accumulators acc[mb][nb].
//   g_zero_row                 the row that out-of-bounds gathers read (also k_conv_wgrad's)
//   tile32_row                 C/D map: row of accumulator register r of a 32x32 block
//   tile_clear                 accumulators = 0
//   row_bases                  GEMM row -> gather bases of a thread's staged rows, forward and data gradient
//   TapGather                  A operand of the tap-uniform K loop: per-tap pointers, block vote, (tap, chunk) iterator, loads
//                              (the two _u kernels; k_conv_x6 keeps its own copy: with this one its data-gradient
//                              instantiations need 2-4 more VGPRs and the 128 x 64 plain-weight one spills at its 168)
//   mma_chunk_kc / _rc         fp32 multiply of one staged 32-wide K chunk, B K-contiguous / row-contiguous in LDS
//   tile_store / tile_stats    epilogue: store (bias or accumulate) and the BatchNorm tile statistics
// k_conv_wgrad (conv_mfma.hip) uses the zero row only: its instruction streams change with any of the other pieces.
#pragma once
#include "conv_common.h"

namespace iswm {

static __device__ __attribute__((aligned(16))) float g_zero_row[64];   // zero-initialised: target of padded / out-of-range rows

// C/D map of v_mfma_f32_32x32x*: lane l holds column l & 31; register r of lane half lh = l >> 5 holds this row of the 32x32
// block whose first row is row0
__device__ __forceinline__ int tile32_row(int row0, int r, int lh) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * lh; }

template <int MB, int NB>
__device__ __forceinline__ void tile_clear(f32x16 (&acc)[MB][NB]) {
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
}

// Gather bases of the AR rows m_first + 32 j a thread stages.  The rows live in the output grid Ho x Wo (forward) or the input
// grid H x W (data gradient: a.x = dy); pb is the first pixel of the row's image in the GATHERED tensor.
//   forward:        (hb, wb) = (oh, ow) * stride - pad      tap (kh, kw) gathers (hb + kh*dil, wb + kw*dil)
//   data gradient:  (hb, wb) = (ih, iw) + pad               tap (kh, kw) gathers ((hb - kh*dil) / stride, ...) where that divides
// Rows past M get an hb no tap brings in bounds.  par: the parity row order of x6_row_pixel (a k_conv_x6 option).
template <bool DGRAD, int AR>
__device__ __forceinline__ void row_bases(const ConvArgs& a, int m_first, bool par, int (&hb)[AR], int (&wb)[AR], int (&pb)[AR]) {
    const int RH = DGRAD ? a.H : a.Ho, RW = DGRAD ? a.W : a.Wo;
    const int GH = DGRAD ? a.Ho : a.H, GW = DGRAD ? a.Wo : a.W;
#pragma unroll
    for (int j = 0; j < AR; ++j) {
        int m = m_first + 32 * j;
        if (m < a.M) {
            int n, rh, rw;
            x6_row_pixel(m, a.N, RH, RW, par, n, rh, rw);
            hb[j] = DGRAD ? rh + a.pad : rh * a.stride - a.pad;
            wb[j] = DGRAD ? rw + a.pad : rw * a.stride - a.pad;
            pb[j] = n * GH * GW;
        } else {
            hb[j] = -(1 << 28);
            wb[j] = 0;
            pb[j] = 0;
        }
    }
}

// A operand of the tap-uniform K loop (gathered channels % 32 == 0, so a 32-wide chunk never straddles two taps): per TAP each
// thread derives the pointers of its AR rows once, per CHUNK it adds a constant.  Rows in the zero padding point at g_zero_row
// with step 0, so the loads are unconditional; a tap out of bounds for EVERY row of the tile is skipped by one block vote.
// q = t & 7: the thread's float4 column of the chunk.
template <bool DGRAD, int AR>
struct TapGather {
    int hb[AR], wb[AR], pb[AR];
    const float* aptr[AR];
    int astep[AR];
    int tap, cc, taps, nCC;

    __device__ __forceinline__ void init(const ConvArgs& a, int m_first, bool par) {
        row_bases<DGRAD>(a, m_first, par, hb, wb, pb);
        taps = a.KH * a.KW;
        nCC = (DGRAD ? a.Cout : a.Cin) >> 5;
        tap = -1;
        cc = nCC - 1;
    }
    // advance to the next (tap, channel chunk) that has work; block-uniform.  setup_b(tap): the caller's B-side pointers
    template <class SetupB>
    __device__ __forceinline__ bool next(const ConvArgs& a, int q, SetupB&& setup_b) {
        if (++cc < nCC) return true;
        cc = 0;
        do {
            if (++tap >= taps) return false;
        } while (!setup(a, q, setup_b));
        return true;
    }
    template <class SetupB>
    __device__ __forceinline__ bool setup(const ConvArgs& a, int q, SetupB&& setup_b) {
        const int GH = DGRAD ? a.Ho : a.H, GW = DGRAD ? a.Wo : a.W;     // gathered tensor dims
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        const int dh = kh * a.dil, dw = kw * a.dil;
        int any = 0;
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            int gh, gw;
            bool ok;
            if (DGRAD) {
                int th = hb[j] - dh, tw = wb[j] - dw;
                gh = th;
                gw = tw;
                ok = th >= 0 && tw >= 0;
                if (a.stride != 1) {
                    gh = th / a.stride;
                    gw = tw / a.stride;
                    ok = ok && (gh * a.stride == th) && (gw * a.stride == tw);
                }
                ok = ok && gh < GH && gw < GW;
            } else {
                gh = hb[j] + dh;
                gw = wb[j] + dw;
                ok = (unsigned)gh < (unsigned)GH && (unsigned)gw < (unsigned)GW;
            }
            aptr[j] = (ok ? a.x + (size_t)(pb[j] + gh * GW + gw) * a.ldx : g_zero_row) + q * 4;
            astep[j] = ok ? 32 : 0;
            any |= ok;
        }
        setup_b(tap);
        return __syncthreads_or(any) != 0;
    }
    __device__ __forceinline__ void load(float4 (&ra)[AR]) {
#pragma unroll
        for (int j = 0; j < AR; ++j) {
            ra[j] = ldg4(aptr[j]);
            aptr[j] += astep[j];
        }
    }
};

// acc += A chunk x B chunk on v_mfma_f32_32x32x2_f32.  Ab: this lane's A row of the K-contiguous tile (pitch KC_PITCH) at k = 4 lh;
// one b128 read feeds 4 MFMAs.  Bb: the same for a K-contiguous B (kc), or column li of k row 4 lh of a [k][BN] tile (rc).
template <int MB, int NB>
__device__ __forceinline__ void mma_chunk_kc(const float* Ab, const float* Bb, f32x16 (&acc)[MB][NB]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float af[MB][4], bf[NB][4];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            *reinterpret_cast<float4*>(af[mb]) = *reinterpret_cast<const float4*>(Ab + mb * 32 * KC_PITCH + g * 8);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
            *reinterpret_cast<float4*>(bf[nb]) = *reinterpret_cast<const float4*>(Bb + nb * 32 * KC_PITCH + g * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = mfma32(af[mb][j], bf[nb][j], acc[mb][nb]);
    }
}

template <int BN, int MB, int NB>
__device__ __forceinline__ void mma_chunk_rc(const float* Ab, const float* Bb, f32x16 (&acc)[MB][NB]) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float af[MB][4], bf[NB][4];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
            *reinterpret_cast<float4*>(af[mb]) = *reinterpret_cast<const float4*>(Ab + mb * 32 * KC_PITCH + g * 8);
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int j = 0; j < 4; ++j) bf[nb][j] = Bb[(g * 8 + j) * BN + nb * 32];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) acc[mb][nb] = mfma32(af[mb][j], bf[nb][j], acc[mb][nb]);
    }
}

// Store the tile at rows m0.., columns n0.. of a.y: + bias (forward) or, data gradient, into or onto dx (a.accumulate).
// rowpix: pixel of each tile row where the rows are not in pixel order (parity order of k_conv_x6), else nullptr.
template <int BM, int BN, bool DGRAD>
__device__ __forceinline__ void tile_store(const ConvArgs& a, const f32x16 (&acc)[BM / 64][BN / 64], int m0, int n0,
                                           const int* rowpix = nullptr) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int NC = DGRAD ? a.Cin : a.Cout;
#pragma unroll
    for (int nb = 0; nb < BN / 64; ++nb) {
        const int col = n0 + wn * (BN / 2) + nb * 32 + li;
        const bool cok = col < NC;
        const float bv = (!DGRAD && a.bias != nullptr && cok) ? a.bias[col] : 0.f;
#pragma unroll
        for (int mb = 0; mb < BM / 64; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int lr = tile32_row(wm * (BM / 2) + mb * 32, r, lh);
                const int row = m0 + lr;
                if (cok && row < a.M) {
                    float* o = &a.y[(size_t)(rowpix != nullptr ? rowpix[lr] : row) * a.ldy + col];
                    if (DGRAD) *o = a.accumulate ? *o + acc[mb][nb][r] : acc[mb][nb][r];
                    else *o = acc[mb][nb][r] + bv;
                }
            }
    }
}

// Per-tile BatchNorm statistics of a forward tile, numerically centred: column sum S_t first, then the sum of squared deviations
// from the TILE mean (M2_t).  iswm_bn_finalize merges tiles with the pairwise (Chan) update in double, so the batch variance never
// suffers the E[x^2]-mean^2 cancellation -- this is what keeps 100 stacked train-mode BN layers within 1e-3 of the CPU.  Tiles are
// BM rows, so the host passes tile_rows = BM to iswm_bn_finalize.  red: 4 * BN floats of LDS the K loop is done with.
template <int BM, int BN>
__device__ __forceinline__ void tile_stats(const ConvArgs& a, const f32x16 (&acc)[BM / 64][BN / 64], float* red, int mt, int n0) {
    constexpr int MB = BM / 64, NB = BN / 64;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int m0 = mt * BM;
    const int cnt = min(BM, a.M - m0);   // red: [4][BN]: sum(wm=0), sum(wm=1), M2(wm=0), M2(wm=1)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        float s = 0.f;   // rows past M were staged as zeros, so they add nothing
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) s += acc[mb][nb][r];
        s += __shfl_xor(s, 32);
        if (lh == 0) red[wm * BN + wn * (BN / 2) + nb * 32 + li] = s;
    }
    __syncthreads();
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int c = wn * (BN / 2) + nb * 32 + li;
        const float mean = (red[c] + red[BN + c]) / (float)cnt;
        float qv = 0.f;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = tile32_row(m0 + wm * (BM / 2) + mb * 32, r, lh);
                float dv = acc[mb][nb][r] - mean;
                qv += row < a.M ? dv * dv : 0.f;
            }
        qv += __shfl_xor(qv, 32);
        if (lh == 0) red[(2 + wm) * BN + c] = qv;
    }
    __syncthreads();
    if (t < BN && n0 + t < a.Cout) {
        a.stats[(size_t)mt * a.Cout + n0 + t] = red[t] + red[BN + t];
        a.stats[(size_t)(a.MT + mt) * a.Cout + n0 + t] = red[2 * BN + t] + red[3 * BN + t];
    }
}

}  // namespace iswm
