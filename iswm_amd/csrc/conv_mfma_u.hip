// Tap-uniform fast path of the implicit-GEMM convolution (forward and data gradient).
//
// When the channel count of the gathered operand is a multiple of the K chunk (32) -- every conv of
// the network except the 3-channel stem, the 304-channel decoder input and the 48/16-wide projections --
// a K chunk never straddles two filter taps, so the K loop becomes (tap, channel-chunk):
//   * per TAP each thread derives its gather pointers once (ih/iw, bounds, 64-bit address); per CHUNK it
//     only adds a constant stride -- no integer division and no per-row predicate in the inner loop.
//     Rows that fall into the zero padding point at a device zero buffer with stride 0, so the loads are
//     unconditional (no exec-mask branches) and land in L1;
//   * a tap whose gather is out of bounds for EVERY row of the tile (the ASPP rates on a 33x33 map: 36-60 %
//     of the taps) is skipped with one block-wide vote -- the all-padding taps are never multiplied;
//   * the lower per-chunk VALU cost makes 64x64 tiles with 4 workgroups per CU viable, which removes
//     most of the tile-quantisation loss on the 33x33 stages (137 row tiles x 2 column tiles = 274
//     workgroups of 128x128 for 512 slots).
// MFMA scheme, LDS layouts and epilogues are those of conv_mfma.hip.
#include <stdlib.h>

#include "conv_tile32.h"

namespace iswm {

template <int BM, int BN>
struct TileCfg {
    static constexpr int MB = BM / 64;        // 32x32 MFMA tiles per wave along M
    static constexpr int NB = BN / 64;
    static constexpr int AR = BM / 32;        // A rows staged per thread
    static constexpr int BR = BN / 32;
    static constexpr int OCC = (BM == 64 && BN == 64) ? 4 : 2;   // workgroups per CU (LDS / VGPR budget)
};

// ------------------------------------------------------------------------------------------
// forward
// ------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(256, (TileCfg<BM, BN>::OCC)) void k_conv_fwd_u(const ConvArgs a) {
    using T = TileCfg<BM, BN>;
    constexpr int MB = T::MB, NB = T::NB, AR = T::AR, BR = T::BR;
    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * KC_PITCH];
    float* As = smem;
    float* Bs = smem + 2 * BM * KC_PITCH;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L / a.NT, nt = L - mt * a.NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int q = t & 7, r0 = t >> 3;

    TapGather<false, AR> ga;
    ga.init(a, m0 + r0, false);
    const float* wbase[BR];
    bool wok[BR];
#pragma unroll
    for (int j = 0; j < BR; ++j) {
        int n = n0 + r0 + 32 * j;
        wok[j] = n < a.Cout;
        wbase[j] = a.w + (size_t)(wok[j] ? n : 0) * a.Ktot + q * 4;
    }
    const float* bptr[BR];
    int bstep[BR];
    auto setup_b = [&](int tap) {
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            bptr[j] = wok[j] ? wbase[j] + (size_t)tap * a.Cin : g_zero_row + q * 4;
            bstep[j] = wok[j] ? 32 : 0;
        }
    };

    float4 ra[AR], rb[BR];
    auto gload = [&]() {
        ga.load(ra);
#pragma unroll
        for (int j = 0; j < BR; ++j) {
            rb[j] = ldg4(bptr[j]);
            bptr[j] += bstep[j];
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AR; ++j)
            *reinterpret_cast<float4*>(&As[(buf * BM + r0 + 32 * j) * KC_PITCH + q * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < BR; ++j)
            *reinterpret_cast<float4*>(&Bs[(buf * BN + r0 + 32 * j) * KC_PITCH + q * 4]) = rb[j];
    };

    f32x16 acc[MB][NB];
    tile_clear(acc);

    bool more = ga.next(a, q, setup_b);
    if (more) {
        gload();
        lstore(0);
    }
    __syncthreads();
    int cur = 0;
    while (more) {
        const bool more2 = ga.next(a, q, setup_b);
        if (more2) gload();
        const float* Ab = &As[(cur * BM + wm * (BM / 2) + li) * KC_PITCH + lh * 4];
        const float* Bb = &Bs[(cur * BN + wn * (BN / 2) + li) * KC_PITCH + lh * 4];
        mma_chunk_kc(Ab, Bb, acc);
        if (more2) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        more = more2;
    }

    tile_store<BM, BN, false>(a, acc, m0, n0);
    if (a.stats != nullptr) tile_stats<BM, BN>(a, acc, smem, mt, n0);
}

// ------------------------------------------------------------------------------------------
// data gradient: rows are INPUT pixels, K = (tap, cout); a.x = dy (pitch a.ldx), a.y = dx (pitch a.ldy)
// ------------------------------------------------------------------------------------------
template <int BM, int BN>
__global__ __launch_bounds__(256, (TileCfg<BM, BN>::OCC)) void k_conv_dgrad_u(const ConvArgs a) {
    using T = TileCfg<BM, BN>;
    constexpr int MB = T::MB, NB = T::NB, AR = T::AR;
    constexpr int BQ = BN / 4, BKR = 256 / BQ, BPASS = 32 / BKR;
    __shared__ __attribute__((aligned(16))) float smem[2 * BM * KC_PITCH + 2 * 32 * BN];
    float* As = smem;
    float* Bs = smem + 2 * BM * KC_PITCH;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L / a.NT, nt = L - mt * a.NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int q = t & 7, r0 = t >> 3;
    const int bq = t % BQ, bk0 = t / BQ;

    TapGather<true, AR> ga;
    ga.init(a, m0 + r0, false);
    const bool nok = n0 + bq * 4 < a.Cin;
    const size_t bchunk = (size_t)32 * ga.taps * a.Cin;   // weight floats between consecutive cout chunks

    const float* bptr[BPASS];
    auto setup_b = [&](int tap) {
#pragma unroll
        for (int j = 0; j < BPASS; ++j)
            bptr[j] = nok ? a.w + ((size_t)(bk0 + BKR * j) * ga.taps + tap) * a.Cin + n0 + bq * 4 : g_zero_row;
    };
    const size_t bstep = nok ? bchunk : 0;

    float4 ra[AR], rb[BPASS];
    auto gload = [&]() {
        ga.load(ra);
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            rb[j] = ldg4(bptr[j]);
            bptr[j] += bstep;
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < AR; ++j)
            *reinterpret_cast<float4*>(&As[(buf * BM + r0 + 32 * j) * KC_PITCH + q * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < BPASS; ++j)
            *reinterpret_cast<float4*>(&Bs[(buf * 32 + bk0 + BKR * j) * BN + bq * 4]) = rb[j];
    };

    f32x16 acc[MB][NB];
    tile_clear(acc);

    bool more = ga.next(a, q, setup_b);
    if (more) {
        gload();
        lstore(0);
    }
    __syncthreads();
    int cur = 0;
    while (more) {
        const bool more2 = ga.next(a, q, setup_b);
        if (more2) gload();
        const float* Ab = &As[(cur * BM + wm * (BM / 2) + li) * KC_PITCH + lh * 4];
        const float* Bb = &Bs[(cur * 32 + lh * 4) * BN + wn * (BN / 2) + li];
        mma_chunk_rc<BN>(Ab, Bb, acc);
        if (more2) lstore(cur ^ 1);
        __syncthreads();
        cur ^= 1;
        more = more2;
    }
    tile_store<BM, BN, true>(a, acc, m0, n0);
}

// Tile choice: a CU works through ceil(tiles / 256) tiles (co-resident workgroups share its SIMDs), so
// the estimated time is rounds x tile area / intrinsic efficiency of the shape.
void conv_pick_tile(int64_t M, int cols, int* bm, int* bn) {
    struct Cand {
        int bm, bn;
        double eff;
    };
    const Cand cands[3] = {{128, 128, 1.00}, {128, 64, 0.92}, {64, 64, 0.80}};
    double best = 1e300;
    *bm = 128;
    *bn = 128;
    for (const Cand& c : cands) {
        if (c.bn == 128 && (cols <= 64 || (cols % 128 != 0 && cols % 128 <= 64))) continue;
        int64_t tiles = ((M + c.bm - 1) / c.bm) * ((cols + c.bn - 1) / c.bn);
        double cost = (double)((tiles + 255) / 256) * c.bm * c.bn / c.eff;
        if (cost < best) {
            best = cost;
            *bm = c.bm;
            *bn = c.bn;
        }
    }
}

// bm x bn from conv_pick_tile; false when there is no such instantiation
bool launch_conv_fwd_u(ConvArgs a, hipStream_t s, int bm, int bn) {
    if (a.Cin % 32 != 0) return false;
    a.MT = (a.M + bm - 1) / bm;
    a.NT = (a.Cout + bn - 1) / bn;
    dim3 grid(a.MT * a.NT), blk(256);
    if (bm == 128 && bn == 128) hipLaunchKernelGGL((k_conv_fwd_u<128, 128>), grid, blk, 0, s, a);
    else if (bm == 128 && bn == 64) hipLaunchKernelGGL((k_conv_fwd_u<128, 64>), grid, blk, 0, s, a);
    else if (bm == 64 && bn == 64) hipLaunchKernelGGL((k_conv_fwd_u<64, 64>), grid, blk, 0, s, a);
    else return false;
    return true;
}

bool launch_conv_dgrad_u(ConvArgs a, hipStream_t s, int bm, int bn) {
    if (a.Cout % 32 != 0) return false;
    a.MT = (a.M + bm - 1) / bm;
    a.NT = (a.Cin + bn - 1) / bn;
    dim3 grid(a.MT * a.NT), blk(256);
    if (bm == 128 && bn == 128) hipLaunchKernelGGL((k_conv_dgrad_u<128, 128>), grid, blk, 0, s, a);
    else if (bm == 128 && bn == 64) hipLaunchKernelGGL((k_conv_dgrad_u<128, 64>), grid, blk, 0, s, a);
    else if (bm == 64 && bn == 64) hipLaunchKernelGGL((k_conv_dgrad_u<64, 64>), grid, blk, 0, s, a);
    else return false;
    return true;
}

}  // namespace iswm
