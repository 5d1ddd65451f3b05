// Implicit-GEMM 2-D convolution for gfx950 on the exact-fp32 matrix instruction
// v_mfma_f32_32x32x2_f32: forward, data gradient and weight gradient.
//
// Replaces the nn.Conv2d calls of the reference hot path (network/backbone/resnet.py:27-35,
// 144,184-187; network/_deeplab.py:37,44-51,124,134,149,162) and their autograd backward.
//
// Design:
//   * activations NHWC, weights OHWI: the GEMM K axis (tap, channel) is contiguous in
//     memory for both operands of the forward pass, so tiles are staged with 16-byte
//     loads and no im2col buffer ever exists;
//   * one workgroup = 4 waves (2x2), block tile 128 x {128,64} x 32, each wave owns a
//     64 x {64,32} sub-tile as 32x32 MFMA accumulators; two workgroups per CU;
//   * global -> register -> LDS staging, double-buffered in LDS, one barrier per K chunk:
//     the loads of chunk k+1 are issued before the MFMAs of chunk k and written to the
//     other LDS buffer after them;
//   * an operand whose K axis is contiguous in memory ("KC": activations / OHWI weights
//     in fwd, dy in dgrad) is kept [row][k] in LDS with a 36-float row pitch and read as
//     ds_read_b128 (conflict-free: 16 rows x 144 B hit 16 distinct 16-byte slots); one
//     b128 read feeds 4 MFMAs (lane half h supplies k = 4h+j for MFMA j);
//   * an operand whose ROW axis is contiguous ("RC": weights in dgrad, dy and x in
//     wgrad) is kept [k][row] and read with ds_read_b32 (32 consecutive floats per half);
//   * padding taps are zero-filled at load time; dilation is just a tap offset;
//   * the forward epilogue optionally emits per-tile per-channel sum / sum-of-squares for
//     the training-mode BatchNorm that follows every conv (deterministic two-stage stats);
//   * wgrad flattens (tap, cin) into the GEMM N axis and splits the pixel (K) axis across
//     workgroups into slabs that a second kernel sums in a fixed order (bit-reproducible).
// The C entry points that choose between these kernels and the other families are in conv_api.hip.
#include "conv_tile32.h"

namespace iswm {

// ------------------------------------------------------------------------------------------
// forward:  y[m, co] = sum_k A[m, k] * W[co, k],  m = (n, oh, ow),  k = (kh, kw, ci)
// ------------------------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(256, 2) void k_conv_fwd(const ConvArgs a) {
    constexpr int BM = 128;
    constexpr int NB = BN / 64;    // 32-wide MFMA column tiles per wave
    constexpr int BROWS = BN / 32; // weight rows staged per thread
    __shared__ __attribute__((aligned(16))) float smem[2 * (BM + BN) * KC_PITCH];
    float* As = smem;
    float* Bs = smem + 2 * BM * KC_PITCH;

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L / a.NT, nt = L - mt * a.NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int q = t & 7, r0 = t >> 3;

    int ihb[4], iwb[4], pb[4];
    row_bases<false>(a, m0 + r0, false, ihb, iwb, pb);
    const int Cin4 = a.Cin >> 2, K4 = a.Ktot >> 2;
    const float* wrow[BROWS];
    bool wok[BROWS];
#pragma unroll
    for (int j = 0; j < BROWS; ++j) {
        int n = n0 + r0 + 32 * j;
        wok[j] = n < a.Cout;
        wrow[j] = a.w + (size_t)(wok[j] ? n : 0) * a.Ktot;
    }

    float4 ra[4], rb[BROWS];
    auto gload = [&](int kc) {
        const int k4 = kc * 8 + q;
        const bool kv = k4 < K4;
        const int tap = k4 / Cin4, c4 = k4 - tap * Cin4;
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        const int dh = kh * a.dil, dw = kw * a.dil;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int ih = ihb[j] + dh, iw = iwb[j] + dw;
            bool ok = kv && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
            ra[j] = ok ? ldg4(a.x + (size_t)(pb[j] + ih * a.W + iw) * a.ldx + c4 * 4)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < BROWS; ++j)
            rb[j] = (kv && wok[j]) ? ldg4(wrow[j] + k4 * 4) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<float4*>(&As[(buf * BM + r0 + 32 * j) * KC_PITCH + q * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < BROWS; ++j)
            *reinterpret_cast<float4*>(&Bs[(buf * BN + r0 + 32 * j) * KC_PITCH + q * 4]) = rb[j];
    };

    f32x16 acc[2][NB];
    tile_clear(acc);

    const int nK = (a.Ktot + 31) >> 5;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kc = 0; kc < nK; ++kc) {
        const int cur = kc & 1;
        const bool more = kc + 1 < nK;
        if (more) gload(kc + 1);
        const float* Ab = &As[(cur * BM + wm * 64 + li) * KC_PITCH + lh * 4];
        const float* Bb = &Bs[(cur * BN + wn * (BN / 2) + li) * KC_PITCH + lh * 4];
        mma_chunk_kc(Ab, Bb, acc);
        if (more) lstore(cur ^ 1);
        __syncthreads();
    }

    tile_store<BM, BN, false>(a, acc, m0, n0);
    if (a.stats != nullptr) tile_stats<BM, BN>(a, acc, smem, mt, n0);
}

// ------------------------------------------------------------------------------------------
// dgrad:  dx[m, ci] = sum_k dyG[m, k] * W[k, ci],  m = (n, ih, iw),  k = (kh, kw, co)
// A: gather from dy (K-contiguous).  B: OHWI weights read with ci contiguous (row-contiguous).
// ------------------------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(256, 2) void k_conv_dgrad(const ConvArgs a) {
    constexpr int BM = 128;
    constexpr int NB = BN / 64;
    constexpr int BQ = BN / 4;         // float4 columns of the B tile
    constexpr int BKR = 256 / BQ;      // k rows covered per pass
    constexpr int BPASS = 32 / BKR;    // passes per thread
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

    // rows are INPUT pixels here: a.H/a.W input dims, a.Ho/a.Wo the dims of dy
    int thb[4], twb[4], pb[4];
    row_bases<true>(a, m0 + r0, false, thb, twb, pb);
    const int Co4 = a.Cout >> 2, K4 = a.Ktot >> 2;
    const int taps = a.KH * a.KW;
    const bool nok = n0 + bq * 4 < a.Cin;

    float4 ra[4], rb[BPASS];
    auto gload = [&](int kc) {
        const int k4 = kc * 8 + q;
        const bool kv = k4 < K4;
        const int tap = k4 / Co4, c4 = k4 - tap * Co4;
        const int kh = tap / a.KW, kw = tap - kh * a.KW;
        const int dh = kh * a.dil, dw = kw * a.dil;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            int th = thb[j] - dh, tw = twb[j] - dw;
            int oh = th, ow = tw;
            bool ok = kv && th >= 0 && tw >= 0;
            if (a.stride != 1) {
                oh = th / a.stride;
                ow = tw / a.stride;
                ok = ok && (oh * a.stride == th) && (ow * a.stride == tw);
            }
            ok = ok && oh < a.Ho && ow < a.Wo;
            ra[j] = ok ? ldg4(a.x + (size_t)(pb[j] + oh * a.Wo + ow) * a.ldx + c4 * 4)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            int k = kc * 32 + bk0 + BKR * j;
            bool ok = nok && k < a.Ktot;
            int tp = k / a.Cout, co = k - tp * a.Cout;
            rb[j] = ok ? ldg4(a.w + ((size_t)co * taps + tp) * a.Cin + n0 + bq * 4)
                       : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            *reinterpret_cast<float4*>(&As[(buf * BM + r0 + 32 * j) * KC_PITCH + q * 4]) = ra[j];
#pragma unroll
        for (int j = 0; j < BPASS; ++j)
            *reinterpret_cast<float4*>(&Bs[(buf * 32 + bk0 + BKR * j) * BN + bq * 4]) = rb[j];
    };

    f32x16 acc[2][NB];
    tile_clear(acc);

    const int nK = (a.Ktot + 31) >> 5;
    gload(0);
    lstore(0);
    __syncthreads();
    for (int kc = 0; kc < nK; ++kc) {
        const int cur = kc & 1;
        const bool more = kc + 1 < nK;
        if (more) gload(kc + 1);
        const float* Ab = &As[(cur * BM + wm * 64 + li) * KC_PITCH + lh * 4];
        const float* Bb = &Bs[(cur * 32 + lh * 4) * BN + wn * (BN / 2) + li];
        mma_chunk_rc<BN>(Ab, Bb, acc);
        if (more) lstore(cur ^ 1);
        __syncthreads();
    }
    tile_store<BM, BN, true>(a, acc, m0, n0);
}

// ------------------------------------------------------------------------------------------
// wgrad:  dw[co, j] = sum_p dy[p, co] * xG[p, j],  j = (kh, kw, ci) flattened, p = (n, oh, ow)
// Both operands row-contiguous; the pixel axis is split across blockIdx.y into slabs.
// ------------------------------------------------------------------------------------------
// MODE 0: any geometry.  MODE 1: stride 1 and Ho == H, Wo == W ("same" convs: every 3x3 of the net
// except the two strided ones) -- the gathered pixel of output pixel p is p + dh*W + dw, so addresses
// advance by a constant and only the bounds test needs (oh, ow).  MODE 2: 1x1 stride 1 -- no bounds.
// X6: bf16x6 arithmetic (conv_mfma_x6.hip).  Both operands arrive with the GEMM K axis (pixels) STRIDED in
// memory, so the three bf16 planes are kept [k][row] in LDS (natural 8-byte writes) and the k-contiguous MFMA
// fragments are produced by gfx950's transposing LDS read ds_read_b64_tr_b16 (4 k x 16 rows per 16 lanes);
// row pitch 2*rows + 64 B puts the 4 k-rows of one read on disjoint bank quarters.
// NP (X6 only): bf16 planes per operand -- 3 = exact split / six MFMAs (bf16x6), 1 = rounded operands / one MFMA (bf16)
template <int BM, int BN, int MODE, bool X6, int NP = 3>
__global__ __launch_bounds__(256, 2) void k_conv_wgrad(const ConvArgs a) {
    constexpr int MB = BM / 64, NB = BN / 64;
    constexpr int AQ = BM / 4, AKR = 256 / AQ, APASS = 32 / AKR;
    constexpr int BQ = BN / 4, BKR = 256 / BQ, BPASS = 32 / BKR;
    // X6 row pitches (bytes).  128-column planes are packed (256 B rows, 48 KB per workgroup -> 3 per CU) and
    // the column offset is XORed with 64*(k&3), which lands the 4 k-rows of one transposing read on disjoint
    // bank quarters exactly as the +64 B padding does for the 64-column planes.
    constexpr int XPA = BM == 128 ? 256 : BM * 2 + 64, XPB = BN == 128 ? 256 : BN * 2 + 64;
    constexpr int SWA = BM == 128 ? 64 : 0, SWB = BN == 128 ? 64 : 0;   // swizzle step (bytes)
    constexpr int XPLA = 32 * XPA, XPLB = 32 * XPB;                  // X6 plane sizes (bytes)
    constexpr int SMEM_BYTES = X6 ? NP * (XPLA + XPLB) : 2 * 32 * (BM + BN) * 4;
    __shared__ __attribute__((aligned(16))) unsigned char smem_raw[SMEM_BYTES];
    float* smem = reinterpret_cast<float*>(smem_raw);
    float* As = smem;
    float* Bs = smem + 2 * 32 * BM;
    unsigned char* Ax = smem_raw;               // X6: [3][32][XPA]
    unsigned char* Bx = smem_raw + NP * XPLA;   // X6: [NP][32][XPB]

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave >> 1, wn = wave & 1, li = lane & 31, lh = lane >> 5;
    const int L = xcd_remap(blockIdx.x, gridDim.x);
    const int mt = L / a.NT, nt = L - mt * a.NT;
    const int m0 = mt * BM, n0 = nt * BN;
    const int split = blockIdx.y;
    const int P = a.M;  // pixels of dy
    const int p_begin = split * a.psplit;
    const int p_end = min(P, p_begin + a.psplit);

    const int aq = t % AQ, ak0 = t / AQ;
    const int bq = t % BQ, bk0 = t / BQ;
    const bool aok = m0 + aq * 4 < a.Cout;

    // this thread's B column: one (tap, ci4) for the whole K loop
    const int Cin4 = a.Cin >> 2;
    const int n4 = (n0 >> 2) + bq;
    const bool bok = n4 < (a.Ktot >> 2);
    const int tap = n4 / Cin4, c4 = n4 - tap * Cin4;
    const int kh = tap / a.KW, kw = tap - kh * a.KW;
    const int dh = kh * a.dil - a.pad, dw = kw * a.dil - a.pad;

    // pixel coordinates (n, oh, ow) of this thread's B rows for the CURRENT chunk; advanced by 32 pixels
    // per chunk with a branch-free carry (falls back to division on tiny maps)
    int bn_[BPASS], boh[BPASS], bow[BPASS];
    const int HoWo = a.Ho * a.Wo;
    const int d_oh = 32 / a.Wo, d_ow = 32 - d_oh * a.Wo;
    const bool fast_adv = d_oh + 1 <= a.Ho;
    auto decode = [&](int kc) {
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            int p = p_begin + kc * 32 + bk0 + BKR * j;
            int n = p / HoWo, rem = p - n * HoWo;
            bn_[j] = n;
            boh[j] = rem / a.Wo;
            bow[j] = rem - boh[j] * a.Wo;
        }
    };
    auto advance = [&](int kc) {
        if (MODE == 2) return;
        if (!fast_adv) {
            decode(kc);
            return;
        }
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            int ow = bow[j] + d_ow;
            int c1 = ow >= a.Wo ? 1 : 0;
            bow[j] = ow - (c1 ? a.Wo : 0);
            int oh = boh[j] + d_oh + c1;
            int c2 = oh >= a.Ho ? 1 : 0;
            boh[j] = oh - (c2 ? a.Ho : 0);
            bn_[j] += c2;
        }
    };
    decode(0);

    // Row culling: when every column of this tile belongs to ONE filter tap (kh fixed), output rows whose
    // input row oh*stride + kh*dil - pad is outside the image contribute nothing -- whole 32-pixel chunks
    // inside such rows (the ASPP rates on a 33x33 map) are skipped.
    const int n4_last = (min(n0 + BN, a.Ktot) >> 2) - 1;
    const int tap_last = n4_last / Cin4;
    const int tap_first = (n0 >> 2) / Cin4;
    const int kh_u = tap_first / a.KW;
    const int off_u = kh_u * a.dil - a.pad;
    // valid oh: 0 <= oh*stride + off_u <= H-1
    const int oh_lo = off_u >= 0 ? 0 : (-off_u + a.stride - 1) / a.stride;
    const int oh_hi = (a.H - 1 - off_u) >= 0 ? min(a.Ho - 1, (a.H - 1 - off_u) / a.stride) : -1;
    const bool cull = (tap_first / a.KW == tap_last / a.KW) && (oh_lo > 0 || oh_hi < a.Ho - 1) && HoWo >= 64;
    auto skip = [&](int kc) -> bool {   // block-uniform
        if (!cull) return false;
        const int p0 = p_begin + kc * 32, p1 = min(p0 + 31, p_end - 1);
        const int n0_ = p0 / HoWo, oh0 = (p0 - n0_ * HoWo) / a.Wo;
        const int n1_ = p1 / HoWo, oh1 = (p1 - n1_ * HoWo) / a.Wo;
        if (n0_ == n1_) return oh1 < oh_lo || oh0 > oh_hi;          // rows oh0..oh1 of one image
        if (n1_ == n0_ + 1) return oh0 > oh_hi && oh1 < oh_lo;      // tail of one image + head of the next
        return false;
    };

    float4 ra[APASS], rb[BPASS];
    // All loads are unconditional: rows past the end of the split / outside the image read the zero row
    // (B side), and the A side then only needs a valid address (0 x finite = 0), so it clamps its pixel.
    const float* abase = aok ? a.y + m0 + aq * 4 : g_zero_row;
    const int a_ld = aok ? a.ldy : 0;
    const int shift = dh * a.W + dw;     // MODE 1/2: input pixel = output pixel + shift
    auto gload = [&](int kc) {
#pragma unroll
        for (int j = 0; j < APASS; ++j) {
            int p = min(p_begin + kc * 32 + ak0 + AKR * j, P - 1);
            ra[j] = ldg4(abase + (size_t)p * a_ld);
        }
#pragma unroll
        for (int j = 0; j < BPASS; ++j) {
            int p = p_begin + kc * 32 + bk0 + BKR * j;
            bool ok = bok && p < p_end;
            const float* src;
            if (MODE == 2) {
                src = a.x + (size_t)p * a.ldx + c4 * 4;
            } else if (MODE == 1) {
                int ih = boh[j] + dh, iw = bow[j] + dw;
                ok = ok && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
                src = a.x + (size_t)(p + shift) * a.ldx + c4 * 4;
            } else {
                int ih = boh[j] * a.stride + dh, iw = bow[j] * a.stride + dw;
                ok = ok && (unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W;
                src = a.x + (size_t)((bn_[j] * a.H + ih) * a.W + iw) * a.ldx + c4 * 4;
            }
            rb[j] = ldg4(ok ? src : g_zero_row);
        }
    };
    auto lstore = [&](int buf) {
        if constexpr (X6) {
#pragma unroll
            for (int j = 0; j < APASS; ++j) {
                const int kr = ak0 + AKR * j;
                unsigned char* p = Ax + kr * XPA + ((aq * 8) ^ ((kr & 3) * SWA));
                if constexpr (NP == 1) {
                    *reinterpret_cast<uint2*>(p) = round_bf16x4(ra[j]);
                } else {
                    uint2 h, m, l;
                    split3(ra[j], h, m, l);
                    *reinterpret_cast<uint2*>(p) = h;
                    *reinterpret_cast<uint2*>(p + XPLA) = m;
                    *reinterpret_cast<uint2*>(p + 2 * XPLA) = l;
                }
            }
#pragma unroll
            for (int j = 0; j < BPASS; ++j) {
                const int kr = bk0 + BKR * j;
                unsigned char* p = Bx + kr * XPB + ((bq * 8) ^ ((kr & 3) * SWB));
                if constexpr (NP == 1) {
                    *reinterpret_cast<uint2*>(p) = round_bf16x4(rb[j]);
                } else {
                    uint2 h, m, l;
                    split3(rb[j], h, m, l);
                    *reinterpret_cast<uint2*>(p) = h;
                    *reinterpret_cast<uint2*>(p + XPLB) = m;
                    *reinterpret_cast<uint2*>(p + 2 * XPLB) = l;
                }
            }
        } else {
#pragma unroll
            for (int j = 0; j < APASS; ++j)
                *reinterpret_cast<float4*>(&As[(buf * 32 + ak0 + AKR * j) * BM + aq * 4]) = ra[j];
#pragma unroll
            for (int j = 0; j < BPASS; ++j)
                *reinterpret_cast<float4*>(&Bs[(buf * 32 + bk0 + BKR * j) * BN + bq * 4]) = rb[j];
        }
    };

    f32x16 acc[MB][NB];
#pragma unroll
    for (int i = 0; i < MB; ++i)
#pragma unroll
        for (int j = 0; j < NB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

    const int nK = (p_end - p_begin + 31) >> 5;
    int kc = 0;
    bool first = true;
    auto next = [&]() -> bool {   // move to the next chunk that has work (coordinates follow kc)
        for (;;) {
            if (!first) {
                ++kc;
                if (kc < nK) advance(kc);
            }
            first = false;
            if (kc >= nK) return false;
            if (!skip(kc)) return true;
        }
    };
    if constexpr (X6) {
        // transposing-read lane roles: 16-lane group g = lane>>4 covers rows 16*(g&1).. of the 32-row MFMA tile
        // for k half h = g>>1; lane 4q+p of the group addresses k-row q, columns 4p..4p+3
        const int tg = lane >> 4, ti = lane & 15, tq = ti >> 2, tp = ti & 3;
        const int th = tg >> 1, tc = (tg & 1) * 16 + tp * 4;
        typedef short s16x4 __attribute__((ext_vector_type(4)));
        typedef __attribute__((address_space(3))) s16x4* lds_s16x4;
        auto tr_frag = [&](const unsigned char* plane, int pitch, int sw, int col0, int ks) -> uint4 {
            const unsigned char* p = plane + (ks * 16 + th * 8 + tq) * pitch + (((col0 + tc) * 2) ^ (tq * sw));
            s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p));
            s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p + 4 * pitch));
            uint2 a2 = __builtin_bit_cast(uint2, lo), b2 = __builtin_bit_cast(uint2, hi);
            return make_uint4(a2.x, a2.y, b2.x, b2.y);
        };
        bool more = next();
        if (more) gload(kc);
        while (more) {
            lstore(0);
            __syncthreads();
            const bool more2 = next();
            if (more2) gload(kc);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                uint4 ah[MB], am[MB], al[MB], bh[NB], bm[NB], bl[NB];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    const int c0 = wm * (BM / 2) + mb * 32;
                    ah[mb] = tr_frag(Ax, XPA, SWA, c0, ks);
                    if constexpr (NP == 3) {
                        am[mb] = tr_frag(Ax + XPLA, XPA, SWA, c0, ks);
                        al[mb] = tr_frag(Ax + 2 * XPLA, XPA, SWA, c0, ks);
                    }
                }
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int c0 = wn * (BN / 2) + nb * 32;
                    bh[nb] = tr_frag(Bx, XPB, SWB, c0, ks);
                    if constexpr (NP == 3) {
                        bm[nb] = tr_frag(Bx + XPLB, XPB, SWB, c0, ks);
                        bl[nb] = tr_frag(Bx + 2 * XPLB, XPB, SWB, c0, ks);
                    }
                }
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        f32x16 c = acc[mb][nb];
                        if constexpr (NP == 3) {
                            c = mfma_bf16(al[mb], bh[nb], c);
                            c = mfma_bf16(ah[mb], bl[nb], c);
                            c = mfma_bf16(am[mb], bm[nb], c);
                            c = mfma_bf16(am[mb], bh[nb], c);
                            c = mfma_bf16(ah[mb], bm[nb], c);
                        }
                        c = mfma_bf16(ah[mb], bh[nb], c);
                        acc[mb][nb] = c;
                    }
            }
            __syncthreads();
            more = more2;
        }
    } else {
        bool more = next();
        if (more) {
            gload(kc);
            lstore(0);
        }
        __syncthreads();
        int cur = 0;
        while (more) {
            const bool more2 = next();
            if (more2) gload(kc);
            const float* Ab = &As[(cur * 32 + lh * 4) * BM + wm * (BM / 2) + li];
            const float* Bb = &Bs[(cur * 32 + lh * 4) * BN + wn * (BN / 2) + li];
    #pragma unroll
            for (int g = 0; g < 4; ++g) {
                float af[MB][4], bf[NB][4];
    #pragma unroll
                for (int mb = 0; mb < MB; ++mb)
    #pragma unroll
                    for (int j = 0; j < 4; ++j) af[mb][j] = Ab[(g * 8 + j) * BM + mb * 32];
    #pragma unroll
                for (int nb = 0; nb < NB; ++nb)
    #pragma unroll
                    for (int j = 0; j < 4; ++j) bf[nb][j] = Bb[(g * 8 + j) * BN + nb * 32];
    #pragma unroll
                for (int j = 0; j < 4; ++j)
    #pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
    #pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = mfma32(af[mb][j], bf[nb][j], acc[mb][nb]);
            }
            if (more2) lstore(cur ^ 1);
            __syncthreads();
            cur ^= 1;
            more = more2;
        }
    }
    float* out = a.stats + (size_t)split * a.Cout * a.Ktot;  // slab (or dw itself when nsplit == 1)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int col = n0 + wn * (BN / 2) + nb * 32 + li;
        const bool cok = col < a.Ktot;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                int row = m0 + wm * (BM / 2) + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                if (cok && row < a.Cout) out[(size_t)row * a.Ktot + col] = acc[mb][nb][r];
            }
    }
}

__global__ void k_reduce_slabs(const float* __restrict__ slabs, float* __restrict__ dst, int64_t n4,
                               int nsplit) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4;
         i += (int64_t)gridDim.x * blockDim.x) {
        // a small weight (a 1x1 on a large map: 4 096 float4, 64-128 splits) leaves each thread a long chain of dependent
        // round trips: eight loads in flight per thread, summed in the fixed order 1, 2, 3, ...
        const float4* p = reinterpret_cast<const float4*>(slabs) + i;
        float4 s = p[0];
        int k = 1;
        for (; k + 7 < nsplit; k += 8) {
            float4 v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = p[(int64_t)(k + u) * n4];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                s.x += v[u].x;
                s.y += v[u].y;
                s.z += v[u].z;
                s.w += v[u].w;
            }
        }
        for (; k < nsplit; ++k) {
            const float4 v = p[(int64_t)k * n4];
            s.x += v.x;
            s.y += v.y;
            s.z += v.z;
            s.w += v.w;
        }
        reinterpret_cast<float4*>(dst)[i] = s;
    }
}

void launch_reduce_slabs(const float* slabs, float* dst, int64_t n4, int nsplit, hipStream_t s) {
    hipLaunchKernelGGL(k_reduce_slabs, dim3(stream_grid(n4, 256)), dim3(256), 0, s, slabs, dst, n4, nsplit);
}

// The three launchers the entry points (conv_api.hip) need; the tile width / plan is the caller's.
void launch_conv_fwd_f32(ConvArgs a, hipStream_t s, int bn) {
    a.MT = (a.M + 127) / 128;
    a.NT = (a.Cout + bn - 1) / bn;
    if (bn == 64) hipLaunchKernelGGL(k_conv_fwd<64>, dim3(a.MT * a.NT), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_conv_fwd<128>, dim3(a.MT * a.NT), dim3(256), 0, s, a);
}

void launch_conv_dgrad_f32(ConvArgs a, hipStream_t s, int bn) {
    a.MT = (a.M + 127) / 128;
    a.NT = (a.Cin + bn - 1) / bn;
    if (bn == 64) hipLaunchKernelGGL(k_conv_dgrad<64>, dim3(a.MT * a.NT), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(k_conv_dgrad<128>, dim3(a.MT * a.NT), dim3(256), 0, s, a);
}

// a.stats: the slabs (p.nsplit > 1) or dw itself
void launch_conv_wgrad(ConvArgs a, hipStream_t s, const WgPlan& p) {
    a.MT = p.MT; a.NT = p.NT; a.nsplit = p.nsplit; a.psplit = p.psplit;
    dim3 grid(p.MT * p.NT, p.nsplit);
    const int mode = p.mode;
    const bool x6 = p.x6, one = p.planes == 1;
#define WLAUNCH(BM_, BN_, X_, NP_)                                                                          \
    do {                                                                                                    \
        if (mode == 2) hipLaunchKernelGGL((k_conv_wgrad<BM_, BN_, 2, X_, NP_>), grid, dim3(256), 0, s, a);      \
        else if (mode == 1) hipLaunchKernelGGL((k_conv_wgrad<BM_, BN_, 1, X_, NP_>), grid, dim3(256), 0, s, a); \
        else hipLaunchKernelGGL((k_conv_wgrad<BM_, BN_, 0, X_, NP_>), grid, dim3(256), 0, s, a);                \
    } while (0)
    if (p.bm == 128 && one) WLAUNCH(128, 128, true, 1);
    else if (p.bm == 128 && x6) WLAUNCH(128, 128, true, 3);
    else if (p.bm == 128) WLAUNCH(128, 128, false, 3);
    else if (one) WLAUNCH(64, 64, true, 1);
    else if (x6) WLAUNCH(64, 64, true, 3);
    else WLAUNCH(64, 64, false, 3);
#undef WLAUNCH
}

}  // namespace iswm
