// Lovasz-Softmax (Berman et al. 2018), per image, next to the weighted CE: the criterion that is the convex extension of the
// Jaccard loss itself.  Its gradient hangs on the ORDER of the per-class errors, so this file holds a segmented sort.
//   V_b = valid pixels of image b (valid_label), p = softmax(z) (log_softmax), g_ic = [y_i == c], S = the classes >= 1 or all
//   e_ic = |g_ic - p_ic| in [0, 1];  G_bc = sum_i g_ic;  segment (b, c in S) is PRESENT iff G_bc > 0
//   order: descending e; among equal e, g = 1 before g = 0; then ascending pixel index; valid pixels only
//   at sorted position j:  cg_j = #{g = 1 at positions <= j},  U_j = G + (j + 1 - cg_j),  I_j = G - cg_j
//   omega_j = 1 / U_j (g = 1)  or  I_j / ((U_j - 1) U_j) (g = 0):  the Jaccard increments J_j - J_{j-1} in closed form -- integers
//             up to one division; the difference of two fp32 numbers near 1 would lose every digit at 2e5 pixels
//   L_bc = sum_j e_(j) omega_j;   N = number of present segments
//   L = lambda_ce sum_V w nll / sum_V w + lambda_lv (sum_present L_bc) / N
// Stages (every dependency between workgroups is a kernel boundary; no kernel waits on another workgroup):
//   k_lovasz_keys     logits + labels -> uint32 key per (segment, pixel): ((bits(e) << 1) | g) + 1, 0 at an invalid pixel; the CE
//                     partials in k_loss_fwd's order.  Non-negative floats order as their bits and e <= 1 keeps bits(e) < 2^30, so
//                     the key orders by (e, then g) and the invalid pixels fall to the end of a descending sort.
//   k_lovasz_count    keys -> per segment {valid pixels, G} (integer atomics on zeroed counters: exact in any order)
//   sort              stable descending LSD radix sort of every segment, LV_DIGITS digits of 8 bits, pixel index as payload:
//                     per digit  k_lv_digit_count (tile x bin table), k_lv_digit_scan (one workgroup per segment: exclusive
//                     scan in (bin, tile) order), k_lv_scatter.  The rank of a key inside its tile comes from wave ballots
//                     (lanes of equal digit, in lane order) and wave-private LDS counters: equal digits keep their input order,
//                     no atomic returns a rank, and a hot bin costs no more than a cold one.
//   weights           k_lv_gcount / k_lv_gscan / k_lv_apply: segmented integer scan of the sorted keys' g bits, omega_j by the
//                     closed form, m[segment, perm[j]] = omega_j (0 at invalid pixels and in absent segments), per-tile partials
//                     of sum e omega; k_lv_finalize: fixed order, double -> {sum_present L_bc, N}
//   k_lv_loss         {CE sums, sum L_bc, N} -> {loss, lambda_ce / sum w, lambda_lv / N}
//   k_lovasz_bwd      logits + labels + m -> the finished gradient, once
// Per pixel and class in S at C = 2, uint8 labels: keys 9 B read + 4 written, count 4, four digits x (4 read to count + 8 read and
// 8 written to scatter; the first reads 4) = 76, weights 4 + 8 read + 4 written, backward 9 + 4 read + 8 written: 130 B.
#include "loss_common.h"

namespace iswm {

constexpr int LV_DIGITS = 4, LV_BINS = 256, LV_KPT = 16, LV_TILE = 256 * LV_KPT, LV_SPAN = LV_TILE / 4;
constexpr int64_t LV_PMAX = (int64_t)1 << 24;

__device__ __forceinline__ bool key_g(uint32_t key) { return key != 0u && (key & 1u) == 0u; }      // ((.. | g) + 1): g = 1 is even
__device__ __forceinline__ float key_e(uint32_t key) { return __uint_as_float((key - 1u) >> 1); }

template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_lovasz_keys(const float* __restrict__ logits, const LabelT* __restrict__ labels, int Crt,
                                                     int64_t HW, int64_t npix, const float* __restrict__ cw, int ignore_index,
                                                     int first, uint32_t* __restrict__ keys, float* __restrict__ partials,
                                                     int nblocks) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const int nS = C - first;
    __shared__ float red[2][4];
    float s1 = 0.f, s2 = 0.f;
    // gather_pixels, loss_pixel and block_reduce as in k_loss_fwd: the two CE partials are iswm_loss_fwd's bit for bit
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
            const int64_t i = i0 + u * stride, b = i / HW, p = i - b * HW;
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c >= first && c < C) {
                    const float pc = expf(log_softmax(z[u][c], m, lg));
                    const bool g = c == (int)y[u];
                    const float e = fminf(fmaxf(fabsf((g ? 1.f : 0.f) - pc), 0.f), 1.f);        // a NaN becomes 0
                    keys[(b * nS + (c - first)) * HW + p] = valid ? (((__float_as_uint(e) << 1) | (g ? 1u : 0u)) + 1u) : 0u;
                }
        }
    }
    float s[2] = {s1, s2};
    block_reduce(s, red);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = block_total(red[0]);
        partials[nblocks + blockIdx.x] = block_total(red[1]);
    }
}

// one wave's sum of n floats in double: lane l adds p[l], p[l + 64], ... in that order, then a shuffle tree -- k_loss_finalize's
// additions in its order.  The loads are issued 16 at a time: one load per addition is a chain of memory latencies (4112
// partials took 16.6 us in the kernel trace).  The sum is lane 0's.
__device__ __forceinline__ double lv_wave_sum(const float* __restrict__ p, int n, int lane) {
    constexpr int DEPTH = 16;
    double a = 0.0;
    int i = lane;
    for (; i + (DEPTH - 1) * 64 < n; i += DEPTH * 64) {
        float v[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) v[k] = p[i + k * 64];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) a += (double)v[k];
    }
    for (; i < n; i += 64) a += (double)p[i];
    for (int o = 32; o > 0; o >>= 1) a += __shfl_down(a, o);
    return a;
}

// block v, one wave: the partials of value v -> sums[v], kept in double
__global__ __launch_bounds__(64) void k_lv_ce_sums(const float* __restrict__ partials, int blocks, double* __restrict__ sums) {
    const double a = lv_wave_sum(partials + (int64_t)blockIdx.x * blocks, blocks, threadIdx.x);
    if (threadIdx.x == 0) sums[blockIdx.x] = a;
}

// counts[seg] = {valid pixels, G}; block (tile, segment).  Integer atomics, return value unused: exact whatever the order.
__global__ __launch_bounds__(256) void k_lovasz_count(const uint32_t* __restrict__ keys, int P, int* __restrict__ counts) {
    __shared__ int red[2][4];
    const int64_t base = (int64_t)blockIdx.y * P;
    int nv = 0, ng = 0;
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int idx = blockIdx.x * LV_TILE + k * 256 + threadIdx.x;
        const uint32_t key = idx < P ? keys[base + idx] : 0u;
        nv += key != 0u ? 1 : 0;
        ng += key_g(key) ? 1 : 0;
    }
    int s[2] = {nv, ng};
    block_reduce(s, red);
    if (threadIdx.x == 0) {
        const int tv = block_total(red[0]), tg = block_total(red[1]);
        if (tv) atomicAdd(&counts[2 * blockIdx.y], tv);
        if (tg) atomicAdd(&counts[2 * blockIdx.y + 1], tg);
    }
}

// ---- the sort ---------------------------------------------------------------------------------------------------------------
// A tile is LV_TILE consecutive keys of one segment; wave w of the workgroup owns the LV_SPAN keys w * LV_SPAN .. and reads them 64
// at a time, so the order inside a tile is (wave, round, lane) = the input order.  The digit is taken inverted (255 - d): an
// ascending stable sort of the inverted digits is the descending stable sort asked for.
__device__ __forceinline__ uint32_t lv_digit(uint32_t key, int shift) { return 255u - ((key >> shift) & 255u); }

// the lanes of the wave that hold the same digit as this one (among the lanes with ok); 64-bit: the wave is 64 wide
__device__ __forceinline__ unsigned long long lv_match(uint32_t d, bool ok) {
    unsigned long long m = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const unsigned long long bb = __ballot(bit);
        m &= bit ? bb : ~bb;
    }
    return m;
}

// table[segment][tile][bin] = the tile's count of every (inverted) digit
__global__ __launch_bounds__(256) void k_lv_digit_count(const uint32_t* __restrict__ keys, int P, int ntiles, int shift,
                                                        uint32_t* __restrict__ table) {
    __shared__ uint32_t wh[4][LV_BINS];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int k = 0; k < 4; ++k) wh[k][t] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.y * P;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int k = 0; k < LV_KPT; ++k) {
        const int idx = blockIdx.x * LV_TILE + w * LV_SPAN + k * 64 + lane;
        const bool ok = idx < P;
        const uint32_t d = lv_digit(ok ? keys[base + idx] : 0u, shift);
        const unsigned long long m = lv_match(d, ok);
        if (ok && (m & lt) == 0ull) wh[w][d] += (uint32_t)__popcll(m);      // the group's first lane; row w is this wave's alone
        __syncthreads();
    }
    table[((int64_t)blockIdx.y * ntiles + blockIdx.x) * LV_BINS + t] = (wh[0][t] + wh[1][t]) + (wh[2][t] + wh[3][t]);
}

// one workgroup per segment, thread t = bin t: the exclusive scan of the table in (bin, tile) order, in place.  Integers: exact.
__global__ __launch_bounds__(256) void k_lv_digit_scan(uint32_t* __restrict__ table, int ntiles) {
    __shared__ uint32_t tot[2][LV_BINS];
    const int t = threadIdx.x;
    uint32_t* T = table + (int64_t)blockIdx.x * ntiles * LV_BINS;
    constexpr int DEPTH = 8;                            // loads in flight per thread: one load per addition is a latency chain
    uint32_t mine = 0u;
    int i = 0;
    for (; i + DEPTH <= ntiles; i += DEPTH) {
        uint32_t v[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) v[k] = T[(int64_t)(i + k) * LV_BINS + t];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) mine += v[k];
    }
    for (; i < ntiles; ++i) mine += T[(int64_t)i * LV_BINS + t];
    tot[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < LV_BINS; o <<= 1) {
        tot[cur ^ 1][t] = tot[cur][t] + (t >= o ? tot[cur][t - o] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = tot[cur][t] - mine;
    for (i = 0; i + DEPTH <= ntiles; i += DEPTH) {
        uint32_t v[DEPTH];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) v[k] = T[(int64_t)(i + k) * LV_BINS + t];
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            T[(int64_t)(i + k) * LV_BINS + t] = run;
            run += v[k];
        }
    }
    for (; i < ntiles; ++i) {
        const uint32_t v = T[(int64_t)i * LV_BINS + t];
        T[(int64_t)i * LV_BINS + t] = run;
        run += v;
    }
}

// perm_in == nullptr: the first pass, the payload is the key's own index in its segment
__global__ __launch_bounds__(256) void k_lv_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ perm_in, int P,
                                                    int ntiles, int shift, const uint32_t* __restrict__ table,
                                                    uint32_t* __restrict__ keys_out, uint32_t* __restrict__ perm_out) {
    __shared__ uint32_t wh[4][LV_BINS], tot[2][LV_BINS], delta[LV_BINS], lkey[LV_TILE], lperm[LV_TILE];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    for (int k = 0; k < 4; ++k) wh[k][t] = 0u;
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.y * P;
    const unsigned long long lt = (1ull << lane) - 1ull;
    uint32_t key[LV_KPT], rank[LV_KPT];
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int idx = blockIdx.x * LV_TILE + w * LV_SPAN + k * 64 + lane;
        const bool ok = idx < P;
        key[k] = ok ? keys_in[base + idx] : 0u;
        const uint32_t d = lv_digit(key[k], shift);
        const unsigned long long m = lv_match(d, ok);
        const uint32_t before = wh[w][d];                                   // this wave's earlier rounds
        __syncthreads();
        if (ok && (m & lt) == 0ull) wh[w][d] = before + (uint32_t)__popcll(m);
        __syncthreads();
        rank[k] = before + (uint32_t)__popcll(m & lt);
    }
    // The tile is put in order in LDS first and written from there: slot s of the ordered tile goes to the address that follows
    // slot s - 1's wherever both hold the same digit, so a wave's stores are runs (16 keys per bin on average) instead of 64
    // single words -- written straight from the registers, the three passes over the low digits took 80 us each where the
    // pass over the top digit (a few bins) took 31.
    //   tot      exclusive scan over the bins of the tile's counts: where a bin starts in the ordered tile
    //   wh[w]    that plus the earlier waves' counts: where wave w's keys of the bin start
    //   delta    the scanned table's entry minus tot: slot s of bin d goes to delta[d] + s (unsigned wrap-around is fine)
    {
        const uint32_t c0 = wh[0][t], c1 = wh[1][t], c2 = wh[2][t], c3 = wh[3][t];
        const uint32_t mine = (c0 + c1) + (c2 + c3);
        tot[0][t] = mine;
        __syncthreads();
        int cur = 0;
        for (int o = 1; o < LV_BINS; o <<= 1) {
            tot[cur ^ 1][t] = tot[cur][t] + (t >= o ? tot[cur][t - o] : 0u);
            cur ^= 1;
            __syncthreads();
        }
        const uint32_t start = tot[cur][t] - mine;
        wh[0][t] = start;
        wh[1][t] = start + c0;
        wh[2][t] = start + c0 + c1;
        wh[3][t] = start + c0 + c1 + c2;
        delta[t] = table[((int64_t)blockIdx.y * ntiles + blockIdx.x) * LV_BINS + t] - start;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int idx = blockIdx.x * LV_TILE + w * LV_SPAN + k * 64 + lane;
        if (idx < P) {
            const uint32_t slot = wh[w][lv_digit(key[k], shift)] + rank[k];
            if (slot < (uint32_t)LV_TILE) {
                lkey[slot] = key[k];
                lperm[slot] = perm_in ? perm_in[base + idx] : (uint32_t)idx;
            }
        }
    }
    __syncthreads();
    const int here = P - blockIdx.x * LV_TILE < LV_TILE ? P - blockIdx.x * LV_TILE : LV_TILE;       // keys in this tile
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int slot = k * 256 + t;
        if (slot < here) {
            const uint32_t ks = lkey[slot];
            const uint32_t pos = delta[lv_digit(ks, shift)] + (uint32_t)slot;
            if (pos < (uint32_t)P) {
                keys_out[base + pos] = ks;
                perm_out[base + pos] = lperm[slot];
            }
        }
    }
}

// ---- the Jaccard weights --------------------------------------------------------------------------------------------------------
// tcount[segment][tile] = the tile's number of g = 1 keys (tiles of the SORTED keys, LV_TILE positions each)
__global__ __launch_bounds__(256) void k_lv_gcount(const uint32_t* __restrict__ sorted, int P, int ntiles, uint32_t* __restrict__ tcount) {
    __shared__ int red[1][4];
    const int64_t base = (int64_t)blockIdx.y * P;
    int ng = 0;
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int idx = blockIdx.x * LV_TILE + k * 256 + threadIdx.x;
        ng += (idx < P && key_g(sorted[base + idx])) ? 1 : 0;
    }
    int s[1] = {ng};
    block_reduce(s, red);
    if (threadIdx.x == 0) tcount[(int64_t)blockIdx.y * ntiles + blockIdx.x] = (uint32_t)block_total(red[0]);
}

// one workgroup per segment: exclusive scan over the tiles, in place; thread t takes a contiguous run of tiles
__global__ __launch_bounds__(256) void k_lv_gscan(uint32_t* __restrict__ tcount, int ntiles) {
    __shared__ uint32_t tot[2][256];
    const int t = threadIdx.x, per = (ntiles + 255) / 256;
    uint32_t* T = tcount + (int64_t)blockIdx.x * ntiles;
    const int lo = t * per, hi = lo + per < ntiles ? lo + per : ntiles;
    uint32_t mine = 0u;
    for (int i = lo; i < hi; ++i) mine += T[i];
    tot[0][t] = mine;
    __syncthreads();
    int cur = 0;
    for (int o = 1; o < 256; o <<= 1) {
        tot[cur ^ 1][t] = tot[cur][t] + (t >= o ? tot[cur][t - o] : 0u);
        cur ^= 1;
        __syncthreads();
    }
    uint32_t run = tot[cur][t] - mine;
    for (int i = lo; i < hi; ++i) {
        const uint32_t v = T[i];
        T[i] = run;
        run += v;
    }
}

// thread t takes the LV_KPT consecutive positions t * LV_KPT .. of the tile: a running count in the thread, an exclusive scan of
// the threads' totals across the workgroup (shuffles inside a wave, the four wave totals through LDS), the tile's offset on top
__global__ __launch_bounds__(256) void k_lv_apply(const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ perm, int P,
                                                  int ntiles, const uint32_t* __restrict__ tcount, const int* __restrict__ counts,
                                                  float* __restrict__ m, float* __restrict__ partials) {
    __shared__ uint32_t wtot[4];
    __shared__ float red[1][4];
    const int t = threadIdx.x, w = t >> 6, lane = t & 63;
    const int64_t base = (int64_t)blockIdx.y * P;
    const uint32_t G = (uint32_t)counts[2 * blockIdx.y + 1];
    uint32_t key[LV_KPT], mine = 0u;
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int j = blockIdx.x * LV_TILE + t * LV_KPT + k;
        key[k] = j < P ? sorted[base + j] : 0u;
        mine += key_g(key[k]) ? 1u : 0u;
    }
    uint32_t incl = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t v = __shfl_up(incl, o);
        incl += lane >= o ? v : 0u;
    }
    if (lane == 63) wtot[w] = incl;
    __syncthreads();
    uint32_t cg = tcount[(int64_t)blockIdx.y * ntiles + blockIdx.x] + (incl - mine);
    for (int k = 0; k < w; ++k) cg += wtot[k];
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < LV_KPT; ++k) {
        const int j = blockIdx.x * LV_TILE + t * LV_KPT + k;
        if (j >= P) continue;
        const bool g = key_g(key[k]);
        cg += g ? 1u : 0u;
        float om = 0.f;
        if (key[k] != 0u && G > 0u) {                                       // a valid pixel of a present segment
            const unsigned long long U = (unsigned long long)G + ((unsigned long long)j + 1ull - cg), I = G - cg;
            om = g ? (float)(1.0 / (double)U) : (float)((double)I / (double)((U - 1ull) * U));   // g = 0: U - 1 >= G > 0
            acc = fmaf(key_e(key[k]), om, acc);
        }
        const uint32_t pi = perm[base + j];
        if (pi < (uint32_t)P) m[base + pi] = om;
    }
    float s[1] = {acc};
    block_reduce(s, red);
    if (t == 0) partials[(int64_t)blockIdx.y * ntiles + blockIdx.x] = block_total(red[0]);
}

// one workgroup of 16 waves, 16 segments at a time: wave w sums the tiles' partials of its segment in double (lv_wave_sum: fixed
// order), thread 0 adds the present segments in segment order -> out = {sum_present L_bc, N}
__global__ __launch_bounds__(1024) void k_lv_finalize(const float* __restrict__ partials, const int* __restrict__ counts, int nseg,
                                                      int ntiles, double* __restrict__ out) {
    __shared__ double part[16];
    __shared__ int on[16];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc = 0.0, n = 0.0;
    for (int s0 = 0; s0 < nseg; s0 += 16) {
        const int s = s0 + w;
        const double a = s < nseg ? lv_wave_sum(partials + (int64_t)s * ntiles, ntiles, lane) : 0.0;
        if (lane == 0) {
            part[w] = a;
            on[w] = s < nseg && counts[2 * s + 1] > 0;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int k = 0; k < 16; ++k)
                if (on[k]) {
                    acc += part[k];
                    n += 1.0;
                }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = acc;
        out[1] = n;
    }
}

// sums = {sum w nll, sum w, sum_present L_bc, N} -> out = {loss, lambda_ce / sum w, lambda_lv / N}; a term whose normaliser is 0
// (no valid pixel, no present segment) is 0 and so is its coefficient
__global__ void k_lv_loss(const double* __restrict__ sums, double lce, double llv, float* __restrict__ out) {
    const bool ce = lce != 0.0 && sums[1] > 0.0, lv = llv != 0.0 && sums[3] > 0.0;
    out[0] = (float)((ce ? lce * (sums[0] / sums[1]) : 0.0) + (lv ? llv * (sums[2] / sums[3]) : 0.0));
    out[1] = ce ? (float)(lce / sums[1]) : 0.f;
    out[2] = lv ? (float)(llv / sums[3]) : 0.f;
}

// for valid i:  dL/dz_ik = upstream [ coef[0] w_y (p_ik - g_ik) + coef[1] (q_ik - p_ik sum_c q_ic) ],  q_ic = m_ic (1 - 2 g_ic) p_ic
// over c in S (m is 0 in an absent segment);  else 0
template <typename LabelT, int CT>
__global__ __launch_bounds__(256) void k_lovasz_bwd(const float* __restrict__ logits, const LabelT* __restrict__ labels, int Crt,
                                                    int64_t HW, int64_t npix, const float* __restrict__ cw, int ignore_index,
                                                    int first, const float* __restrict__ mw, const float* __restrict__ coef,
                                                    const float* __restrict__ upstream, float* __restrict__ grad) {
    constexpr int UNR = LOSS_UNR, CMAX = CT > 0 ? CT : OVL_CMAX;
    const int C = CT > 0 ? CT : Crt;
    const int nS = C - first;
    const float up = upstream[0], a = coef[0], lv = coef[1];
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
            const int64_t i = i0 + u * stride, b = i / HW, p = i - b * HW;
            float m = z[u][0];
#pragma unroll
            for (int c = 1; c < CMAX; ++c) m = c < C ? fmaxf(m, z[u][c]) : m;
            float se = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) se += c < C ? expf(z[u][c] - m) : 0.f;
            const float lg = logf(se);
            const float aw = valid ? a * (cw ? cw[yy] : 1.f) : 0.f;
            float pc[CMAX], q[CMAX], dot = 0.f;
#pragma unroll
            for (int c = 0; c < CMAX; ++c) {
                pc[c] = c < C ? expf(log_softmax(z[u][c], m, lg)) : 0.f;
                const float mc = (valid && c >= first && c < C) ? mw[(b * nS + (c - first)) * HW + p] : 0.f;
                q[c] = (c == (int)yy ? -mc : mc) * pc[c];
                dot += q[c];
            }
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) {
                    const float g = c == (int)yy ? 1.f : 0.f;
                    grad[off[u] + c * HW] = valid ? up * (aw * (pc[c] - g) + lv * (q[c] - pc[c] * dot)) : 0.f;
                }
        }
    }
}

}  // namespace iswm

using namespace iswm;

static const char* const LOVASZ_TAKES = "the Lovasz loss takes";
static int64_t lv_align(int64_t bytes) { return (bytes + 255) & ~(int64_t)255; }
static int lv_tiles(int64_t P) { return (int)((P + LV_TILE - 1) / LV_TILE); }

// the sizes the sort takes: 1 <= P <= 2^24 keys per segment, nseg * P < 2^31, nseg within one grid dimension
static int refuse_segments(const char* fn, int64_t nseg, int64_t P) {
    ISWM_REQUIRE(P >= 1 && P <= LV_PMAX, "%s: %lld keys per segment (the sort takes 1 to %lld)", fn, (long long)P, (long long)LV_PMAX);
    ISWM_REQUIRE(nseg >= 1 && nseg <= 65535 && nseg * P < ((int64_t)1 << 31),
                 "%s: %lld segments of %lld keys (at most 65535 segments and fewer than 2^31 keys in all)", fn, (long long)nseg,
                 (long long)P);
    return 0;
}
static int refuse_classes(const char* fn, int classes, int C) {
    ISWM_REQUIRE(classes == 0 || classes == 1, "%s: classes is 0 (foreground) or 1 (all)", fn);
    ISWM_REQUIRE(classes == 1 || C >= 2, "%s: no foreground class among %d (empty class set)", fn, C);
    return 0;
}

extern "C" int iswm_lovasz_digits(void) { return LV_DIGITS; }
extern "C" int iswm_lovasz_tile(void) { return LV_TILE; }

// four key / index buffers of nseg * P words for the ping-pong, then the tile x bin table (the weights stage keeps its tile
// counts and partials in the table's space); 0 with a message for sizes the sort does not take
extern "C" int64_t iswm_lovasz_workspace(int64_t nseg, int64_t P) {
    if (refuse_segments("lovasz_workspace", nseg, P)) return 0;
    return 4 * lv_align(nseg * P * 4) + lv_align(nseg * lv_tiles(P) * (int64_t)LV_BINS * 4);
}

extern "C" int iswm_lovasz_keys(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                                const float* class_weight, int ignore_index, int classes, uint32_t* keys, int32_t* counts,
                                float* partials, double* sums, iswm_stream_t stream) {
    if (refuse_pixel_args("lovasz_keys", logits && labels && keys && counts && partials && sums, B > 0 && HW > 0, C, LOVASZ_TAKES,
                          label_bytes)) return 1;
    if (refuse_classes("lovasz_keys", classes, C)) return 1;
    const int first = classes ? 0 : 1;
    const int64_t nseg = (int64_t)B * (C - first);
    if (refuse_segments("lovasz_keys", nseg, HW)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_lovasz_keys<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C, HW,
                           npix, class_weight, ignore_index, first, keys, partials, blocks);
    });
    hipLaunchKernelGGL(k_lv_ce_sums, dim3(2), dim3(64), 0, s, partials, blocks, sums);
    if (hipMemsetAsync(counts, 0, (size_t)nseg * 2 * sizeof(int32_t), s) != hipSuccess) return check_launch("lovasz_keys");
    hipLaunchKernelGGL(k_lovasz_count, dim3(lv_tiles(HW), (int)nseg), dim3(256), 0, s, keys, (int)HW, counts);
    return check_launch("lovasz_keys");
}

extern "C" int iswm_lovasz_sort(const uint32_t* keys, int64_t nseg, int64_t P, void* workspace, int64_t workspace_bytes,
                                uint32_t* sorted, uint32_t* perm, iswm_stream_t stream) {
    ISWM_REQUIRE(keys && workspace && sorted && perm, "lovasz_sort: null pointer");
    ISWM_REQUIRE(keys != sorted, "lovasz_sort: sorted must not be the input");
    if (refuse_segments("lovasz_sort", nseg, P)) return 1;
    ISWM_REQUIRE(workspace_bytes >= iswm_lovasz_workspace(nseg, P), "lovasz_sort: workspace of %lld bytes, %lld needed",
                 (long long)workspace_bytes, (long long)iswm_lovasz_workspace(nseg, P));
    const int64_t words = lv_align(nseg * P * 4);
    char* ws = (char*)workspace;
    uint32_t* kb[2] = {(uint32_t*)ws, (uint32_t*)(ws + words)};
    uint32_t* pb[2] = {(uint32_t*)(ws + 2 * words), (uint32_t*)(ws + 3 * words)};
    uint32_t* table = (uint32_t*)(ws + 4 * words);
    const int ntiles = lv_tiles(P);
    const dim3 grid(ntiles, (int)nseg);
    hipStream_t s = (hipStream_t)stream;
    const uint32_t *kin = keys, *pin = nullptr;
    for (int d = 0; d < LV_DIGITS; ++d) {
        uint32_t* kout = d == LV_DIGITS - 1 ? sorted : kb[d & 1];
        uint32_t* pout = d == LV_DIGITS - 1 ? perm : pb[d & 1];
        hipLaunchKernelGGL(k_lv_digit_count, grid, dim3(256), 0, s, kin, (int)P, ntiles, 8 * d, table);
        hipLaunchKernelGGL(k_lv_digit_scan, dim3((int)nseg), dim3(256), 0, s, table, ntiles);
        hipLaunchKernelGGL(k_lv_scatter, grid, dim3(256), 0, s, kin, pin, (int)P, ntiles, 8 * d, (const uint32_t*)table, kout, pout);
        kin = kout;
        pin = pout;
    }
    return check_launch("lovasz_sort");
}

extern "C" int iswm_lovasz_weights(const uint32_t* sorted, const uint32_t* perm, const int32_t* counts, int64_t nseg, int64_t P,
                                   void* workspace, int64_t workspace_bytes, float* m, double* out, iswm_stream_t stream) {
    ISWM_REQUIRE(sorted && perm && counts && workspace && m && out, "lovasz_weights: null pointer");
    if (refuse_segments("lovasz_weights", nseg, P)) return 1;
    ISWM_REQUIRE(workspace_bytes >= iswm_lovasz_workspace(nseg, P), "lovasz_weights: workspace of %lld bytes, %lld needed",
                 (long long)workspace_bytes, (long long)iswm_lovasz_workspace(nseg, P));
    const int ntiles = lv_tiles(P);
    char* tbl = (char*)workspace + 4 * lv_align(nseg * P * 4);
    uint32_t* tcount = (uint32_t*)tbl;
    float* partials = (float*)(tbl + lv_align(nseg * ntiles * 4));
    const dim3 grid(ntiles, (int)nseg);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_lv_gcount, grid, dim3(256), 0, s, sorted, (int)P, ntiles, tcount);
    hipLaunchKernelGGL(k_lv_gscan, dim3((int)nseg), dim3(256), 0, s, tcount, ntiles);
    hipLaunchKernelGGL(k_lv_apply, grid, dim3(256), 0, s, sorted, perm, (int)P, ntiles, (const uint32_t*)tcount, counts, m, partials);
    hipLaunchKernelGGL(k_lv_finalize, dim3(1), dim3(1024), 0, s, (const float*)partials, counts, (int)nseg, ntiles, out);
    return check_launch("lovasz_weights");
}

extern "C" int iswm_lovasz_loss(const double* sums, double ce_weight, double lovasz_weight, float* out, iswm_stream_t stream) {
    ISWM_REQUIRE(sums && out, "lovasz_loss: null pointer");
    ISWM_REQUIRE(ce_weight >= 0.0 && lovasz_weight >= 0.0 && ce_weight < INFINITY && lovasz_weight < INFINITY,
                 "lovasz_loss: the term weights must be finite and not negative");
    hipLaunchKernelGGL(k_lv_loss, dim3(1), dim3(1), 0, (hipStream_t)stream, sums, ce_weight, lovasz_weight, out);
    return check_launch("lovasz_loss");
}

extern "C" int iswm_lovasz_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                               const float* class_weight, int ignore_index, int classes, const float* m, const float* coef,
                               const float* upstream, float* grad, iswm_stream_t stream) {
    if (refuse_pixel_args("lovasz_bwd", logits && labels && m && coef && upstream && grad, B > 0 && HW > 0, C, LOVASZ_TAKES,
                          label_bytes)) return 1;
    if (refuse_classes("lovasz_bwd", classes, C)) return 1;
    const int first = classes ? 0 : 1;
    if (refuse_segments("lovasz_bwd", (int64_t)B * (C - first), HW)) return 1;
    const int64_t npix = (int64_t)B * HW;
    const int blocks = iswm_loss_blocks(npix);
    hipStream_t s = (hipStream_t)stream;
    by_label_and_classes(label_bytes, C, [&](auto label, auto ct) {
        using T = decltype(label);
        hipLaunchKernelGGL((k_lovasz_bwd<T, decltype(ct)::value>), dim3(blocks), dim3(256), 0, s, logits, (const T*)labels, C, HW,
                           npix, class_weight, ignore_index, first, m, coef, upstream, grad);
    });
    return check_launch("lovasz_bwd");
}
