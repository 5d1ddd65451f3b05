// Boundary validation metrics: exact distances between the contour of a predicted mask and the contour of its label mask, and
// per (image, class, direction) the statistics boundary F1, ASSD and the percentile Hausdorff distance are formed from
// (include/iswm_hip_bm.h).  One call, four launches, 4 B of workspace per pixel and class plane and nothing else.
//
//   plane (n, c), c in K = {first .. C-1}:  G = {valid, y == c}   P = {valid, pred == c}   valid: by the LABEL alone
//   S(A) = {p in A : some 4-neighbour q inside the image is valid and q not in A}
//
//   k_bm_contours   one thread per image pixel: the two contour bits.  Only the class the pixel's label names can have the pixel
//                   on S(G), only the class its prediction names can have it on S(P), so the 4 neighbours are read once per pixel
//                   and one word per class plane is written: bit 0 = on S(P), bit 1 = on S(G).  A kernel of its own (not folded
//                   into the column sweep): the sweep is a chain of H dependent steps on few threads, and reading two more
//                   columns of two tensors there would triple its loads.
//   k_bm_columns    k_edt_columns of boundary.hip restated on those bits: one thread per (plane, column), a sweep down writes the
//                   vertical distance to the nearest S(P) pixel and to the nearest S(G) pixel at or above the row, a sweep up takes
//                   the minimum with the nearest at or below; two 16-bit fields of one word, BM_NONE = none in the column.  Rows
//                   go in batches of BM_BATCH loads issued before they are used.
//   k_bm_rows       one workgroup per (plane, row): both fields squared into LDS (8 B x W: 32 KiB at W = 4096), then ONLY a pixel
//                   of S(P) searches the S(G) array and only a pixel of S(G) searches the S(P) array: min over x' of
//                   (x - x')^2 + g^2(x'), outward from x, stopping once dx^2 >= best.  A pixel on both contours does both
//                   searches (both give 0).  The row's words are then overwritten in place (the block has its row in LDS):
//                   bit 30 = on S(P), bit 31 = on S(G), bits 0..29 = d2 to the other contour (0 where that contour is empty:
//                   k_bm_finalize sees the emptiness in the counts).  A pixel on both contours has d2 = 0 both ways, so one field
//                   serves.
//   k_bm_finalize   one workgroup of 1024 threads per plane, both directions: a pass over the plane's words takes n, within and max2
//                   (integers), dsum (double: thread t adds its pixels t, t + 1024, .. in that order, the 64 lanes of a wave are
//                   added by a shuffle tree, the 16 wave sums in turn by thread 0 -- no floating-point atomic, the same bits every
//                   run) and the histogram of the top 9 bits of d2; two more passes take the next two 8-bit digits among the keys
//                   that match the digits found so far (the exact radix select of the OHEM criterion, one segment per direction,
//                   histograms in LDS).  The passes after the first are skipped when neither direction has both contours.
//   (x - x')^2 + g^2 <= 2 * 4095^2 < 2^25 and BM_INF + 4095^2 < 2^31: no overflow in 32 bits at sides up to 4096.
#include "loss_common.h"      // valid_label
#include "../../include/iswm_hip_bm.h"

namespace iswm {

constexpr int BM_MAX_SIDE = 4096;
constexpr uint32_t BM_NONE = 0xFFFFu;           // a 16-bit field: no pixel of the contour in this column
constexpr uint32_t BM_INF = 1u << 30;           // a squared field in LDS: the same
constexpr int BM_BATCH = 8;
constexpr uint32_t BM_ON_P = 1u << 30, BM_ON_G = 1u << 31, BM_D2 = (1u << 30) - 1u;      // the word k_bm_rows leaves
constexpr int BM_FIN_THREADS = 1024, BM_FIN_UNR = 8, BM_TOP_BINS = 512;                  // d2 < 2^25: digits of 9, 8 and 8 bits

template <typename PredT, typename LabelT>
__global__ __launch_bounds__(256) void k_bm_contours(const PredT* __restrict__ pred, const LabelT* __restrict__ labels, int C, int H,
                                                     int W, int K, int first, int ignore_index, int64_t npix,
                                                     uint32_t* __restrict__ ws) {
    const int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const int64_t HW = (int64_t)H * W, b = i / HW, p = i - b * HW;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const long long lab = (long long)labels[i], pr = (long long)pred[i];
    bool onP = false, onG = false;
    if (valid_label(lab, C, ignore_index)) {
        const int dy[4] = {-1, 1, 0, 0}, dx[4] = {0, 0, -1, 1};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int yy = y + dy[u], xx = x + dx[u];
            if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
            const int64_t j = i + (int64_t)dy[u] * W + dx[u];
            const long long lq = (long long)labels[j];
            if (!valid_label(lq, C, ignore_index)) continue;
            onG |= lq != lab;
            onP |= (long long)pred[j] != pr;
        }
    }
    for (int k = 0; k < K; ++k) {
        const long long c = first + k;
        ws[(b * K + k) * HW + p] = (onP && pr == c ? 1u : 0u) | (onG && lab == c ? 2u : 0u);
    }
}

__global__ __launch_bounds__(256) void k_bm_columns(uint32_t* __restrict__ ws, int H, int W, int64_t ncols) {
    const int64_t col = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
    if (col >= ncols) return;
    const int64_t plane = col / W;
    const int x = (int)(col - plane * W);
    uint32_t* wp = ws + plane * H * W + x;
    int lastP = -1, lastG = -1;
    for (int y0 = 0; y0 < H; y0 += BM_BATCH) {
        uint32_t v[BM_BATCH];
#pragma unroll
        for (int u = 0; u < BM_BATCH; ++u) v[u] = y0 + u < H ? wp[(int64_t)(y0 + u) * W] : 0u;
#pragma unroll
        for (int u = 0; u < BM_BATCH; ++u) {
            const int y = y0 + u;
            if (y >= H) break;
            if (v[u] & 1u) lastP = y;
            if (v[u] & 2u) lastG = y;
            const uint32_t dP = lastP < 0 ? BM_NONE : (uint32_t)(y - lastP), dG = lastG < 0 ? BM_NONE : (uint32_t)(y - lastG);
            wp[(int64_t)y * W] = dP | (dG << 16);
        }
    }
    int nextP = -1, nextG = -1;
    for (int y0 = H - 1; y0 >= 0; y0 -= BM_BATCH) {
        uint32_t v[BM_BATCH];
#pragma unroll
        for (int u = 0; u < BM_BATCH; ++u) v[u] = y0 - u >= 0 ? wp[(int64_t)(y0 - u) * W] : 0u;
#pragma unroll
        for (int u = 0; u < BM_BATCH; ++u) {
            const int y = y0 - u;
            if (y < 0) break;
            uint32_t dP = v[u] & 0xFFFFu, dG = v[u] >> 16;
            if (dP == 0u) nextP = y;
            if (dG == 0u) nextG = y;
            const uint32_t uP = nextP < 0 ? BM_NONE : (uint32_t)(nextP - y), uG = nextG < 0 ? BM_NONE : (uint32_t)(nextG - y);
            dP = uP < dP ? uP : dP;
            dG = uG < dG ? uG : dG;
            wp[(int64_t)y * W] = dP | (dG << 16);
        }
    }
}

// min over x' of (x - x')^2 + a[x'], outward from x; 0 where the array holds no contour at all
__device__ __forceinline__ uint32_t bm_search(const uint32_t* a, int x, int W) {
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
    return best >= BM_INF ? 0u : best;
}

__global__ __launch_bounds__(256) void k_bm_rows(uint32_t* __restrict__ ws, int W) {
    extern __shared__ uint32_t sq[];            // [0, W): squared distance to S(P) down the column, [W, 2W): to S(G)
    const int64_t base = (int64_t)blockIdx.x * W;
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const uint32_t v = ws[base + x], dP = v & 0xFFFFu, dG = v >> 16;
        sq[x] = dP == BM_NONE ? BM_INF : dP * dP;
        sq[W + x] = dG == BM_NONE ? BM_INF : dG * dG;
    }
    __syncthreads();
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        uint32_t out = 0u;
        if (sq[x] == 0u) out |= BM_ON_P | bm_search(sq + W, x, W);
        if (sq[W + x] == 0u) out |= BM_ON_G | bm_search(sq, x, W);
        ws[base + x] = out;
    }
}

// thread 0's return value is the block's sum: the 64 lanes of each wave by a shuffle tree, the wave sums in turn
__device__ __forceinline__ double bm_block_sum(double v, double* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0)
        for (int w = 0; w < BM_FIN_THREADS / 64; ++w) t += red[w];
    return t;
}

// thread 0: the bin that holds the key of 1-based rank `rank` (1 <= rank <= the histogram's total), and the rank within it
__device__ __forceinline__ uint32_t bm_pick(const uint32_t* hist, int bins, uint32_t& rank) {
    uint32_t below = 0u;
    for (int d = 0; d < bins - 1; ++d) {
        if (below + hist[d] >= rank) {
            rank -= below;
            return (uint32_t)d;
        }
        below += hist[d];
    }
    rank -= below;
    return (uint32_t)(bins - 1);
}

__global__ __launch_bounds__(BM_FIN_THREADS) void k_bm_finalize(const uint32_t* __restrict__ ws, int64_t HW, uint32_t tau2,
                                                                int percent, int64_t* __restrict__ stats,
                                                                double* __restrict__ dsum) {
    __shared__ uint32_t hist[2][BM_TOP_BINS];
    __shared__ double red[2][BM_FIN_THREADS / 64];
    __shared__ int cnt[2][3];                   // n, within, max2
    __shared__ uint32_t prefix[2], rank[2];
    __shared__ int active[2];
    const int tid = threadIdx.x;
    const uint32_t* wp = ws + (int64_t)blockIdx.x * HW;
    const uint32_t flag[2] = {BM_ON_P, BM_ON_G};
    for (int i = tid; i < 2 * BM_TOP_BINS; i += BM_FIN_THREADS) (&hist[0][0])[i] = 0u;
    if (tid < 2) {
        cnt[tid][0] = cnt[tid][1] = 0;
        cnt[tid][2] = -1;
    }
    __syncthreads();
    int n[2] = {0, 0}, within[2] = {0, 0}, mx[2] = {-1, -1};
    double s[2] = {0.0, 0.0};
    for (int64_t i0 = tid; i0 < HW; i0 += (int64_t)BM_FIN_THREADS * BM_FIN_UNR) {
        uint32_t v[BM_FIN_UNR];
#pragma unroll
        for (int u = 0; u < BM_FIN_UNR; ++u) {
            const int64_t i = i0 + (int64_t)u * BM_FIN_THREADS;
            v[u] = i < HW ? wp[i] : 0u;
        }
#pragma unroll
        for (int u = 0; u < BM_FIN_UNR; ++u) {
            if (!(v[u] & (BM_ON_P | BM_ON_G))) continue;
            const uint32_t d2 = v[u] & BM_D2;
            const double root = sqrt((double)d2);
#pragma unroll
            for (int dir = 0; dir < 2; ++dir)
                if (v[u] & flag[dir]) {
                    n[dir] += 1;
                    within[dir] += d2 <= tau2 ? 1 : 0;
                    mx[dir] = (int)d2 > mx[dir] ? (int)d2 : mx[dir];
                    s[dir] += root;
                    atomicAdd(&hist[dir][d2 >> 16], 1u);
                }
        }
    }
#pragma unroll
    for (int dir = 0; dir < 2; ++dir)
        if (n[dir]) {
            atomicAdd(&cnt[dir][0], n[dir]);
            atomicAdd(&cnt[dir][1], within[dir]);
            atomicMax(&cnt[dir][2], mx[dir]);
        }
    const double total[2] = {bm_block_sum(s[0], red[0]), bm_block_sum(s[1], red[1])};       // (each ends in a barrier: cnt is whole)
    if (tid == 0) {
        for (int dir = 0; dir < 2; ++dir) {
            int64_t* st = stats + ((int64_t)blockIdx.x * 2 + dir) * 4;
            const bool both = cnt[dir][0] > 0 && cnt[1 - dir][0] > 0;
            st[0] = cnt[dir][0];
            st[1] = both ? cnt[dir][1] : 0;
            st[2] = both ? cnt[dir][2] : -1;
            st[3] = -1;
            dsum[(int64_t)blockIdx.x * 2 + dir] = both ? total[dir] : 0.0;
            active[dir] = both ? 1 : 0;
            if (both) {
                rank[dir] = (uint32_t)(((int64_t)percent * cnt[dir][0] + 99) / 100);
                prefix[dir] = bm_pick(hist[dir], BM_TOP_BINS, rank[dir]);
            }
        }
    }
    __syncthreads();
    if (!active[0] && !active[1]) return;
    for (int shift = 8; shift >= 0; shift -= 8) {                                           // the digits of bits 8..15, then 0..7
        for (int i = tid; i < 2 * BM_TOP_BINS; i += BM_FIN_THREADS) (&hist[0][0])[i] = 0u;
        __syncthreads();
        const uint32_t want[2] = {prefix[0], prefix[1]};
        const bool on[2] = {active[0] != 0, active[1] != 0};
        for (int64_t i0 = tid; i0 < HW; i0 += (int64_t)BM_FIN_THREADS * BM_FIN_UNR) {
            uint32_t v[BM_FIN_UNR];
#pragma unroll
            for (int u = 0; u < BM_FIN_UNR; ++u) {
                const int64_t i = i0 + (int64_t)u * BM_FIN_THREADS;
                v[u] = i < HW ? wp[i] : 0u;
            }
#pragma unroll
            for (int u = 0; u < BM_FIN_UNR; ++u) {
                if (!(v[u] & (BM_ON_P | BM_ON_G))) continue;
                const uint32_t d2 = v[u] & BM_D2;
#pragma unroll
                for (int dir = 0; dir < 2; ++dir)
                    if (on[dir] && (v[u] & flag[dir]) && (d2 >> (shift + 8)) == want[dir])
                        atomicAdd(&hist[dir][(d2 >> shift) & 255u], 1u);
            }
        }
        __syncthreads();
        if (tid == 0)
            for (int dir = 0; dir < 2; ++dir)
                if (active[dir]) prefix[dir] = (prefix[dir] << 8) | bm_pick(hist[dir], 256, rank[dir]);
        __syncthreads();
    }
    if (tid == 0)
        for (int dir = 0; dir < 2; ++dir)
            if (active[dir]) stats[((int64_t)blockIdx.x * 2 + dir) * 4 + 3] = (int64_t)prefix[dir];
}

}  // namespace iswm

using namespace iswm;

static bool bm_shape(int B, int C, int H, int W, int first_class) {
    return B > 0 && C > 0 && H > 0 && W > 0 && H <= BM_MAX_SIDE && W <= BM_MAX_SIDE && (first_class == 0 || first_class == 1) &&
           C - first_class >= 1 && (int64_t)B * (C - first_class) * H < ((int64_t)1 << 31) &&
           (int64_t)B * (C - first_class) * W < ((int64_t)1 << 31) * 256 && (int64_t)B * H * W < ((int64_t)1 << 31) * 256;
}

extern "C" int64_t iswm_boundary_metrics_workspace(int B, int C, int H, int W, int first_class) {
    if (!bm_shape(B, C, H, W, first_class)) return -1;
    return (int64_t)B * (C - first_class) * H * W * (int64_t)sizeof(uint32_t);
}

template <typename PredT, typename LabelT>
static void bm_launch_contours(const void* pred, const void* labels, int C, int H, int W, int K, int first, int ignore_index,
                               int64_t npix, uint32_t* ws, hipStream_t s) {
    hipLaunchKernelGGL((k_bm_contours<PredT, LabelT>), dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, s, (const PredT*)pred,
                       (const LabelT*)labels, C, H, W, K, first, ignore_index, npix, ws);
}

extern "C" int iswm_boundary_metrics(const void* pred, int pred_bytes, const void* labels, int label_bytes, int B, int C, int H, int W,
                                     int first_class, int ignore_index, int tolerance, int percent, int64_t* stats, double* dsum,
                                     void* workspace, int64_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(pred && labels && stats && dsum && workspace, "boundary_metrics: null pointer");
    ISWM_REQUIRE(H <= BM_MAX_SIDE && W <= BM_MAX_SIDE, "boundary_metrics: a %d x %d plane (the contour distances take sides up to %d)",
                 H, W, BM_MAX_SIDE);
    ISWM_REQUIRE(first_class == 0 || first_class == 1, "boundary_metrics: first_class is 0 (every class) or 1 (the foreground classes)");
    ISWM_REQUIRE(C - first_class >= 1, "boundary_metrics: %d classes from class %d on leave no class plane", C, first_class);
    ISWM_REQUIRE(bm_shape(B, C, H, W, first_class), "boundary_metrics: bad shape");
    ISWM_REQUIRE(pred_bytes == 1 || pred_bytes == 8, "boundary_metrics: predictions must be uint8 or int64");
    ISWM_REQUIRE(label_bytes == 1 || label_bytes == 8, "boundary_metrics: labels must be uint8 or int64");
    ISWM_REQUIRE(percent >= 1 && percent <= 100, "boundary_metrics: percent %d (the rank's percentile lies in 1 .. 100)", percent);
    ISWM_REQUIRE(tolerance >= 0 && tolerance <= BM_MAX_SIDE, "boundary_metrics: tolerance %d (0 .. %d pixels)", tolerance, BM_MAX_SIDE);
    ISWM_REQUIRE(workspace_bytes >= iswm_boundary_metrics_workspace(B, C, H, W, first_class), "boundary_metrics: workspace too small");
    const int K = C - first_class;
    const int64_t npix = (int64_t)B * H * W, ncols = (int64_t)B * K * W, nrows = (int64_t)B * K * H;
    hipStream_t s = (hipStream_t)stream;
    uint32_t* ws = (uint32_t*)workspace;
    if (pred_bytes == 1 && label_bytes == 1)
        bm_launch_contours<uint8_t, uint8_t>(pred, labels, C, H, W, K, first_class, ignore_index, npix, ws, s);
    else if (pred_bytes == 1)
        bm_launch_contours<uint8_t, int64_t>(pred, labels, C, H, W, K, first_class, ignore_index, npix, ws, s);
    else if (label_bytes == 1)
        bm_launch_contours<int64_t, uint8_t>(pred, labels, C, H, W, K, first_class, ignore_index, npix, ws, s);
    else
        bm_launch_contours<int64_t, int64_t>(pred, labels, C, H, W, K, first_class, ignore_index, npix, ws, s);
    hipLaunchKernelGGL(k_bm_columns, dim3((unsigned)((ncols + 255) / 256)), dim3(256), 0, s, ws, H, W, ncols);
    hipLaunchKernelGGL(k_bm_rows, dim3((unsigned)nrows), dim3(256), 2 * W * sizeof(uint32_t), s, ws, W);
    hipLaunchKernelGGL(k_bm_finalize, dim3((unsigned)(B * K)), dim3(BM_FIN_THREADS), 0, s, (const uint32_t*)ws, (int64_t)H * W,
                       (uint32_t)tolerance * (uint32_t)tolerance, percent, stats, dsum);
    return check_launch("boundary_metrics");
}
