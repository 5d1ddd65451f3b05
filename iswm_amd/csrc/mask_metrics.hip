// Sequence-validation metrics on the device: the per-frame and per-pair work behind the reference's TemporalMetrics,
// FrontTrackingMetrics and RegionMetrics (metrics/utils/mask_utils.py, metrics/front_tracking_metrics.py,
// metrics/region_metrics.py) on batched [N, H, W] masks.  Everything below the C ABI is integer work except the
// per-frame scores, which are summed in fp64 by one thread per frame in the reference's (row / rank) order.
//
//   morph      binary dilation / erosion by a (2r+1)^2 rectangle with a neutral border (cv2's default border:
//              pixels outside the frame never erode or dilate anything).  r-fold 3x3 == one (2r+1)^2 pass.
//   ccl        8-connected components: union-find per 32x32 tile in LDS, atomicMin union-find across tile
//              borders, then flatten.  Parents only ever point to smaller raster indices, so each root is the
//              minimum raster index (within the frame) of its component -- canonical, independent of atomic
//              order.  Areas: per-tile counts at the tile roots, moved to the final root with one atomic each.
//   preprocess MaskUtils.preprocess_mask: >0, close, open, ccl, largest component of area >= 0.001*H*W
//              (ties: smallest root), weight 1 / max(0.4, 1 - 0.2*(n_valid-1)).
//   fronts     leftmost column equal to 1 per row (only a weight-1 frame has any), count / sum y / sum x.
//   scores     front error, stability + motion, region score.
#include "common.h"

namespace iswm {

constexpr int MM_TILE = 32;             // ccl tile edge: 1024 pixels, 4 per thread of a 256-thread workgroup
constexpr int MM_MAX_DIM = 2048;        // LDS row arrays of the per-frame score kernels are sized by it
constexpr int MM_REGION_MIN_AREA = 50;  // RegionMetrics.min_area_threshold

__device__ __forceinline__ bool is_fg(const void* src, int dtype, size_t i) {
    return dtype == 0 ? static_cast<const unsigned char*>(src)[i] != 0 : static_cast<const long long*>(src)[i] > 0;
}

// dst = dilate (any) / erode (all) of (src > 0) over the in-frame part of the (2r+1)^2 window
__global__ __launch_bounds__(256) void k_morph(const void* __restrict__ src, int dtype, unsigned char* __restrict__ dst,
                                               int H, int W, int r, int dilate) {
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int y0 = max(0, y - r), y1 = min(H - 1, y + r), x0 = max(0, x - r), x1 = min(W - 1, x + r);
    bool v = !dilate;
    for (int yy = y0; yy <= y1 && v == !dilate; ++yy)
        for (int xx = x0; xx <= x1; ++xx)
            if (is_fg(src, dtype, base + (size_t)yy * W + xx) == (bool)dilate) {
                v = dilate;
                break;
            }
    dst[base + p] = v ? 1 : 0;
}

// ---- union-find with parents pointing to smaller indices --------------------------------------------------------
template <int SCOPE>
__device__ __forceinline__ int uf_find(int* p, int x) {
    int q = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, SCOPE);
    while (q != x) {
        x = q;
        q = __hip_atomic_load(&p[x], __ATOMIC_RELAXED, SCOPE);
    }
    return x;
}

// link the larger root under the smaller; a stale read is caught by atomicMin's return value, and every write only
// lowers a parent to another index of the same component
template <int SCOPE>
__device__ __forceinline__ void uf_unite(int* p, int a, int b) {
    bool done;
    do {
        a = uf_find<SCOPE>(p, a);
        b = uf_find<SCOPE>(p, b);
        if (a < b) {
            const int old = atomicMin(&p[b], a);
            done = old == b;
            b = old;
        } else if (b < a) {
            const int old = atomicMin(&p[a], b);
            done = old == a;
            a = old;
        } else {
            done = true;
        }
    } while (!done);
}

// pass 1: one workgroup per 32x32 tile.  labels[i] = frame raster index of the pixel's tile-local root (or -1),
// areas[i] = the tile-local component's pixel count at its root, 0 elsewhere
__global__ __launch_bounds__(256) void k_ccl_tile(const unsigned char* __restrict__ m, int H, int W, int tiles_x,
                                                  int* __restrict__ labels, int* __restrict__ areas) {
    __shared__ int par[MM_TILE * MM_TILE];
    __shared__ int cnt[MM_TILE * MM_TILE];
    const size_t base = (size_t)blockIdx.y * H * W;
    const int tx = blockIdx.x % tiles_x, ty = blockIdx.x / tiles_x;
    const int gx0 = tx * MM_TILE, gy0 = ty * MM_TILE;
    auto fg = [&](int l) {
        const int gx = gx0 + (l & (MM_TILE - 1)), gy = gy0 + l / MM_TILE;
        return gx < W && gy < H && m[base + (size_t)gy * W + gx] != 0;
    };
    for (int l = threadIdx.x; l < MM_TILE * MM_TILE; l += 256) {
        par[l] = fg(l) ? l : -1;
        cnt[l] = 0;
    }
    __syncthreads();
    for (int l = threadIdx.x; l < MM_TILE * MM_TILE; l += 256) {
        if (par[l] < 0) continue;
        const int lx = l & (MM_TILE - 1), ly = l / MM_TILE;
        if (lx > 0 && par[l - 1] >= 0) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, l - 1);
        if (ly > 0) {
            const int u = l - MM_TILE;
            if (par[u] >= 0) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, u);
            if (lx > 0 && par[u - 1] >= 0) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, u - 1);
            if (lx < MM_TILE - 1 && par[u + 1] >= 0) uf_unite<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, u + 1);
        }
    }
    __syncthreads();
    for (int l = threadIdx.x; l < MM_TILE * MM_TILE; l += 256)
        if (par[l] >= 0) atomicAdd(&cnt[uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l)], 1);
    __syncthreads();
    for (int l = threadIdx.x; l < MM_TILE * MM_TILE; l += 256) {
        const int gx = gx0 + (l & (MM_TILE - 1)), gy = gy0 + l / MM_TILE;
        if (gx >= W || gy >= H) continue;
        const size_t i = base + (size_t)gy * W + gx;
        int lab = -1;
        if (par[l] >= 0) {
            const int r = uf_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l);      // local order == raster order in the tile
            lab = (gy0 + r / MM_TILE) * W + gx0 + (r & (MM_TILE - 1));
        }
        labels[i] = lab;
        areas[i] = cnt[l];
    }
}

// pass 2: every foreground pixel unites with its left / upper neighbours that lie in another tile
__global__ __launch_bounds__(256) void k_ccl_merge(const unsigned char* __restrict__ m, int H, int W, int* labels) {
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
    const int lx = x & (MM_TILE - 1), ly = y & (MM_TILE - 1);
    if ((lx != 0 && lx != MM_TILE - 1 && ly != 0) || !m[base + p]) return;
    int* L = labels + base;
    const int me = (int)p;
    auto link = [&](int xx, int yy) {
        if (xx < 0 || xx >= W || yy < 0) return;
        if ((xx / MM_TILE) == (x / MM_TILE) && (yy / MM_TILE) == (y / MM_TILE)) return;
        const int q = yy * W + xx;
        if (m[base + q]) uf_unite<__HIP_MEMORY_SCOPE_AGENT>(L, me, q);
    };
    link(x - 1, y);
    link(x - 1, y - 1);
    link(x, y - 1);
    link(x + 1, y - 1);
}

// pass 3: labels[i] = root; a tile root that is not the final root hands its count to the final root
__global__ __launch_bounds__(256) void k_ccl_flatten(int H, int W, int* labels, int* areas) {
    const int64_t HW = (int64_t)H * W;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const size_t base = (size_t)blockIdx.y * HW;
    int* L = labels + base;
    if (L[p] < 0) return;
    const int r = uf_find<__HIP_MEMORY_SCOPE_AGENT>(L, (int)p);
    __hip_atomic_store(&L[p], r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r != (int)p) {
        const int c = areas[base + p];
        if (c) {
            areas[base + p] = 0;
            atomicAdd(&areas[base + r], c);
        }
    }
}

// ---- preprocess_mask: selection of the largest valid component ---------------------------------------------------
struct SelStat {
    unsigned long long key;   // area << 32 | ~root: the max is the largest area, ties to the smallest root
    unsigned int n_valid;
    unsigned int pad;
};

__global__ __launch_bounds__(256) void k_select_reduce(const int* __restrict__ areas, int64_t HW, double min_area,
                                                       SelStat* __restrict__ st) {
    __shared__ unsigned long long sk[256];
    __shared__ unsigned int sn[256];
    const size_t base = (size_t)blockIdx.y * HW;
    unsigned long long key = 0;
    unsigned int n = 0;
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
        const int a = areas[base + p];
        if (a > 0 && (double)a >= min_area) {
            ++n;
            const unsigned long long k = ((unsigned long long)a << 32) | (0xffffffffu - (unsigned int)p);
            key = k > key ? k : key;
        }
    }
    sk[threadIdx.x] = key;
    sn[threadIdx.x] = n;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s) {
            sk[threadIdx.x] = sk[threadIdx.x + s] > sk[threadIdx.x] ? sk[threadIdx.x + s] : sk[threadIdx.x];
            sn[threadIdx.x] += sn[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0 && sn[0]) {
        atomicMax(&st[blockIdx.y].key, sk[0]);
        atomicAdd(&st[blockIdx.y].n_valid, sn[0]);
    }
}

__global__ __launch_bounds__(256) void k_select_write(const int* __restrict__ labels, int64_t HW,
                                                      const SelStat* __restrict__ st, unsigned char* __restrict__ out,
                                                      double* __restrict__ weight, int64_t* __restrict__ area) {
    const int f = blockIdx.y;
    const SelStat s = st[f];
    const int root = s.n_valid ? (int)(0xffffffffu - (unsigned int)(s.key & 0xffffffffu)) : -1;
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p == 0) {
        weight[f] = s.n_valid == 0 ? 0.0 : s.n_valid == 1 ? 1.0 : fmax(0.4, 1.0 - 0.2 * (double)(s.n_valid - 1));
        area[f] = s.n_valid ? (int64_t)(s.key >> 32) : 0;
    }
    if (p < HW) out[(size_t)f * HW + p] = (root >= 0 && labels[(size_t)f * HW + p] == root) ? 1 : 0;
}

// ---- fronts ------------------------------------------------------------------------------------------------------
// one workgroup per frame, one wave per row: fronts[f][y] = first x with value 1, else -1; stats = count, sum y, sum x
__global__ __launch_bounds__(256) void k_fronts(const unsigned char* __restrict__ m, const double* __restrict__ weight,
                                                int H, int W, int* __restrict__ fronts, int64_t* __restrict__ stats) {
    __shared__ int64_t acc[4][3];
    const int f = blockIdx.x, wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned char* mf = m + (size_t)f * H * W;
    const bool ones = weight == nullptr || weight[f] == 1.0;       // mask * weight == 1 only where the weight is 1
    int64_t c = 0, sy = 0, sx = 0;
    for (int y = wave; y < H; y += 4) {
        int first = -1;
        if (ones) {
            for (int x0 = 0; x0 < W; x0 += 64) {
                const int x = x0 + lane;
                const unsigned long long b = __ballot(x < W && mf[(size_t)y * W + x] == 1);
                if (b) {
                    first = x0 + __ffsll((long long)b) - 1;
                    break;
                }
            }
        }
        if (lane == 0) {
            fronts[(size_t)f * H + y] = first;
            if (first >= 0) {
                ++c;
                sy += y;
                sx += first;
            }
        }
    }
    if (lane == 0) {
        acc[wave][0] = c;
        acc[wave][1] = sy;
        acc[wave][2] = sx;
    }
    __syncthreads();
    if (threadIdx.x < 3)
        stats[(size_t)f * 3 + threadIdx.x] =
            acc[0][threadIdx.x] + acc[1][threadIdx.x] + acc[2][threadIdx.x] + acc[3][threadIdx.x];
}

// ---- FrontTrackingMetrics.calculate_error, one workgroup per (pred, gt) pair ---------------------------------------
__global__ __launch_bounds__(256) void k_front_error(const int* __restrict__ fp, const int* __restrict__ fg, int H,
                                                    double tau, double* __restrict__ out) {
    __shared__ int sf[2][MM_MAX_DIM];
    __shared__ double se[2][MM_MAX_DIM], sw[2][MM_MAX_DIM];
    __shared__ unsigned char sv[2][MM_MAX_DIM];
    const int f = blockIdx.x;
    for (int y = threadIdx.x; y < H; y += 256) {
        sf[0][y] = fp[(size_t)f * H + y];
        sf[1][y] = fg[(size_t)f * H + y];
    }
    __syncthreads();
    // direction d: points of sf[d] against their nearest point of sf[1-d]; argmin of the integer squared distance,
    // first (smallest row) wins ties == `dist < min_dist` over sqrt of the same integers
    for (int t = threadIdx.x; t < 2 * H; t += 256) {
        const int d = t / H, y = t - d * H, x = sf[d][y];
        sv[d][y] = 0;
        if (x < 0) continue;
        long long best = -1;
        int bdx = 0;
        for (int yy = 0; yy < H; ++yy) {
            const int xx = sf[1 - d][yy];
            if (xx < 0) continue;
            const long long dy = y - yy, dx = x - xx, d2 = dy * dy + dx * dx;
            if (best < 0 || d2 < best) {
                best = d2;
                bdx = dx < 0 ? (int)-dx : (int)dx;
            }
        }
        if (best < 0) continue;
        const double dist = sqrt((double)best);
        if (dist < tau) {
            const double w = 1.0 / ((double)bdx + 1e-6);
            se[d][y] = dist * w;
            sw[d][y] = w;
            sv[d][y] = 1;
        }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    int n[2] = {0, 0}, nv[2] = {0, 0};
    double e[2] = {0.0, 0.0}, w[2] = {0.0, 0.0};
    for (int d = 0; d < 2; ++d)
        for (int y = 0; y < H; ++y) {
            n[d] += sf[d][y] >= 0;
            if (sv[d][y]) {
                e[d] += se[d][y];
                w[d] += sw[d][y];
                ++nv[d];
            }
        }
    double r;
    if (n[1] && !n[0]) r = tau * 2.0;
    else if (!n[1] && n[0]) r = tau * 1.5;
    else if (!n[1] && !n[0]) r = 0.0;
    else if (nv[0] == 0 || nv[1] == 0) r = tau * 2.0;
    else {
        const double pred_avg = e[0] / w[0], gt_avg = e[1] / w[1];
        const double coverage = (double)nv[1] / (double)n[1];
        const double max_error = pred_avg >= gt_avg ? pred_avg : gt_avg;
        r = max_error + (1.0 - coverage) * tau * 0.5;
    }
    out[f] = r;
}

// ---- MaskUtils.calculate_stability + calculate_motion, one workgroup per (current, previous) pair ----------------
__global__ __launch_bounds__(256) void k_pair_scores(const int* __restrict__ cf, const int64_t* __restrict__ cst,
                                                     const unsigned char* __restrict__ pm, const double* __restrict__ pw,
                                                     const int64_t* __restrict__ pst, int H, int W,
                                                     double* __restrict__ stab, double* __restrict__ motion) {
    __shared__ double ss[MM_MAX_DIM];
    __shared__ unsigned char sv[MM_MAX_DIM];
    const int f = blockIdx.x;
    const int ws = (int)((double)W * 0.1);
    const bool prev_ones = pw[f] == 1.0;
    const unsigned char* prow = pm + (size_t)f * H * W;
    for (int y = threadIdx.x; y < H; y += 256) {
        sv[y] = 0;
        const int c = cf[(size_t)f * H + y];
        if (c < 0 || !prev_ones) continue;
        const int s = max(0, c - ws), e = min(W, c + ws);
        for (int x = s; x < e; ++x)
            if (prow[(size_t)y * W + x] == 1) {
                const int diff = c > x ? c - x : x - c;
                ss[y] = 1.0 / (1.0 + (double)diff / (double)ws);
                sv[y] = 1;
                break;
            }
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    int n = 0;
    for (int y = 0; y < H; ++y)
        if (sv[y]) {
            sum += ss[y];
            ++n;
        }
    stab[f] = n ? sum / n : 0.0;
    const int64_t* c = cst + (size_t)f * 3;
    const int64_t* p = pst + (size_t)f * 3;
    if (c[0] == 0 || p[0] == 0) {
        motion[f] = 0.0;
    } else {
        const double dy = (double)c[1] / (double)c[0] - (double)p[1] / (double)p[0];
        const double dx = (double)c[2] / (double)c[0] - (double)p[2] / (double)p[0];
        const double dist = sqrt(dy * dy + dx * dx);
        motion[f] = 1.0 / (1.0 + dist / ((double)H * 0.1));
    }
}

// ---- RegionMetrics.calculate_region_metrics ------------------------------------------------------------------------
struct RegionStat {
    unsigned long long pred, gt, inter, uni, total;   // pixel counts; total = area of the components >= 50 px
    unsigned int n;                                   // components >= 50 px
    unsigned int pad;
};

__global__ __launch_bounds__(256) void k_region_counts(const void* __restrict__ pred, int pdt, const void* __restrict__ gt,
                                                       int gdt, const unsigned char* __restrict__ rep, int64_t HW,
                                                       RegionStat* __restrict__ st) {
    __shared__ unsigned long long sh[4][256];
    const size_t base = (size_t)blockIdx.y * HW;
    unsigned long long c[4] = {0, 0, 0, 0};
    for (int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (int64_t)gridDim.x * 256) {
        const bool a = is_fg(pred, pdt, base + p), g = is_fg(gt, gdt, base + p), r = rep[base + p] != 0;
        c[0] += a;
        c[1] += g;
        c[2] += r && g;
        c[3] += r || g;
    }
    for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] = c[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (threadIdx.x < s)
            for (int k = 0; k < 4; ++k) sh[k][threadIdx.x] += sh[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        RegionStat* r = &st[blockIdx.y];
        if (sh[0][0]) atomicAdd(&r->pred, sh[0][0]);
        if (sh[1][0]) atomicAdd(&r->gt, sh[1][0]);
        if (sh[2][0]) atomicAdd(&r->inter, sh[2][0]);
        if (sh[3][0]) atomicAdd(&r->uni, sh[3][0]);
    }
}

// component areas >= 50 appended to list[f] (order undefined; the rank pass sorts them)
__global__ __launch_bounds__(256) void k_region_compact(const int* __restrict__ areas, int64_t HW, int cap,
                                                        int* __restrict__ list, RegionStat* __restrict__ st) {
    const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int a = areas[(size_t)blockIdx.y * HW + p];
    if (a < MM_REGION_MIN_AREA) return;
    RegionStat* r = &st[blockIdx.y];
    const unsigned int k = atomicAdd(&r->n, 1u);
    if (k < (unsigned int)cap) list[(size_t)blockIdx.y * cap + k] = a;
    atomicAdd(&r->total, (unsigned long long)a);
}

// rank sort, descending: entry k goes to #(larger) + #(equal before k); equal areas are interchangeable
__global__ __launch_bounds__(256) void k_region_rank(const int* __restrict__ list, int cap, const RegionStat* __restrict__ st,
                                                     int* __restrict__ sorted) {
    const int f = blockIdx.y, n = (int)min(st[f].n, (unsigned int)cap);
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int* l = list + (size_t)f * cap;
    const int a = l[k];
    int rank = 0;
    for (int j = 0; j < n; ++j) {
        const int b = l[j];
        rank += (b > a) || (b == a && j < k);
    }
    sorted[(size_t)f * cap + rank] = a;
}

__global__ void k_region_final(const int* __restrict__ sorted, int cap, const RegionStat* __restrict__ st, int N,
                               double* __restrict__ score, int* __restrict__ valid) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= N) return;
    const RegionStat s = st[f];
    if (s.pred == 0 || s.gt == 0) {
        score[f] = 0.0;
        valid[f] = 0;
        return;
    }
    const double sim = (double)s.inter / (double)s.uni;
    double frag = 0.0;
    const int n = (int)s.n;
    if (n > 0) {
        const int* a = sorted + (size_t)f * cap;
        const double total = (double)s.total;
        frag = (double)a[0] / total;
        if (n > 1) {
            double penalty = 0.0;
            for (int i = 0; i + 1 < n; ++i) penalty += (double)a[i + 1] / total * (double)(i + 1) / (double)n;
            frag -= penalty * 0.5;
        }
        frag = fmax(0.0, fmin(1.0, frag));
    }
    score[f] = 0.7 * frag + 0.3 * sim;
    valid[f] = 1;
}

}  // namespace iswm

using namespace iswm;

namespace {

bool mm_dims_ok(int N, int H, int W) { return N >= 1 && N <= 65535 && H >= 1 && W >= 1 && H <= MM_MAX_DIM && W <= MM_MAX_DIM; }

dim3 pix_grid(int N, int H, int W) { return dim3((unsigned)(((int64_t)H * W + 255) / 256), (unsigned)N); }

int region_cap(int H, int W) { return (int)((int64_t)H * W / MM_REGION_MIN_AREA + 1); }

size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

int ccl_launch(const unsigned char* m, int N, int H, int W, int* labels, int* areas, hipStream_t s) {
    const int tx = (W + MM_TILE - 1) / MM_TILE, ty = (H + MM_TILE - 1) / MM_TILE;
    hipLaunchKernelGGL(k_ccl_tile, dim3(tx * ty, N), dim3(256), 0, s, m, H, W, tx, labels, areas);
    hipLaunchKernelGGL(k_ccl_merge, pix_grid(N, H, W), dim3(256), 0, s, m, H, W, labels);
    hipLaunchKernelGGL(k_ccl_flatten, pix_grid(N, H, W), dim3(256), 0, s, H, W, labels, areas);
    return check_launch("ccl");
}

}  // namespace

extern "C" int iswm_mask_morph(const void* src, int src_dtype, int N, int H, int W, int radius, int dilate,
                               uint8_t* dst, iswm_stream_t stream) {
    ISWM_REQUIRE(src && dst, "mask_morph: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W) && radius >= 0 && radius <= 16, "mask_morph: bad size");
    ISWM_REQUIRE(src_dtype == 0 || src_dtype == 1, "mask_morph: dtype codes are 0 (uint8) and 1 (int64)");
    hipLaunchKernelGGL(k_morph, pix_grid(N, H, W), dim3(256), 0, (hipStream_t)stream, src, src_dtype, dst, H, W, radius,
                       dilate ? 1 : 0);
    return check_launch("mask_morph");
}

extern "C" int iswm_ccl(const uint8_t* mask, int N, int H, int W, int32_t* labels, int32_t* areas, iswm_stream_t stream) {
    ISWM_REQUIRE(mask && labels && areas, "ccl: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W), "ccl: bad size");
    return ccl_launch(mask, N, H, W, labels, areas, (hipStream_t)stream);
}

extern "C" size_t iswm_mask_preprocess_workspace(int N, int H, int W) {
    if (!mm_dims_ok(N, H, W)) return 0;
    const size_t px = (size_t)N * H * W;
    return 2 * align256(px) + 2 * align256(px * 4) + align256((size_t)N * sizeof(SelStat));
}

extern "C" int iswm_mask_preprocess(const void* src, int src_dtype, int N, int H, int W, uint8_t* out, double* weight,
                                    int64_t* area, void* workspace, size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(src && out && weight && area && workspace, "mask_preprocess: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W), "mask_preprocess: bad size");
    ISWM_REQUIRE(src_dtype == 0 || src_dtype == 1, "mask_preprocess: dtype codes are 0 (uint8) and 1 (int64)");
    ISWM_REQUIRE(workspace_bytes >= iswm_mask_preprocess_workspace(N, H, W), "mask_preprocess: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t px = (size_t)N * H * W;
    char* w = static_cast<char*>(workspace);
    unsigned char* a = reinterpret_cast<unsigned char*>(w);
    unsigned char* b = a + align256(px);
    int* labels = reinterpret_cast<int*>(b + align256(px));
    int* areas = reinterpret_cast<int*>(reinterpret_cast<char*>(labels) + align256(px * 4));
    SelStat* st = reinterpret_cast<SelStat*>(reinterpret_cast<char*>(areas) + align256(px * 4));
    const dim3 g = pix_grid(N, H, W);
    // close (dilate r1, erode r1) then open (erode r1, dilate r1): the two erosions fold into one r2 pass
    hipLaunchKernelGGL(k_morph, g, dim3(256), 0, s, src, src_dtype, a, H, W, 1, 1);
    hipLaunchKernelGGL(k_morph, g, dim3(256), 0, s, (const void*)a, 0, b, H, W, 2, 0);
    hipLaunchKernelGGL(k_morph, g, dim3(256), 0, s, (const void*)b, 0, a, H, W, 1, 1);
    if (int rc = ccl_launch(a, N, H, W, labels, areas, s)) return rc;
    if (hipMemsetAsync(st, 0, (size_t)N * sizeof(SelStat), s) != hipSuccess) {
        set_error("mask_preprocess: hipMemsetAsync failed");
        return 2;
    }
    const int64_t HW = (int64_t)H * W;
    const double min_area = (double)HW * 0.001;       // mask.size * 0.001, fp64 as in the reference
    hipLaunchKernelGGL(k_select_reduce, dim3((unsigned)std::min<int64_t>((HW + 4095) / 4096, 64), N), dim3(256), 0, s,
                       (const int*)areas, HW, min_area, st);
    hipLaunchKernelGGL(k_select_write, g, dim3(256), 0, s, labels, HW, st, out, weight, area);
    return check_launch("mask_preprocess");
}

extern "C" int iswm_mask_fronts(const uint8_t* mask, const double* weight, int N, int H, int W, int32_t* fronts,
                                int64_t* stats, iswm_stream_t stream) {
    ISWM_REQUIRE(mask && fronts && stats, "mask_fronts: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W), "mask_fronts: bad size");
    hipLaunchKernelGGL(k_fronts, dim3(N), dim3(256), 0, (hipStream_t)stream, mask, weight, H, W, fronts, stats);
    return check_launch("mask_fronts");
}

extern "C" int iswm_front_error(const int32_t* pred_fronts, const int32_t* gt_fronts, int N, int H, double tau,
                                double* out, iswm_stream_t stream) {
    ISWM_REQUIRE(pred_fronts && gt_fronts && out, "front_error: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, 1) && tau > 0.0, "front_error: bad size");
    hipLaunchKernelGGL(k_front_error, dim3(N), dim3(256), 0, (hipStream_t)stream, pred_fronts, gt_fronts, H, tau, out);
    return check_launch("front_error");
}

extern "C" int iswm_mask_pair_scores(const int32_t* curr_fronts, const int64_t* curr_stats, const uint8_t* prev_mask,
                                     const double* prev_weight, const int64_t* prev_stats, int N, int H, int W,
                                     double* stability, double* motion, iswm_stream_t stream) {
    ISWM_REQUIRE(curr_fronts && curr_stats && prev_mask && prev_weight && prev_stats && stability && motion,
                 "mask_pair_scores: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W), "mask_pair_scores: bad size");
    hipLaunchKernelGGL(k_pair_scores, dim3(N), dim3(256), 0, (hipStream_t)stream, curr_fronts, curr_stats, prev_mask,
                       prev_weight, prev_stats, H, W, stability, motion);
    return check_launch("mask_pair_scores");
}

extern "C" size_t iswm_region_workspace(int N, int H, int W) {
    if (!mm_dims_ok(N, H, W)) return 0;
    const size_t px = (size_t)N * H * W, cap = (size_t)N * region_cap(H, W);
    return 2 * align256(px) + 2 * align256(px * 4) + 2 * align256(cap * 4) + align256((size_t)N * sizeof(RegionStat));
}

extern "C" int iswm_region_score(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int N, int H, int W,
                                 double* score, int32_t* valid, void* workspace, size_t workspace_bytes,
                                 iswm_stream_t stream) {
    ISWM_REQUIRE(pred && gt && score && valid && workspace, "region_score: null pointer");
    ISWM_REQUIRE(mm_dims_ok(N, H, W), "region_score: bad size");
    ISWM_REQUIRE((pred_dtype == 0 || pred_dtype == 1) && (gt_dtype == 0 || gt_dtype == 1),
                 "region_score: dtype codes are 0 (uint8) and 1 (int64)");
    ISWM_REQUIRE(workspace_bytes >= iswm_region_workspace(N, H, W), "region_score: workspace too small");
    hipStream_t s = (hipStream_t)stream;
    const size_t px = (size_t)N * H * W;
    const int cap = region_cap(H, W);
    char* w = static_cast<char*>(workspace);
    unsigned char* a = reinterpret_cast<unsigned char*>(w);
    unsigned char* rep = a + align256(px);
    int* labels = reinterpret_cast<int*>(rep + align256(px));
    int* areas = reinterpret_cast<int*>(reinterpret_cast<char*>(labels) + align256(px * 4));
    int* list = reinterpret_cast<int*>(reinterpret_cast<char*>(areas) + align256(px * 4));
    int* sorted = reinterpret_cast<int*>(reinterpret_cast<char*>(list) + align256((size_t)N * cap * 4));
    RegionStat* st = reinterpret_cast<RegionStat*>(reinterpret_cast<char*>(sorted) + align256((size_t)N * cap * 4));
    const dim3 g = pix_grid(N, H, W);
    // repair_small_gaps: 3x dilate then 2x erode by 3x3 == dilate r3 then erode r2 (neutral border)
    hipLaunchKernelGGL(k_morph, g, dim3(256), 0, s, pred, pred_dtype, a, H, W, 3, 1);
    hipLaunchKernelGGL(k_morph, g, dim3(256), 0, s, (const void*)a, 0, rep, H, W, 2, 0);
    if (hipMemsetAsync(st, 0, (size_t)N * sizeof(RegionStat), s) != hipSuccess) {
        set_error("region_score: hipMemsetAsync failed");
        return 2;
    }
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(k_region_counts, dim3((unsigned)std::min<int64_t>((HW + 4095) / 4096, 64), N), dim3(256), 0, s,
                       pred, pred_dtype, gt, gt_dtype, (const unsigned char*)rep, HW, st);
    if (int rc = ccl_launch(rep, N, H, W, labels, areas, s)) return rc;
    hipLaunchKernelGGL(k_region_compact, g, dim3(256), 0, s, (const int*)areas, HW, cap, list, st);
    hipLaunchKernelGGL(k_region_rank, dim3((unsigned)((cap + 255) / 256), N), dim3(256), 0, s, (const int*)list, cap,
                       (const RegionStat*)st, sorted);
    hipLaunchKernelGGL(k_region_final, dim3((N + 63) / 64), dim3(64), 0, s, (const int*)sorted, cap, (const RegionStat*)st,
                       N, score, valid);
    return check_launch("region_score");
}
