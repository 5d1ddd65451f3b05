// GPU-resident tile store (iswm_amd/datasets.py): the kernels that keep a decoded image / mask
// data set on the device and feed k_augment from it without the host computing a table.
//   * k_label_prepare (+ k_count_finalize): masks are stored as decoded (mode L); every non-zero byte becomes class 1,
//     in place, 16 bytes per lane per access, and the two class counts come back from the same pass;
//   * k_label_count (+ k_count_finalize): {n(0), n(1), n(other)} of a uint8 label batch ADDED to a device accumulator
//     (the class-weight pass reads it back once);
//   * k_aug_tables: Pillow's resampling tables (Resample.c precompute_coeffs + normalize_coeffs_8bpc, Geometry.c
//     ImagingScaleAffine) for every sample of a batch, in the block layout k_augment reads -- the device form of
//     utils/ext_transforms.py _resample_tables / _nearest_table, same fp64 operations in the same order;
//   * k_gather_normalize: B equal-sized tiles at arbitrary arena offsets -> normalised fp32 NCHW (k_predict_normalize's
//     expression) + the uint8 label batch.
// No atomics: per-workgroup partial counts go to a slab that ONE workgroup sums in index order.
// All fp64 arithmetic of this file is uncontracted and the build has no fast-math flag: division, floor and the
// double -> int conversions are the IEEE / C forms numpy uses (tests/test_dataset_gpu.py compares the tables bit for bit).
#pragma clang fp contract(off)
#include "common.h"

namespace iswm {

constexpr int DS_BLOCK = 256;
constexpr int AUG_TAB_PRECISION_BITS = 22;   // Pillow: 32 - 8 - 2

using AugSampleT = iswm_aug_sample;

// 0x80 in every byte of x that is non-zero (no carry crosses a byte: 0x7f + 0x7f = 0xfe)
__device__ __forceinline__ unsigned nonzero_bytes(unsigned x) {
    return (x | ((x & 0x7f7f7f7fu) + 0x7f7f7f7fu)) & 0x80808080u;
}

// sums up to three int64 values over the workgroup; the result is valid in thread 0
template <int K>
__device__ __forceinline__ void block_sum(long long (&v)[K]) {
    __shared__ long long red[K][DS_BLOCK / 64];
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off, 64);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[k][wave] = v[k];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) {
            long long s = 0;
            for (int w = 0; w < DS_BLOCK / 64; ++w) s += red[k][w];
            v[k] = s;
        }
}

// labels: n16 chunks of 16 bytes.  slab[block] = ones written by the block
__global__ __launch_bounds__(DS_BLOCK) void k_label_prepare(uint4* __restrict__ labels, long long n16,
                                                            long long* __restrict__ slab) {
    long long ones[1] = {0};
    for (long long i = (long long)blockIdx.x * DS_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * DS_BLOCK) {
        uint4 v = labels[i];
        v.x = nonzero_bytes(v.x) >> 7;
        v.y = nonzero_bytes(v.y) >> 7;
        v.z = nonzero_bytes(v.z) >> 7;
        v.w = nonzero_bytes(v.w) >> 7;
        ones[0] += __popc(v.x) + __popc(v.y) + __popc(v.z) + __popc(v.w);
        labels[i] = v;
    }
    block_sum<1>(ones);
    if (threadIdx.x == 0) slab[blockIdx.x] = ones[0];
}

// slab[block][2] = {n(label == 0), n(label == 1)} of the block's share; a label equal to `ignore` counts as neither
__global__ __launch_bounds__(DS_BLOCK) void k_label_count(const unsigned char* __restrict__ labels, long long n,
                                                          int ignore, long long* __restrict__ slab) {
    const long long n16 = n / 16;
    const uint4* lv = reinterpret_cast<const uint4*>(labels);
    long long c[2] = {0, 0};
    for (long long i = (long long)blockIdx.x * DS_BLOCK + threadIdx.x; i < n16; i += (long long)gridDim.x * DS_BLOCK) {
        const uint4 v = lv[i];
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            c[0] += 4 - __popc(nonzero_bytes(w[k]));
            c[1] += 4 - __popc(nonzero_bytes(w[k] ^ 0x01010101u));
        }
    }
    if (blockIdx.x == 0)                                        // the < 16 bytes behind the last whole chunk
        for (long long i = n16 * 16 + threadIdx.x; i < n; i += DS_BLOCK) {
            c[0] += labels[i] == 0;
            c[1] += labels[i] == 1;
        }
    if (ignore == 0) c[0] = 0;
    if (ignore == 1) c[1] = 0;
    block_sum<2>(c);
    if (threadIdx.x == 0) {
        slab[2 * blockIdx.x] = c[0];
        slab[2 * blockIdx.x + 1] = c[1];
    }
}

// one workgroup: the slab's K columns summed in index order.  K == 1 (label_prepare): counts = {total - ones, ones};
// K == 2 (label_count): counts += {zeros, ones, total - zeros - ones}
template <int K>
__global__ __launch_bounds__(DS_BLOCK) void k_count_finalize(const long long* __restrict__ slab, int nb, long long total,
                                                             long long* __restrict__ counts) {
    long long v[K];
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = 0;
    for (int i = threadIdx.x; i < nb; i += DS_BLOCK)
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] += slab[(size_t)K * i + k];
    block_sum<K>(v);
    if (threadIdx.x == 0) {
        if constexpr (K == 1) {
            counts[0] = total - v[0];
            counts[1] = v[0];
        } else {
            counts[0] += v[0];
            counts[1] += v[1];
            counts[2] += total - v[0] - v[1];
        }
    }
}

// ---- Pillow's tables ----------------------------------------------------------------------------------------------
// ints of one sample's block: xintab[rs_w] | yintab[rs_h] | hbounds[rs_w][2] | hk[rs_w][ksize_h] | vbounds[rs_h][2] |
// vk[rs_h][ksize_v]
__device__ __forceinline__ long long aug_table_ints(const AugSampleT& s) {
    return (long long)s.rs_w * (3 + s.ksize_h) + (long long)s.rs_h * (3 + s.ksize_v);
}

// Geometry.c ImagingScaleAffine along one axis: xo = a * 0.5, then xo += a per output index; index = (int)xo.
// ONE lane walks the axis: the running sum's rounding is part of the result.
__device__ void nearest_axis(int in_size, int out_size, int* __restrict__ tab) {
    const double a = (double)in_size / (double)out_size;
    double xo = 0.0 + a * 0.5;
    for (int i = 0; i < out_size; ++i) {
        int idx = xo < 0.0 ? -1 : (int)xo;
        idx = idx < 0 ? 0 : (idx > in_size - 1 ? in_size - 1 : idx);
        tab[i] = idx;
        xo = xo + a;
    }
}

// Resample.c precompute_coeffs (BILINEAR, box = the whole axis) + normalize_coeffs_8bpc for output index xx
__device__ void resample_row(int in_size, int out_size, int ksize, int xx, int* __restrict__ bounds,
                             int* __restrict__ kk) {
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale >= 1.0 ? scale : 1.0;
    const double support = 1.0 * filterscale;
    const double center = 0.0 + ((double)xx + 0.5) * scale;
    const double ss = 1.0 / filterscale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < ksize; ++x) {                       // the weights summed in x order, as the C loop
        const double arg = fabs(((double)x + (double)xmin - center + 0.5) * ss);
        double w = arg < 1.0 ? 1.0 - arg : 0.0;
        if (x >= xmax) w = 0.0;
        ww = ww + w;
    }
    for (int x = 0; x < ksize; ++x) {                       // the same expression gives the same w again
        const double arg = fabs(((double)x + (double)xmin - center + 0.5) * ss);
        double w = arg < 1.0 ? 1.0 - arg : 0.0;
        if (x >= xmax) w = 0.0;
        if (ww != 0.0) w = w / ww;
        kk[x] = (int)floor(0.5 + w * (double)(1 << AUG_TAB_PRECISION_BITS));
    }
    bounds[0] = xmin;
    bounds[1] = xmax;
}

// grid (row_blocks + 1, B).  Blocks x < row_blocks take the rs_w + rs_h resample rows of sample y, one per thread;
// the last block walks the two nearest axes (lane 0 of wave 0: columns, lane 0 of wave 1: rows).
// A sample whose block would not fit in `cap` ints (or whose fields are not positive) is left unwritten.
__global__ __launch_bounds__(DS_BLOCK) void k_aug_tables(const AugSampleT* __restrict__ samples, int* __restrict__ tables,
                                                         long long cap) {
    const AugSampleT s = samples[blockIdx.y];
    if (s.src_h < 1 || s.src_w < 1 || s.rs_h < 1 || s.rs_w < 1 || s.ksize_h < 1 || s.ksize_v < 1 || s.tab_off < 0 ||
        (long long)s.tab_off + aug_table_ints(s) > cap)
        return;
    int* xintab = tables + s.tab_off;
    int* yintab = xintab + s.rs_w;
    int* hb = yintab + s.rs_h;
    int* hk = hb + 2 * s.rs_w;
    int* vb = hk + (size_t)s.rs_w * s.ksize_h;
    int* vk = vb + 2 * s.rs_h;
    const int row_blocks = gridDim.x - 1;
    if ((int)blockIdx.x == row_blocks) {
        if (threadIdx.x == 0) nearest_axis(s.src_w, s.rs_w, xintab);
        if (threadIdx.x == 64) nearest_axis(s.src_h, s.rs_h, yintab);
        return;
    }
    for (int i = blockIdx.x * DS_BLOCK + threadIdx.x; i < s.rs_w + s.rs_h; i += row_blocks * DS_BLOCK) {
        if (i < s.rs_w)
            resample_row(s.src_w, s.rs_w, s.ksize_h, i, hb + 2 * i, hk + (size_t)i * s.ksize_h);
        else
            resample_row(s.src_h, s.rs_h, s.ksize_v, i - s.rs_w, vb + 2 * (i - s.rs_w),
                         vk + (size_t)(i - s.rs_w) * s.ksize_v);
    }
}

// ---- validation batches ---------------------------------------------------------------------------------------
// offsets [B][2] = (image byte offset, label byte offset), both multiples of 16.  A thread takes 4 consecutive
// pixels of one tile: three aligned 4-byte image loads, one label load.
__global__ __launch_bounds__(DS_BLOCK) void k_gather_normalize(const unsigned char* __restrict__ images,
                                                               const unsigned char* __restrict__ labels,
                                                               const long long* __restrict__ offsets, int B, int64_t HW,
                                                               float m0, float m1, float m2, float s0, float s1, float s2,
                                                               float* __restrict__ out,
                                                               unsigned char* __restrict__ out_lbl) {
    const int64_t Q = (HW + 3) / 4;                          // 4-pixel groups per tile
    const int64_t total = (int64_t)B * Q;
    for (int64_t i = (int64_t)blockIdx.x * DS_BLOCK + threadIdx.x; i < total; i += (int64_t)gridDim.x * DS_BLOCK) {
        const int64_t b = i / Q, p0 = (i - b * Q) * 4;
        const unsigned char* im = images + offsets[2 * b] + p0 * 3;
        const unsigned char* lb = labels + offsets[2 * b + 1] + p0;
        unsigned char px[12], lab[4];
        const int np = HW - p0 >= 4 ? 4 : (int)(HW - p0);
        if (np == 4) {
            const unsigned* iw = reinterpret_cast<const unsigned*>(im);
            const unsigned w[3] = {iw[0], iw[1], iw[2]};
            const unsigned lw = *reinterpret_cast<const unsigned*>(lb);
#pragma unroll
            for (int k = 0; k < 12; ++k) px[k] = (unsigned char)(w[k >> 2] >> (8 * (k & 3)));
#pragma unroll
            for (int k = 0; k < 4; ++k) lab[k] = (unsigned char)(lw >> (8 * k));
        } else {                                             // the tile's last, partial group: never read past the tile
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < np;
                px[3 * k] = in ? im[3 * k] : 0;
                px[3 * k + 1] = in ? im[3 * k + 1] : 0;
                px[3 * k + 2] = in ? im[3 * k + 2] : 0;
                lab[k] = in ? lb[k] : 0;
            }
        }
        float* o = out + b * 3 * HW + p0;
        unsigned char* ol = out_lbl + b * HW + p0;
        float r[4], g[4], bl[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = __fdiv_rn(__fdiv_rn((float)px[3 * k], 255.0f) - m0, s0);
            g[k] = __fdiv_rn(__fdiv_rn((float)px[3 * k + 1], 255.0f) - m1, s1);
            bl[k] = __fdiv_rn(__fdiv_rn((float)px[3 * k + 2], 255.0f) - m2, s2);
        }
        if ((HW & 3) == 0) {                                 // every plane and every group is 16-byte aligned
            *reinterpret_cast<float4*>(o) = make_float4(r[0], r[1], r[2], r[3]);
            *reinterpret_cast<float4*>(o + HW) = make_float4(g[0], g[1], g[2], g[3]);
            *reinterpret_cast<float4*>(o + 2 * HW) = make_float4(bl[0], bl[1], bl[2], bl[3]);
            *reinterpret_cast<unsigned*>(ol) = (unsigned)lab[0] | (unsigned)lab[1] << 8 | (unsigned)lab[2] << 16 |
                                               (unsigned)lab[3] << 24;
        } else {
            for (int k = 0; k < np; ++k) {
                o[k] = r[k];
                o[HW + k] = g[k];
                o[2 * HW + k] = bl[k];
                ol[k] = lab[k];
            }
        }
    }
}

static int prepare_blocks(long long nbytes) { return stream_grid(nbytes / 16, DS_BLOCK); }
static int count_blocks(long long n) { return stream_grid(n / 16 + 1, DS_BLOCK); }

// table ints a HOST copy of the samples needs: max over samples of tab_off + block size; -1 on a bad record
static long long host_table_ints(const AugSampleT* s, int B) {
    long long need = 0;
    for (int b = 0; b < B; ++b) {
        if (s[b].src_h < 1 || s[b].src_w < 1 || s[b].rs_h < 1 || s[b].rs_w < 1 || s[b].ksize_h < 1 || s[b].ksize_v < 1 ||
            s[b].tab_off < 0)
            return -1;
        const long long end = (long long)s[b].tab_off + (long long)s[b].rs_w * (3 + s[b].ksize_h) +
                              (long long)s[b].rs_h * (3 + s[b].ksize_v);
        if (end > need) need = end;
    }
    return need;
}

}  // namespace iswm

using namespace iswm;

extern "C" size_t iswm_label_prepare_workspace(long long nbytes) {
    if (nbytes <= 0) return 0;
    return (size_t)prepare_blocks(nbytes) * sizeof(long long);
}

extern "C" int iswm_label_prepare(unsigned char* labels, long long nbytes, long long* counts, void* workspace,
                                  size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(labels && counts && workspace, "label_prepare: null pointer");
    ISWM_REQUIRE(nbytes > 0 && nbytes % 16 == 0 && aligned16(labels),
                 "label_prepare: need nbytes > 0, a multiple of 16, and a 16-byte aligned arena");
    const int nb = prepare_blocks(nbytes);
    ISWM_REQUIRE(workspace_bytes >= (size_t)nb * sizeof(long long),
                 "label_prepare: workspace too small (see iswm_label_prepare_workspace)");
    hipLaunchKernelGGL(k_label_prepare, dim3(nb), dim3(DS_BLOCK), 0, (hipStream_t)stream, reinterpret_cast<uint4*>(labels),
                       nbytes / 16, (long long*)workspace);
    if (int rc = check_launch("label_prepare")) return rc;
    hipLaunchKernelGGL(k_count_finalize<1>, dim3(1), dim3(DS_BLOCK), 0, (hipStream_t)stream, (const long long*)workspace,
                       nb, nbytes, counts);
    return check_launch("label_prepare_finalize");
}

extern "C" size_t iswm_label_count_workspace(long long n) {
    if (n <= 0) return 0;
    return (size_t)count_blocks(n) * 2 * sizeof(long long);
}

extern "C" int iswm_label_count(const unsigned char* labels, long long n, int ignore_index, long long* counts_accum,
                                void* workspace, size_t workspace_bytes, iswm_stream_t stream) {
    ISWM_REQUIRE(labels && counts_accum && workspace, "label_count: null pointer");
    ISWM_REQUIRE(n > 0 && aligned16(labels), "label_count: need n > 0 and 16-byte aligned labels");
    ISWM_REQUIRE(ignore_index >= -1 && ignore_index <= 255, "label_count: ignore_index is -1 (none) or a uint8 value");
    const int nb = count_blocks(n);
    ISWM_REQUIRE(workspace_bytes >= (size_t)nb * 2 * sizeof(long long),
                 "label_count: workspace too small (see iswm_label_count_workspace)");
    hipLaunchKernelGGL(k_label_count, dim3(nb), dim3(DS_BLOCK), 0, (hipStream_t)stream, labels, n, ignore_index,
                       (long long*)workspace);
    if (int rc = check_launch("label_count")) return rc;
    hipLaunchKernelGGL(k_count_finalize<2>, dim3(1), dim3(DS_BLOCK), 0, (hipStream_t)stream, (const long long*)workspace,
                       nb, n, counts_accum);
    return check_launch("label_count_finalize");
}

extern "C" size_t iswm_aug_tables_workspace(const void* host_samples, int B) {
    static_assert(sizeof(AugSampleT) == 64, "iswm_aug_sample layout");
    if (!host_samples || B <= 0) return 0;
    const long long ints = host_table_ints((const AugSampleT*)host_samples, B);
    return ints <= 0 ? 0 : (size_t)ints * sizeof(int);
}

extern "C" int iswm_aug_tables(const void* samples, int B, int max_rs, int* tables, size_t tables_bytes,
                               iswm_stream_t stream) {
    ISWM_REQUIRE(samples && tables, "aug_tables: null pointer");
    ISWM_REQUIRE(B > 0 && B <= 65535 && max_rs > 0, "aug_tables: need 0 < B <= 65535 and max_rs > 0");
    ISWM_REQUIRE(tables_bytes >= sizeof(int), "aug_tables: empty table buffer (see iswm_aug_tables_workspace)");
    const int row_blocks = (int)((2LL * max_rs + DS_BLOCK - 1) / DS_BLOCK);
    hipLaunchKernelGGL(k_aug_tables, dim3(row_blocks + 1, B), dim3(DS_BLOCK), 0, (hipStream_t)stream,
                       (const AugSampleT*)samples, tables, (long long)(tables_bytes / sizeof(int)));
    return check_launch("aug_tables");
}

extern "C" int iswm_gather_normalize(const unsigned char* images, const unsigned char* labels, const long long* offsets,
                                     int B, int H, int W, const float* mean3, const float* std3, float* out_nchw,
                                     unsigned char* out_labels, iswm_stream_t stream) {
    ISWM_REQUIRE(images && labels && offsets && mean3 && std3 && out_nchw && out_labels, "gather_normalize: null pointer");
    ISWM_REQUIRE(B > 0 && H > 0 && W > 0, "gather_normalize: bad size");
    ISWM_REQUIRE(aligned16(images) && aligned16(labels) && aligned16(out_nchw) && aligned16(out_labels),
                 "gather_normalize: arenas and outputs must be 16-byte aligned");
    const int64_t HW = (int64_t)H * W;
    hipLaunchKernelGGL(k_gather_normalize, dim3(stream_grid((int64_t)B * ((HW + 3) / 4), DS_BLOCK)), dim3(DS_BLOCK), 0,
                       (hipStream_t)stream, images, labels, offsets, B, HW, mean3[0], mean3[1], mean3[2], std3[0], std3[1],
                       std3[2], out_nchw, out_labels);
    return check_launch("gather_normalize");
}
