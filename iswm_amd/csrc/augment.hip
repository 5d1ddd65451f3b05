// Training-input pipeline on the device: the reference's per-sample PIL chain
//   ExtRandomScale (bilinear / nearest resize) -> ExtRandomCrop(pad_if_needed) -> ExtRandomHorizontalFlip
//   -> ExtToTensor -> ExtNormalize                        (train.py:355-362, utils/ext_transforms.py:94-115,212-396)
// as ONE kernel over the whole batch, reading the uint8 source tiles and writing the normalised fp32 NCHW batch
// plus the uint8 label batch.  Only the crop window is ever computed.
//
// Bit-exactness with Pillow (the arithmetic the reference runs on, Resample.c / Geometry.c):
//   * image: Pillow's 8-bit antialiased BILINEAR resample is a horizontal pass into a uint8 temporary followed by a
//     vertical pass, each a fixed-point (22 fractional bits) weighted sum rounded and clipped to uint8.  The
//     per-output-column / per-output-row bounds and integer weights are computed on the host in double exactly as
//     precompute_coeffs / normalize_coeffs_8bpc do and passed in a table; the kernel evaluates the same two integer
//     sums (the horizontal values of the rows a pixel needs are recomputed on the fly -- at most 5 x 5 taps);
//   * label: Pillow's NEAREST resize walks source coordinates by repeated double addition; the host performs the
//     same additions and passes the integer source index per output column / row;
//   * ToTensor / Normalize: v / 255.0f, then (x - mean) / std in IEEE fp32, as torch does.
#pragma clang fp contract(off)
#include "common.h"

namespace iswm {

constexpr int AUG_PRECISION_BITS = 22;   // Pillow: 32 - 8 - 2

using AugSample = iswm_aug_sample;

__device__ __forceinline__ int clip8(int v) {
    v >>= AUG_PRECISION_BITS;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// tables of one sample (ints): xintab[rs_w] | yintab[rs_h] | hbounds[rs_w][2] | hk[rs_w][ksize_h] |
//                              vbounds[rs_h][2] | vk[rs_h][ksize_v]
// One pixel of the crop BEFORE any flip: (cy, cx) are crop coordinates, img / lbl the sample's source tile.
__device__ __forceinline__ void aug_pixel(const unsigned char* __restrict__ img, const unsigned char* __restrict__ lbl,
                                          const AugSample& s, const int* __restrict__ tables, int cy, int cx, int& v0,
                                          int& v1, int& v2, int& lab) {
    const int ry = s.crop_i + cy - s.pad, rx = s.crop_j + cx - s.pad;         // coordinates in the resized image
    v0 = v1 = v2 = lab = 0;                                                  // padding: image 0, label 0
    if (ry >= 0 && ry < s.rs_h && rx >= 0 && rx < s.rs_w) {
        const int* tab = tables + s.tab_off;
        const int* xintab = tab;
        const int* yintab = xintab + s.rs_w;
        const int* hb = yintab + s.rs_h;
        const int* hk = hb + 2 * s.rs_w;
        const int* vb = hk + (size_t)s.rs_w * s.ksize_h;
        const int* vk = vb + 2 * s.rs_h;
        lab = lbl[(long long)yintab[ry] * s.src_w + xintab[rx]];
        const int xmin = hb[2 * rx], xcnt = hb[2 * rx + 1];
        const int ymin = vb[2 * ry], ycnt = vb[2 * ry + 1];
        const int* kx = hk + (size_t)rx * s.ksize_h;
        const int* ky = vk + (size_t)ry * s.ksize_v;
        int a0 = 1 << (AUG_PRECISION_BITS - 1), a1 = a0, a2 = a0;
        for (int r = 0; r < ycnt; ++r) {
            const unsigned char* row = img + ((long long)(ymin + r) * s.src_w + xmin) * 3;
            int h0 = 1 << (AUG_PRECISION_BITS - 1), h1 = h0, h2 = h0;
            for (int c = 0; c < xcnt; ++c) {
                const int k = kx[c];
                h0 += row[3 * c] * k;
                h1 += row[3 * c + 1] * k;
                h2 += row[3 * c + 2] * k;
            }
            const int k = ky[r];
            a0 += clip8(h0) * k;
            a1 += clip8(h1) * k;
            a2 += clip8(h2) * k;
        }
        v0 = clip8(a0);
        v1 = clip8(a1);
        v2 = clip8(a2);
    }
}

// ToTensor + Normalize of one pixel into the NCHW batch
__device__ __forceinline__ void aug_store(float* __restrict__ o, size_t plane, int v0, int v1, int v2, float m0, float m1,
                                          float m2, float s0, float s1, float s2) {
    o[0] = __fdiv_rn(__fdiv_rn((float)v0, 255.0f) - m0, s0);
    o[plane] = __fdiv_rn(__fdiv_rn((float)v1, 255.0f) - m1, s1);
    o[2 * plane] = __fdiv_rn(__fdiv_rn((float)v2, 255.0f) - m2, s2);
}

__global__ __launch_bounds__(256) void k_augment(const unsigned char* __restrict__ images,
                                                 const unsigned char* __restrict__ labels,
                                                 const AugSample* __restrict__ samples, const int* __restrict__ tables,
                                                 int B, int TH, int TW, float m0, float m1, float m2, float s0, float s1,
                                                 float s2, float* __restrict__ out, unsigned char* __restrict__ out_lbl) {
    const long long npix = (long long)B * TH * TW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / ((long long)TH * TW));
        const int rem = (int)(i - (long long)b * TH * TW);
        const int y = rem / TW, x = rem - y * TW;
        const AugSample s = samples[b];
        int v0, v1, v2, lab;
        aug_pixel(images + s.img_off, labels + s.lbl_off, s, tables, y, s.flip ? TW - 1 - x : x, v0, v1, v2, lab);
        const size_t plane = (size_t)TH * TW;
        aug_store(out + (size_t)b * 3 * plane + (size_t)y * TW + x, plane, v0, v1, v2, m0, m1, m2, s0, s1, s2);
        out_lbl[i] = (unsigned char)lab;
    }
}

// ---- rotation, vertical flip, colour jitter ----------------------------------------------------
using AugExtra = iswm_aug_extra;

constexpr int AUG_SUM_BLOCKS = 64;       // partial grey sums per sample (k_augment_gray_sum's grid.x)

// Pillow Geometry.c affine_fixed (nearest): integer arithmetic only.  One thread per pixel of the rotated tile.
__global__ __launch_bounds__(256) void k_aug_rotate(const unsigned char* __restrict__ images,
                                                    const unsigned char* __restrict__ labels,
                                                    const AugSample* __restrict__ samples,
                                                    const AugExtra* __restrict__ extras, unsigned char* __restrict__ rimg,
                                                    long long rimg_bytes, unsigned char* __restrict__ rlbl,
                                                    long long rlbl_bytes) {
    const AugExtra e = extras[blockIdx.y];
    if (e.rot_mode == 0) return;
    const AugSample s = samples[blockIdx.y];
    const long long hw = (long long)s.src_h * s.src_w;
    if (s.src_h < 1 || s.src_w < 1 || e.rot_img_off < 0 || e.rot_lbl_off < 0 || e.rot_img_off + hw * 3 > rimg_bytes ||
        e.rot_lbl_off + hw > rlbl_bytes)
        return;
    const unsigned char* img = images + s.img_off;
    const unsigned char* lbl = labels + s.lbl_off;
    unsigned char* oi = rimg + e.rot_img_off;
    unsigned char* ol = rlbl + e.rot_lbl_off;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < hw; i += (long long)gridDim.x * 256) {
        const int y = (int)(i / s.src_w), x = (int)(i - (long long)y * s.src_w);
        const long long xin = ((long long)e.a[2] + (long long)y * e.a[1] + (long long)x * e.a[0]) >> 16;
        const long long yin = ((long long)e.a[5] + (long long)y * e.a[4] + (long long)x * e.a[3]) >> 16;
        int v0 = 0, v1 = 0, v2 = 0, lab = 0;
        if (xin >= 0 && xin < s.src_w && yin >= 0 && yin < s.src_h) {
            const long long p = yin * s.src_w + xin;
            v0 = img[3 * p];
            v1 = img[3 * p + 1];
            v2 = img[3 * p + 2];
            lab = lbl[p];
        }
        oi[3 * i] = (unsigned char)v0;
        oi[3 * i + 1] = (unsigned char)v1;
        oi[3 * i + 2] = (unsigned char)v2;
        ol[i] = (unsigned char)lab;
    }
}

__device__ __forceinline__ int aug_gray(int r, int g, int b) { return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16; }

// Pillow Blend.c ImagingBlend(degenerate d, image v, alpha f) for one 8-bit value; fp32, no contraction
__device__ __forceinline__ int aug_blend(int d, int v, float f) {
    if (f == 0.0f) return d;
    if (f == 1.0f) return v;
    const float t = (float)d + f * (float)(v - d);
    if (f >= 0.0f && f <= 1.0f) return (int)(unsigned char)(int)t;
    return t <= 0.0f ? 0 : (t >= 255.0f ? 255 : (int)t);
}

__device__ __forceinline__ int aug_clip255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// Pillow Convert.c rgb2hsv_row, H shifted, hsv2rgb: the C expressions with their float / double types
__device__ __forceinline__ void aug_hue(int& r, int& g, int& b, int shift) {
    const int maxc = max(r, max(g, b)), minc = min(r, min(g, b));
    int uh = 0, us = 0;
    const int uv = maxc;
    if (minc != maxc) {
        const float cr = (float)(maxc - minc);
        const float s = __fdiv_rn(cr, (float)maxc);
        const float rc = __fdiv_rn((float)(maxc - r), cr);
        const float gc = __fdiv_rn((float)(maxc - g), cr);
        const float bc = __fdiv_rn((float)(maxc - b), cr);
        float h;
        if (r == maxc)
            h = bc - gc;
        else if (g == maxc)
            h = (float)(2.0 + (double)rc - (double)bc);
        else
            h = (float)(4.0 + (double)gc - (double)rc);
        const double hh = (double)h / 6.0 + 1.0;           // in (0.8, 1.9): fmod(hh, 1.0) == hh - floor(hh), exactly
        h = (float)(hh - floor(hh));
        uh = aug_clip255((int)((double)h * 255.0));
        us = aug_clip255((int)((double)s * 255.0));
    }
    uh = (uh + shift) & 255;
    if (us == 0) {
        r = g = b = uv;
        return;
    }
    const double h6 = (double)(float)uh * 6.0 / 255.0;
    const int i = (int)floor(h6);
    const float f = (float)(h6 - (double)(float)i);
    const float fs = (float)((double)(float)us / 255.0);
    const double v = (double)(float)uv;
    const int p = aug_clip255((int)round(v * (1.0 - (double)fs)));
    const int q = aug_clip255((int)round(v * (1.0 - (double)fs * (double)f)));
    const int t = aug_clip255((int)round(v * (1.0 - (double)fs * (1.0 - (double)f))));
    switch (i % 6) {
        case 0: r = uv; g = t; b = p; break;
        case 1: r = q; g = uv; b = p; break;
        case 2: r = p; g = uv; b = t; break;
        case 3: r = p; g = q; b = uv; break;
        case 4: r = t; g = p; b = uv; break;
        default: r = uv; g = p; b = q; break;
    }
}

// ops[first, last) of the sample's list on one pixel; `mean` is the contrast op's degenerate value
__device__ __forceinline__ void aug_ops(const AugExtra& e, int first, int last, int mean, int& v0, int& v1, int& v2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {                           // constant indices: the record stays in registers
        if (k < first || k >= last) continue;
        const int op = e.ops[k];
        if (op == ISWM_AUG_OP_BRIGHTNESS) {
            const float f = e.factor[ISWM_AUG_OP_BRIGHTNESS];
            v0 = aug_blend(0, v0, f);
            v1 = aug_blend(0, v1, f);
            v2 = aug_blend(0, v2, f);
        } else if (op == ISWM_AUG_OP_CONTRAST) {
            const float f = e.factor[ISWM_AUG_OP_CONTRAST];
            v0 = aug_blend(mean, v0, f);
            v1 = aug_blend(mean, v1, f);
            v2 = aug_blend(mean, v2, f);
        } else if (op == ISWM_AUG_OP_SATURATION) {
            const float f = e.factor[ISWM_AUG_OP_SATURATION];
            const int l = aug_gray(v0, v1, v2);
            v0 = aug_blend(l, v0, f);
            v1 = aug_blend(l, v1, f);
            v2 = aug_blend(l, v2, f);
        } else if (op == ISWM_AUG_OP_HUE) {
            aug_hue(v0, v1, v2, e.hue_shift);
        }
    }
}

__device__ __forceinline__ int aug_contrast_pos(const AugExtra& e) {
    int pos = -1;
#pragma unroll
    for (int k = 3; k >= 0; --k)
        if (k < e.n_ops && e.ops[k] == ISWM_AUG_OP_CONTRAST) pos = k;
    return pos;
}

// grid (AUG_SUM_BLOCKS, B): slab[b][block] = sum over the block's share of the crop of the grey of each pixel after the
// ops placed before the sample's contrast op (flips leave the sum alone and are skipped)
__global__ __launch_bounds__(256) void k_augment_gray_sum(const unsigned char* __restrict__ images,
                                                          const unsigned char* __restrict__ labels,
                                                          const unsigned char* __restrict__ rimg,
                                                          const unsigned char* __restrict__ rlbl,
                                                          const AugSample* __restrict__ samples,
                                                          const AugExtra* __restrict__ extras,
                                                          const int* __restrict__ tables, int TH, int TW,
                                                          long long* __restrict__ slab) {
    const int b = blockIdx.y;
    const AugExtra e = extras[b];
    const int cpos = aug_contrast_pos(e);
    long long sum = 0;
    if (cpos >= 0) {
        const AugSample s = samples[b];
        const unsigned char* img = e.rot_mode ? rimg + e.rot_img_off : images + s.img_off;
        const unsigned char* lbl = e.rot_mode ? rlbl + e.rot_lbl_off : labels + s.lbl_off;
        const int npix = TH * TW;                           // <= 2^30 (iswm_augment_batch_ex): i + stride cannot wrap
        for (int i = blockIdx.x * 256 + threadIdx.x; i < npix; i += AUG_SUM_BLOCKS * 256) {
            const int y = i / TW, x = i - y * TW;
            int v0, v1, v2, lab;
            aug_pixel(img, lbl, s, tables, y, x, v0, v1, v2, lab);
            aug_ops(e, 0, cpos, 0, v0, v1, v2);
            sum += aug_gray(v0, v1, v2);
        }
    }
    __shared__ long long red[4];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) slab[(size_t)b * AUG_SUM_BLOCKS + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// grid B, one wave: the sample's partials summed in index order; mean[b] = int(sum / count + 0.5) (fp64 division)
__global__ __launch_bounds__(64) void k_augment_gray_mean(const long long* __restrict__ slab, long long count,
                                                          int* __restrict__ mean) {
    static_assert(AUG_SUM_BLOCKS == 64, "one partial per lane");
    long long sum = slab[(size_t)blockIdx.x * AUG_SUM_BLOCKS + threadIdx.x];
    for (int off = 32; off > 0; off >>= 1) sum += __shfl_down(sum, off, 64);
    if (threadIdx.x == 0) mean[blockIdx.x] = (int)((double)sum / (double)count + 0.5);
}

__global__ __launch_bounds__(256) void k_augment_ex(const unsigned char* __restrict__ images,
                                                    const unsigned char* __restrict__ labels,
                                                    const unsigned char* __restrict__ rimg,
                                                    const unsigned char* __restrict__ rlbl,
                                                    const AugSample* __restrict__ samples,
                                                    const AugExtra* __restrict__ extras, const int* __restrict__ tables,
                                                    const int* __restrict__ means, int B, int TH, int TW, float m0,
                                                    float m1, float m2, float s0, float s1, float s2,
                                                    float* __restrict__ out, unsigned char* __restrict__ out_lbl) {
    const long long npix = (long long)B * TH * TW;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < npix; i += (long long)gridDim.x * 256) {
        const int b = (int)(i / ((long long)TH * TW));
        const int rem = (int)(i - (long long)b * TH * TW);
        const int y = rem / TW, x = rem - y * TW;
        const AugSample s = samples[b];
        const AugExtra e = extras[b];
        const unsigned char* img = e.rot_mode ? rimg + e.rot_img_off : images + s.img_off;
        const unsigned char* lbl = e.rot_mode ? rlbl + e.rot_lbl_off : labels + s.lbl_off;
        int v0, v1, v2, lab;
        aug_pixel(img, lbl, s, tables, (s.flip & 2) ? TH - 1 - y : y, (s.flip & 1) ? TW - 1 - x : x, v0, v1, v2, lab);
        const int n_ops = e.n_ops < 4 ? e.n_ops : 4;
        if (n_ops > 0) aug_ops(e, 0, n_ops, means ? means[b] : 0, v0, v1, v2);
        const size_t plane = (size_t)TH * TW;
        aug_store(out + (size_t)b * 3 * plane + (size_t)y * TW + x, plane, v0, v1, v2, m0, m1, m2, s0, s1, s2);
        out_lbl[i] = (unsigned char)lab;
    }
}

}  // namespace iswm

using namespace iswm;

extern "C" int iswm_augment_batch(const unsigned char* images, const unsigned char* labels, const void* samples,
                                  const int* tables, int B, int crop_h, int crop_w, const float* mean3,
                                  const float* std3, float* out_nchw, unsigned char* out_labels, iswm_stream_t stream) {
    ISWM_REQUIRE(images && labels && samples && tables && out_nchw && out_labels && mean3 && std3,
                 "augment_batch: null pointer");
    ISWM_REQUIRE(B > 0 && crop_h > 0 && crop_w > 0, "augment_batch: bad size");
    static_assert(sizeof(AugSample) == 64, "iswm_aug_sample layout");
    const long long npix = (long long)B * crop_h * crop_w;
    hipLaunchKernelGGL(k_augment, dim3(stream_grid(npix, 256)), dim3(256), 0, (hipStream_t)stream, images, labels,
                       (const AugSample*)samples, tables, B, crop_h, crop_w, mean3[0], mean3[1], mean3[2], std3[0],
                       std3[1], std3[2], out_nchw, out_labels);
    return check_launch("augment_batch");
}

extern "C" int iswm_aug_rotate(const unsigned char* images, const unsigned char* labels, const void* samples,
                               const void* extras, int B, long long max_hw, unsigned char* rot_images,
                               size_t rot_images_bytes, unsigned char* rot_labels, size_t rot_labels_bytes,
                               iswm_stream_t stream) {
    ISWM_REQUIRE(images && labels && samples && extras && rot_images && rot_labels, "aug_rotate: null pointer");
    ISWM_REQUIRE(B > 0 && B <= 65535 && max_hw > 0, "aug_rotate: need 0 < B <= 65535 and max_hw > 0");
    ISWM_REQUIRE(rot_images_bytes > 0 && rot_labels_bytes > 0, "aug_rotate: empty scratch arena");
    static_assert(sizeof(AugExtra) == 96, "iswm_aug_extra layout");
    hipLaunchKernelGGL(k_aug_rotate, dim3(stream_grid(max_hw, 256), B), dim3(256), 0, (hipStream_t)stream, images, labels,
                       (const AugSample*)samples, (const AugExtra*)extras, rot_images, (long long)rot_images_bytes,
                       rot_labels, (long long)rot_labels_bytes);
    return check_launch("aug_rotate");
}

extern "C" size_t iswm_augment_batch_ex_workspace(int B, int crop_h, int crop_w) {
    if (B <= 0 || crop_h <= 0 || crop_w <= 0) return 0;
    return (size_t)B * AUG_SUM_BLOCKS * sizeof(long long) + (size_t)B * sizeof(int);    // partials | means
}

extern "C" int iswm_augment_batch_ex(const unsigned char* images, const unsigned char* labels,
                                     const unsigned char* rot_images, const unsigned char* rot_labels,
                                     const void* samples, const void* extras, const int* tables, int B, int crop_h,
                                     int crop_w, const float* mean3, const float* std3, int any_contrast, float* out_nchw,
                                     unsigned char* out_labels, void* workspace, size_t workspace_bytes,
                                     iswm_stream_t stream) {
    ISWM_REQUIRE(images && labels && samples && extras && tables && out_nchw && out_labels && mean3 && std3 && workspace,
                 "augment_batch_ex: null pointer");
    ISWM_REQUIRE((rot_images == nullptr) == (rot_labels == nullptr),
                 "augment_batch_ex: rot_images and rot_labels are both given or both null");
    ISWM_REQUIRE(B > 0 && B <= 65535 && crop_h > 0 && crop_w > 0 && (long long)crop_h * crop_w <= (1LL << 30),
                 "augment_batch_ex: bad size (need 0 < B <= 65535 and 0 < crop_h * crop_w <= 2^30)");
    ISWM_REQUIRE(workspace_bytes >= iswm_augment_batch_ex_workspace(B, crop_h, crop_w) &&
                     (reinterpret_cast<uintptr_t>(workspace) & 7) == 0,
                 "augment_batch_ex: workspace too small or not 8-byte aligned (see iswm_augment_batch_ex_workspace)");
    long long* slab = (long long*)workspace;
    int* means = (int*)(slab + (size_t)B * AUG_SUM_BLOCKS);
    if (any_contrast) {
        hipLaunchKernelGGL(k_augment_gray_sum, dim3(AUG_SUM_BLOCKS, B), dim3(256), 0, (hipStream_t)stream, images, labels,
                           rot_images, rot_labels, (const AugSample*)samples, (const AugExtra*)extras, tables, crop_h,
                           crop_w, slab);
        if (int rc = check_launch("augment_gray_sum")) return rc;
        hipLaunchKernelGGL(k_augment_gray_mean, dim3(B), dim3(64), 0, (hipStream_t)stream, (const long long*)slab,
                           (long long)crop_h * crop_w, means);
        if (int rc = check_launch("augment_gray_mean")) return rc;
    }
    const long long npix = (long long)B * crop_h * crop_w;
    hipLaunchKernelGGL(k_augment_ex, dim3(stream_grid(npix, 256)), dim3(256), 0, (hipStream_t)stream, images, labels,
                       rot_images, rot_labels, (const AugSample*)samples, (const AugExtra*)extras, tables,
                       any_contrast ? (const int*)means : (const int*)nullptr, B, crop_h, crop_w, mean3[0], mean3[1],
                       mean3[2], std3[0], std3[1], std3[2], out_nchw, out_labels);
    return check_launch("augment_batch_ex");
}
