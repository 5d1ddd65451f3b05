// Validation image panels on the device: what the reference's save_validation_results (train.py:461-523) computes on
// the host for one frame -- Denormalize -> * 255 -> uint8, softmax -> max -> (confidence, pred), decode_target of the
// label and of the prediction, the 0.7-alpha composite it asks matplotlib for -- plus an error map, in one pass over
// (normalised input, the classifier's low-resolution logits, labels).  DESIGN.md section 16.
//   * original: t = ((x - M) / S) * 255.0f with M = float32(-mean / std), S = float32(1 / std) (utils/utils.py:14-24
//     through torchvision's normalize), every operation IEEE fp32 and uncontracted, truncated toward zero.  Not the
//     source pixel: for 224 of the 768 (channel, value) pairs of ToTensor + Normalize output it is value - 1, as in the
//     reference's files.  Values no uint8 image produces are clamped (t < 0 or NaN -> 0, t > 255 -> 255).
//   * pred: the first maximal class of the bilinearly up-sampled logits (ops.argmax_nchw's strict compare), the
//     logits sampled as k_bilinear_to_nchw_fwd samples them (sample4 below), so the mask is the one the metrics score.
//   * conf = (uint8)(p * 255.0f), p = 1 / sum_c expf(l_c - m), m = max_c l_c, summed in class order: fg_prob's
//     arithmetic (predict.hip) with the maximal class in place of fg; C <= 16 keeps the logits in registers, larger
//     C samples twice.
//   * target_rgb / pred_rgb = palette[label] / palette[pred]; overlay = (3 * original + 7 * pred_rgb + 5) / 10;
//     error: see error_colour.
// The launch shape is k_predict_maps's: grid (blocks_per_image, N), 16 consecutive raster pixels per thread, 16-B
// stores for a chunk that lies wholly inside one image (one per grey map, three per RGB panel), bytewise otherwise.
#include "bilinear.h"
#include "rowmap.h"

// Every fp32 expression of this file is written out operation by operation and nothing may be fused behind its back:
// a * b + c below is two roundings, fmaf one.  The sampling and softmax code uses the plain operators, which this
// pragma governs, and not __fmul_rn / __fadd_rn: those are header functions compiled under the default contraction
// mode, and their product and sum may still be fused once they are inlined.
#pragma clang fp contract(off)

namespace iswm {

constexpr int VP_BLOCK = 256;
constexpr int VP_PIX = 16;
constexpr int VP_MAX_GROUPS = 4;

struct ValPanelsArgs {
    const float* x;
    const float* yl;
    const void* labels;
    const unsigned char* palette;
    unsigned char *original, *pred, *conf, *target_rgb, *pred_rgb, *overlay, *error;
    float* prob;
    int label_dtype, Hi, Wi, ldx, C, Ho, Wo;
    float sh, sw;
    float dm[3], ds[3];
};

// src_index (bilinear.h) as every kernel of the library carries it: scale * (dst + 0.5f) - 0.5f is ONE fused
// multiply-add there (the compiler contracts it; tests/streaming_ref.py restates it so), written out here
__device__ __forceinline__ Lerp src_index_fma(float scale, int dst, int in_size) {
    float src = fmaf(scale, (float)dst + 0.5f, -0.5f);
    if (src < 0.f) src = 0.f;
    Lerp r;
    r.i0 = (int)src;
    if (r.i0 > in_size - 1) r.i0 = in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

// lh.l0 * (lw.l0 * a + lw.l1 * b) + lh.l1 * (lw.l0 * d + lw.l1 * e) for the four channels c0 .. c0 + 3, each with the
// roundings k_bilinear_to_nchw_fwd gives that lane of its float4 group (read from the kernel's assembly; DESIGN.md
// section 16): lanes 0 and 1 take the two rows as one packed fma each and add two rounded products, lanes 2 and 3 fuse
// the last product.  model(x) is that kernel's output, so these are its logits bit for bit; the GPU test pins it.
__device__ __forceinline__ float4 sample4(const float* pa, const float* pb, const float* pd, const float* pe,
                                          const Lerp& lh, const Lerp& lw, int c0) {
    const float4 a = ld4(pa + c0), b = ld4(pb + c0), d = ld4(pd + c0), e = ld4(pe + c0);
    float4 o;
    {
        const float top = fmaf(lw.l1, b.x, lw.l0 * a.x), bot = fmaf(lw.l0, d.x, lw.l1 * e.x);
        o.x = lh.l0 * top + lh.l1 * bot;
    }
    {
        const float top = fmaf(lw.l0, a.y, lw.l1 * b.y), bot = fmaf(lw.l1, e.y, lw.l0 * d.y);
        o.y = lh.l0 * top + lh.l1 * bot;
    }
    {
        const float top = fmaf(lw.l0, a.z, lw.l1 * b.z), bot = fmaf(lw.l0, d.z, lw.l1 * e.z);
        o.z = fmaf(lh.l0, top, lh.l1 * bot);
    }
    {
        const float top = fmaf(lw.l0, a.w, lw.l1 * b.w), bot = fmaf(lw.l0, d.w, lw.l1 * e.w);
        o.w = fmaf(lh.l0, top, lh.l1 * bot);
    }
    return o;
}

__device__ __forceinline__ float lane(const float4& v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// (p_max, argmax) of one pixel: the first maximal class (strict compare in class order, torch.max's rule) and
// 1 / sum_c expf(l_c - m)
template <int G>
__device__ __forceinline__ float max_prob(const float* pa, const float* pb, const float* pd, const float* pe,
                                          const Lerp& lh, const Lerp& lw, int C, int* cls) {
    float m;
    int bi = 0;
    float s = 0.f;
    if constexpr (G > 0) {
        float4 v[G];
#pragma unroll
        for (int g = 0; g < G; ++g) v[g] = sample4(pa, pb, pd, pe, lh, lw, 4 * g);
        m = v[0].x;
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < C && lane(v[g], k) > m) {
                    m = lane(v[g], k);
                    bi = 4 * g + k;
                }
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (4 * g + k < C) s = s + expf(lane(v[g], k) - m);
    } else {                     // C > 16: sample twice (the same arithmetic gives the same logits)
        m = sample4(pa, pb, pd, pe, lh, lw, 0).x;
        for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 v = sample4(pa, pb, pd, pe, lh, lw, c0);
            for (int k = 0; k < 4 && c0 + k < C; ++k)
                if (lane(v, k) > m) {
                    m = lane(v, k);
                    bi = c0 + k;
                }
        }
        for (int c0 = 0; c0 < C; c0 += 4) {
            const float4 v = sample4(pa, pb, pd, pe, lh, lw, c0);
            for (int k = 0; k < 4 && c0 + k < C; ++k) s = s + expf(lane(v, k) - m);
        }
    }
    *cls = bi;
    return __fdiv_rn(1.0f, s);
}

// the reference's Denormalize -> * 255 -> astype(uint8) for one value; out-of-range and NaN clamp (numpy wraps)
__device__ __forceinline__ unsigned int denorm_u8(float x, float m, float s) {
    const float t = __fmul_rn(__fdiv_rn(__fsub_rn(x, m), s), 255.0f);
    if (!(t >= 0.f)) return 0u;
    if (t > 255.f) return 255u;
    return (unsigned int)t;
}

// colours are 0x00BBGGRR.  label 255 (ignore): grey; right: black on background, white on foreground; a missed
// foreground pixel blue, a false one red, the wrong foreground class magenta
__device__ __forceinline__ unsigned int error_colour(unsigned int label, unsigned int pred) {
    if (label == 255u) return 0x808080u;
    if (pred == label) return label == 0u ? 0x000000u : 0xffffffu;
    if (label == 0u) return 0x0000ffu;
    if (pred == 0u) return 0xff0000u;
    return 0xff00ffu;
}

__device__ __forceinline__ unsigned int byte_of(const unsigned int (&w)[4], int j) { return (w[j >> 2] >> (8 * (j & 3))) & 255u; }

// one grey map: 16 bytes of a chunk
__device__ __forceinline__ void store_grey(unsigned char* __restrict__ out, int64_t q0, int j0, int j1,
                                           const unsigned int (&w)[4]) {
    if (j0 == 0 && j1 == VP_PIX) {
        *reinterpret_cast<uint4*>(out + q0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
#pragma unroll
        for (int j = 0; j < VP_PIX; ++j)
            if (j >= j0 && j < j1) out[q0 + j] = (unsigned char)byte_of(w, j);
    }
}

// one RGB panel: the 48 bytes of a chunk's 16 colours (0x00BBGGRR) as R, G, B per pixel
__device__ __forceinline__ void store_rgb(unsigned char* __restrict__ out, int64_t q0, int j0, int j1,
                                          const unsigned int (&col)[VP_PIX]) {
    if (j0 == 0 && j1 == VP_PIX) {
        unsigned int w[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) w[i] = 0u;
#pragma unroll
        for (int j = 0; j < VP_PIX; ++j)
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int idx = 3 * j + c;
                w[idx >> 2] |= ((col[j] >> (8 * c)) & 255u) << (8 * (idx & 3));
            }
        uint4* o = reinterpret_cast<uint4*>(out + 3 * q0);
        o[0] = make_uint4(w[0], w[1], w[2], w[3]);
        o[1] = make_uint4(w[4], w[5], w[6], w[7]);
        o[2] = make_uint4(w[8], w[9], w[10], w[11]);
    } else {
#pragma unroll
        for (int j = 0; j < VP_PIX; ++j)
            if (j >= j0 && j < j1) {
                unsigned char* o = out + 3 * (q0 + j);
                o[0] = (unsigned char)(col[j] & 255u);
                o[1] = (unsigned char)((col[j] >> 8) & 255u);
                o[2] = (unsigned char)((col[j] >> 16) & 255u);
            }
    }
}

// grid (blocks_per_image, N).  Image n owns the raster pixels [n*H*W, (n+1)*H*W) of the [N, H, W] maps; a thread takes
// the 16-pixel chunks of the whole tensor that overlap its image and produces the pixels of the chunk inside it, as
// k_predict_maps does.  A NULL output is skipped, and so is everything only it needs (the host entry checks that
// every requested output has its inputs).
template <int G>
__global__ __launch_bounds__(VP_BLOCK) void k_val_panels(const ValPanelsArgs a) {
    __shared__ unsigned int pal[256];
    if (a.palette) {
        for (int i = threadIdx.x; i < 256; i += VP_BLOCK)
            pal[i] = (unsigned int)a.palette[3 * i] | ((unsigned int)a.palette[3 * i + 1] << 8) |
                     ((unsigned int)a.palette[3 * i + 2] << 16);
    }
    __syncthreads();

    const int n = blockIdx.y;
    const int64_t HW = (int64_t)a.Ho * a.Wo;
    const int64_t p_begin = (int64_t)n * HW, p_end = p_begin + HW;
    const int64_t k_begin = p_begin / VP_PIX, k_end = (p_end + VP_PIX - 1) / VP_PIX;
    const float* base = a.yl ? a.yl + (size_t)n * a.Hi * a.Wi * a.ldx : nullptr;

    for (int64_t k = k_begin + (int64_t)blockIdx.x * VP_BLOCK + threadIdx.x; k < k_end;
         k += (int64_t)gridDim.x * VP_BLOCK) {
        const int64_t q0 = k * VP_PIX;
        const int j0 = q0 < p_begin ? (int)(p_begin - q0) : 0;
        const int j1 = q0 + VP_PIX > p_end ? (int)(p_end - q0) : VP_PIX;
        const bool full = j0 == 0 && j1 == VP_PIX;

        // original: three planes of x -> three times 16 bytes
        unsigned int wo[3][4] = {{0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}, {0u, 0u, 0u, 0u}};
        if (a.x) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                // pixel j of the chunk is xp[j]; for j < j0 that lies before the plane and is never read
                const float* xp = a.x + ((int64_t)n * 3 + c) * HW + (q0 - p_begin);
                float xv[VP_PIX];
                if (full && (reinterpret_cast<uintptr_t>(xp) & 15) == 0) {
#pragma unroll
                    for (int j = 0; j < VP_PIX; j += 4) {
                        const float4 v = *reinterpret_cast<const float4*>(xp + j);
                        xv[j] = v.x;
                        xv[j + 1] = v.y;
                        xv[j + 2] = v.z;
                        xv[j + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int j = 0; j < VP_PIX; ++j) xv[j] = (j >= j0 && j < j1) ? xp[j] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < VP_PIX; ++j) wo[c][j >> 2] |= denorm_u8(xv[j], a.dm[c], a.ds[c]) << (8 * (j & 3));
            }
        }

        // labels as bytes (the low byte of an int64 class index)
        unsigned int wl[4] = {0u, 0u, 0u, 0u};
        if (a.labels) {
            if (a.label_dtype == 0) {
                const unsigned char* lp = static_cast<const unsigned char*>(a.labels) + q0;
                if (full && (reinterpret_cast<uintptr_t>(lp) & 15) == 0) {
                    const uint4 v = *reinterpret_cast<const uint4*>(lp);
                    wl[0] = v.x;
                    wl[1] = v.y;
                    wl[2] = v.z;
                    wl[3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < VP_PIX; ++j)
                        if (j >= j0 && j < j1) wl[j >> 2] |= (unsigned int)lp[j] << (8 * (j & 3));
                }
            } else {
                const long long* lp = static_cast<const long long*>(a.labels) + q0;
#pragma unroll
                for (int j = 0; j < VP_PIX; ++j)
                    if (j >= j0 && j < j1) wl[j >> 2] |= ((unsigned int)lp[j] & 255u) << (8 * (j & 3));
            }
        }

        // class index, confidence and p_max
        unsigned int wp[4] = {0u, 0u, 0u, 0u}, wc[4] = {0u, 0u, 0u, 0u};
        float pv[VP_PIX];
#pragma unroll
        for (int j = 0; j < VP_PIX; ++j) pv[j] = 0.f;
        if (a.yl) {
            const int rem = (int)(q0 + j0 - p_begin);
            int oh = rem / a.Wo, ow = rem - oh * a.Wo;
            Lerp lh = src_index_fma(a.sh, oh, a.Hi);
#pragma unroll
            for (int j = 0; j < VP_PIX; ++j) {
                if (j < j0 || j >= j1) continue;
                const Lerp lw = src_index_fma(a.sw, ow, a.Wi);
                const float* pa = base + ((size_t)lh.i0 * a.Wi + lw.i0) * a.ldx;
                const float* pb = base + ((size_t)lh.i0 * a.Wi + lw.i1) * a.ldx;
                const float* pd = base + ((size_t)lh.i1 * a.Wi + lw.i0) * a.ldx;
                const float* pe = base + ((size_t)lh.i1 * a.Wi + lw.i1) * a.ldx;
                int cls;
                const float p = max_prob<G>(pa, pb, pd, pe, lh, lw, a.C, &cls);
                pv[j] = p;
                wp[j >> 2] |= (unsigned int)cls << (8 * (j & 3));
                wc[j >> 2] |= (unsigned int)(p * 255.0f) << (8 * (j & 3));
                if (++ow == a.Wo) {
                    ow = 0;
                    lh = src_index_fma(a.sh, ++oh, a.Hi);
                }
            }
        }

        if (a.pred) store_grey(a.pred, q0, j0, j1, wp);
        if (a.conf) store_grey(a.conf, q0, j0, j1, wc);
        if (a.prob) {
            if (full) {
#pragma unroll
                for (int j = 0; j < VP_PIX; j += 4)
                    *reinterpret_cast<float4*>(a.prob + q0 + j) = make_float4(pv[j], pv[j + 1], pv[j + 2], pv[j + 3]);
            } else {
#pragma unroll
                for (int j = 0; j < VP_PIX; ++j)
                    if (j >= j0 && j < j1) a.prob[q0 + j] = pv[j];
            }
        }

        unsigned int co[VP_PIX], cp[VP_PIX], ct[VP_PIX];
#pragma unroll
        for (int j = 0; j < VP_PIX; ++j) {
            co[j] = byte_of(wo[0], j) | (byte_of(wo[1], j) << 8) | (byte_of(wo[2], j) << 16);
            cp[j] = a.palette ? pal[byte_of(wp, j)] : 0u;
        }
        if (a.original) store_rgb(a.original, q0, j0, j1, co);
        if (a.pred_rgb) store_rgb(a.pred_rgb, q0, j0, j1, cp);
        if (a.target_rgb) {
#pragma unroll
            for (int j = 0; j < VP_PIX; ++j) ct[j] = pal[byte_of(wl, j)];
            store_rgb(a.target_rgb, q0, j0, j1, ct);
        }
        if (a.overlay) {
#pragma unroll
            for (int j = 0; j < VP_PIX; ++j) {
                unsigned int v = 0u;
#pragma unroll
                for (int c = 0; c < 3; ++c)
                    v |= ((3u * ((co[j] >> (8 * c)) & 255u) + 7u * ((cp[j] >> (8 * c)) & 255u) + 5u) / 10u) << (8 * c);
                ct[j] = v;
            }
            store_rgb(a.overlay, q0, j0, j1, ct);
        }
        if (a.error) {
#pragma unroll
            for (int j = 0; j < VP_PIX; ++j) ct[j] = error_colour(byte_of(wl, j), byte_of(wp, j));
            store_rgb(a.error, q0, j0, j1, ct);
        }
    }
}

// workgroups per image: about one chunk per thread, at most ~2048 workgroups in all (predict_maps's rule)
static int panels_blocks_per_image(int N, int H, int W) {
    const int64_t chunks = ((int64_t)H * W + VP_PIX - 1) / VP_PIX + 1;
    int64_t b = (chunks + VP_BLOCK - 1) / VP_BLOCK;
    const int64_t cap = N >= 2048 ? 1 : 2048 / N;
    if (b > cap) b = cap;
    if (b < 1) b = 1;
    return (int)b;
}

}  // namespace iswm

using namespace iswm;

extern "C" int iswm_val_panels(const float* x, const float* yl, const void* labels, int label_dtype, int N, int Hi,
                               int Wi, int ldx, int C, int H, int W, const float* denorm_mean3,
                               const float* denorm_std3, const unsigned char* palette, unsigned char* original,
                               unsigned char* pred, unsigned char* conf, float* prob, unsigned char* target_rgb,
                               unsigned char* pred_rgb, unsigned char* overlay, unsigned char* error,
                               iswm_stream_t stream) {
    ISWM_REQUIRE(original || pred || conf || prob || target_rgb || pred_rgb || overlay || error,
                 "val_panels: no output requested (every output pointer is null)");
    ISWM_REQUIRE(N > 0 && N <= 65535 && H > 0 && W > 0, "val_panels: bad size");
    ISWM_REQUIRE((int64_t)H * W <= 0x7fffffff, "val_panels: %d x %d pixels per image are too many", H, W);
    const bool need_x = original || overlay;
    const bool need_yl = pred || conf || prob || pred_rgb || overlay || error;
    const bool need_labels = target_rgb || error;
    const bool need_palette = target_rgb || pred_rgb || overlay;
    ISWM_REQUIRE(!need_x || (x && denorm_mean3 && denorm_std3),
                 "val_panels: original / overlay need x and the two denormalisation triples (null pointer)");
    ISWM_REQUIRE(!need_yl || yl, "val_panels: pred / conf / prob / pred_rgb / overlay / error need the logits (null pointer)");
    ISWM_REQUIRE(!need_labels || labels, "val_panels: target_rgb / error need the labels (null pointer)");
    ISWM_REQUIRE(!need_palette || palette, "val_panels: target_rgb / pred_rgb / overlay need the palette (null pointer)");
    ISWM_REQUIRE(!need_labels || label_dtype == 0 || label_dtype == 1, "val_panels: dtype codes are 0 (uint8) and 1 (int64)");
    if (need_yl) {
        ISWM_REQUIRE(Hi > 0 && Wi > 0, "val_panels: bad low-resolution size %d x %d", Hi, Wi);
        ISWM_REQUIRE(C > 0 && C <= 256 && ldx % 4 == 0 && ldx >= ((C + 3) / 4) * 4,
                     "val_panels: need 1 <= C <= 256, ldx %% 4 == 0, ldx >= pad4(C)");
    }
    ISWM_REQUIRE((!need_x || aligned16(x)) && (!need_yl || aligned16(yl)), "val_panels: x and yl must be 16-byte aligned");
    ISWM_REQUIRE(aligned16(original) && aligned16(pred) && aligned16(conf) && aligned16(prob) && aligned16(target_rgb) &&
                     aligned16(pred_rgb) && aligned16(overlay) && aligned16(error),
                 "val_panels: output pointers must be 16-byte aligned");
    ValPanelsArgs a = {};
    a.x = need_x ? x : nullptr;
    a.yl = need_yl ? yl : nullptr;
    a.labels = need_labels ? labels : nullptr;
    a.palette = need_palette ? palette : nullptr;
    a.original = original;
    a.pred = pred;
    a.conf = conf;
    a.prob = prob;
    a.target_rgb = target_rgb;
    a.pred_rgb = pred_rgb;
    a.overlay = overlay;
    a.error = error;
    a.label_dtype = label_dtype;
    a.Hi = Hi;
    a.Wi = Wi;
    a.ldx = ldx;
    a.C = C;
    a.Ho = H;
    a.Wo = W;
    if (need_yl) {
        a.sh = (float)Hi / (float)H;
        a.sw = (float)Wi / (float)W;
    }
    for (int c = 0; c < 3 && need_x; ++c) {
        a.dm[c] = denorm_mean3[c];
        a.ds[c] = denorm_std3[c];
    }
    const dim3 grid(panels_blocks_per_image(N, H, W), N);
    const int groups = need_yl ? (C + 3) / 4 : 1;
#define ISWM_VP(G) hipLaunchKernelGGL(k_val_panels<G>, grid, dim3(VP_BLOCK), 0, (hipStream_t)stream, a)
    switch (groups > VP_MAX_GROUPS ? 0 : groups) {
        case 1: ISWM_VP(1); break;
        case 2: ISWM_VP(2); break;
        case 3: ISWM_VP(3); break;
        case 4: ISWM_VP(4); break;
        default: ISWM_VP(0); break;
    }
#undef ISWM_VP
    return check_launch("val_panels");
}
