// Depthwise 3x3 convolution (pad == dil, stride 1 or 2) for MobileNetV2's inverted-residual blocks, where the depthwise
// stage is the memory-bound core of the network: forward fused with the BatchNorm tile statistics, and ONE backward launch
// for the data gradient and all nine taps of the weight gradient.  Pitched NHWC fp32, the torch parameter w[c][kh][kw]
// as is, channels >= Cw of a wider (zero-padded) buffer see zero weights -- the conventions of dwconv.hip, whose
// kernels these reproduce bit for bit (same fmaf chains in the same tap order).
//
// Tiling: a workgroup owns a run of consecutive raster-order pixels x a block of CQ channel quads (CQ = 16, 12 or 8 so
// that 96 / 144 / 576 / 960 channels leave no idle lanes); a thread owns one quad (16-byte accesses) and walks pixels
// RL apart.  The 3x3 window is NOT staged in LDS: a run of 64-128 raster pixels is about one image row, its three input
// rows are shared with the runs just before and after it, and xcd_remap puts those runs on the same XCD, so the halo
// rows are L2 hits while every element comes from HBM once.  What the kernels keep on chip instead is what the old path
// re-read from memory: the forward holds its y values in registers for the centred second moment, the backward holds the
// 9 x 4 weight-gradient sums of its run in registers.
#include "common.h"
#include "../../include/iswm_hip_sep.h"
#include "planes.h"

namespace iswm {

struct Dw3Args {
    const float* x;      // forward: input [N,H,W,ldx];  backward: the same (null: no weight gradient)
    const float* w;      // [Cw][9]
    const float* dy;     // backward: [N,Ho,Wo,ldy]
    float* y;            // forward: output [N,Ho,Wo,ldy];  backward: dx [N,H,W,lddx] (null: no data gradient)
    float* partials;     // forward: BatchNorm partials [2][tiles][C] or null;  backward: [chunks][9][C]
    int N, H, W, C, Cw, Ho, Wo, stride, dil, ldx, ldy, lddx;
    int CQ, RL, colblocks;
    int tiles, R;        // forward: statistic tiles of R output pixels
    int in_chunk, out_chunk, accumulate;     // backward: pixels per workgroup on the input / output grid
    int Pin, Pout;       // N*H*W, N*Ho*Wo
};

__device__ __forceinline__ float4 dw3_w4(const float* w, int c, int tap, int Cw) {
    float4 r;
    r.x = c + 0 < Cw ? w[(size_t)(c + 0) * 9 + tap] : 0.f;
    r.y = c + 1 < Cw ? w[(size_t)(c + 1) * 9 + tap] : 0.f;
    r.z = c + 2 < Cw ? w[(size_t)(c + 2) * 9 + tap] : 0.f;
    r.w = c + 3 < Cw ? w[(size_t)(c + 3) * 9 + tap] : 0.f;
    return r;
}

__device__ __forceinline__ float4 dw3_ld(const float* p) { return *reinterpret_cast<const float4*>(p); }

__device__ __forceinline__ void dw3_fma(float4& acc, const float4 a, const float4 b) {
    acc.x = fmaf(a.x, b.x, acc.x);
    acc.y = fmaf(a.y, b.y, acc.y);
    acc.z = fmaf(a.z, b.z, acc.z);
    acc.w = fmaf(a.w, b.w, acc.w);
}

// y = dwconv(x, w) and, with partials, per tile of R consecutive output pixels the column sum and the sum of squared
// deviations from the TILE mean (the pair iswm_bn_finalize merges).  block = CQ quads x RL pixel lanes, R = RL * PPT.
template <int PPT>
__global__ __launch_bounds__(256) void k_dw3_fwd_stats(const Dw3Args a) {
    __shared__ float4 red[256];
    __shared__ float4 mean_s[16];
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = lid / a.colblocks, cb = lid - tile * a.colblocks;
    const int pl = threadIdx.x / a.CQ, cg = threadIdx.x - pl * a.CQ;
    const int c4 = cb * a.CQ + cg, c = c4 * 4;
    const bool active = c4 < (a.C >> 2);
    const int r0 = tile * a.R, r1 = min(a.Pout, r0 + a.R);
    float4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = active ? dw3_w4(a.w, c, t, a.Cw) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 yv[PPT];
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int p = r0 + pl + j * a.RL;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (active && p < r1) {
            const int ow = p % a.Wo, q = p / a.Wo;
            const int oh = q % a.Ho, n = q / a.Ho;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = oh * a.stride + (kh - 1) * a.dil;
                if ((unsigned)ih >= (unsigned)a.H) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = ow * a.stride + (kw - 1) * a.dil;
                    if ((unsigned)iw >= (unsigned)a.W) continue;
                    dw3_fma(acc, dw3_ld(a.x + ((size_t)(n * a.H + ih) * a.W + iw) * a.ldx + c), wv[kh * 3 + kw]);
                }
            }
            *reinterpret_cast<float4*>(a.y + (size_t)p * a.ldy + c) = acc;
            s.x += acc.x; s.y += acc.y; s.z += acc.z; s.w += acc.w;
        }
        yv[j] = acc;
    }
    if (!a.partials) return;      // eval-mode BatchNorm: no statistics (uniform over the grid)
    const float cnt = (float)(r1 - r0);
    red[threadIdx.x] = s;
    __syncthreads();
    if (active && pl == 0) {
        for (int k = 1; k < a.RL; ++k) {      // fixed order
            const float4 v = red[k * a.CQ + cg];
            s.x += v.x; s.y += v.y; s.z += v.z; s.w += v.w;
        }
        *reinterpret_cast<float4*>(a.partials + (size_t)tile * a.C + c) = s;
        mean_s[cg] = make_float4(s.x / cnt, s.y / cnt, s.z / cnt, s.w / cnt);
    }
    __syncthreads();
    float4 m2 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (active) {
        const float4 mu = mean_s[cg];
#pragma unroll
        for (int j = 0; j < PPT; ++j)
            if (r0 + pl + j * a.RL < r1) {
                const float dx = yv[j].x - mu.x, dy = yv[j].y - mu.y, dz = yv[j].z - mu.z, dw = yv[j].w - mu.w;
                m2.x += dx * dx; m2.y += dy * dy; m2.z += dz * dz; m2.w += dw * dw;
            }
    }
    __syncthreads();
    red[threadIdx.x] = m2;
    __syncthreads();
    if (active && pl == 0) {
        for (int k = 1; k < a.RL; ++k) {
            const float4 v = red[k * a.CQ + cg];
            m2.x += v.x; m2.y += v.y; m2.z += v.z; m2.w += v.w;
        }
        *reinterpret_cast<float4*>(a.partials + (size_t)(a.tiles + tile) * a.C + c) = m2;
    }
}

// One workgroup = chunk `ch` of both pixel grids (output pixels [ch*out_chunk, ..) and input pixels [ch*in_chunk, ..): the
// same image region, so the dy rows of the second phase are the first phase's, still in L2) x a block of CQ channel quads.
//   phase 1: part[ch][tap][c] = sum over the chunk's output pixels of dy[p][c] * x[pin(p, tap)][c]   (fp32 fmaf per thread,
//            the RL pixel lanes summed in double in a fixed order)
//   phase 2: dx[n,ih,iw,c] (=|+=) sum over taps with (ih + dil - kh*dil) divisible by stride of dy[n,oh,ow,c] * w[c,kh,kw]
__global__ __launch_bounds__(256) void k_dw3_bwd(const Dw3Args a) {
    __shared__ float4 red[3][256];
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int ch = lid / a.colblocks, cb = lid - ch * a.colblocks;
    const int pl = threadIdx.x / a.CQ, cg = threadIdx.x - pl * a.CQ;
    const int c4 = cb * a.CQ + cg, c = c4 * 4;
    const bool active = c4 < (a.C >> 2);
    if (a.x) {
        float4 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int p0 = min(a.Pout, ch * a.out_chunk), p1 = min(a.Pout, p0 + a.out_chunk);
        if (active)
            for (int p = p0 + pl; p < p1; p += a.RL) {
                const int ow = p % a.Wo, q = p / a.Wo;
                const int oh = q % a.Ho, n = q / a.Ho;
                const float4 g = dw3_ld(a.dy + (size_t)p * a.ldy + c);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int ih = oh * a.stride + (kh - 1) * a.dil;
                    if ((unsigned)ih >= (unsigned)a.H) continue;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int iw = ow * a.stride + (kw - 1) * a.dil;
                        if ((unsigned)iw >= (unsigned)a.W) continue;
                        dw3_fma(acc[kh * 3 + kw], g, dw3_ld(a.x + ((size_t)(n * a.H + ih) * a.W + iw) * a.ldx + c));
                    }
                }
            }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            red[0][threadIdx.x] = acc[3 * r + 0];
            red[1][threadIdx.x] = acc[3 * r + 1];
            red[2][threadIdx.x] = acc[3 * r + 2];
            __syncthreads();
            if (active && pl < 3) {      // pixel lane t sums tap 3r + t over the lanes (RL >= 16)
                double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                for (int k = 0; k < a.RL; ++k) {      // fixed order
                    const float4 v = red[pl][k * a.CQ + cg];
                    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
                }
                *reinterpret_cast<float4*>(a.partials + ((size_t)ch * 9 + 3 * r + pl) * a.C + c) =
                    make_float4((float)s0, (float)s1, (float)s2, (float)s3);
            }
            __syncthreads();
        }
    }
    if (!a.y || !active) return;
    float4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = dw3_w4(a.w, c, t, a.Cw);
    const int i0 = min(a.Pin, ch * a.in_chunk), i1 = min(a.Pin, i0 + a.in_chunk);
    for (int p = i0 + pl; p < i1; p += a.RL) {
        const int iw = p % a.W, q = p / a.W;
        const int ih = q % a.H, n = q / a.H;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
            const int th = ih + a.dil - kh * a.dil;
            if (th < 0 || (th & (a.stride - 1))) continue;      // stride is 1 or 2
            const int oh = th >> (a.stride - 1);
            if (oh >= a.Ho) continue;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int tw = iw + a.dil - kw * a.dil;
                if (tw < 0 || (tw & (a.stride - 1))) continue;
                const int ow = tw >> (a.stride - 1);
                if (ow >= a.Wo) continue;
                dw3_fma(acc, dw3_ld(a.dy + ((size_t)(n * a.Ho + oh) * a.Wo + ow) * a.ldy + c), wv[kh * 3 + kw]);
            }
        }
        float4* o = reinterpret_cast<float4*>(a.y + (size_t)p * a.lddx + c);
        if (a.accumulate) {
            const float4 old = *o;
            acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w;
        }
        *o = acc;
    }
}

// dw[c][tap] = sum over chunks of part[chunk][tap][c], in double, in a fixed order: block = one tap x 4 channels, 64 chunk lanes
__global__ __launch_bounds__(256) void k_dw3_wgrad_merge(const float* __restrict__ part, int chunks, int C, int Cw,
                                                         float* __restrict__ dw) {
    __shared__ double red[64][4];
    const int cl = threadIdx.x & 3, kl = threadIdx.x >> 2;
    const int cblocks = (Cw + 3) / 4;
    const int tap = blockIdx.x / cblocks, c = (blockIdx.x - tap * cblocks) * 4 + cl;
    double s = 0.0;
    if (c < Cw)
        for (int k = kl; k < chunks; k += 64) s += (double)part[((size_t)k * 9 + tap) * C + c];
    red[kl][cl] = s;
    __syncthreads();
    if (kl == 0 && c < Cw) {
        for (int k = 1; k < 64; ++k) s += red[k][cl];
        dw[(size_t)c * 9 + tap] = (float)s;
    }
}

// channel quads per workgroup: the widest of 16 / 12 / 8 that divides the quad count (16 when none does)
static void dw3_layout(int C, Dw3Args& a) {
    const int C4 = C / 4;
    a.CQ = C4 % 16 == 0 ? 16 : (C4 % 12 == 0 ? 12 : (C4 % 8 == 0 ? 8 : 16));
    a.RL = a.CQ == 8 ? 32 : 16;
    a.colblocks = (C4 + a.CQ - 1) / a.CQ;
}

// statistic tile: 4 pixels per thread, 8 once that still leaves every CU several workgroups
static int dw3_ppt(const iswm_conv_desc* d) {
    Dw3Args a{};
    dw3_layout(d->Cin, a);
    const long long P = (long long)d->N * d->Ho * d->Wo;
    return P / (a.RL * 8) * a.colblocks >= 4096 ? 8 : 4;
}

static int dw3_chunks(const iswm_conv_desc* d) {
    long long c = ((long long)d->N * d->Ho * d->Wo + 255) / 256;
    if (c > 2048) c = 2048;
    if (c < 1) c = 1;
    return (int)c;
}

}  // namespace iswm

using namespace iswm;

static int dw3_validate(const iswm_conv_desc* d, int Cw, const char* what) {
    ISWM_REQUIRE(d, "%s: null descriptor", what);
    ISWM_REQUIRE(d->Cin == d->Cout && d->Cin > 0 && d->Cin % 4 == 0, "%s: depthwise needs Cin == Cout, a multiple of 4", what);
    ISWM_REQUIRE(Cw > 0 && Cw <= d->Cin, "%s: weight channels %d outside (0, %d]", what, Cw, d->Cin);
    ISWM_REQUIRE(d->KH == 3 && d->KW == 3 && (d->stride == 1 || d->stride == 2) && d->dil >= 1 && d->pad == d->dil,
                 "%s: needs a 3x3 filter, stride 1 or 2, pad == dil", what);
    ISWM_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: bad geometry", what);
    ISWM_REQUIRE(d->Ho == (d->H - 1) / d->stride + 1 && d->Wo == (d->W - 1) / d->stride + 1,
                 "%s: Ho/Wo do not match the geometry", what);
    ISWM_REQUIRE(d->ldx >= d->Cin && d->ldy >= d->Cin && d->ldx % 4 == 0 && d->ldy % 4 == 0, "%s: bad pitch", what);
    ISWM_REQUIRE((long long)d->N * d->H * d->W < (1ll << 31) - 65536, "%s: more than 2^31 pixels", what);
    return 0;
}

static Dw3Args dw3_args(const iswm_conv_desc* d, int Cw) {
    Dw3Args a{};
    a.N = d->N; a.H = d->H; a.W = d->W; a.C = d->Cin; a.Cw = Cw; a.Ho = d->Ho; a.Wo = d->Wo;
    a.stride = d->stride; a.dil = d->dil; a.ldx = d->ldx; a.ldy = d->ldy;
    a.Pin = d->N * d->H * d->W; a.Pout = d->N * d->Ho * d->Wo;
    dw3_layout(d->Cin, a);
    return a;
}

extern "C" int iswm_dwconv3x3_stat_tile_rows(const iswm_conv_desc* d) {
    if (!d || d->Cin <= 0 || d->Cin % 4) return 0;
    Dw3Args a{};
    dw3_layout(d->Cin, a);
    return a.RL * dw3_ppt(d);
}

extern "C" int iswm_dwconv3x3_stat_tiles(const iswm_conv_desc* d) {
    const int R = iswm_dwconv3x3_stat_tile_rows(d);
    if (R <= 0) return 0;
    return (int)(((long long)d->N * d->Ho * d->Wo + R - 1) / R);
}

extern "C" int iswm_dwconv3x3_fwd_stats(const iswm_conv_desc* d, const float* x, const float* w, int Cw, float* y,
                                        float* stat_partials, iswm_stream_t stream) {
    if (int e = dw3_validate(d, Cw, "dwconv3x3_fwd_stats")) return e;
    ISWM_REQUIRE(x && w && y && aligned16(x) && aligned16(y) && aligned16(stat_partials), "dwconv3x3_fwd_stats: bad pointer");
    Dw3Args a = dw3_args(d, Cw);
    a.x = x; a.w = w; a.y = y; a.partials = stat_partials;
    const int ppt = dw3_ppt(d);
    a.R = a.RL * ppt;
    a.tiles = iswm_dwconv3x3_stat_tiles(d);
    const dim3 grid((unsigned)a.tiles * a.colblocks), block(a.CQ * a.RL);
    if (ppt == 8)
        hipLaunchKernelGGL(k_dw3_fwd_stats<8>, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_dw3_fwd_stats<4>, grid, block, 0, (hipStream_t)stream, a);
    return check_launch("dwconv3x3_fwd_stats");
}

extern "C" size_t iswm_dwconv3x3_bwd_workspace(const iswm_conv_desc* d) {
    if (!d || d->Cin <= 0) return 0;
    return (size_t)dw3_chunks(d) * 9 * d->Cin * sizeof(float);
}

extern "C" int iswm_dwconv3x3_bwd(const iswm_conv_desc* d, const float* x, const float* dy, const float* w, int Cw,
                                  float* dx, int lddx, int accumulate, float* dw, void* workspace,
                                  size_t workspace_bytes, iswm_stream_t stream) {
    if (int e = dw3_validate(d, Cw, "dwconv3x3_bwd")) return e;
    ISWM_REQUIRE(dy && w && aligned16(dy) && (dx || dw), "dwconv3x3_bwd: bad pointer");
    ISWM_REQUIRE(!dx || (aligned16(dx) && lddx >= d->Cin && lddx % 4 == 0), "dwconv3x3_bwd: bad dx pointer / pitch");
    ISWM_REQUIRE(!dw || (x && aligned16(x) && workspace && aligned16(workspace) &&
                         workspace_bytes >= iswm_dwconv3x3_bwd_workspace(d)),
                 "dwconv3x3_bwd: the weight gradient needs x and a workspace of iswm_dwconv3x3_bwd_workspace bytes");
    Dw3Args a = dw3_args(d, Cw);
    a.x = dw ? x : nullptr; a.dy = dy; a.w = w; a.y = dx; a.partials = (float*)workspace; a.accumulate = accumulate;
    a.lddx = lddx;
    const int chunks = dw3_chunks(d);
    a.in_chunk = (a.Pin + chunks - 1) / chunks;
    a.out_chunk = (a.Pout + chunks - 1) / chunks;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dw3_bwd, dim3((unsigned)chunks * a.colblocks), dim3(a.CQ * a.RL), 0, s, a);
    if (dw)
        hipLaunchKernelGGL(k_dw3_wgrad_merge, dim3(9 * ((Cw + 3) / 4)), dim3(256), 0, s, (const float*)workspace, chunks,
                           d->Cin, Cw, dw);
    return check_launch("dwconv3x3_bwd");
}

// ---- pre-activation form (include/iswm_hip_sep.h): y = dwconv(relu?(x), w) with 1 <= pad <= dil, for the separable units of
// the Xception blocks, whose depthwise output feeds a 1x1 convolution directly (no BatchNorm in between: no statistics)
// and whose first ReLU reads the un-rectified residual stream.  The tiling, the fmaf chains and the weight-gradient
// reduction are those of the kernels above, so y / dx are bit-identical to csrc/dwconv.hip on relu?(x) and dw to
// k_dw3_bwd where pad == dil.
namespace iswm {

struct Dw3PreArgs : Dw3Args {
    const float* xm;     // backward: the pre-ReLU input the mask of dx is read from (null: no mask)
    void* yx;            // forward: output, fp32 (ps == 0), three bf16 planes (ps > 0) or one rounded plane (ps == -1)
    long long ps;
    int pad, relu, Cy;   // forward: columns [C, Cy) of y are written as zeros
};

__device__ __forceinline__ float4 dw3_relu(const float4 v) {
    return make_float4(v.x > 0.f ? v.x : 0.f, v.y > 0.f ? v.y : 0.f, v.z > 0.f ? v.z : 0.f, v.w > 0.f ? v.w : 0.f);
}

// block = CQ quads x RL pixel lanes over a run of R = 4 RL output pixels; the quads cover Cy channels, those >= C store zeros
__global__ __launch_bounds__(256) void k_dw3_pre_fwd(const Dw3PreArgs a) {
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int tile = lid / a.colblocks, cb = lid - tile * a.colblocks;
    const int pl = threadIdx.x / a.CQ, cg = threadIdx.x - pl * a.CQ;
    const int c4 = cb * a.CQ + cg, c = c4 * 4;
    if (c4 >= (a.Cy >> 2)) return;
    const bool data = c < a.C;
    float4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = data ? dw3_w4(a.w, c, t, a.Cw) : make_float4(0.f, 0.f, 0.f, 0.f);
    const int r0 = tile * a.R, r1 = min(a.Pout, r0 + a.R);
    for (int p = r0 + pl; p < r1; p += a.RL) {
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (data) {
            const int ow = p % a.Wo, q = p / a.Wo;
            const int oh = q % a.Ho, n = q / a.Ho;
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int ih = oh * a.stride - a.pad + kh * a.dil;
                if ((unsigned)ih >= (unsigned)a.H) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int iw = ow * a.stride - a.pad + kw * a.dil;
                    if ((unsigned)iw >= (unsigned)a.W) continue;
                    float4 xv = dw3_ld(a.x + ((size_t)(n * a.H + ih) * a.W + iw) * a.ldx + c);
                    if (a.relu) xv = dw3_relu(xv);
                    dw3_fma(acc, xv, wv[kh * 3 + kw]);
                }
            }
        }
        st4x(a.yx, (int64_t)p * a.ldy + c, a.ps, acc);
    }
}

// k_dw3_bwd with the taps at -pad + k dil, relu?(x) as the weight gradient's operand and dx masked by x > 0 (a quad whose
// four inputs are all <= 0 reads no dy at all)
__global__ __launch_bounds__(256) void k_dw3_pre_bwd(const Dw3PreArgs a) {
    __shared__ float4 red[3][256];
    const int lid = xcd_remap(blockIdx.x, gridDim.x);
    const int ch = lid / a.colblocks, cb = lid - ch * a.colblocks;
    const int pl = threadIdx.x / a.CQ, cg = threadIdx.x - pl * a.CQ;
    const int c4 = cb * a.CQ + cg, c = c4 * 4;
    const bool active = c4 < (a.C >> 2);
    if (a.x) {
        float4 acc[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) acc[t] = make_float4(0.f, 0.f, 0.f, 0.f);
        const int p0 = min(a.Pout, ch * a.out_chunk), p1 = min(a.Pout, p0 + a.out_chunk);
        if (active)
            for (int p = p0 + pl; p < p1; p += a.RL) {
                const int ow = p % a.Wo, q = p / a.Wo;
                const int oh = q % a.Ho, n = q / a.Ho;
                const float4 g = dw3_ld(a.dy + (size_t)p * a.ldy + c);
#pragma unroll
                for (int kh = 0; kh < 3; ++kh) {
                    const int ih = oh * a.stride - a.pad + kh * a.dil;
                    if ((unsigned)ih >= (unsigned)a.H) continue;
#pragma unroll
                    for (int kw = 0; kw < 3; ++kw) {
                        const int iw = ow * a.stride - a.pad + kw * a.dil;
                        if ((unsigned)iw >= (unsigned)a.W) continue;
                        float4 xv = dw3_ld(a.x + ((size_t)(n * a.H + ih) * a.W + iw) * a.ldx + c);
                        if (a.relu) xv = dw3_relu(xv);
                        dw3_fma(acc[kh * 3 + kw], g, xv);
                    }
                }
            }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            red[0][threadIdx.x] = acc[3 * r + 0];
            red[1][threadIdx.x] = acc[3 * r + 1];
            red[2][threadIdx.x] = acc[3 * r + 2];
            __syncthreads();
            if (active && pl < 3) {      // pixel lane t sums tap 3r + t over the lanes (RL >= 16)
                double s0 = 0, s1 = 0, s2 = 0, s3 = 0;
                for (int k = 0; k < a.RL; ++k) {      // fixed order
                    const float4 v = red[pl][k * a.CQ + cg];
                    s0 += v.x; s1 += v.y; s2 += v.z; s3 += v.w;
                }
                *reinterpret_cast<float4*>(a.partials + ((size_t)ch * 9 + 3 * r + pl) * a.C + c) =
                    make_float4((float)s0, (float)s1, (float)s2, (float)s3);
            }
            __syncthreads();
        }
    }
    if (!a.y || !active) return;
    float4 wv[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) wv[t] = dw3_w4(a.w, c, t, a.Cw);
    const int i0 = min(a.Pin, ch * a.in_chunk), i1 = min(a.Pin, i0 + a.in_chunk);
    for (int p = i0 + pl; p < i1; p += a.RL) {
        const int iw = p % a.W, q = p / a.W;
        const int ih = q % a.H, n = q / a.H;
        float4 m = make_float4(1.f, 1.f, 1.f, 1.f);
        if (a.xm) m = dw3_ld(a.xm + (size_t)p * a.ldx + c);
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        if (m.x > 0.f || m.y > 0.f || m.z > 0.f || m.w > 0.f) {
#pragma unroll
            for (int kh = 0; kh < 3; ++kh) {
                const int th = ih + a.pad - kh * a.dil;
                if (th < 0 || (th & (a.stride - 1))) continue;      // stride is 1 or 2
                const int oh = th >> (a.stride - 1);
                if (oh >= a.Ho) continue;
#pragma unroll
                for (int kw = 0; kw < 3; ++kw) {
                    const int tw = iw + a.pad - kw * a.dil;
                    if (tw < 0 || (tw & (a.stride - 1))) continue;
                    const int ow = tw >> (a.stride - 1);
                    if (ow >= a.Wo) continue;
                    dw3_fma(acc, dw3_ld(a.dy + ((size_t)(n * a.Ho + oh) * a.Wo + ow) * a.ldy + c), wv[kh * 3 + kw]);
                }
            }
            acc = make_float4(m.x > 0.f ? acc.x : 0.f, m.y > 0.f ? acc.y : 0.f, m.z > 0.f ? acc.z : 0.f, m.w > 0.f ? acc.w : 0.f);
        }
        float4* o = reinterpret_cast<float4*>(a.y + (size_t)p * a.lddx + c);
        if (a.accumulate) {
            const float4 old = *o;
            acc.x += old.x; acc.y += old.y; acc.z += old.z; acc.w += old.w;
        }
        *o = acc;
    }
}

}  // namespace iswm

// The backward's quads cover C channels; a count with no layout free of idle lanes (728: 182 quads) is laid over the next
// multiple of 32 channels instead (184 quads = 23 blocks of 8: 2 idle quads in all, not 10) -- quads past C are idle either way
static void dw3_pre_bwd_layout(int C, Dw3Args& a) {
    const int C4 = C / 4;
    const bool whole = C4 % 16 == 0 || C4 % 12 == 0 || C4 % 8 == 0;
    dw3_layout(whole || C4 < 16 ? C : (C + 31) / 32 * 32, a);
}

static int dw3_pre_validate(const iswm_conv_desc* d, int Cw, const char* what) {
    ISWM_REQUIRE(d, "%s: null descriptor", what);
    ISWM_REQUIRE(d->Cin == d->Cout && d->Cin > 0 && d->Cin % 4 == 0, "%s: depthwise needs Cin == Cout, a multiple of 4", what);
    ISWM_REQUIRE(Cw > 0 && Cw <= d->Cin, "%s: weight channels %d outside (0, %d]", what, Cw, d->Cin);
    ISWM_REQUIRE(d->KH == 3 && d->KW == 3 && (d->stride == 1 || d->stride == 2) && d->dil >= 1 && d->pad >= 1 && d->pad <= d->dil,
                 "%s: needs a 3x3 filter, stride 1 or 2, 1 <= pad <= dil", what);
    ISWM_REQUIRE(d->N > 0 && d->H > 0 && d->W > 0, "%s: bad geometry", what);
    const int eh = d->H + 2 * d->pad - 2 * d->dil - 1, ew = d->W + 2 * d->pad - 2 * d->dil - 1;
    ISWM_REQUIRE(eh >= 0 && ew >= 0 && d->Ho == eh / d->stride + 1 && d->Wo == ew / d->stride + 1,
                 "%s: Ho/Wo do not match the geometry (or the map has no output)", what);
    ISWM_REQUIRE(d->ldx >= d->Cin && d->ldy >= d->Cin && d->ldx % 4 == 0 && d->ldy % 4 == 0, "%s: bad pitch", what);
    ISWM_REQUIRE((long long)d->N * d->H * d->W < (1ll << 31) - 65536, "%s: more than 2^31 pixels", what);
    return 0;
}

extern "C" int iswm_dwconv3x3_pre_fwd(const iswm_conv_desc* d, const float* x, const float* w, int Cw, int relu_in, void* y,
                                      int64_t y_ps, int ycols, iswm_stream_t stream) {
    if (int e = dw3_pre_validate(d, Cw, "dwconv3x3_pre_fwd")) return e;
    ISWM_REQUIRE(x && w && y && aligned16(x) && aligned16(y), "dwconv3x3_pre_fwd: bad pointer");
    ISWM_REQUIRE(ycols >= d->Cin && ycols <= d->ldy && ycols % 4 == 0, "dwconv3x3_pre_fwd: ycols %d outside [Cin, ldy] or no multiple of 4",
                 ycols);
    // (8-byte plane accesses: pitch and plane stride in bf16 elements, multiples of 4; the convolutions ask for 8)
    ISWM_REQUIRE(y_ps >= -1 && (y_ps <= 0 || (y_ps % 4 == 0 && y_ps >= (int64_t)d->N * d->Ho * d->Wo * d->ldy)),
                 "dwconv3x3_pre_fwd: bad plane stride");
    Dw3PreArgs a{};
    static_cast<Dw3Args&>(a) = dw3_args(d, Cw);
    a.x = x; a.w = w; a.yx = y; a.ps = y_ps; a.pad = d->pad; a.relu = relu_in != 0; a.Cy = ycols;
    dw3_layout(ycols, a);
    a.R = a.RL * 4;
    a.tiles = (a.Pout + a.R - 1) / a.R;
    hipLaunchKernelGGL(k_dw3_pre_fwd, dim3((unsigned)a.tiles * a.colblocks), dim3(a.CQ * a.RL), 0, (hipStream_t)stream, a);
    return check_launch("dwconv3x3_pre_fwd");
}

extern "C" size_t iswm_dwconv3x3_pre_bwd_workspace(const iswm_conv_desc* d) {
    if (!d || d->Cin <= 0 || d->Ho <= 0 || d->Wo <= 0) return 0;
    return (size_t)dw3_chunks(d) * 9 * d->Cin * sizeof(float);
}

extern "C" int iswm_dwconv3x3_pre_bwd(const iswm_conv_desc* d, const float* x, const float* dy, const float* w, int Cw,
                                      int relu_in, float* dx, int lddx, int accumulate, float* dw, void* workspace,
                                      size_t workspace_bytes, iswm_stream_t stream) {
    if (int e = dw3_pre_validate(d, Cw, "dwconv3x3_pre_bwd")) return e;
    ISWM_REQUIRE(dy && w && aligned16(dy) && (dx || dw), "dwconv3x3_pre_bwd: bad pointer");
    ISWM_REQUIRE(!dx || (aligned16(dx) && lddx >= d->Cin && lddx % 4 == 0), "dwconv3x3_pre_bwd: bad dx pointer / pitch");
    ISWM_REQUIRE(!(dw || (dx && relu_in)) || (x && aligned16(x)),
                 "dwconv3x3_pre_bwd: the weight gradient and the mask of dx need x, the input before the ReLU");
    ISWM_REQUIRE(!dw || (workspace && aligned16(workspace) && workspace_bytes >= iswm_dwconv3x3_pre_bwd_workspace(d)),
                 "dwconv3x3_pre_bwd: the weight gradient needs a workspace of iswm_dwconv3x3_pre_bwd_workspace bytes");
    Dw3PreArgs a{};
    static_cast<Dw3Args&>(a) = dw3_args(d, Cw);
    a.x = dw ? x : nullptr; a.xm = relu_in ? x : nullptr; a.dy = dy; a.w = w; a.y = dx; a.partials = (float*)workspace;
    a.accumulate = accumulate; a.lddx = lddx; a.pad = d->pad; a.relu = relu_in != 0;
    dw3_pre_bwd_layout(d->Cin, a);
    const int chunks = dw3_chunks(d);
    a.in_chunk = (a.Pin + chunks - 1) / chunks;
    a.out_chunk = (a.Pout + chunks - 1) / chunks;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_dw3_pre_bwd, dim3((unsigned)chunks * a.colblocks), dim3(a.CQ * a.RL), 0, s, a);
    if (dw)
        hipLaunchKernelGGL(k_dw3_wgrad_merge, dim3(9 * ((Cw + 3) / 4)), dim3(256), 0, s, (const float*)workspace, chunks,
                           d->Cin, Cw, dw);
    return check_launch("dwconv3x3_pre_bwd");
}
