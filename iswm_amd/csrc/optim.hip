// Fused optimizer steps over one flat fp32 arena (all parameters of the model live in one
// allocation, gradients in a second, optimizer state in a third -- a single launch updates
// the 40-59 M parameters of DeepLabV3+-ResNet50/101).  HBM-bound: SGD-momentum reads p,g,m and
// writes p,m = 20 B/param; Adam reads p,g,m,v and writes p,m,v = 28 B/param.
//
// Arithmetic restates torch.optim.SGD(momentum, nesterov, weight_decay) and
// torch.optim.Adam / AdamW (defaults) exactly as setup_optimizer builds them, train.py:421-444.
// The learning rate (and Adam's bias corrections) are read from device memory so a captured
// hipGraph can be replayed while the host-side CosineAnnealingLR (train.py:446-452) changes them.
#include "common.h"

namespace iswm {

__global__ __launch_bounds__(256) void k_sgd(float* __restrict__ p, const float* __restrict__ g,
                                             float* __restrict__ buf, int64_t n4, int64_t n,
                                             const float* __restrict__ lr_dev, float mu, float wd, int nesterov) {
    const float lr = lr_dev[0];
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 bv = reinterpret_cast<float4*>(buf)[i];
        float pp[4] = {pv.x, pv.y, pv.z, pv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float d = gg[k] + wd * pp[k];      // g + wd*p
            bb[k] = mu * bb[k] + d;            // buf = mu*buf + g   (buf starts at 0 == torch's first-step clone)
            float u = nesterov ? d + mu * bb[k] : bb[k];
            pp[k] = pp[k] - lr * u;
        }
        reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        reinterpret_cast<float4*>(buf)[i] = make_float4(bb[0], bb[1], bb[2], bb[3]);
    }
    if (blockIdx.x == 0) {
        int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) {
            float d = g[i] + wd * p[i];
            float b = mu * buf[i] + d;
            buf[i] = b;
            p[i] = p[i] - lr * (nesterov ? d + mu * b : b);
        }
    }
}

__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, float lr, float bc1, float bc2s,
                                         float b1, float b2, float eps, float wd, int decoupled) {
    if (decoupled) p = p * (1.f - lr * wd);
    else g = g + wd * p;
    m = m + (g - m) * (1.f - b1);                 // exp_avg.lerp_(g, 1-b1)
    v = v * b2 + (1.f - b2) * g * g;              // exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2)
    float denom = sqrtf(v) / bc2s + eps;
    p = p - (lr / bc1) * (m / denom);
}

__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g,
                                              float* __restrict__ m, float* __restrict__ v, int64_t n,
                                              const float* __restrict__ hyper, float b1, float b2, float eps,
                                              float wd, int decoupled) {
    const float lr = hyper[0], bc1 = hyper[1], bc2s = sqrtf(hyper[2]);
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pp = p[i], mm = m[i], vv = v[i];
        adam_one(pp, g[i], mm, vv, lr, bc1, bc2s, b1, b2, eps, wd, decoupled);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
    }
}

// ---- gradient-norm clipping and EMA weights inside the step ----------------------------------
// The squared norm of the gradient arena is one extra 4 B/param read: every workgroup leaves ONE double in its own slot
// (no atomics, the grid is a function of n alone), a single-workgroup finalize adds the slots in a fixed order and
// writes {coef, norm, sum of squares} to device memory, and the extended step kernels multiply g by coef as they load
// it -- the gradient arena is never rescaled.  Everything accumulates in double: the pass is HBM-bound, and double
// removes the overflow of fp32 squares and any dependence on the summation order from the result's fp32 rounding.
constexpr int SQNORM_SLOTS = 2048;          // == the cap of stream_grid: slot b belongs to workgroup b

// the clip factor meets g in ONE rounded fp32 multiply that no later add may fuse with: with coef == 1.0f the extended
// kernels then compute bit for bit what k_sgd / k_adam do
__device__ __forceinline__ float clip_mul(float g, float coef) {
#pragma clang fp contract(off)
    return g * coef;
}

__device__ __forceinline__ double block_sum_256(double s) {
    __shared__ double wave_sums[4];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = s;
    __syncthreads();
    return (wave_sums[0] + wave_sums[1]) + (wave_sums[2] + wave_sums[3]);      // valid in every thread
}

__global__ __launch_bounds__(256) void k_sqnorm(const float* __restrict__ g, int64_t n4, int64_t n,
                                                double* __restrict__ slots, int accumulate) {
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 v = reinterpret_cast<const float4*>(g)[i];
        s0 = fma((double)v.x, (double)v.x, s0);
        s1 = fma((double)v.y, (double)v.y, s1);
        s2 = fma((double)v.z, (double)v.z, s2);
        s3 = fma((double)v.w, (double)v.w, s3);
    }
    if (blockIdx.x == 0) {
        int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) s0 = fma((double)g[i], (double)g[i], s0);
    }
    double s = block_sum_256((s0 + s1) + (s2 + s3));
    if (threadIdx.x == 0) slots[blockIdx.x] = accumulate ? slots[blockIdx.x] + s : s;
    if (blockIdx.x == 0 && !accumulate)                 // the slots no workgroup of this launch owns start at zero
        for (int k = gridDim.x + threadIdx.x; k < SQNORM_SLOTS; k += blockDim.x) slots[k] = 0.0;
}

// out[0] = coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_, fp32), out[1] = norm = sqrt(sum),
// the double behind out[2..3] = sum.  A NaN norm gives a NaN coef (error_if_nonfinite=False: it propagates).
__global__ __launch_bounds__(256) void k_clip_finalize(const double* __restrict__ slots, float max_norm,
                                                       float* __restrict__ out) {
    double s = 0.0;
    for (int k = threadIdx.x; k < SQNORM_SLOTS; k += 256) s += slots[k];
    s = block_sum_256(s);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(s);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = c < 1.f ? c : (c != c ? c : 1.f);
        out[1] = norm;
        *reinterpret_cast<double*>(out + 2) = s;
    }
}

// k_sgd with the clip factor at the load of g and the EMA after the parameter update; ema += hyper[3] * (p_new - ema),
// hyper[3] = 1 - d_t.  Without either (CLIP, EMA false) this IS k_sgd.
template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_sgd_ex(float* __restrict__ p, const float* __restrict__ g,
                                                float* __restrict__ buf, int64_t n4, int64_t n,
                                                const float* __restrict__ hyper, float mu, float wd, int nesterov,
                                                const float* __restrict__ clip, float* __restrict__ ema) {
    const float lr = hyper[0];
    const float coef = CLIP ? clip[0] : 1.f;
    const float w = EMA ? hyper[3] : 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 pv = reinterpret_cast<float4*>(p)[i];
        float4 gv = reinterpret_cast<const float4*>(g)[i];
        float4 bv = reinterpret_cast<float4*>(buf)[i];
        float pp[4] = {pv.x, pv.y, pv.z, pv.w}, gg[4] = {gv.x, gv.y, gv.z, gv.w}, bb[4] = {bv.x, bv.y, bv.z, bv.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float gk = CLIP ? clip_mul(gg[k], coef) : gg[k];
            float d = gk + wd * pp[k];
            bb[k] = mu * bb[k] + d;
            float u = nesterov ? d + mu * bb[k] : bb[k];
            pp[k] = pp[k] - lr * u;
        }
        reinterpret_cast<float4*>(p)[i] = make_float4(pp[0], pp[1], pp[2], pp[3]);
        reinterpret_cast<float4*>(buf)[i] = make_float4(bb[0], bb[1], bb[2], bb[3]);
        if (EMA) {
            float4 ev = reinterpret_cast<float4*>(ema)[i];
            ev.x += w * (pp[0] - ev.x);
            ev.y += w * (pp[1] - ev.y);
            ev.z += w * (pp[2] - ev.z);
            ev.w += w * (pp[3] - ev.w);
            reinterpret_cast<float4*>(ema)[i] = ev;
        }
    }
    if (blockIdx.x == 0) {
        int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) {
            float gk = CLIP ? clip_mul(g[i], coef) : g[i];
            float d = gk + wd * p[i];
            float b = mu * buf[i] + d;
            buf[i] = b;
            float pn = p[i] - lr * (nesterov ? d + mu * b : b);
            p[i] = pn;
            if (EMA) ema[i] += w * (pn - ema[i]);
        }
    }
}

// adam_one for a clipped gradient.  The one difference is the L2 term, written as the fused multiply-add that the
// compiler contracts `g + wd * p` to in adam_one: next to the clip multiply it otherwise pairs the two products into one
// packed multiply and adds them unfused, which is a different rounding from k_adam's at coef == 1.
// This is a second copy of adam_one that must follow both its source and what the compiler makes of it (k_adam itself is
// not to be touched): what keeps the two in step is the bit-for-bit comparison of iswm_adam_step_ex at coef == 1 with
// iswm_adam_step in tests/test_optim_ext_gpu.py (test_clipped_adam_step, test_second_trip_with_clip_and_ema).  Change
// adam_one, the compiler or its flags, and that test says whether this copy still matches.
__device__ __forceinline__ void adam_one_clipped(float& p, float g, float& m, float& v, float lr, float bc1, float bc2s,
                                                 float b1, float b2, float eps, float wd, int decoupled) {
    if (decoupled) p = p * (1.f - lr * wd);
    else g = fmaf(wd, p, g);
    m = m + (g - m) * (1.f - b1);
    v = v * b2 + (1.f - b2) * g * g;
    float denom = sqrtf(v) / bc2s + eps;
    p = p - (lr / bc1) * (m / denom);
}

template <bool CLIP, bool EMA>
__global__ __launch_bounds__(256) void k_adam_ex(float* __restrict__ p, const float* __restrict__ g,
                                                 float* __restrict__ m, float* __restrict__ v, int64_t n,
                                                 const float* __restrict__ hyper, float b1, float b2, float eps,
                                                 float wd, int decoupled, const float* __restrict__ clip,
                                                 float* __restrict__ ema) {
    const float lr = hyper[0], bc1 = hyper[1], bc2s = sqrtf(hyper[2]);
    const float coef = CLIP ? clip[0] : 1.f;
    const float w = EMA ? hyper[3] : 0.f;
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        float pp = p[i], mm = m[i], vv = v[i];
        if (CLIP) adam_one_clipped(pp, clip_mul(g[i], coef), mm, vv, lr, bc1, bc2s, b1, b2, eps, wd, decoupled);
        else adam_one(pp, g[i], mm, vv, lr, bc1, bc2s, b1, b2, eps, wd, decoupled);
        p[i] = pp;
        m[i] = mm;
        v[i] = vv;
        if (EMA) ema[i] += w * (pp - ema[i]);
    }
}

__global__ __launch_bounds__(256) void k_swap(float* __restrict__ a, float* __restrict__ b, int64_t n4, int64_t n) {
    for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n4; i += (int64_t)gridDim.x * blockDim.x) {
        float4 av = reinterpret_cast<float4*>(a)[i];
        float4 bv = reinterpret_cast<float4*>(b)[i];
        reinterpret_cast<float4*>(a)[i] = bv;
        reinterpret_cast<float4*>(b)[i] = av;
    }
    if (blockIdx.x == 0) {
        int64_t i = n4 * 4 + threadIdx.x;
        if (i < n) {
            float t = a[i];
            a[i] = b[i];
            b[i] = t;
        }
    }
}

}  // namespace iswm

using namespace iswm;

extern "C" int iswm_grad_sqnorm_slots(void) { return SQNORM_SLOTS; }

extern "C" int iswm_grad_sqnorm(const float* g, int64_t n, double* slots, int accumulate, iswm_stream_t stream) {
    ISWM_REQUIRE(g && slots && n > 0, "grad_sqnorm: bad argument");
    ISWM_REQUIRE(aligned16(g) && (reinterpret_cast<uintptr_t>(slots) & 7) == 0, "grad_sqnorm: g must be 16-byte, slots 8-byte aligned");
    hipLaunchKernelGGL(k_sqnorm, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, g, n / 4, n, slots,
                       accumulate);
    return check_launch("grad_sqnorm");
}

extern "C" int iswm_clip_finalize(const double* slots, float max_norm, float* clip_dev, iswm_stream_t stream) {
    ISWM_REQUIRE(slots && clip_dev && max_norm > 0.f, "clip_finalize: bad argument (max_norm must be positive)");
    ISWM_REQUIRE((reinterpret_cast<uintptr_t>(clip_dev) & 7) == 0, "clip_finalize: clip_dev must be 8-byte aligned");
    hipLaunchKernelGGL(k_clip_finalize, dim3(1), dim3(256), 0, (hipStream_t)stream, slots, max_norm, clip_dev);
    return check_launch("clip_finalize");
}

extern "C" int iswm_sgd_step_ex(float* p, const float* g, float* buf, int64_t n, const float* hyper_dev, float momentum,
                                float weight_decay, int nesterov, const float* clip_dev, float* ema,
                                iswm_stream_t stream) {
    ISWM_REQUIRE(p && g && buf && hyper_dev && n > 0, "sgd_step_ex: bad argument");
    ISWM_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf) && aligned16(ema),
                 "sgd_step_ex: arenas must be 16-byte aligned");
    const dim3 grid(stream_grid(n / 4 + 1, 256));
#define ISWM_SGD_EX(CLIP, EMA)                                                                                      \
    hipLaunchKernelGGL((k_sgd_ex<CLIP, EMA>), grid, dim3(256), 0, (hipStream_t)stream, p, g, buf, n / 4, n, hyper_dev, \
                       momentum, weight_decay, nesterov, clip_dev, ema)
    if (clip_dev && ema) ISWM_SGD_EX(true, true);
    else if (clip_dev) ISWM_SGD_EX(true, false);
    else if (ema) ISWM_SGD_EX(false, true);
    else ISWM_SGD_EX(false, false);
#undef ISWM_SGD_EX
    return check_launch("sgd_step_ex");
}

extern "C" int iswm_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                                 float beta1, float beta2, float eps, float weight_decay, int decoupled,
                                 const float* clip_dev, float* ema, iswm_stream_t stream) {
    ISWM_REQUIRE(p && g && m && v && hyper_dev && n > 0, "adam_step_ex: bad argument");
    const dim3 grid(stream_grid(n, 256));
#define ISWM_ADAM_EX(CLIP, EMA)                                                                                    \
    hipLaunchKernelGGL((k_adam_ex<CLIP, EMA>), grid, dim3(256), 0, (hipStream_t)stream, p, g, m, v, n, hyper_dev, \
                       beta1, beta2, eps, weight_decay, decoupled, clip_dev, ema)
    if (clip_dev && ema) ISWM_ADAM_EX(true, true);
    else if (clip_dev) ISWM_ADAM_EX(true, false);
    else if (ema) ISWM_ADAM_EX(false, true);
    else ISWM_ADAM_EX(false, false);
#undef ISWM_ADAM_EX
    return check_launch("adam_step_ex");
}

extern "C" int iswm_swap_f32(float* a, float* b, int64_t n, iswm_stream_t stream) {
    ISWM_REQUIRE(a && b && a != b && n > 0, "swap_f32: bad argument");
    ISWM_REQUIRE(aligned16(a) && aligned16(b), "swap_f32: both ranges must be 16-byte aligned");
    hipLaunchKernelGGL(k_swap, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, a, b, n / 4, n);
    return check_launch("swap_f32");
}

extern "C" int iswm_sgd_step(float* p, const float* g, float* buf, int64_t n, const float* lr_dev, float momentum,
                             float weight_decay, int nesterov, iswm_stream_t stream) {
    ISWM_REQUIRE(p && g && buf && lr_dev && n > 0, "sgd_step: bad argument");
    ISWM_REQUIRE(aligned16(p) && aligned16(g) && aligned16(buf), "sgd_step: arenas must be 16-byte aligned");
    hipLaunchKernelGGL(k_sgd, dim3(stream_grid(n / 4 + 1, 256)), dim3(256), 0, (hipStream_t)stream, p, g, buf,
                       n / 4, n, lr_dev, momentum, weight_decay, nesterov);
    return check_launch("sgd_step");
}

extern "C" int iswm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                              float beta1, float beta2, float eps, float weight_decay, int decoupled,
                              iswm_stream_t stream) {
    ISWM_REQUIRE(p && g && m && v && hyper_dev && n > 0, "adam_step: bad argument");
    hipLaunchKernelGGL(k_adam, dim3(stream_grid(n, 256)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n,
                       hyper_dev, beta1, beta2, eps, weight_decay, decoupled);
    return check_launch("adam_step");
}
