// Source index and weights of a bilinear resize with align_corners=False, shared by resize.hip and predict.hip.
// Restates ATen's area_pixel_compute_source_index:
//   scale = in/out (float); src = scale*(dst+0.5)-0.5, clamped at 0; i0 = (int)src;
//   i1 = i0 + (i0 < in-1); l1 = src - i0; l0 = 1 - l1.
#pragma once
#include "common.h"

namespace iswm {

struct Lerp {
    int i0, i1;
    float l0, l1;
};

__device__ __forceinline__ Lerp src_index(float scale, int dst, int in_size) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    Lerp r;
    r.i0 = (int)src;
    if (r.i0 > in_size - 1) r.i0 = in_size - 1;
    r.i1 = r.i0 + (r.i0 < in_size - 1 ? 1 : 0);
    r.l1 = src - (float)r.i0;
    r.l0 = 1.f - r.l1;
    return r;
}

}  // namespace iswm
