// What the weight-gradient kernels over [pixel][channel] LDS images share: k_wgrad_pl / k_wgrad_plw / k_wgrad_pls
// (conv_wgrad_pl.hip, images filled by LDS-DMA from pre-split planes) and k_stem_wgrad (conv_stem.hip, images written by
// the threads after an exact split).
//
// An image is KS pixel rows of 256 B = 128 bf16 channels per plane; the 16-byte channel group g of row r sits at byte
// (16 g) ^ (64 (r & 3)), so the four k-rows of one transposing read (ds_read_b64_tr_b16) fall on disjoint bank quarters.
// A lane of the 16-lane group tg = lane >> 4 addresses k-row 8 (tg >> 1) + tq (tq = (lane & 15) >> 2) and the four channels
// col0 + 16 (tg & 1) + 4 (lane & 3) ..: two reads eight rows apart give the 32x32x16 MFMA operand of 32 channels x 16 pixels.
//
// This is schedule-sensitive code: a piece is shared only if no kernel's device code gets worse with it than
// with its own copy -- an identical instruction stream, or equal resources, bit-equal results and no shape slower
// (tools/isa_diff.py; profiles/wgrad_refactor_isa.txt and wgrad_refactor_ab.txt have the tables and every figure).
// Shared here, all four kernels compiling to the SAME stream as before: the transposing fragment read and the six-product
// multiply.  Everything else stays in each kernel body:
//   the pixel walk as one struct (WgWalk), the DMA lane role and column set-up as functions and the direct tile store as a
//     function taking the values as a callable, in k_wgrad_pl and k_wgrad_plw: 2463 -> 2395 and 2117 -> 2118 instructions,
//     every resource field equal, bit-equal on all 33 planes routes, the whole step inside the parent's range -- but in the
//     isolated per-shape comparison one of the four k_wgrad_pl shapes (in one job of three) and one of three k_wgrad_plw
//     shapes came out slower than the parent by more than the parent's own spread, so they are not in;
//   k_wgrad_pls with any of those pieces: its loader waves are timing-sensitive although they run three stages ahead.  One
//     walk + one DMA tail for rect / always / general (3453 -> 3042 instructions), the two branches with a common tail
//     (-> 3275) and the parent's structure with WgWalk and the column function (+1) all left 3 .. 6 of the 19 bench shapes
//     slower than the parent by more than its own spread (sum of the shapes +0.4 .. +0.9 %);
//   the fragment ADDRESS of a lane as a function of (plane, lane, k-row, column) or as a macro: the streams change
//     (macro: k_stem_wgrad 923 -> 922 instructions) -- it stays a one-line lambda in each kernel body;
//   the direct store adding k_wgrad_pl's LDS half into the accumulators first: k_wgrad_pl<1> VGPR 110 -> 134;
//   WgArgs deriving from iswm_conv_desc (the fourteen geometry ints copied in one statement): k_wgrad_plw SGPR 84 -> 85
//     (one plane) and 88 -> 90 (three planes) -- the kernel argument keeps its own fields.
#pragma once
#include "conv_common.h"

namespace iswm {

typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4* lds_s16x4;

// 32 channels x 16 pixels at p = plane + (krow0 + 8 th + tq) * 256 + ((2 (col0 + tc)) ^ (64 tq)) [th = lane >> 5, tq = (lane & 15) >> 2,
// tc = 16 ((lane >> 4) & 1) + 4 (lane & 3)] as the k-contiguous operand of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ uint4 wg_tr_frag(const unsigned char* p) {
    s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p));
    s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4)(p + 4 * 256));
    uint2 a2 = __builtin_bit_cast(uint2, lo), b2 = __builtin_bit_cast(uint2, hi);
    return make_uint4(a2.x, a2.y, b2.x, b2.y);
}

// acc += a . b for one 32 x 32 block and 16 pixels: six bf16 products of the three planes (NP == 3), smallest terms first:
// al*bh, ah*bl, am*bm, am*bh, ah*bm, ah*bh -- or the single product of conv math bf16 (NP == 1).
// a, b: the NP fragments of the row and the column block (indexed with constants once inlined: registers).
template <int NP>
__device__ __forceinline__ void wg_mul(f32x16& acc, const uint4* a, const uint4* b) {
    f32x16 c = acc;
    if constexpr (NP == 3) {
        c = mfma_bf16(a[2], b[0], c);
        c = mfma_bf16(a[0], b[2], c);
        c = mfma_bf16(a[1], b[1], c);
        c = mfma_bf16(a[1], b[0], c);
        c = mfma_bf16(a[0], b[1], c);
    }
    c = mfma_bf16(a[0], b[0], c);
    acc = c;
}

}  // namespace iswm
