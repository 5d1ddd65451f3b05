// What the second-generation planes convolution kernels share: k_conv_pl2 (conv_mfma_pl2.hip, 128-column tiles),
// k_conv_pl2w (conv_mfma_pl2w.hip, 256-column tiles) and k_conv_pl2t (conv_mfma_pl2t.hip, the fused ASPP launch).
//
// A stage is 64 channels of a (16 * rbw)-row activation tile: NP planes of [row][128 B] in LDS, two stage buffers, filled
// by LDS-DMA in 8-row x 128-B pieces (wave w owns the row groups w, w + 8, ...); the 16-byte group g of row r sits in slot
// g ^ ((r >> 1) & 7) (swizzle applied to the DMA SOURCE), which makes the ds_read_b128 fragment reads conflict-free.  Every
// wave multiplies all rows of the stage by its own weight fragments (v_mfma_f32_16x16x32_bf16) while the loads of the
// following stage are issued between the row blocks.
//
// This is schedule-sensitive code, so a piece lives here only if every kernel compiles to the SAME
// instruction stream with it as with its own copy (profiles/pl2_refactor_isa.txt).  That holds for the stage shape, the
// lane roles, the fragment read and the six-product multiply (and for glds16b / mfma16, now in conv_common.h).  It does
// not hold -- hipcc permutes registers or moves address arithmetic across the scheduling fences -- for the pinned
// row-block loop, the row-group bookkeeping (sentinel fill, pixel-or-zero-row pointers, issueA, the next-stage DMA slot),
// the BatchNorm sums of the epilogues and the stage-stream driver when they are taken out of the kernel body into
// functions with the state passed by reference: those stay in each kernel, in the same form in all three.
#pragma once
#include "conv_common.h"

namespace iswm {

// one definition per including translation unit (the _pl2 suffix: conv_tile32.h owns the name g_zero_row)
static __device__ __attribute__((aligned(128))) unsigned short g_zero_row_pl2[64];   // 128 B of zeros
static __device__ float4 g_dump_pl2[64];         // where an epilogue's out-of-range lanes store (never read)

// ---- shape of a stage: BM tile rows, NP planes ------------------------------------------------------------------------
template <int BM_, int NP_>
struct Pl2Stage {
    static constexpr int BM = BM_, NP = NP_;
    static constexpr int RG = BM / 8;                 // 8-row DMA groups of the tile
    static constexpr int NRG = (RG + 7) / 8;          // ... per wave
    static constexpr int PLANE = BM * 128;            // bytes of one plane of one stage
    static constexpr int STAGE = NP * PLANE;
};

// ---- the DMA side -----------------------------------------------------------------------------------------------------
// DMA role of a lane: row (lane >> 3) of an 8-row group, source 16-byte group pl2_dma_group() of the 128-byte row
__device__ __forceinline__ int pl2_dma_group(int lane, int wave) { return (lane & 7) ^ ((4 * (wave & 1) + (lane >> 4)) & 7); }

// ihb of a row group without a row in the tile: every tap test of the kernels fails on it
constexpr int PL2_NO_ROW = -(1 << 28);

// ---- the multiply -----------------------------------------------------------------------------------------------------
// fragment address of a lane inside a plane: row (lane & 15) of a 16-row block, k group (lane >> 4) [+4 in the second half
// of the stage -> slot ^ 4 -> byte ^ 64], on top of the byte offset `rows0` of the wave's first row block.  (A macro: as a
// function hipcc commutes one operand pair of the address computation.)
#define PL2_FBASE(rows0, lane) ((rows0) + ((lane) & 15) * 128 + ((((lane) >> 4) ^ (((lane) & 15) >> 1)) * 16))

template <int NP>
struct Pl2AFrag {
    uint4 v[NP];
};

// acc += w . x for one 16 x 16 block and one 32-deep k half: six bf16 products of the three planes (NP == 3), smallest
// terms first: bh*al, bl*ah, bm*am, bh*am, bm*ah, bh*ah -- or the single product of conv math bf16 (NP == 1).
// Weights are the MFMA's row operand: lane = pixel, 4 registers = 4 consecutive channels (16-byte stores).
// b: the NP weight fragments of that block and half (indexed with constants once inlined: registers).
template <int NP>
__device__ __forceinline__ void pl2_mul(f32x4& acc, const uint4* b, const Pl2AFrag<NP>& f) {
    f32x4 c = acc;
    if constexpr (NP == 3) {
        c = mfma16(b[0], f.v[2], c);
        c = mfma16(b[2], f.v[0], c);
        c = mfma16(b[1], f.v[1], c);
        c = mfma16(b[0], f.v[1], c);
        c = mfma16(b[1], f.v[0], c);
    }
    c = mfma16(b[0], f.v[0], c);
    acc = c;
}

// Fragment read of block idx = half * RBW + rb (k half `half` of row block `rb`) of stage buffer st: one ds_read_b128 per plane.
template <class S, int RBW>
__device__ __forceinline__ void pl2_aload(Pl2AFrag<S::NP>& f, const unsigned char* smem, int st, int fbase, int idx) {
    const int half = idx / RBW, rb = idx - half * RBW;
    const unsigned char* p = smem + st * S::STAGE + (fbase ^ (half * 64)) + rb * 2048;
#pragma unroll
    for (int pl = 0; pl < S::NP; ++pl) f.v[pl] = *reinterpret_cast<const uint4*>(p + pl * S::PLANE);
}

}  // namespace iswm
