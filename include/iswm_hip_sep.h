/*
 * iswm_hip_sep.h -- extension header of libiswm_hip.so: entry points added after the ABI of iswm_hip.h was frozen at its
 * export count.  Plain C, the conventions and the records of iswm_hip.h (included below); the host binds these
 * prototypes with the same parser, into a table of their own (iswm_amd/_lib.py, EXT_EXPORTS).  It declares prototypes
 * only: no record and no constant.
 *
 * ---- pre-activation depthwise 3x3 (csrc/dwconv3.hip): the depthwise half of a separable unit
 * [ReLU-on-load?] depthwise -> pointwise -> BatchNorm of the Xception blocks.  KH == KW == 3, stride 1 or 2, dil >= 1 and
 * 1 <= pad <= dil (the public Xception definition pads its exit-flow convolutions by 1 under dilation 2 or 4: the map
 * shrinks by 2 (dil - pad) per convolution), Ho = (H + 2 pad - 2 dil - 1) / stride + 1 >= 1.  Operands as in
 * iswm_dwconv3x3_*: pitched NHWC fp32 x, the torch parameter w[Cw][9], channels >= Cw see zero weights.
 *   iswm_dwconv3x3_pre_fwd : y = dwconv(relu_in ? max(x, 0) : x, w).  y is an fp32 tensor (y_ps == 0, pitch d->ldy floats),
 *                            three bf16 planes (y_ps > 0) or one rounded bf16 plane (y_ps == -1), pitch and plane stride
 *                            in bf16 elements, as in the *_planes entry points.  Columns [Cin, ycols) of y are written as
 *                            zeros (Cin <= ycols <= ldy, ycols % 4 == 0): the padding a 1x1 convolution over a wider
 *                            input buffer reads.  No statistics.  The fp32 y is bit-identical to iswm_dwconv2d_fwd on
 *                            relu?(x).
 *   iswm_dwconv3x3_pre_bwd : dw[Cw][9] from relu?(x) and dy, and dx (=|+=) mask * dgrad(dy, w) with mask = (x > 0) when
 *                            relu_in, else 1 -- from ONE pass, merged like iswm_dwconv3x3_bwd (fixed order, no atomics).
 *                            x is the saved input BEFORE the ReLU; it is needed for dw and, with relu_in, for dx.
 *                            dx == NULL or dw == NULL skips that half.
 */
#ifndef ISWM_HIP_SEP_H
#define ISWM_HIP_SEP_H

#include "iswm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int iswm_dwconv3x3_pre_fwd(const iswm_conv_desc* d, const float* x, const float* w, int Cw, int relu_in, void* y,
                           int64_t y_ps, int ycols, iswm_stream_t stream);
size_t iswm_dwconv3x3_pre_bwd_workspace(const iswm_conv_desc* d);
int iswm_dwconv3x3_pre_bwd(const iswm_conv_desc* d, const float* x, const float* dy, const float* w, int Cw, int relu_in,
                           float* dx, int lddx, int accumulate, float* dw, void* workspace, size_t workspace_bytes,
                           iswm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISWM_HIP_SEP_H */
