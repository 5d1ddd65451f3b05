/*
 * iswm_hip.h -- C ABI of libiswm_hip.so, the MI355X (gfx950) kernels behind the
 * DeepLabV3+ training hot path of Alanlee0323/ISWM.
 *
 * The reference has no FFI layer of its own: its hot path is a chain of stock
 * torch.nn modules.  Each entry point below replaces the ATen op
 * that one reference call site runs; the call site is cited next to it (paths
 * relative to the reference checkout).  The host side (iswm_amd/, Python) binds
 * these with ctypes -- plain pointers and sizes, no torch types.
 *
 * Conventions
 *   - all tensors are device pointers to fp32 unless stated otherwise;
 *   - activations are NHWC ("channels last"): element (n,h,w,c) of a tensor with
 *     pixel pitch ld lives at ((n*H+h)*W+w)*ld + c.  ld >= C lets an op read or
 *     write a channel slice of a wider buffer;
 *   - conv weights are OHWI: [Cout][KH][KW][Cin] (a torch [Cout,Cin,KH,KW]
 *     parameter in channels_last memory format has exactly this layout);
 *   - every function enqueues on `stream` and returns immediately; it never
 *     synchronises, allocates or frees (safe under hipGraph capture);
 *   - return 0 on success, non-zero on a rejected argument or a launch error;
 *     iswm_last_error() then holds a thread-local message.
 */
#ifndef ISWM_HIP_H
#define ISWM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* iswm_stream_t; /* hipStream_t */

const char* iswm_last_error(void);
int iswm_version(void);

/* `relu` of the iswm_bn_apply* / iswm_bn_backward* entry points: the activation behind the BatchNorm.  ReLU6 clamps to [0, 6]
 * and its backward passes the gradient where 0 < out < 6. */
enum { ISWM_ACT_NONE = 0, ISWM_ACT_RELU = 1, ISWM_ACT_RELU6 = 6 };
/* `relu` of iswm_conv2d_dgrad_pl2_bn: the gate on dx before its sums are taken (described at that entry point) */
enum { ISWM_GATE_NONE = 0, ISWM_GATE_RECOMPUTED = 2, ISWM_GATE_RESIDUAL = 3 };

/* ---- convolution (implicit GEMM on v_mfma_f32_32x32x2_f32) ------------------
 * nn.Conv2d call sites: network/backbone/resnet.py:27-35,144,184-187;
 * network/_deeplab.py:37,44-51,124,134,149,162.  groups == 1, square dilation.
 * Requirements: Cin % 4 == 0, Cout % 4 == 0, ldx % 4 == 0, ldy % 4 == 0,
 * 16-byte aligned pointers (the host pads the 3-channel stem input to 4 and the
 * num_classes-wide classifier to a multiple of 4). */
typedef struct {
    int N, H, W, Cin;   /* input  [N,H,W,Cin]  */
    int Ho, Wo, Cout;   /* output [N,Ho,Wo,Cout] */
    int KH, KW, stride, pad, dil;
    int ldx;            /* pixel pitch of x  (floats) */
    int ldy;            /* pixel pitch of y  (floats) */
} iswm_conv_desc;

/* Arithmetic of the convolution kernels: 0 = exact fp32 MFMA (v_mfma_f32_32x32x2_f32);
 * 1 = "bf16x6": each fp32 operand is split exactly into three bf16 pieces and the product is formed
 * from six bf16 MFMAs with fp32 accumulation (error ~1e-7 relative, i.e. fp32 level, at up to 2.7x the
 * fp32 MFMA rate).  Default 1; the environment variable ISWM_CONV_MATH=f32 selects 0 at load time.
 * Mode 2 ("bf16", ISWM_CONV_MATH=bf16) is MIXED PRECISION, not fp32-grade: operands rounded to nearest bf16, ONE
 * bf16 MFMA per product, fp32 accumulation and fp32 tensors -- through the packed forward / data-gradient entry
 * points and the weight gradient; the plain entry points stay on the fp32 MFMA kernels in this mode.
 * Geometries the bf16x6 kernels do not cover (gathered channel count not a multiple of 32: the stem, the
 * 304-channel decoder input) always run on the fp32 MFMA kernels. */
int iswm_set_conv_math(int mode);
int iswm_get_conv_math(void);
/* name of the device kernel a call with this geometry launches (kind 0 fwd, 1 dgrad, 2 wgrad, 3 fwd_packed,
 * 4 dgrad_packed, 5 fwd_pl2 and 6 dgrad_pl2 / dgrad_pl2_bn, 7 wgrad_planes), from the same plan the call launches by.
 * Kind 1 names two entry points: it describes iswm_conv2d_dgrad_wt where iswm_conv2d_dgrad_wants_wt answers 1 (the call
 * the op wrappers then make) and iswm_conv2d_dgrad otherwise --
 * lets a profiler label its timings with the symbol rocprofv3 reports */
int iswm_conv2d_kernel_name(const iswm_conv_desc* d, int kind, char* buf, int buflen);
/* M tiling the forward kernel will use for this geometry: rows per tile (128 or 64) and number of
 * tiles == rows of the BN partials */
int iswm_conv2d_stat_tile_rows(const iswm_conv_desc* d);
int iswm_conv2d_stat_tiles(const iswm_conv_desc* d);
/* y = conv(x, w) (+ bias).  If stat_partials != NULL it receives per-M-tile
 * per-channel statistics [2][tiles][Cout] = {S_t, M2_t} (see iswm_colstat) for the training-mode
 * BatchNorm that follows every conv (network/backbone/resnet.py:89-93).
 * The partials describe the convolution BEFORE the bias: they are the same bits with bias == NULL, and with a bias they are
 * the statistics of y - bias, not of y (M2_t is the same either way, S_t lacks n_t * bias).  A caller that normalises a
 * biased output takes its statistics from iswm_colstat_res instead.  The same holds for iswm_conv2d_fwd_packed and
 * iswm_conv2d_fwd_pl2 (tests/test_bn_partials_gpu.py). */
int iswm_conv2d_fwd(const iswm_conv_desc* d, const float* x, const float* w, const float* bias,
                    float* y, float* stat_partials, iswm_stream_t stream);
/* dx (=|+=) conv_transpose(dy, w): autograd backward of the conv wrt its input;
 * accumulate != 0 adds into dx (branches that share an input, residual joins) */
int iswm_conv2d_dgrad(const iswm_conv_desc* d, const float* dy, const float* w, float* dx,
                      int accumulate, iswm_stream_t stream);
/* bf16x6 data gradient: needs the weights transposed to [Cin][KH][KW][Cout] (K axis contiguous for the
 * matrix cores).  iswm_conv2d_dgrad_wants_wt tells the host when to use this pair instead of
 * iswm_conv2d_dgrad (current conv math is bf16x6 and Cout % 32 == 0). */
int iswm_transpose_weights(const iswm_conv_desc* d, const float* w, float* wt, iswm_stream_t stream);
int iswm_conv2d_dgrad_wants_wt(const iswm_conv_desc* d);
int iswm_conv2d_dgrad_wt(const iswm_conv_desc* d, const float* dy, const float* wt, float* dx, int accumulate,
                         iswm_stream_t stream);
/* bf16x6 with pre-split weights: iswm_conv2d_pack_weights splits a weight tensor into its three bf16 planes and
 * stores them in MFMA fragment order (kind 0: for the forward conv, 1: for the data gradient, which also transposes);
 * the *_packed kernels then load the weight operand straight into registers.  iswm_conv2d_packed_weight_bytes
 * returns the buffer size, or 0 when the packed path does not apply (conv math f32, or the gathered channel
 * count -- Cin forward, Cout data gradient -- is not a multiple of 32). */
size_t iswm_conv2d_packed_weight_bytes(const iswm_conv_desc* d, int kind);
int iswm_conv2d_pack_weights(const iswm_conv_desc* d, int kind, const float* w, void* packed, iswm_stream_t stream);
/* Batched form: all conv weights of a model in ONE launch (a step otherwise issues two tiny pack kernels per conv).
 * jobs_dev is a DEVICE array of iswm_pack_job, hence `void*`, sorted by first_block; job i owns workgroups [first_block, first_block +
 * iswm_pack_job_blocks(...)); total_blocks is the sum.  iswm_packed_weight_bytes is the buffer size for
 * (Cout, taps, Cin, kind), 0 if the gathered channel count (Cin forward, Cout data gradient) is not 32-aligned.
 * kind 2 / 3: forward / data-gradient weights in the fragment order of the planes kernels (iswm_conv2d_fwd_pl2 /
 * iswm_conv2d_dgrad_pl2; gathered channel count a multiple of 64). */
typedef struct iswm_pack_job {
    const float* w;         /* [Cout][taps][Cin] (OHWI) */
    void* packed;
    int Cout, taps, Cin, kind;
    int first_block, reserved;
} iswm_pack_job;
size_t iswm_packed_weight_bytes(int Cout, int taps, int Cin, int kind);
int iswm_pack_job_blocks(int Cout, int taps, int Cin, int kind);
int iswm_pack_weights_batch(const void* jobs_dev, int njobs, int total_blocks, iswm_stream_t stream);
/* layout of the BN partials iswm_conv2d_fwd_packed writes: tiles x Cout floats per plane (sum, centred M2).
 * *tile_rows > 0: every tile holds that many rows (the last one the remainder); *tile_rows == 0: the tiles are
 * image patches of varying size and their row counts follow the planes as floats (partials + 2*tiles*Cout), so
 * the buffer is 2*tiles*Cout + tiles floats -- iswm_bn_finalize takes tile_rows = 0 for that layout. */
int iswm_conv2d_fwd_packed_stat_layout(const iswm_conv_desc* d, int* tiles, int* tile_rows);
/* (stat_partials: the statistics of the convolution BEFORE the bias, as iswm_conv2d_fwd's) */
int iswm_conv2d_fwd_packed(const iswm_conv_desc* d, const float* x, const void* wpk, const float* bias,
                           float* y, float* stat_partials, iswm_stream_t stream);
int iswm_conv2d_dgrad_packed(const iswm_conv_desc* d, const float* dy, const void* wpk, float* dx, int accumulate,
                             iswm_stream_t stream);
/* ---- "planes": activations stored PRE-SPLIT for the bf16x6 kernels.  A planes tensor is three bf16 tensors
 * [plane][pixel][ld] (hi, mid, lo -- the exact truncation split, hi + mid + lo == the fp32 value), plane_stride
 * bf16 elements apart (one plane under conv math "bf16": the value rounded to nearest).  The producer of an
 * activation writes the split once; the convolution stages its activation operand HBM -> LDS by LDS-DMA with no
 * split arithmetic in the loop.  In the *_planes entry points the pitch of the planes operand (d->ldx forward,
 * d->ldy data gradient) counts bf16 elements and must be a multiple of 8; same call sites as iswm_conv2d_fwd. */
int iswm_split_planes(const float* x, int64_t M, int C, int ldx, void* planes, int ldp, int64_t plane_stride,
                      iswm_stream_t stream);
int iswm_join_planes(const void* planes, int ldp, int64_t plane_stride, int64_t M, int C, float* x, int ldx,
                     iswm_stream_t stream);
/* Planes-aware forms of the memory-bound passes that produce or consume convolution operands.  A tensor argument typed
 * `void*` with a `*_ps` companion is an fp32 tensor when *_ps == 0 (pitch in floats), three bf16 planes when *_ps > 0
 * (pitch and plane stride in bf16 elements) and one rounded bf16 plane when *_ps == -1.  The fp32-only entry points
 * further down are these with every *_ps == 0. */
int iswm_bn_apply_pl(const float* y, int64_t M, int C, int ldy, const float* scale, const float* shift, const float* mean,
                     const void* residual, int ldr, int64_t res_ps, int relu, void* out, int ldo, int64_t out_ps,
                     iswm_stream_t stream);
int iswm_bn_backward_pl(const float* dout, int ldd, const void* out, int ldo, int64_t out_ps, const float* y, int ldy,
                        int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                        const float* mask_scale, const float* mask_shift, int relu, int training, float* dgamma,
                        float* dbeta, void* dy, int lddy, int64_t dy_ps, float* dres, int lddres, void* workspace,
                        size_t workspace_bytes, iswm_stream_t stream);
int iswm_maxpool3x3s2_fwd_pl(const float* x, int N, int H, int W, int C, void* y, int64_t y_ps, uint8_t* idx, int Ho,
                             int Wo, iswm_stream_t stream);
int iswm_gap_fwd_pl(const void* x, int64_t x_ps, int N, int HW, int C, int ldx, float* y, iswm_stream_t stream);
int iswm_bcast_fwd_pl(const float* v, int N, int HW, int C, void* y, int ldy, int64_t y_ps, iswm_stream_t stream);
int iswm_bilinear_fwd_pl(const float* x, int N, int Hi, int Wi, int C, int ldx, void* y, int64_t y_ps, int Ho, int Wo,
                         int ldy, iswm_stream_t stream);
/* second-generation planes kernels: (16*rbw) x 128 tiles, weights packed for the 16x16x32 MFMA (own packing) */
size_t iswm_conv2d_pl2_weight_bytes(const iswm_conv_desc* d, int kind);
int iswm_conv2d_pl2_pack_weights(const iswm_conv_desc* d, int kind, const float* w, void* packed, iswm_stream_t stream);
int iswm_conv2d_pl2_tile_rows(const iswm_conv_desc* d, int kind);
/* (stat_partials: [2][ceil(M / iswm_conv2d_pl2_tile_rows(d, 0))][Cout], the statistics of the convolution BEFORE the bias, as
 * iswm_conv2d_fwd's) */
int iswm_conv2d_fwd_pl2(const iswm_conv_desc* d, const void* xp, int64_t plane_stride, const void* wpk,
                        const float* bias, float* y, float* stat_partials, iswm_stream_t stream);
int iswm_conv2d_dgrad_pl2(const iswm_conv_desc* d, const void* dyp, int64_t plane_stride, const void* wpk,
                          float* dx, int accumulate, iswm_stream_t stream);
/* The same data gradient, also emitting the first pass of the BatchNorm backward that CONSUMES dx (the BatchNorm of the stage
 * whose activation the conv read -- reference resnet.py:103-118: bn1 / bn2 of a Bottleneck): per tile row t and input channel c
 *   partials[0][t][c] = sum dz,  partials[1][t][c] = sum dz * xhat,   dz = dx * [ReLU pattern],  xhat = (y - mean) * invstd
 * over the finished dx (after accumulation).  y: that stage's raw conv output [N*H*W][ldy]; relu: ISWM_GATE_NONE = no activation,
 * ISWM_GATE_RECOMPUTED = pattern (y - mean) * mask_scale + mask_shift > 0, exactly as iswm_bn_backward does; ISWM_GATE_RESIDUAL =
 * the producer is a RESIDUAL stage (bn3 of a Bottleneck, resnet.py:110-118): pattern = hi plane of its saved output planes (mask_hi,
 * pitch ld_mask bf16 elements) > 0, and dx is stored MASKED -- the one tensor is then both dout of that stage's BatchNorm backward
 * (call it with ISWM_ACT_NONE) and the gradient of its identity branch: no reduction pass, no separate dres.  partials: 2 * tiles * Cin doubles,
 * tiles = iswm_conv2d_dgrad_pl2_stat_tiles(d).  iswm_bn_backward_stats_pl then runs only the finalize and apply passes
 * (8 bytes per element of HBM traffic less than iswm_bn_backward_pl). */
int iswm_conv2d_dgrad_pl2_stat_tiles(const iswm_conv_desc* d);
int iswm_conv2d_dgrad_pl2_bn(const iswm_conv_desc* d, const void* dyp, int64_t plane_stride, const void* wpk, float* dx,
                             int accumulate, const float* y, int ldy, const float* mean, const float* invstd,
                             const float* mask_scale, const float* mask_shift, int relu, const void* mask_hi,
                             int ld_mask, double* partials, int tiles, iswm_stream_t stream);
int iswm_bn_backward_stats_pl(const float* dout, int ldd, const void* out, int ldo, int64_t out_ps, const float* y, int ldy,
                              int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                              const float* mask_scale, const float* mask_shift, int relu, int training, float* dgamma,
                              float* dbeta, void* dy, int lddy, int64_t dy_ps, float* dres, int lddres,
                              const double* partials, int tiles, void* workspace, size_t workspace_bytes,
                              iswm_stream_t stream);
/* ---- ASPP as one launch (conv_mfma_pl2t.hip): the parallel branches of network/_deeplab.py:143-172 -- ASPP.convs[0] (1x1),
 * convs[1..3] (ASPPConv, 3x3 at the three atrous rates, :121-128) -- over ONE tile table.  Rows (pixels) are sorted by their set
 * of in-bounds filter taps so that a tile runs exactly the taps that reach it; the tiles of all branches are dealt heaviest
 * first to a persistent grid; the data gradient of the four branches is a single GEMM over their 28 taps (dx written once).
 * The descriptor gives N, H, W (= Ho, Wo), Cin, Cout (PER BRANCH), stride 1, ldx, ldy; ksize[b] / dil[b] describe branch b
 * (odd square filter, pad = dil * (k - 1) / 2).  The PLAN (tap table, row order, tile table) is built on the host once per
 * geometry -- iswm_aspp_plan_bytes / iswm_aspp_plan -- and copied to the device by the caller; kind 0 forward, 1 data
 * gradient.  Pointer arrays (wpk, y, stats, dw) are host arrays of nbranch device pointers.
 *   iswm_aspp_fwd : y[b] = conv(x planes, w_b) into fp32 [N*H*W][ldy] + optional BatchNorm partials stats[b] = [2][T][Cout],
 *                   T = ceil(N*H*W / 144) tile rows of 144 (feed iswm_bn_finalize with tile_rows = 144);
 *                   wpk[b] = iswm_conv2d_pl2_pack_weights(kind 0) of branch b.
 *   iswm_aspp_bwd : dx (=|+=) sum_b conv^T(dy_b, w_b); dyp = planes of the concatenated gradient [N*H*W][ld_dy], branch b at
 *                   channels [b*Cout, (b+1)*Cout); wpk[b] = iswm_conv2d_pl2_pack_weights(kind 1) of branch b.  With xp / dw /
 *                   workspace it also runs the four weight gradients (iswm_conv2d_wgrad_planes per branch; workspace >= the
 *                   largest iswm_conv2d_wgrad_planes_workspace of the branches). */
size_t iswm_aspp_plan_bytes(const iswm_conv_desc* d, int nbranch, const int* ksize, const int* dil, int kind);
int iswm_aspp_plan(const iswm_conv_desc* d, int nbranch, const int* ksize, const int* dil, int kind, void* host_plan,
                   int grid_hint);
int iswm_aspp_fwd(const iswm_conv_desc* d, int nbranch, const int* ksize, const int* dil, const void* plan_dev, const void* xp,
                  int64_t x_ps, const void* const* wpk, float* const* y, float* const* stats, iswm_stream_t stream);
int iswm_aspp_bwd(const iswm_conv_desc* d, int nbranch, const int* ksize, const int* dil, const void* plan_dev, const void* dyp,
                  int64_t dy_ps, int ld_dy, const void* const* wpk, float* dx, int accumulate, const void* xp, int64_t x_ps,
                  float* const* dw, float* workspace, size_t workspace_bytes, iswm_stream_t stream);
/* weight gradient with BOTH operands pre-split (x: planes of the conv input, pitch d->ldx; dy: planes of the gradient of
 * the conv output, pitch d->ldy; pitches and plane strides in bf16 elements).  Needs Cin % 8 == 0 and Cout % 8 == 0
 * (iswm_conv2d_wgrad_planes_ok); same result layout, workspace protocol and call sites as iswm_conv2d_wgrad. */
int iswm_conv2d_wgrad_planes_ok(const iswm_conv_desc* d);
size_t iswm_conv2d_wgrad_planes_workspace(const iswm_conv_desc* d);
int iswm_conv2d_wgrad_planes(const iswm_conv_desc* d, const void* xp, int64_t x_ps, const void* dyp, int64_t dy_ps, float* dw,
                             float* workspace, size_t workspace_bytes, iswm_stream_t stream);
/* ---- depthwise convolution (groups == channels): first half of AtrousSeparableConvolution,
 * network/_deeplab.py:95-119.  The descriptor has Cin == Cout == channel count of the (possibly zero-padded)
 * activation; w is the torch parameter [Cw][1][KH][KW] as stored, Cw <= Cin (extra channels see zero weights).
 * HBM-bound streaming kernels; the weight gradient reduces in a fixed order (workspace of doubles). */
int iswm_dwconv2d_fwd(const iswm_conv_desc* d, const float* x, const float* w, int Cw, const float* bias, float* y,
                      iswm_stream_t stream);
int iswm_dwconv2d_dgrad(const iswm_conv_desc* d, const float* dy, const float* w, int Cw, float* dx, int accumulate,
                        iswm_stream_t stream);
size_t iswm_dwconv2d_wgrad_workspace(const iswm_conv_desc* d);
int iswm_dwconv2d_wgrad(const iswm_conv_desc* d, const float* x, const float* dy, int Cw, float* dw, void* workspace,
                        size_t workspace_bytes, iswm_stream_t stream);
/* ---- depthwise 3x3 (KH == KW == 3, pad == dil, stride 1 or 2): the depthwise -> BatchNorm stage of MobileNetV2's
 * inverted-residual blocks (csrc/dwconv3.hip).  Same operand conventions as iswm_dwconv2d_*, and y / dx are bit-identical
 * to iswm_dwconv2d_fwd / iswm_dwconv2d_dgrad.
 *   iswm_dwconv3x3_fwd_stats : y = dwconv(x, w) and, when stat_partials != NULL, the BatchNorm partials [2][tiles][Cin]
 *                              (sum, centred M2) over tiles of iswm_dwconv3x3_stat_tile_rows(d) consecutive output pixels
 *                              in raster order, the last tile short -- the layout iswm_bn_finalize takes from iswm_colstat.
 *                              The two queries are pure host functions of the descriptor.
 *   iswm_dwconv3x3_bwd       : dx (=|+=) the data gradient and dw[Cw][9] the weight gradient from ONE pass over dy and x
 *                              (fp32 per-workgroup partials in the workspace, merged in double in a fixed order: no
 *                              atomics, run-to-run identical).  dx [N,H,W,lddx] has a pitch of its own; dx == NULL or
 *                              dw == NULL skips that half (x and the workspace are needed for dw only). */
int iswm_dwconv3x3_stat_tile_rows(const iswm_conv_desc* d);
int iswm_dwconv3x3_stat_tiles(const iswm_conv_desc* d);
int iswm_dwconv3x3_fwd_stats(const iswm_conv_desc* d, const float* x, const float* w, int Cw, float* y,
                             float* stat_partials, iswm_stream_t stream);
size_t iswm_dwconv3x3_bwd_workspace(const iswm_conv_desc* d);
int iswm_dwconv3x3_bwd(const iswm_conv_desc* d, const float* x, const float* dy, const float* w, int Cw, float* dx,
                       int lddx, int accumulate, float* dw, void* workspace, size_t workspace_bytes, iswm_stream_t stream);
/* dw[Cout][KH][KW][Cin] = sum over pixels.  workspace holds split-K slabs. */
size_t iswm_conv2d_wgrad_workspace(const iswm_conv_desc* d);
int iswm_conv2d_wgrad(const iswm_conv_desc* d, const float* x, const float* dy, float* dw,
                      float* workspace, size_t workspace_bytes, iswm_stream_t stream);

/* ---- BatchNorm2d (training and eval), ReLU, residual add ---------------------
 * nn.BatchNorm2d eps 1e-5 momentum 0.1 + nn.ReLU + FloatFunctional.add:
 * network/backbone/resnet.py:99-120, network/_deeplab.py:38-39,125-126,135-136. */
/* Tile statistics.  partials[2][tiles][C]: [0] = per-tile column sum S_t, [1] = per-tile
 * sum of squared deviations from the TILE mean (M2_t).  Tile t covers rows
 * [t*tile_rows, min(M, (t+1)*tile_rows)).  The conv forward epilogue emits the same pair
 * with tile_rows = 128 (iswm_conv2d_stat_tiles); iswm_colstat computes it for any [M, C]
 * (pitch ld) tensor with tiles = ceil(M / iswm_colstat_tile_rows(M)) <= iswm_colstat_tiles(M). */
int iswm_colstat_tiles(int64_t M);
int64_t iswm_colstat_tile_rows(int64_t M);
int iswm_colstat(const float* x, int64_t M, int C, int ld, float* partials, iswm_stream_t stream);
/* merge tiles (pairwise/Chan update in double) -> batch mean / biased var, update running
 * stats (unbiased var, momentum), emit scale = gamma*invstd, shift = beta, and save mean /
 * invstd (iswm_bn_apply evaluates (y - mean)*scale + shift). */
int iswm_bn_finalize(const float* partials, int tiles, int C, int64_t count, int64_t tile_rows,
                     const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                     float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                     iswm_stream_t stream);
/* The same pair with the residual of the tile sum: partials[3][tiles][C], [2] = R_t = sum over the tile of (x - mu_t) about the
 * fp32 centre mu_t = S_t / n_t that M2_t is taken about.  S_t is an fp32 sum, so mu_t is not the tile's true mean; with R_t the
 * merge is exact:  mean = sum (n_t mu_t + R_t) / N,  M2 = sum [M2_t + 2 (mu_t - mean) R_t + n_t (mu_t - mean)^2].  Planes [0], [1]
 * are bit-identical to iswm_colstat's.  Without R_t the variance is off by ~2^-23 |mean| / sigma (3e-5 at |mean| = 2000 sigma). */
int iswm_colstat_res(const float* x, int64_t M, int C, int ld, float* partials, iswm_stream_t stream);
int iswm_bn_finalize_res(const float* partials, int tiles, int C, int64_t count, int64_t tile_rows,
                         const float* gamma, const float* beta, float* running_mean, float* running_var, float momentum,
                         float eps, float* scale, float* shift, float* save_mean, float* save_invstd,
                         iswm_stream_t stream);
/* eval mode: scale/shift from the running statistics */
int iswm_bn_eval_coeffs(int C, const float* gamma, const float* beta, const float* running_mean,
                        const float* running_var, float eps, float* scale, float* shift,
                        float* save_mean, float* save_invstd, iswm_stream_t stream);
/* out = act((y - mean[c])*scale[c] + shift[c] (+ residual)); relu: ISWM_ACT_NONE, ISWM_ACT_RELU or ISWM_ACT_RELU6 */
int iswm_bn_apply(const float* y, int64_t M, int C, int ldy, const float* scale, const float* shift,
                  const float* mean, const float* residual, int ldr, int relu, float* out, int ldo,
                  iswm_stream_t stream);
/* backward of out = act(BN(y) (+ residual)), relu an ISWM_ACT_* code:  dz = dout * (out > 0 if ReLU, 0 < out < 6 if ReLU6);
 *   dbeta = sum dz, dgamma = sum dz*xhat (two deterministic stages, accumulated in double as
 *   ATen's CPU kernel does);
 *   dy = gamma*invstd*(dz - dbeta/M - xhat*dgamma/M) (training) or gamma*invstd*dz (eval);
 *   dres (optional) = dz, the gradient of the identity branch.
 * workspace: iswm_bn_bwd_workspace(M, C) bytes, 16-byte aligned.  mask_scale / mask_shift (optional, ISWM_ACT_RELU without
 * residual): the forward's scale and shift -- the ReLU sign pattern is then recomputed as (y - mean)*scale + shift > 0 (bit-identical to iswm_bn_apply) and `out` is not read. */
size_t iswm_bn_bwd_workspace(int64_t M, int C);
int iswm_bn_backward(const float* dout, int ldd, const float* out, int ldo, const float* y, int ldy,
                     int64_t M, int C, const float* mean, const float* invstd, const float* gamma,
                     const float* mask_scale, const float* mask_shift,
                     int relu, int training, float* dgamma, float* dbeta, float* dy, int lddy,
                     float* dres, int lddres, void* workspace, size_t workspace_bytes,
                     iswm_stream_t stream);
/* out[c] = sum over tiles of partials[0][t][c] (bias gradient from iswm_colstat partials);
 * scratch: C floats */
int iswm_colsum_finalize(const float* partials, int tiles, int C, float* out, float* scratch,
                         iswm_stream_t stream);

/* ---- pooling ------------------------------------------------------------------ */
/* nn.MaxPool2d(3, 2, 1), network/backbone/resnet.py:148.  idx[n,ho,wo,c] = winning
 * tap 0..8 (first max in scan order, as ATen). */
int iswm_maxpool3x3s2_fwd(const float* x, int N, int H, int W, int C, float* y, uint8_t* idx, int Ho,
                          int Wo, iswm_stream_t stream);
int iswm_maxpool3x3s2_bwd(const float* dy, const uint8_t* idx, int N, int H, int W, int C, int Ho,
                          int Wo, float* dx, iswm_stream_t stream);
/* nn.AdaptiveAvgPool2d(1), network/_deeplab.py:133: y[n,c] = mean over HW */
int iswm_gap_fwd(const float* x, int N, int HW, int C, int ldx, float* y, iswm_stream_t stream);
/* dx[n,p,c] (+)= dy[n,c]/HW  (accumulate != 0 adds into dx) */
int iswm_gap_bwd(const float* dy, int N, int HW, int C, float* dx, int lddx, int accumulate,
                 iswm_stream_t stream);
/* broadcast a [N,C] vector over HW pixels (bilinear upsample of a 1x1 map,
 * network/_deeplab.py:141) into a channel slice, and its backward (sum over HW) */
int iswm_bcast_fwd(const float* v, int N, int HW, int C, float* y, int ldy, iswm_stream_t stream);
int iswm_bcast_bwd(const float* dy, int lddy, int N, int HW, int C, float* dv, iswm_stream_t stream);

/* ---- bilinear resize, align_corners=False ------------------------------------
 * F.interpolate call sites: network/_deeplab.py:58, network/utils.py:22. */
int iswm_bilinear_fwd(const float* x, int N, int Hi, int Wi, int C, int ldx, float* y, int Ho, int Wo,
                      int ldy, iswm_stream_t stream);
int iswm_bilinear_bwd(const float* dy, int N, int Hi, int Wi, int C, int lddy, int Ho, int Wo, float* dx,
                      int lddx, iswm_stream_t stream);
/* final upsample fused with the NHWC -> NCHW layout change of the logits
 * (network/utils.py:22-24): x NHWC [N,Hi,Wi,ldx] (first C channels) -> y NCHW */
int iswm_bilinear_nhwc_to_nchw_fwd(const float* x, int N, int Hi, int Wi, int C, int ldx, float* y,
                                   int Ho, int Wo, iswm_stream_t stream);
int iswm_bilinear_nhwc_to_nchw_bwd(const float* dy, int N, int Hi, int Wi, int C, int lddx, int Ho,
                                   int Wo, float* dx, iswm_stream_t stream);

/* ---- layout / elementwise helpers ---------------------------------------------- */
/* NCHW [N,C,H,W] -> NHWC with Cp >= C channels (extra channels zero) */
int iswm_nchw_to_nhwc(const float* x, int N, int C, int HW, float* y, int Cp, iswm_stream_t stream);
int iswm_nhwc_to_nchw(const float* x, int N, int C, int HW, int ldx, float* y, iswm_stream_t stream);
/* copy C channels between pitched [M, *] buffers (torch.cat / its backward,
 * network/_deeplab.py:59,171) */
int iswm_copy_channels(const float* src, int lds, float* dst, int ldd, int64_t M, int C,
                       iswm_stream_t stream);
int iswm_add_inplace(float* dst, const float* src, int64_t n, iswm_stream_t stream);
int iswm_scale_inplace(float* x, int64_t n, const float* scalar_dev, float host_mul, iswm_stream_t stream);
/* The heads' last two layers with the 1x1 classifier folded into the BatchNorm passes of the stage in front of it --
 * Conv2d(256, 256, 3) -> BatchNorm2d -> ReLU -> Conv2d(256, num_classes, 1), network/_deeplab.py:44-52 (DeepLabHeadV3Plus) and
 * :84-90 (DeepLabHead): forward = one pass over the raw conv output y to logits [M][4] (the 256-channel activation is never
 * stored); backward = the stage's BatchNorm backward fed by dlogit [M][4] and the zero-padded classifier weight wc4 [4][C],
 * returning the classifier's weight gradient dwc4 with it.  C == 256, num_classes <= 4. */
int iswm_bn_apply_classify(const float* y, int64_t M, int C, int ldy, const float* scale, const float* shift, const float* mean,
                           const float* wc4, const float* bias4, float* logits, int ldl, iswm_stream_t stream);
size_t iswm_bn_classify_bwd_workspace(int64_t M, int C);
int iswm_bn_backward_classify(const float* dlogit, int ldl, const float* wc4, const float* y, int ldy, int64_t M, int C,
                              const float* mean, const float* invstd, const float* gamma, const float* mask_scale,
                              const float* mask_shift, int training, float* dgamma, float* dbeta, float* dwc4, void* dy, int lddy,
                              int64_t dy_ps, void* workspace, size_t workspace_bytes, iswm_stream_t stream);
/* Convolutions whose channel counts are not multiples of the kernels' granule (nn.Conv2d(3, 64, 7) at network/backbone/resnet.py:137,
 * Conv2d(304, 256, 3) / Conv2d(256, 48, 1) / Conv2d(256, num_classes, 1) at network/_deeplab.py:36-52): zero-padded OHWI copy of an OIHW
 * parameter with element strides[4] = (O, I, H, W); the inverse for its gradient; zero bytes [byte0, byte1) of every row of a
 * (planes or fp32) activation buffer -- the padding channels themselves.  They replace torch.zeros / slice-copy / zero_() on the step. */
int iswm_pad_weights(const float* w, int cout, int cin, int kh, int kw, const int64_t* strides, int cout_p, int cin_p, float* out_ohwi,
                     iswm_stream_t stream);
int iswm_unpad_weights(const float* dw_ohwi, int cout_p, int cin_p, int cout, int cin, int kh, int kw, float* grad,
                       const int64_t* strides, iswm_stream_t stream);
/* the flat gradient arena of the fused optimizers before a backward pass (optimizer.zero_grad(), train.py:607) */
int iswm_fill_zero(void* p, size_t bytes, iswm_stream_t stream);
int iswm_zero_cols(void* y, int64_t M, int64_t ld_bytes, int byte0, int byte1, int64_t plane_bytes, int nplanes, iswm_stream_t stream);
/* nn.Dropout(p), network/_deeplab.py:165: counter-based Philox mask */
int iswm_dropout_fwd(const float* x, float* y, uint8_t* mask, int64_t n, float p, uint64_t seed,
                     uint64_t offset, iswm_stream_t stream);
int iswm_dropout_bwd(const float* dy, const uint8_t* mask, float* dx, int64_t n, float p,
                     iswm_stream_t stream);

/* ---- fused weighted cross-entropy / focal loss ---------------------------------
 * nn.CrossEntropyLoss(weight, ignore_index=255), train.py:454-459 and
 * FocalLoss.forward, utils/loss.py:23-35.  logits NCHW [B,C,H,W]; labels uint8 or
 * int64 [B,H,W].  mode 0: weighted mean (CE); 1: focal mean over all pixels;
 * 2: focal sum.  One pass writes the UNNORMALISED gradient and per-block partial
 * sums {sum w*nll or sum focal, sum w}; iswm_loss_finalize reduces them into
 * sums[2] and loss[1] (deterministic two-stage reduction). */
int iswm_loss_blocks(int64_t npix);
int iswm_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                  const float* class_weight, int ignore_index, float alpha, float gamma, int mode,
                  float* grad_unnorm, float* partials, iswm_stream_t stream);
int iswm_loss_finalize(const float* partials, int blocks, int mode, int64_t npix, float* sums,
                       float* loss, iswm_stream_t stream);
/* grad *= upstream * (mode 0: 1/sums[1]; mode 1: 1/npix; mode 2: 1) */
int iswm_loss_bwd_scale(float* grad, int64_t n, const float* sums, const float* upstream, int mode,
                        int64_t npix, iswm_stream_t stream);
/* ---- region-overlap losses (soft Dice / Tversky / focal-Tversky) + weighted CE ---
 * Over the valid pixels (label != ignore_index and 0 <= label < C), p = softmax:
 *   I_c = sum p_c [y == c], P_c = sum p_c, G_c = sum [y == c],
 *   T_c = (I_c + s) / (I_c + alpha (P_c - I_c) + beta (G_c - I_c) + s),
 *   L = ce_weight * sum(w nll) / sum(w) + overlap_weight * mean_{c in S} max(1 - T_c, 0)^gamma,
 *   S = the classes >= 1 (classes 0) or all of them (classes 1).  1 <= C <= 8.
 * fwd: one pass over logits and labels (no per-pixel store) into partials
 *   [(2 + 3C) * iswm_loss_blocks(B * HW)] and their fixed-order double sums
 *   sums[2 + 3C] = {sum w nll, sum w, I[C], P[C], G[C]} (device memory); sums[0..1]
 *   are iswm_loss_fwd's mode-0 sums bit for bit.  Under data parallelism the host
 *   all-reduces sums before coeffs.
 * coeffs: sums -> loss[1] and coef[1 + 2C] = {ce_weight / sum w, overlap_weight *
 *   dL_ov/dI_c [C], overlap_weight * dL_ov/dP_c [C]}, in double on the device; the
 *   derivative of max(1 - T, 0)^gamma is taken as 0 where 1 - T <= 0.  ce_weight 0
 *   leaves the CE term out (finite on a batch with no valid pixel).
 * bwd: reads logits and labels again and writes upstream[0] * dL/dlogits once
 *   (exactly 0 at invalid pixels); upstream is a device scalar. */
int iswm_overlap_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                          const float* class_weight, int ignore_index, float* partials, double* sums,
                          iswm_stream_t stream);
int iswm_overlap_loss_coeffs(const double* sums, int C, double ce_weight, double overlap_weight, double alpha,
                             double beta, double gamma, double smooth, int classes, float* loss, float* coef,
                             iswm_stream_t stream);
int iswm_overlap_loss_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                          const float* class_weight, int ignore_index, const float* coef, const float* upstream,
                          float* grad, iswm_stream_t stream);
/* ---- hard-pixel mining (OHEM / bootstrapped cross-entropy) ---------------------------
 * Over the valid pixels V (label != ignore_index and 0 <= label < C), nll as iswm_loss_fwd forms it:
 *   k = min(min_kept, |V|),  nu = min(nu0, k-th largest nll over V)  (nu0 = float(-ln thresh); nu = nu0 if k == 0),
 *   K = {i in V : nll_i >= nu} (ties at nu all kept),  L = sum_K w nll / sum_K w  (0 if K is empty),
 *   dL/dz = upstream w (p - onehot) / sum_K w on K, exactly 0 elsewhere.  1 <= C <= 8.
 * keys: one int32 per pixel = the bit pattern of nll (-0.0 and NaN stored as +0), -1 at an invalid pixel; non-negative
 *   floats order as these integers.  counts [iswm_loss_blocks(B * HW)] is a workspace (the blocks' valid counts);
 *   nvalid[1] (int64) = |V|, their sum.
 * hist / scan: an exact radix select over the keys, iswm_ohem_digits() = 3 digits of 11 + 10 + 10 bits from the top.
 *   hist(digit) ADDS to hist[iswm_ohem_bins() = 2048] (int64, zeroed by the caller) the counts of that digit among the keys that carry
 *   the prefix chosen so far; scan(digit) picks the bin holding the wanted rank and leaves state[4] (int64) =
 *   {prefix, remaining rank, k, -} for the next digit; scan(0) forms k from nvalid and min_kept, scan(2) writes nu[1].
 *   Call hist(0), scan(0), hist(1), scan(1), hist(2), scan(2).  Nothing is read back by the host.
 * sums: partials [3 * iswm_loss_blocks(npix)] and sums[3] (double) = {sum_K w nll, sum_K w, |K|}; kept is decided as
 *   key >= bits(nu) on the stored keys.  With nu = 0 sums[0..1] are iswm_loss_fwd's mode-0 sums bit for bit.
 * loss: out[2] = {L, 1 / sum_K w} (both 0 if K is empty).   bwd: the finished gradient, written once.
 * Under data parallelism the host all-reduces nvalid (before scan(0)), each hist (before its scan) and sums (before
 * loss); every result is then the global batch's.  All results are bit-reproducible (integer counts, fixed-order sums). */
int iswm_ohem_digits(void);
int iswm_ohem_bins(void);
int iswm_ohem_keys(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                   int ignore_index, int32_t* keys, int32_t* counts, int64_t* nvalid, iswm_stream_t stream);
int iswm_ohem_hist(const int32_t* keys, int64_t npix, const int64_t* state, int digit, int64_t* hist,
                   iswm_stream_t stream);
int iswm_ohem_scan(const int64_t* hist, const int64_t* nvalid, int digit, int64_t min_kept, float nu0,
                   int64_t* state, float* nu, iswm_stream_t stream);
int iswm_ohem_sums(const int32_t* keys, const void* labels, int label_bytes, int64_t npix, int C,
                   const float* class_weight, const float* nu, float* partials, double* sums, iswm_stream_t stream);
int iswm_ohem_loss(const double* sums, float* out, iswm_stream_t stream);
int iswm_ohem_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                  const float* class_weight, const int32_t* keys, const float* nu, const float* lossinv,
                  const float* upstream, float* grad, iswm_stream_t stream);
/* ---- Lovasz-Softmax, per image, + weighted CE (lovasz.hip) ------------------------------------
 * Segment (b, c) = image b, class c of S (classes 0: c >= 1; classes 1: every c), nseg = B * |S| segments of P = HW pixels,
 * segment index b * |S| + (c - first).  Over the valid pixels of image b: e = |[y == c] - softmax_c| in [0, 1],
 * sorted descending (ties: g = 1 first, then ascending pixel index); omega_j = the Jaccard increment at position j in
 * closed form;  L = ce_weight * sum(w nll) / sum(w) + lovasz_weight * (sum over segments with G > 0 of sum_j e_j omega_j) / N.
 * 1 <= C <= 8, 1 <= P <= 2^24, nseg <= 65535, nseg * P < 2^31; anything else is refused with a message.
 * keys: keys [nseg, P] = ((bits(e) << 1) | g) + 1, 0 at an invalid pixel; counts [nseg, 2] (int32) = {valid pixels of
 *   the image, G}; partials [2 * iswm_loss_blocks(B * HW)] is a workspace; sums[0..1] (double) = {sum w nll, sum w},
 *   iswm_loss_fwd's mode-0 sums bit for bit once rounded to float.
 * sort: stable descending LSD radix sort of nseg segments of P uint32 keys, iswm_lovasz_digits() digits of 8 bits over
 *   tiles of iswm_lovasz_tile() keys -> sorted [nseg, P], perm [nseg, P] (the key's index in its segment).
 *   workspace: iswm_lovasz_workspace(nseg, P) bytes (0 and a message for sizes the sort does not take).
 * weights: sorted, perm, counts -> m [nseg, P]: m[seg, perm[j]] = omega_j, 0 at invalid pixels and where G = 0;
 *   out[0..1] (double) = {sum over present segments of L_bc, N}.  Same workspace.
 * loss: sums[4] = {sum w nll, sum w, sum L_bc, N} (this process's or all-reduced) -> out[3] = {loss, ce_weight / sum w,
 *   lovasz_weight / N}; a term whose normaliser is 0 is 0 and so is its coefficient.
 * bwd: logits, labels, m, coef = out + 1 -> upstream[0] * dL/dlogits written once, exactly 0 at invalid pixels.
 * Every result is bit-reproducible: integer counts and ranks, fixed-order sums, no float atomics. */
int iswm_lovasz_digits(void);
int iswm_lovasz_tile(void);
int64_t iswm_lovasz_workspace(int64_t nseg, int64_t P);
int iswm_lovasz_keys(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                     const float* class_weight, int ignore_index, int classes, uint32_t* keys, int32_t* counts,
                     float* partials, double* sums, iswm_stream_t stream);
int iswm_lovasz_sort(const uint32_t* keys, int64_t nseg, int64_t P, void* workspace, int64_t workspace_bytes,
                     uint32_t* sorted, uint32_t* perm, iswm_stream_t stream);
int iswm_lovasz_weights(const uint32_t* sorted, const uint32_t* perm, const int32_t* counts, int64_t nseg, int64_t P,
                        void* workspace, int64_t workspace_bytes, float* m, double* out, iswm_stream_t stream);
int iswm_lovasz_loss(const double* sums, double ce_weight, double lovasz_weight, float* out, iswm_stream_t stream);
int iswm_lovasz_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW,
                    const float* class_weight, int ignore_index, int classes, const float* m, const float* coef,
                    const float* upstream, float* grad, iswm_stream_t stream);
/* logits.max(1)[1], train.py:644,659 -- ties resolve to the lowest class index */
int iswm_argmax_nchw(const float* logits, int B, int C, int64_t HW, int64_t* out, iswm_stream_t stream);

/* ---- validation metrics ------------------------------------------------------------
 * StreamMetrics._fast_hist, metrics/stream_metrics.py:24-31: hist[n_classes][n_classes] (int64, row = ground
 * truth, column = prediction) += bincount(n_classes*label + pred) over the pixels whose label lies in
 * [0, n_classes) (255 = ignore falls outside).  Exact integer counting; accumulates into hist.
 * dtype codes: 0 = uint8, 1 = int64.  The _logits form takes the prediction as logits.max(1)[1]
 * (train.py:644,659) without materialising the mask. */
int iswm_confusion_matrix(const void* labels, int label_dtype, const void* preds, int pred_dtype, int64_t npix,
                          int n_classes, int64_t* hist, iswm_stream_t stream);
int iswm_confusion_matrix_logits(const void* labels, int label_dtype, const float* logits, int B, int C, int64_t HW,
                                 int n_classes, int64_t* hist, iswm_stream_t stream);

/* ---- sequence-validation metrics (mask_metrics.hip) ----------------------------------
 * Batched [N, H, W] masks (1 <= H, W <= 2048), current stream, no host copies.  src dtype codes: 0 = uint8,
 * 1 = int64; inputs are binarised with > 0.  Borders are neutral (cv2's default for morphology).
 * morph: dst = dilate (dilate != 0) or erode of the mask by a (2*radius+1)^2 rectangle.
 * ccl: 8-connected components of mask != 0; labels[i] = the smallest frame raster index (y*W+x) of the
 *   pixel's component, -1 for background; areas[i] = the component's pixel count where i is that root, else 0.
 * preprocess: MaskUtils.preprocess_mask (metrics/utils/mask_utils.py:7-50) -- close, open (3x3), largest
 *   component of area >= 0.001*H*W (ties: smallest root) -> out (0/1), weight (1, max(0.4, 1-0.2*(n-1)), or 0
 *   with an empty out), area.
 * fronts: per row the leftmost column whose value (mask * weight; weight NULL = 1) equals 1, else -1;
 *   stats[N][3] = count, sum of rows, sum of columns.
 * front_error: FrontTrackingMetrics.calculate_error on front rows [N][H] of each (pred, gt) pair.
 * pair_scores: MaskUtils.calculate_stability / calculate_motion of (current, previous) pairs.
 * region_score: RegionMetrics.calculate_region_metrics; valid = 0 where either frame is empty. */
int iswm_mask_morph(const void* src, int src_dtype, int N, int H, int W, int radius, int dilate, uint8_t* dst,
                    iswm_stream_t stream);
int iswm_ccl(const uint8_t* mask, int N, int H, int W, int32_t* labels, int32_t* areas, iswm_stream_t stream);
size_t iswm_mask_preprocess_workspace(int N, int H, int W);
int iswm_mask_preprocess(const void* src, int src_dtype, int N, int H, int W, uint8_t* out, double* weight,
                         int64_t* area, void* workspace, size_t workspace_bytes, iswm_stream_t stream);
int iswm_mask_fronts(const uint8_t* mask, const double* weight, int N, int H, int W, int32_t* fronts, int64_t* stats,
                     iswm_stream_t stream);
int iswm_front_error(const int32_t* pred_fronts, const int32_t* gt_fronts, int N, int H, double tau, double* out,
                     iswm_stream_t stream);
int iswm_mask_pair_scores(const int32_t* curr_fronts, const int64_t* curr_stats, const uint8_t* prev_mask,
                          const double* prev_weight, const int64_t* prev_stats, int N, int H, int W, double* stability,
                          double* motion, iswm_stream_t stream);
size_t iswm_region_workspace(int N, int H, int W);
int iswm_region_score(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int N, int H, int W, double* score,
                      int32_t* valid, void* workspace, size_t workspace_bytes, iswm_stream_t stream);

/* ---- training-input pipeline -------------------------------------------------------
 * The reference's per-sample PIL chain ExtRandomScale -> ExtRandomCrop(pad_if_needed) -> ExtRandomHorizontalFlip ->
 * ExtToTensor -> ExtNormalize (train.py:355-362, utils/ext_transforms.py:94-115,212-396) for a whole batch in one
 * launch: uint8 HWC source images + uint8 HW labels in, normalised fp32 NCHW batch + uint8 label batch out.
 * Bit-exact with Pillow's BILINEAR (image) / NEAREST (label) resize: the host computes Pillow's per-column /
 * per-row bounds, 22-bit fixed-point weights and nearest-source indices (iswm_amd/utils/ext_transforms.py) and
 * passes them in `tables`: per sample, at tab_off (ints):
 *   xintab[rs_w] | yintab[rs_h] | hbounds[rs_w][2] (first source column, count) | hk[rs_w][ksize_h] |
 *   vbounds[rs_h][2] | vk[rs_h][ksize_v].
 * images / labels / samples / tables / outputs are device pointers; mean3 / std3 are HOST arrays of 3 floats. */
typedef struct iswm_aug_sample {
    long long img_off;      /* byte offset of this sample's uint8 [src_h][src_w][3] image in `images` */
    long long lbl_off;      /* byte offset of its uint8 [src_h][src_w] label in `labels` */
    int src_h, src_w;
    int rs_h, rs_w;         /* size after the random rescale */
    int pad;                /* border added on every side by pad_if_needed (0: none) */
    int crop_i, crop_j;     /* crop origin (row, column) in the padded image */
    int flip;               /* bit 0: horizontal flip after the crop; bit 1 (iswm_augment_batch_ex only): vertical flip */
    int tab_off;
    int ksize_h, ksize_v;
    int reserved;
} iswm_aug_sample;
int iswm_augment_batch(const unsigned char* images, const unsigned char* labels, const void* samples,
                       const int* tables, int B, int crop_h, int crop_w, const float* mean3, const float* std3,
                       float* out_nchw, unsigned char* out_labels, iswm_stream_t stream);

/* ---- rotation, vertical flip and colour jitter (augment.hip) ---------------------------------
 * The reference's ExtRandomRotation (nearest, no expand, image centre), ExtRandomVerticalFlip and ExtColorJitter
 * (utils/ext_transforms.py:147,236,429) around the chain above, bit for bit Pillow's arithmetic.  Every sample has a
 * second record next to its iswm_aug_sample:
 *   rotation: Pillow's Geometry.c affine_fixed.  The host passes the 16.16 fixed-point coefficients; output pixel
 *     (x, y) of the rotated tile reads source ((a[2] + y*a[1] + x*a[0]) >> 16, (a[5] + y*a[4] + x*a[3]) >> 16) when
 *     both lie inside the tile, else image 0 / label 0.  Pillow's exact transposes (180; 90 / 270 of a square tile)
 *     are the same form with whole-pixel coefficients.  rot_mode 0: the sample is not rotated and not copied.
 *   ops: up to four colour operations applied in order to the uint8 RGB triple of each output pixel:
 *     ISWM_AUG_OP_BRIGHTNESS / _CONTRAST / _SATURATION: Image.blend(degenerate, image, factor[op]) with the degenerate
 *     0 / the rounded mean grey of the whole cropped image as it is when the op runs / the pixel's own grey;
 *     ISWM_AUG_OP_HUE: RGB -> HSV, H += hue_shift (mod 256), HSV -> RGB (Convert.c).
 * aug_rotate: one pass; writes the rotated image (uint8 HWC) and label (uint8 HW) of every sample with rot_mode != 0
 *   at rot_img_off / rot_lbl_off (multiples of 16) of the two scratch arenas; same size as the source tile.  max_hw >=
 *   every src_h * src_w (sizes the grid).  A record whose copy would end past an arena is left unwritten.
 * augment_batch_ex: iswm_augment_batch's chain with, per sample, the source read from the scratch arenas when
 *   rot_mode != 0, bit 1 of iswm_aug_sample.flip = vertical flip after the horizontal one, then the op list, then
 *   ToTensor / Normalize.  any_contrast != 0 (some list holds a contrast op) runs a pre-pass that sums the grey of every
 *   such sample in int64: per-workgroup partials in the workspace, summed per sample by one workgroup in index order.
 *   any_contrast == 0 is the caller's promise that no record holds a contrast op (the records are device memory and the
 *   entry point does not read them back, as with max_rs and max_hw); a contrast op under a broken promise blends
 *   against 0, i.e. acts as a brightness op.  Passing 1 is always right.  crop_h * crop_w <= 2^30.
 *   rot_images / rot_labels may be null when no sample has rot_mode != 0.
 * iswm_augment_batch_ex_workspace(B, crop_h, crop_w) = bytes of the workspace (needed whatever any_contrast is). */
#define ISWM_AUG_OP_BRIGHTNESS 0
#define ISWM_AUG_OP_CONTRAST 1
#define ISWM_AUG_OP_SATURATION 2
#define ISWM_AUG_OP_HUE 3
typedef struct iswm_aug_extra {
    int rot_mode;           /* 0: none, 1: fixed-point affine map */
    int a[6];               /* 16.16 fixed point */
    int n_ops;              /* 0..4 */
    long long rot_img_off;  /* byte offsets of the rotated copy in the scratch arenas */
    long long rot_lbl_off;
    int ops[4];             /* ISWM_AUG_OP_*, in the order they are applied */
    float factor[4];        /* indexed by op code; factor[ISWM_AUG_OP_HUE] is unused */
    int hue_shift;          /* 0..255 */
    int reserved[3];
} iswm_aug_extra;
int iswm_aug_rotate(const unsigned char* images, const unsigned char* labels, const void* samples, const void* extras,
                    int B, long long max_hw, unsigned char* rot_images, size_t rot_images_bytes,
                    unsigned char* rot_labels, size_t rot_labels_bytes, iswm_stream_t stream);
size_t iswm_augment_batch_ex_workspace(int B, int crop_h, int crop_w);
int iswm_augment_batch_ex(const unsigned char* images, const unsigned char* labels, const unsigned char* rot_images,
                          const unsigned char* rot_labels, const void* samples, const void* extras, const int* tables,
                          int B, int crop_h, int crop_w, const float* mean3, const float* std3, int any_contrast,
                          float* out_nchw, unsigned char* out_labels, void* workspace, size_t workspace_bytes,
                          iswm_stream_t stream);

/* ---- GPU-resident tile store (dataset.hip) ------------------------------------------
 * A data set is decoded once into two uint8 device arenas (images HWC RGB, masks HW); every tile starts at a
 * multiple of 16 bytes.  No atomics: per-workgroup partial counts go to the workspace and are summed by one
 * workgroup in index order.  All pointers are device pointers unless stated; the entry points only enqueue.
 * label_prepare: in place, every non-zero byte of the nbytes-long label arena (nbytes % 16 == 0, 16-byte aligned)
 * becomes 1; counts[2] (int64) = {n(0), n(1)} of the result (alignment padding, being 0, is counted in n(0)).
 * label_count: ADDS {n(label == 0), n(label == 1), n(other)} of n uint8 labels (16-byte aligned) to the int64
 * accumulator counts_accum[3]; a label equal to ignore_index (-1: none) is counted as other.
 * aug_tables: fills, for each of the B iswm_aug_sample records, the table block iswm_augment_batch reads at
 * tab_off from src_h, src_w, rs_h, rs_w, ksize_h, ksize_v alone -- Pillow's bounds, 22-bit integer weights and
 * nearest indices, the same int32 values the host computes (fp64, uncontracted, same operation order).  max_rs >=
 * every rs_h and rs_w (sizes the grid).  A record whose block would end past tables_bytes is left unwritten.
 * iswm_aug_tables_workspace(HOST copy of the records, B) = bytes the table buffer needs (0: a bad record).
 * gather_normalize: B tiles of H x W at offsets[B][2] = (image byte offset, label byte offset), multiples of 16,
 * -> fp32 NCHW [B][3][H][W] with iswm_predict_normalize's arithmetic and the uint8 labels [B][H][W], one launch.
 * mean3 / std3 are HOST arrays of 3 floats. */
size_t iswm_label_prepare_workspace(long long nbytes);
int iswm_label_prepare(unsigned char* labels, long long nbytes, long long* counts, void* workspace,
                       size_t workspace_bytes, iswm_stream_t stream);
size_t iswm_label_count_workspace(long long n);
int iswm_label_count(const unsigned char* labels, long long n, int ignore_index, long long* counts_accum,
                     void* workspace, size_t workspace_bytes, iswm_stream_t stream);
size_t iswm_aug_tables_workspace(const void* host_samples, int B);
int iswm_aug_tables(const void* samples, int B, int max_rs, int* tables, size_t tables_bytes, iswm_stream_t stream);
int iswm_gather_normalize(const unsigned char* images, const unsigned char* labels, const long long* offsets, int B,
                          int H, int W, const float* mean3, const float* std3, float* out_nchw,
                          unsigned char* out_labels, iswm_stream_t stream);

/* ---- inference outputs (predict.hip) ------------------------------------------------
 * predict_normalize: uint8 [N][H][W][3] RGB -> fp32 NCHW [N][3][H][W], (v / 255.0f - mean) / std in IEEE fp32
 * (ToTensor + Normalize, predict.py:93-97).
 * predict_maps: low-resolution NHWC logits yl [N][Hi][Wi][ldx] (first C channels; ldx % 4 == 0, ldx >= pad4(C))
 * -> per output pixel of [N][Ho][Wo]: bilinear sample (k_bilinear_to_nchw_fwd's arithmetic), p = softmax(l)[fg],
 * pred = p > thr ? 255 : 0 (fp32 compare), conf = (uint8)(p * 255.0f), band = band_lo <= conf <= band_hi ? 255 : 0,
 * prob = p (optional, NULL: not written); stats [N][5] = {min p, max p, sum p, count(p < thr), count(pred)} (fp64,
 * fixed-order sums, bit-reproducible).  Output pointers 16-byte aligned; workspace: iswm_predict_maps_workspace. */
int iswm_predict_normalize(const unsigned char* img, int N, int H, int W, const float* mean3, const float* std3,
                           float* out_nchw, iswm_stream_t stream);
size_t iswm_predict_maps_workspace(int N, int H, int W);
int iswm_predict_maps(const float* yl, int N, int Hi, int Wi, int ldx, int C, int fg, int Ho, int Wo, float thr,
                      int band_lo, int band_hi, unsigned char* pred, unsigned char* conf, unsigned char* band,
                      float* prob, double* stats, void* workspace, size_t workspace_bytes, iswm_stream_t stream);

/* ---- sliding-window prediction of whole scenes (predict.hip) -------------------------------
 * A scene of H x W is predicted in nty x ntx windows of th x tw and the overlaps are blended.
 * scene_plan_make (pure host): per axis of length L, t = min(tile, L); one window when L <= t, else windows every
 * s = t - overlap, n = ceil((L - t) / s) + 1 of them, window k starting at min(k * s, L - t).  Needs tile >= 1,
 * 0 <= overlap <= 1024 and overlap <= t / 2 on an axis with more than one window.  ramp = max(overlap, 1); an axis
 * with one window has s = t.  Windows are numbered k = ty * ntx + tx.
 * scene_tiles_normalize: uint8 HWC RGB scene [H][W][3] -> windows first_tile .. first_tile + count - 1 as fp32 NCHW
 * [count][3][th][tw], iswm_predict_normalize's arithmetic.  mean3 / std3 are HOST arrays of 3 floats.
 * scene_maps: the low-resolution NHWC logits of ALL windows yl [nty * ntx][Hi][Wi][ldx] -> the maps of
 * iswm_predict_maps for the one [H][W] scene.  Per pixel, over the windows that cover it (ascending ty, then tx):
 * p_t = iswm_predict_maps's probability at the in-window coordinate, w_t = w1d(y - oy, th) * w1d(x - ox, tw) with
 * w1d(i, len) = min(i + 1, len - i, ramp), p = min(sum_t fma(w_t / sum w, p_t), 1).  A gather: no canvas, no
 * atomics, bit-reproducible; a pixel under one window gets that window's p_t exactly, and a plan of one window is
 run as iswm_predict_maps (the same bytes for every C).  Outputs, stats [5] and
 * alignment as iswm_predict_maps with N = 1; workspace: iswm_scene_maps_workspace. */
typedef struct iswm_scene_plan {
    int H, W, th, tw, sy, sx, nty, ntx, ramp;
} iswm_scene_plan;
int iswm_scene_plan_make(int H, int W, int tile, int overlap, iswm_scene_plan* out);
int iswm_scene_tiles_normalize(const unsigned char* scene, const iswm_scene_plan* plan, int first_tile, int count,
                               const float* mean3, const float* std3, float* out_nchw, iswm_stream_t stream);
size_t iswm_scene_maps_workspace(int H, int W);
int iswm_scene_maps(const float* yl, const iswm_scene_plan* plan, int Hi, int Wi, int ldx, int C, int fg, float thr,
                    int band_lo, int band_hi, unsigned char* pred, unsigned char* conf, unsigned char* band,
                    float* prob, double* stats, void* workspace, size_t workspace_bytes, iswm_stream_t stream);

/* ---- flip and multi-scale test-time augmentation (predict.hip) ------------------------------
 * The foreground probability of a frame is averaged over views of it: the frame resampled to Hv x Wv (bilinear,
 * align_corners=False) and, for a flipped view, mirrored left to right.  At most ISWM_PREDICT_MAX_VIEWS views.
 * predict_view_normalize: uint8 [N][H][W][3] RGB -> one view as fp32 NCHW [N][3][Hv][Wv].  Per output (y, x):
 * xs = flip ? Wv - 1 - x : x; the four uint8 taps and weights of source coordinates (y, xs) with scales
 * (float)H / (float)Hv and (float)W / (float)Wv (the index arithmetic of iswm_bilinear_fwd), their bilinear value in
 * fp32, then iswm_predict_normalize's (v / 255.0f - mean) / std.  Hv = H, Wv = W, flip = 0 gives
 * iswm_predict_normalize's bits; flip = 1 those of the mirrored frame.  mean3 / std3 are HOST arrays of 3 floats.
 * predict_views_maps: the low-resolution NHWC logits of every view, views[v].yl [N][Hi][Wi][ldx] (N, ldx, C, fg common
 * to all views), -> the maps of iswm_predict_maps at [N][Ho][Wo].  Per output pixel, views in list order:
 * p_v = iswm_predict_maps's probability of view v at row oh and column (flip ? Wo - 1 - ow : ow), sampled straight from
 * the view's logits with scales (float)Hi / (float)Ho and (float)Wi / (float)Wo; p = (sum_v p_v) / nviews in fp32.  A
 * gather: no canvas, no atomics, every output byte written once, bit-reproducible.  A list of one unflipped view is run
 * as iswm_predict_maps (the same bytes for every C).  Outputs, stats [N][5] and alignment as iswm_predict_maps;
 * workspace: iswm_predict_views_maps_workspace (= iswm_predict_maps_workspace). */
#define ISWM_PREDICT_MAX_VIEWS 16
typedef struct iswm_predict_view {
    const float* yl;    /* the view's low-resolution logits [N][Hi][Wi][ldx], 16-byte aligned */
    int Hi, Wi, flip;
} iswm_predict_view;
int iswm_predict_view_normalize(const unsigned char* img, int N, int H, int W, int Hv, int Wv, int flip,
                                const float* mean3, const float* std3, float* out_nchw, iswm_stream_t stream);
size_t iswm_predict_views_maps_workspace(int N, int H, int W);
int iswm_predict_views_maps(const iswm_predict_view* views, int nviews, int N, int ldx, int C, int fg, int Ho, int Wo,
                            float thr, int band_lo, int band_hi, unsigned char* pred, unsigned char* conf,
                            unsigned char* band, float* prob, double* stats, void* workspace, size_t workspace_bytes,
                            iswm_stream_t stream);

/* ---- validation image panels (val_panels.hip) ----------------------------------------------
 * What save_validation_results (train.py:461-523) draws for a frame, in one launch.  Inputs: x, the normalised fp32
 * NCHW batch [N][3][H][W]; yl, the classifier's low-resolution NHWC logits [N][Hi][Wi][ldx] (first C channels,
 * 1 <= C <= 256; ldx % 4 == 0, ldx >= pad4(C)); labels [N][H][W] as class indices 0 .. 255 with 255 = ignore
 * (label_dtype 0 = uint8, 1 = int64, the low byte is taken); palette, 256 x 3 uint8 RGB on the DEVICE;
 * denorm_mean3 / denorm_std3, HOST arrays of 3 floats holding M = float32(-mean / std) and S = float32(1 / std).
 * Outputs, all uint8 on the device, any of them NULL = skipped (an input only skipped outputs need may be NULL too):
 *   original   [N][H][W][3]  t = ((x - M) / S) * 255.0f in IEEE fp32 (round to nearest, nothing fused), truncated
 *                            toward zero: Denormalize -> * 255 -> astype(uint8) (utils/utils.py:14-24, train.py:491-492).
 *                            t < 0 or NaN gives 0 and t > 255 gives 255 -- numpy's wrap-around is not reproduced; no
 *                            uint8 image reaches either.
 *   pred       [N][H][W]     the first maximal class of the bilinearly up-sampled logits: iswm_argmax_nchw's strict
 *                            compare over k_bilinear_to_nchw_fwd's samples, bit for bit the mask the metrics score.
 *   conf       [N][H][W]     (uint8)(p * 255.0f), p = max_c softmax(l)_c = 1 / sum_c expf(l_c - m), m = max_c l_c,
 *                            summed in class order, fp32 division (train.py:494-495, 515); prob (fp32, optional) = p.
 *   target_rgb, pred_rgb [N][H][W][3]  palette[label], palette[pred] (decode_target, train.py:611-618).
 *   overlay    [N][H][W][3]  (3 * original + 7 * pred_rgb + 5) / 10 per channel in integers: the 0.7-alpha composite.
 *   error      [N][H][W][3]  label 255: grey (128,128,128); pred == label: black for label 0, white otherwise;
 *                            label 0, pred != 0: red; label != 0, pred 0: blue; two different foreground classes:
 *                            magenta.
 * x, yl and every output pointer 16-byte aligned.  No workspace, no allocation, no synchronisation; two calls give
 * the same bytes. */
int iswm_val_panels(const float* x, const float* yl, const void* labels, int label_dtype, int N, int Hi, int Wi,
                    int ldx, int C, int H, int W, const float* denorm_mean3, const float* denorm_std3,
                    const unsigned char* palette, unsigned char* original, unsigned char* pred, unsigned char* conf,
                    float* prob, unsigned char* target_rgb, unsigned char* pred_rgb, unsigned char* overlay,
                    unsigned char* error, iswm_stream_t stream);

/* ---- INT8 post-training quantized inference (qconv.hip, quant.hip)----------------------
 * Activations are int8 NHWC with a pixel pitch in bytes; one symmetric scale s per tensor (value = q * s).
 * qconv: implicit-GEMM convolution on v_mfma_i32_16x16x64_i8, forward only.  x int8 [N][H][W][ldx] (first Cin
 * channels, Cin % 64 == 0, ldx % 16 == 0, 16-byte aligned), w int8 OHWI [Cout][KH][KW][Cin] (Cout % 16 == 0; rows past
 * the real output channels are zero; iswm_qconv_weight_bytes), mul / add fp64 [Cout].  Per output element, in fp64
 * without contraction: v = acc * mul[c] + add[c]; with res: v += res * s_res; with relu: v = max(v, 0); then int8
 * q = clamp(rint(v * inv_s_out), lo, 127) or, out_f32, (float)v.  Channels c < cstore of y (pitch ldy) are written,
 * nothing else.  res int8 [pixel][ldr] (int8 output only). */
typedef struct {
    int N, H, W, Cin;   /* input  [N,H,W,Cin] */
    int Ho, Wo, Cout;   /* output [N,Ho,Wo,Cout] (Cout padded to 16) */
    int KH, KW, stride, pad, dil;
    int ldx;            /* pixel pitch of x (bytes) */
    int ldy;            /* pixel pitch of y (bytes for int8, floats for fp32) */
    int ldr;            /* pixel pitch of res (bytes) */
    int relu;           /* 1: max(v, 0) before quantizing */
    int lo;             /* int8 floor: 0 (ReLU output) or -127 */
    int out_f32;        /* 1: fp32 output */
    int cstore;         /* output channels written, <= Cout */
} iswm_qconv_desc;
size_t iswm_qconv_weight_bytes(const iswm_qconv_desc* d);
int iswm_qconv_fwd(const iswm_qconv_desc* d, const signed char* x, const signed char* w, const double* mul,
                   const double* add, const signed char* res, double s_res, double inv_s_out, void* y,
                   iswm_stream_t stream);
/* absmax: amax[0] = max(amax[0], max |x|) over rows x the first C channels of an fp32 (ps == 0) or planes (ps != 0,
 * the iswm_*_pl convention) tensor of pitch ld; a per-workgroup slab (iswm_absmax_workspace bytes) then one finalize
 * workgroup; no atomics, no sync. */
size_t iswm_absmax_workspace(int64_t rows, int C);
int iswm_absmax(const void* x, int64_t ps, int64_t rows, int C, int ld, float* slab, size_t slab_bytes, float* amax,
                iswm_stream_t stream);
/* quantize_i8: y[r][c] = clamp(rint(x * inv_s), lo, 127) for c < C, 0 for C <= c < ldy (fp64 product) */
int iswm_quantize_i8(const void* x, int64_t ps, int64_t rows, int C, int ld, double inv_s, int lo, signed char* y,
                     int ldy, iswm_stream_t stream);
/* qgap: y[n][c] = clamp(rint((sum_p x[n][p][c] * s_in / HW) * inv_s_in)), the int32 sum exact */
int iswm_qgap(const signed char* x, int N, int HW, int C, int ldx, double s_in, double inv_s_in, signed char* y,
              int ldy, iswm_stream_t stream);
/* qbcast: y[n][p][c] = v[n][c] (C % 4 == 0) */
int iswm_qbcast(const signed char* v, int N, int HW, int C, int ldv, signed char* y, int ldy, iswm_stream_t stream);
/* qbilinear: align_corners=False resize (bilinear.h's indices and fp32 weights); the four taps dequantized with s_in
 * and combined in fp64 as h0 (w0 a + w1 b) + h1 (w0 d + w1 e), quantized with inv_s_out (C % 4 == 0) */
int iswm_qbilinear(const signed char* x, int N, int Hi, int Wi, int C, int ldx, double s_in, int Ho, int Wo,
                   double inv_s_out, signed char* y, int ldy, iswm_stream_t stream);

/* ---- optimizers over a flat fp32 arena ------------------------------------------
 * torch.optim.SGD(momentum=0.9, nesterov=True, weight_decay) / Adam / AdamW as built
 * by setup_optimizer, train.py:421-444.  lr is read from device memory so that a
 * captured graph can be replayed with a new learning rate. */
int iswm_sgd_step(float* p, const float* g, float* buf, int64_t n, const float* lr_dev, float momentum,
                  float weight_decay, int nesterov, iswm_stream_t stream);
/* hyper_dev[4] = {lr, bias_correction1, bias_correction2, unused} */
int iswm_adam_step(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                   float beta1, float beta2, float eps, float weight_decay, int decoupled,
                   iswm_stream_t stream);

/* ---- gradient-norm clipping and EMA weights inside the step ------------------------
 * grad_sqnorm: sum of g[i]^2 over one range, left as one double per workgroup in `slots`
 * (iswm_grad_sqnorm_slots() doubles).  accumulate == 0 starts a total (every slot is written),
 * != 0 adds this range to the total the earlier calls on the same stream left there.  No atomics;
 * the launch geometry depends on n alone, so the same input gives the same bits.  g 16-byte
 * aligned, any n > 0 (float4 loads and a scalar tail); double accumulation throughout. */
int iswm_grad_sqnorm_slots(void);
int iswm_grad_sqnorm(const float* g, int64_t n, double* slots, int accumulate, iswm_stream_t stream);
/* clip_finalize: one workgroup adds the slots in a fixed order (double) and writes
 * clip_dev[0] = coef = min(1, max_norm / (norm + 1e-6)) (torch.nn.utils.clip_grad_norm_; a NaN norm
 * gives a NaN coef), clip_dev[1] = norm = (float)sqrt(sum), and sum as ONE double over clip_dev[2..3]
 * (clip_dev: 4 floats, 8-byte aligned).  max_norm > 0.  The host reads nothing back. */
int iswm_clip_finalize(const double* slots, float max_norm, float* clip_dev, iswm_stream_t stream);
/* The steps above with two optional operands.  clip_dev (or NULL): the step uses g * clip_dev[0], one
 * fp32 multiply as g is loaded; the gradient arena is NOT modified.  ema (or NULL; the arena's layout):
 * after the parameter update ema += hyper_dev[3] * (p_new - ema), hyper_dev[3] = 1 - decay_t.
 * hyper_dev is the 4-float block {lr, bias_correction1, bias_correction2, 1 - decay_t} (SGD reads
 * slots 0 and 3).  Otherwise the arithmetic is that of iswm_sgd_step / iswm_adam_step operation for
 * operation: with coef == 1.0f and ema == NULL the results are bit-identical to theirs. */
int iswm_sgd_step_ex(float* p, const float* g, float* buf, int64_t n, const float* hyper_dev, float momentum,
                     float weight_decay, int nesterov, const float* clip_dev, float* ema, iswm_stream_t stream);
int iswm_adam_step_ex(float* p, const float* g, float* m, float* v, int64_t n, const float* hyper_dev,
                      float beta1, float beta2, float eps, float weight_decay, int decoupled,
                      const float* clip_dev, float* ema, iswm_stream_t stream);
/* swap_f32: a[i] <-> b[i] for i < n, in place; both 16-byte aligned, the ranges disjoint */
int iswm_swap_f32(float* a, float* b, int64_t n, iswm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ISWM_HIP_H */
