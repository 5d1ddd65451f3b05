/*
 * iswm_hip_bd.h -- third extension header of libiswm_hip.so: the signed Euclidean distance map of a label tensor and the
 * boundary (distance-map) criterion on it, added after the ABI of iswm_hip.h, iswm_hip_sep.h and iswm_hip_kd.h was frozen.
 * Plain C, the conventions of iswm_hip.h (included below); the host binds these prototypes with the same parser, into a
 * table of their own (iswm_amd/_lib.py, BD_EXPORTS).  It declares prototypes only: no record and no constant.
 *
 * ---- signed squared distance map (csrc/boundary.hip): exact, in integers, two launches
 *   y = labels [B,H,W] (uint8 or int64: label_bytes 1 or 8), K = {first_class .. C-1} (first_class 1: the foreground classes,
 *   0: every class), H, W <= 4096.  For image n and class c of K:
 *     F = {p : y_p == c and y_p valid}     G = {p : y_p valid and y_p != c}     valid: y != ignore_index and 0 <= y < C
 *     d2(p, S) = min over q in S of (px-qx)^2 + (py-qy)^2
 *     sd2(p) = +d2(p, F) for p in G,  -d2(p, G) for p in F,  0 at invalid pixels,  0 over the whole plane when F or G is empty
 *   Invalid pixels belong to neither set: the 255 a padded crop is filled with makes no contour.  Distances never cross an
 *   image or a class plane.
 *   iswm_signed_edt_workspace : bytes of workspace for the call (4 per pixel and class plane); -1 for a shape the call refuses
 *   iswm_signed_edt           : sd2 (int32 [B, C - first_class, H, W], device)
 *
 * ---- boundary criterion next to the weighted CE (csrc/boundary.hip): two passes, nothing stored per pixel besides sd2
 *   z = logits [B,C,H,W] fp32, V = the valid pixels, N = |V|, p = softmax(z), g_ic = [y_i == c], w = class_weight (NULL: ones),
 *   C <= 8, sd2 = the map above for the same labels, first_class and ignore_index.
 *     phi = sqrtf(sd2) where sd2 > 0,  -(sqrtf(-sd2) - 1) where sd2 < 0,  0 elsewhere;  then clamped to [-clip, clip] if clip > 0
 *     L = lce * sum_V w_y nll / sum_V w_y  +  lbd * sum_V sum_{c in K} p_ic phi_ic / (N |K|)
 *     dL/dz_ik = lce * w_y (p_ik - g_ik) / sum_V w  +  lbd / (N |K|) * p_ik ([k in K] phi_ik - sum_{c in K} p_ic phi_ic)
 *                on V, exactly 0 elsewhere
 *   lce == 0 leaves the CE term out altogether (the loss is then finite without a valid pixel); N == 0 makes the boundary
 *   term and its gradient exactly 0.
 *   iswm_boundary_loss_partials : the length in floats of the partials workspace for npix = B * HW pixels
 *   iswm_boundary_loss_fwd      : sums[4] (double, device) = {sum w nll, sum w, sum p phi, N}; sums[0..1] are iswm_loss_fwd's
 *                                 mode-0 sums bit for bit, N is an exact integer (B * HW <= 2^36).  Under data parallelism
 *                                 the host all-reduces sums before the next call.
 *   iswm_boundary_loss_coeffs   : sums -> out[3] = {L, CE term, boundary term} (fp32) and coef[2] = {lce / sum w,
 *                                 lbd / (N nsel)}, formed in double on the device; nsel = |K|
 *   iswm_boundary_loss_bwd      : grad = upstream[0] * dL/dz, written once (upstream: a device scalar)
 */
#ifndef ISWM_HIP_BD_H
#define ISWM_HIP_BD_H

#include "iswm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t iswm_signed_edt_workspace(int B, int C, int H, int W, int first_class);
int iswm_signed_edt(const void* labels, int label_bytes, int B, int C, int H, int W, int first_class, int ignore_index,
                    int32_t* sd2, void* workspace, int64_t workspace_bytes, iswm_stream_t stream);
int64_t iswm_boundary_loss_partials(int64_t npix);
int iswm_boundary_loss_fwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW, int first_class,
                           const int32_t* sd2, const float* class_weight, int ignore_index, float clip, float* partials,
                           double* sums, iswm_stream_t stream);
int iswm_boundary_loss_coeffs(const double* sums, int nsel, double ce_weight, double boundary_weight, float* out, float* coef,
                              iswm_stream_t stream);
int iswm_boundary_loss_bwd(const float* logits, const void* labels, int label_bytes, int B, int C, int64_t HW, int first_class,
                           const int32_t* sd2, const float* class_weight, int ignore_index, float clip, const float* coef,
                           const float* upstream, float* grad, iswm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISWM_HIP_BD_H */
