/*
 * iswm_hip_bm.h -- fourth extension header of libiswm_hip.so: the boundary validation metrics (boundary F1 at a pixel tolerance,
 * average symmetric surface distance, percentile Hausdorff distance) from exact distances between the contour of a predicted mask
 * and the contour of its label mask, added after the ABI of iswm_hip.h, iswm_hip_sep.h, iswm_hip_kd.h and iswm_hip_bd.h was
 * frozen.  Plain C, the conventions of iswm_hip.h (included below); the host binds these prototypes with the same parser, into a
 * table of their own (iswm_amd/_lib.py, BM_EXPORTS).  It declares prototypes only: no record and no constant.
 *
 * ---- inputs and sets (csrc/boundary_metrics.hip)
 *   pred [B,H,W] and labels [B,H,W], each uint8 or int64 independently (pred_bytes, label_bytes: 1 or 8); C classes;
 *   K = {first_class .. C-1} (first_class 1: the foreground classes, 0: every class); 1 <= H, W <= 4096.
 *   A pixel is valid when its LABEL is: y != ignore_index and 0 <= y < C.  The prediction's value plays no part in validity; a
 *   predicted value outside [0, C) belongs to no class's mask but is still a valid "other" pixel.
 *   Per image n and class c of K:
 *     G = {p valid : y_p == c}                P = {p valid : pred_p == c}
 *     S(A) = {p in A : some 4-neighbour q inside the image is valid and q not in A}        the inner contour of A
 *   This is the contour rule of iswm_hip_bd.h: S(A) is exactly the set where the signed map sd2 of mask A equals -1.  Invalid
 *   pixels and the image edge make no contour; a mask that covers every valid pixel has none.  Distances run in the plain pixel
 *   grid, pass through invalid pixels, and never cross an image or a class plane.
 *
 * ---- per-direction statistics, direction 0 = S(P) -> S(G), direction 1 = S(G) -> S(P)
 *   For X -> Y with d2(p) = min over q in Y of |p - q|^2, an exact integer (<= 2 * 4095^2 < 2^25):
 *     n      = |X|                                                                              as counted when Y is empty
 *     within = #{p in X : d2(p) <= tolerance^2}                                                 0 when Y is empty
 *     max2   = max d2                                                                           -1 when Y is empty
 *     q2     = the d2 of rank r = (percent * n + 99) / 100 (integer division, 1-based, ascending: nearest rank, no
 *              interpolation)                                                                   -1 when Y is empty
 *     dsum   = sum over X of sqrt((double)d2(p)), added in a fixed order                        0 when Y is empty
 *   When X is empty, max2 and q2 are -1 and within and dsum are 0.
 *
 *   iswm_boundary_metrics_workspace : bytes of workspace for the call (4 per pixel and class plane); -1 for a shape the call refuses
 *   iswm_boundary_metrics           : stats (int64 [B, C - first_class, 2, 4] = n, within, max2, q2) and dsum (double
 *                                     [B, C - first_class, 2]), both on the device, on the caller's stream; nothing is read back
 */
#ifndef ISWM_HIP_BM_H
#define ISWM_HIP_BM_H

#include "iswm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t iswm_boundary_metrics_workspace(int B, int C, int H, int W, int first_class);
int iswm_boundary_metrics(const void* pred, int pred_bytes, const void* labels, int label_bytes, int B, int C, int H, int W,
                          int first_class, int ignore_index, int tolerance, int percent, int64_t* stats, double* dsum,
                          void* workspace, int64_t workspace_bytes, iswm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISWM_HIP_BM_H */
