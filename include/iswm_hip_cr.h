/*
 * iswm_hip_cr.h -- fifth extension header of libiswm_hip.so: the local dense-CRF refinement of a predicted foreground probability on
 * the frame it was predicted from (mean field over a dilated window, ConvCRF), and the maps of an fp32 probability, added after the
 * ABI of iswm_hip.h, iswm_hip_sep.h, iswm_hip_kd.h, iswm_hip_bd.h and iswm_hip_bm.h was frozen.  Plain C, the conventions of
 * iswm_hip.h (included below); the host binds these prototypes with the same parser, into a table of their own (iswm_amd/_lib.py,
 * CR_EXPORTS).  It declares prototypes only: no record and no constant.
 *
 * ---- the refinement (csrc/crf.hip), binary: foreground against the rest
 *   prob fp32 [N,H,W], the foreground probability; img uint8 [N,H,W,3], the frame in RGB; out fp32 [N,H,W].
 *   radius R in 1..7, step D in 1..4, iters T in 1..20, w_bilateral (w_b) and w_spatial (w_s) >= 0, theta_alpha, theta_beta,
 *   theta_gamma > 0; 1 <= H, W <= 8192, 1 <= N <= 65535.  Per image, with pixel i = (y, x):
 *     pc = clamp(prob, 1e-6, 1 - 1e-6)      u_i = log pc_i - log(1 - pc_i)      q^0 = pc
 *     neighbours j = (y + dy D, x + dx D) for (dy, dx) in [-R, R]^2 \ {(0, 0)} that lie inside the image; nothing is padded or mirrored
 *     d2 = (dy^2 + dx^2) D^2        dI2 = sum over the 3 channels of (I_i,c - I_j,c)^2, an exact integer <= 195 075
 *     kb_ij = exp(-d2 / (2 theta_alpha^2) - dI2 / (2 theta_beta^2))        ks_ij = exp(-d2 / (2 theta_gamma^2))
 *     Nb_i = sum_j kb_ij        Ns_i = sum_j ks_ij                          (they do not depend on the iteration)
 *     with s_j = 2 q_j^t - 1:   m_b = (sum_j kb_ij s_j) / Nb_i        m_s = (sum_j ks_ij s_j) / Ns_i
 *                               a term whose norm is below 1e-20 is 0 (a pixel with no neighbour, or none of similar colour)
 *     z_i = u_i + w_b m_b + w_s m_s        q_i^(t+1) = 1 / (1 + exp(-z_i))        out = q^T
 *   The mean-field update of a two-label Potts model with normalised messages: each message is a weighted mean of values in
 *   [-1, 1], so |z_i - u_i| <= w_b + w_s.  The sums run row-major over the window, in fp32, with no atomics: two calls give the
 *   same bits.  out may not alias prob.
 *
 *   iswm_crf_refine_workspace : bytes of workspace for the call (8 per pixel); -1 for a shape the call refuses
 *   iswm_crf_refine           : one launch per iteration on the caller's stream; nothing is read back
 *
 * ---- the maps of a probability
 *   iswm_prob_maps_workspace  : bytes of workspace for the call; -1 for a shape the call refuses
 *   iswm_prob_maps            : prob fp32 [N,H,W] -> pred, conf, band (uint8 [N,H,W]) and stats (double [N][5]) by the rules and in
 *                               the layout of iswm_predict_maps (iswm_hip.h): pred = p > thr ? 255 : 0 in fp32, conf =
 *                               (uint8)(p * 255.0f), band = band_lo <= conf <= band_hi ? 255 : 0, stats = min p, max p, sum p,
 *                               count(p < thr), count(pred), summed in that call's fixed order.  Fed the prob that
 *                               iswm_predict_maps wrote, it writes that call's bytes.  prob, pred, conf and band 16-byte aligned.
 *
 * Both calls only enqueue work.  Bad parameters, NULL pointers and a short workspace return non-zero with iswm_last_error set, and
 * nothing is launched.
 */
#ifndef ISWM_HIP_CR_H
#define ISWM_HIP_CR_H

#include "iswm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t iswm_crf_refine_workspace(int N, int H, int W);                      /* -1: a shape the call refuses */
int iswm_crf_refine(const float* prob, const unsigned char* img, int N, int H, int W, int radius, int step, int iters,
                    float w_bilateral, float w_spatial, float theta_alpha, float theta_beta, float theta_gamma,
                    float* out, void* workspace, int64_t workspace_bytes, iswm_stream_t stream);
int64_t iswm_prob_maps_workspace(int N, int H, int W);
int iswm_prob_maps(const float* prob, int N, int H, int W, float thr, int band_lo, int band_hi, unsigned char* pred,
                   unsigned char* conf, unsigned char* band, double* stats, void* workspace, int64_t workspace_bytes,
                   iswm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISWM_HIP_CR_H */
