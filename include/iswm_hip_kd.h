/*
 * iswm_hip_kd.h -- second extension header of libiswm_hip.so: the teacher-student distillation criterion, added after the
 * ABI of iswm_hip.h and of iswm_hip_sep.h was frozen.  Plain C, the conventions of iswm_hip.h (included below); the host
 * binds these prototypes with the same parser, into a table of their own (iswm_amd/_lib.py, KD_EXPORTS).  It declares
 * prototypes only: no record and no constant.
 *
 * ---- distillation next to the weighted CE (csrc/distill.hip): two passes, nothing stored per pixel
 *   s = student logits [B,C,H,W] fp32, t = teacher logits of the same shape, y = labels (uint8 or int64: label_bytes 1 or 8),
 *   V = the pixels with y != ignore_index and 0 <= y < C, tau > 0 the temperature, w = class_weight (NULL: ones), C <= 8.
 *     p = softmax(s)     ptau = softmax(s / tau)     q = softmax(t / tau)     g_ic = [y_i == c]
 *     KL_i = sum_c q_ic (log q_ic - log ptau_ic)
 *     N = |V|     A = #{ i in V : argmax_c s_ic == argmax_c t_ic }   (lowest class index among equal maxima)
 *     L = lce * sum_V w_y nll / sum_V w_y  +  lkd * tau^2 * sum_V KL_i / N
 *     dL/ds_ik = lce * w_y (p_ik - g_ik) / sum_V w  +  lkd * tau * (ptau_ik - q_ik) / N     on V, exactly 0 elsewhere
 *   lce == 0 leaves the CE term out altogether (the loss is then finite without a valid pixel); N == 0 makes the distillation
 *   term and its gradient exactly 0.  The gradient's factor is tau, not tau^2: the 1 / tau of the chain rule is taken.
 *   The scaled logits are z * inv_tau with inv_tau = (float)(1 / tau) from the host, for both tensors alike: a teacher equal to
 *   the student bit for bit gives sum KL == 0.0 and a distillation gradient of exactly 0.
 *   iswm_distill_loss_partials : the length in floats of the partials workspace for npix = B * HW pixels
 *   iswm_distill_loss_fwd      : sums[5] (double, device) = {sum w nll, sum w, sum KL, N, A}; sums[0..1] are iswm_loss_fwd's
 *                                mode-0 sums bit for bit, N and A are exact integers (B * HW <= 2^36).  Under data
 *                                parallelism the host all-reduces sums before the next call.
 *   iswm_distill_loss_coeffs   : sums -> out[3] = {L, CE term, KD term} (fp32) and coef[2] = {lce / sum w, lkd * tau / N},
 *                                formed in double on the device
 *   iswm_distill_loss_bwd      : grad = upstream[0] * dL/ds, written once (upstream: a device scalar)
 */
#ifndef ISWM_HIP_KD_H
#define ISWM_HIP_KD_H

#include "iswm_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

int64_t iswm_distill_loss_partials(int64_t npix);
int iswm_distill_loss_fwd(const float* student, const float* teacher, const void* labels, int label_bytes, int B, int C,
                          int64_t HW, const float* class_weight, int ignore_index, float inv_tau, float* partials,
                          double* sums, iswm_stream_t stream);
int iswm_distill_loss_coeffs(const double* sums, double ce_weight, double distill_weight, double temperature, float* out,
                             float* coef, iswm_stream_t stream);
int iswm_distill_loss_bwd(const float* student, const float* teacher, const void* labels, int label_bytes, int B, int C,
                          int64_t HW, const float* class_weight, int ignore_index, float inv_tau, const float* coef,
                          const float* upstream, float* grad, iswm_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* ISWM_HIP_KD_H */
