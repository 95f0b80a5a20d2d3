/* Weight averaging kernels of librdm_hip.so: the fused AdamW step that also advances an exponential moving average (EMA) of the weights it
 * writes, and the in-place exchange of two float32 buffers that puts the averaged weights in the live weights' place and back.  A header of
 * its own beside rdm_optim.h; the entry points live in the same library and follow the same conventions (status codes, rdm_last_error_string,
 * caller's stream, no allocation, no synchronisation).  Every refusal below is RDM_ERR_BAD_ARGUMENT with a message, returned before anything
 * is launched. */
#ifndef RDM_EMA_H_
#define RDM_EMA_H_
#include "rdm_optim.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The AdamW update of rdm_adamw_fused (sumsq == NULL and n_slots == 0) or of rdm_adamw_fused_clip (otherwise, with the same coefficient) and,
 * in the same single launch, for i < n
 *     ema[i] = ema[i] + (1.f - ema_decay) * (param_new[i] - ema[i])          (float32; 1.f - ema_decay rounded once, on the host)
 * where param_new[i] is the float32 value the launch stores to param[i].  param, exp_avg and exp_avg_sq receive the bytes the plain or the
 * clipped step gives on the same inputs.  128-bit accesses with a scalar tail for all five buffers; nothing at or beyond n is touched;
 * n = 0 launches nothing (coef_out is then not written).  ema_decay == 1.f stores every ema[i] back as it was read.
 * Refused: what rdm_adamw_fused / rdm_adamw_fused_clip refuses; ema NULL or not 16-byte aligned; [ema, ema + n) overlapping
 * [param, param + n); ema_decay outside [0, 1] or NaN; sumsq == NULL with n_slots != 0, and sumsq != NULL with n_slots == 0. */
int rdm_adamw_fused_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr, float beta1,
                        float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const double* sumsq, int32_t n_slots,
                        float max_norm, float* coef_out, float ema_decay, rdm_stream_t stream);

/* a[i] <-> b[i] for i < n in one pass: 128-bit loads and stores with a scalar tail, every element read and written by one thread.  Applied
 * twice it restores both buffers bit for bit.  Nothing at or beyond n is touched; n = 0 launches nothing.
 * Refused: a or b NULL or not 16-byte aligned, n < 0, [a, a + n) overlapping [b, b + n). */
int rdm_ema_swap_f32(float* a, float* b, int64_t n, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_EMA_H_ */
