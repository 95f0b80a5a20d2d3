/* Optimiser-side gradient kernels of librdm_hip.so: gradient accumulation over micro-batches, the squared global norm of a flat gradient, and
 * the fused AdamW step with torch.nn.utils.clip_grad_norm_'s coefficient folded into its gradient scale (Lightning's accumulate_grad_batches
 * and gradient_clip_val; the reference's Trainer sets neither, train.py:49-60).  A header of its own beside rdm_hip.h; the entry points live in
 * the same library and follow the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation).
 * Every refusal below is RDM_ERR_BAD_ARGUMENT with a message, returned before anything is launched. */
#ifndef RDM_OPTIM_H_
#define RDM_OPTIM_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RDM_GRAD_ACC_COPY 0
#define RDM_GRAD_ACC_ADD 1
#define RDM_CLIP_MAX_SLOTS 8

/* mode RDM_GRAD_ACC_COPY: dst[i] = src[i];  RDM_GRAD_ACC_ADD: dst[i] = dst[i] + src[i] (one float32 addition), i < n.  128-bit loads and
 * stores with a scalar tail; nothing beyond n is touched; n = 0 launches nothing.
 * Refused: dst or src NULL or not 16-byte aligned, n < 0, any other mode. */
int rdm_grad_accumulate_f32(float* dst, const float* src, int64_t n, int32_t mode, rdm_stream_t stream);

/* Bytes of workspace rdm_grad_sumsq_f64 needs for n elements: one float64 partial per workgroup.  Positive for n >= 0 (n = 0 included),
 * non-decreasing in n, 0 for n < 0. */
size_t rdm_grad_sumsq_workspace_bytes(int64_t n);

/* *out_slot = sum of grad[i]^2 over i < n, formed in float64 (the square of a float32 is exact there).  Fixed order: a thread adds its
 * elements by rising index, lanes combine by shuffle, wavefronts in sequence, each workgroup stores its partial to ws, and a second launch
 * of one workgroup adds the partials by rising workgroup index.  No atomics: a repeated call gives the same bytes.  n = 0 writes 0.0; a NaN
 * or an infinity in grad gives NaN or infinity.  ws may be shared by successive calls on one stream.
 * Refused: grad, out_slot or ws NULL, grad not 16-byte aligned, out_slot or ws not 8-byte aligned, n < 0, ws_bytes below
 * rdm_grad_sumsq_workspace_bytes(n). */
int rdm_grad_sumsq_f64(const float* grad, int64_t n, double* out_slot, void* ws, size_t ws_bytes, rdm_stream_t stream);

/* rdm_adamw_fused with the gradient clipped by global norm, in the same single launch.  Every thread forms, in float64 and without
 * contraction,
 *     total = sumsq[0] + sumsq[1] + ... + sumsq[n_slots - 1]                      (left to right)
 *     q     = (double)max_norm / (sqrt(total) * fabs((double)grad_scale) + 1e-6)
 *     c     = q > 1.0 ? 1.0 : q                                                   (a NaN q stays NaN, as under torch.clamp(max=1))
 * which is clip_grad_norm_'s coefficient for the SCALED gradient grad_scale * grad, rounds c to float32 and runs the update of rdm_adamw_fused
 * with  grad_scale * (float)c  (one float32 product) in place of grad_scale: bit for bit what rdm_adamw_fused gives when called with that
 * product.  sumsq: DEVICE pointer to n_slots float64 partial sums of squares of the UNSCALED gradient (rdm_grad_sumsq_f64 slots; the ranges
 * of one step share the slots, so all of them are clipped by the one global norm).  coef_out: DEVICE pointer that receives (float)c, or NULL.
 * Refused: what rdm_adamw_fused refuses; sumsq NULL or not 8-byte aligned, n_slots outside 1..RDM_CLIP_MAX_SLOTS, max_norm negative or NaN,
 * coef_out not 4-byte aligned. */
int rdm_adamw_fused_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, int32_t step, float grad_scale, const double* sumsq, int32_t n_slots, float max_norm,
                         float* coef_out, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_OPTIM_H_ */
