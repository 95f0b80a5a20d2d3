/* Metric depth frames of librdm_hip.so: the (batch,128,128) float64 map of log relative depth to depth in metres, in the geometry of the frame
 * that went in, as float32 and / or as the 16-bit plane of a depth PNG, in ONE launch.  The scale comes from the d_1 DORN head's label
 * counts: the head is trained against depth2label_sid of the metric target (module.py:135-143), and the reference's get_depth_sid
 * (utils.py:120-156) turns a label back into metres.  A header of its own beside rdm_hip.h; the entry point lives in the same library and
 * follows the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation). */
#ifndef RDM_DEPTH_H_
#define RDM_DEPTH_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* depth_f32 / depth_u16 (batch,h,w): either may be NULL, not both.
 *   log_map   (batch,128,128) f64, the map of DepthEstimationNet.predict;
 *   counts    (batch,count_n) int64 DORN label counts (predict(return_counts=True), any head shape flattened) or NULL;
 *   log_scale (batch) f64, an extra log scale per sample, or NULL;
 *   sid       HOST pointer to alpha, beta, K, offset: the spacing-increasing discretisation the head was trained with; read only with counts;
 *   view      HOST pointer to vy0, vx0, vh, vw, the rectangle of the (h, w) frame that the map covers, as in rdm_eval_view.h; NULL = (0, 0, h, w);
 *   outside   0: a pixel outside the view is invalid (0);  1: it reads the map's replicated edge;
 *   unit      metres per step of depth_u16, > 0 (0.001: millimetres);
 *   scale_out (batch) f64 or NULL: receives ls_b.
 * Per sample, in IEEE float64 without contraction, in this order:
 *     S_b  = counts ? A + Bc * ((double)sum_b / count_n + offset) / K : 0        ((Bc * x) / K; A = log(alpha), Bc = log(beta / alpha), formed by
 *                                                                                 the launcher on the host; sum_b: the exact int64 sum of the counts)
 *     ls_b = S_b + (log_scale ? log_scale[b] : 0)
 * S_b is the mean over the head of the log of get_depth_sid(label + offset): that log is linear in the label, so the mean needs one integer
 * sum.  offset 0 is the reference's lower bin edge, 0.5 the bin centre.
 * Per pixel (y, x):
 *     v = R_view(log_map_b)(y, x) + ls_b,   D = exp(v)
 * with R_view exactly the resampling of rdm_eval_standard_view_f64 (rdm_eval_view.h: real = fma(128 / vh, (y + 0.5) - vy0, -0.5), the float
 * floor, clamped taps, the cubic coefficients and the fma order of csrc/postproc_dev.h), so under the full view it is rdm_resize_bicubic_f64's.
 *     depth_f32 = (float)D
 *     depth_u16: q = D / unit;  NaN -> 0;  q >= 65535 -> 65535;  otherwise rint(q), ties to even.
 * With outside == 0 a pixel whose centre (y + 0.5, x + 0.5) is not in [vy0, vy0 + vh) x [vx0, vx0 + vw) (the sums formed in float64) stores
 * 0.0f and 0, the "no measurement" value of depth PNGs.
 * Grid (split, batch): split workgroups per sample, each storing its share of the rows (0 = the library's default; more than h is taken as
 * h); every workgroup recomputes ls_b itself and the output does not depend on split.  Plain stores only: no atomics, no memset; a repeated
 * call gives the same bytes, a sample alone the bytes it gives inside a batch.  Any w and any alignment of the outputs is taken: a thread's
 * four adjacent pixels leave as one 16-byte (float32) and one 8-byte (uint16) store where that address is aligned, otherwise and at ragged
 * row ends as scalars.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): log_map NULL; both outputs NULL; batch, h or w not positive; batch above 65535; h * w beyond
 * 2^31 - 1; counts with count_n < 1 or sid NULL; sid with a value that is not finite, alpha <= 0, beta <= alpha or K <= 0; unit not finite or
 * not positive; outside not 0 or 1; split < 0; a view value that is not finite; vh <= 0 or vw <= 0. */
int rdm_depth_frames(const double* log_map, const int64_t* counts, int32_t count_n, const double* log_scale, const double* sid, int32_t batch,
                     int32_t h, int32_t w, const double* view, int32_t outside, double unit, float* depth_f32, uint16_t* depth_u16,
                     double* scale_out, int32_t split, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_DEPTH_H_ */
