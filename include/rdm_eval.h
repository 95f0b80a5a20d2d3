/* Standard-protocol depth evaluation of librdm_hip.so: the predicted log map and the loader's raw depth to the Eigen et al. error sums per
 * sample, at the ground truth's own resolution, in ONE launch per batch.  This is the protocol of the published NYU / KITTI tables (linear
 * depth, valid pixels only, a depth cap, an optional crop, per-image scale alignment); it has no counterpart in the reference, whose validation
 * (module.py:99-117, metrics.py:48-128) is rdm_eval_target_metrics_f64 of rdm_hip.h.  A header of its own beside rdm_hip.h; the entry points
 * live in the same library and follow the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no
 * synchronisation). */
#ifndef RDM_EVAL_H_
#define RDM_EVAL_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RDM_EVAL_ALIGN_NONE 0
#define RDM_EVAL_ALIGN_MEDIAN 1
#define RDM_EVAL_ALIGN_LOGMEAN 2
#define RDM_EVAL_STANDARD_COLS 16

/* Bytes of workspace the call below needs: one float64 per pixel and sample (the prediction between the kernel's passes).  0 for a
 * non-positive size or a plane beyond 2^31 - 1 elements. */
size_t rdm_eval_standard_workspace_bytes(int32_t batch, int32_t h, int32_t w);

/* log_map (B,1,128,128) f64, the map of rdm_predict_tail_f32 / DepthEstimationNet.predict;  depth (B,1,h,w) float32, or float64 with
 * depth_is_f64 != 0 (float32 is widened on load);  rows (B,16) f64;  pred_out (B,1,h,w) f64 or NULL;  crop: HOST pointer to y0, x0, y1, x1 or NULL.
 * Per sample (one workgroup each), in this order:
 *  1. p = exp(R(log_map)), R the bicubic resize of the map to (h, w), bit for bit the values of rdm_resize_bicubic_f64; a 128x128 depth
 *     reads the map as it is.
 *  2. a pixel is VALID when d is finite, min_depth < d < max_depth and, with a crop, y0 <= y < y1 and x0 <= x < x1.
 *  3. scale s:  RDM_EVAL_ALIGN_NONE 1;  _MEDIAN median(d_valid) / median(p_valid), numpy's median (the middle order statistic for odd n,
 *     (a + b) / 2 of the two middle ones for even n), selected exactly;  _LOGMEAN exp(mean ln d - mean ln p) over the valid pixels.
 *  4. q = s * p, then q < min_depth ? min_depth : q > max_depth ? max_depth : q (a NaN stays a NaN).
 *  5. the row, sums over the valid pixels:  0 n;  1-3 number with max(q/d, d/q) < 1.25, 1.25^2, 1.25^3;  4 sum |q-d|/d;  5 sum (q-d)^2/d;
 *     6 sum (q-d)^2;  7 sum (ln q - ln d)^2;  8 sum (ln q - ln d);  9 sum |log10 q - log10 d|;  10 sum |q-d|;  11 s;  12 / 13 the alignment
 *     statistic of d / of p (the medians, or mean ln d / mean ln p; 0 for _NONE);  14 number of valid pixels with s * p outside
 *     [min_depth, max_depth];  15 0.
 *     A sample without a valid pixel gets a row of zeros.  If p is not finite at any valid pixel the row is [n, NaN x 13, 0, 0].
 *  6. pred_out, when given: q at EVERY pixel of the frame, valid or not; for a sample whose row is zeros or NaN it is formed with s = 1.
 * One launch; the workgroups never wait for each other; plain stores, no floating-point atomics, no memset: a repeated call gives the same
 * bytes, and a sample alone gives the row it gives inside a batch.  Any h, w >= 1 up to a plane of 2^31 - 1 elements.
 * The map is taken to cover the WHOLE depth frame; rdm_eval_view.h declares the same call for a map that covers a rectangle of it.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): log_map, depth, rows or workspace NULL; log_map, rows, workspace or pred_out not 8-byte aligned,
 * depth not aligned to its element; a non-positive size, a plane beyond 2^31 - 1 elements,
 * an unknown align, !(0 <= min_depth < max_depth), an empty or out-of-frame crop, workspace_bytes below
 * rdm_eval_standard_workspace_bytes(batch, h, w). */
int rdm_eval_standard_f64(const double* log_map, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, int32_t align,
                          double min_depth, double max_depth, const int32_t* crop, double* rows, void* pred_out, void* workspace,
                          size_t workspace_bytes, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_EVAL_H_ */
