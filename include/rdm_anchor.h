/* Anchored metric depth of librdm_hip.so: the (batch,128,128) float64 map of log relative depth tied to a sparse or partial frame of metric
 * measurements of the same view (SLAM / SfM landmarks, a LiDAR sweep, a ToF frame with holes) by a fitted per-sample log scale and a smooth
 * correction field, in THREE launches: sums of the log residuals over square cells of the frame, the fit and the smoothed field of one sample
 * per workgroup, and rdm_depth_frames (rdm_depth.h) with the field interpolated at every pixel.  A header of its own beside rdm_hip.h; the entry
 * points live in the same library and follow the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no
 * synchronisation, no environment).  All three: plain stores only, no floating-point atomics, no memset; a repeated call gives the same bytes
 * and a sample alone gives the bytes it gives inside a batch.  Every float64 step below is ONE IEEE operation, without contraction, in the
 * order written; the only operations that are not correctly rounded are the float64 ln of launch 1 and the float64 exp of launch 3.
 *
 * Notation, per sample b:  v(y, x) = R_view(log_map_b)(y, x), exactly the resampling of rdm_depth_frames / rdm_eval_standard_view_f64
 * (rdm_eval_view.h: real = fma(128 / vh, (y + 0.5) - vy0, -0.5), the float floor, clamped taps, the cubic coefficients and the fma order of
 * csrc/postproc_dev.h);  a(y, x) the anchor frame in metres.  Pixel (y, x) is an ANCHOR when a is finite, a > 0, min_depth <= (double)a <=
 * max_depth (rdm_cloud.h's validity) and its centre (y + 0.5, x + 0.5) lies in [vy0, vy0 + vh) x [vx0, vx0 + vw), the sums formed in float64. */
#ifndef RDM_ANCHOR_H_
#define RDM_ANCHOR_H_
#include "rdm_depth.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RDM_ANCHOR_FIT_NONE 0
#define RDM_ANCHOR_FIT_LOGMEAN 1
#define RDM_ANCHOR_MAX_CELLS 5120 /* gy * gx of launch 2: its four cell planes (28 bytes per cell) are 140 KiB of the 160 KiB of LDS */
#define RDM_ANCHOR_MAX_RADIUS 96  /* Rg = ceil(3 * sigma) of launch 2: the tap table travels by value (sigma <= 32 cells) */

/* Launch 1, cell sums.  The frame is cut into square cells of `cell` pixels: gy = ceil(h / cell) by gx = ceil(w / cell) cells, cell (cy, cx)
 * holding the ch = min(cell, h - cy * cell) by cw = min(cell, w - cx * cell) pixels from (cy * cell, cx * cell) on (ragged last cells).
 *   log_map (batch,128,128) f64;  anchors (batch,h,w) f32 metres;  prior (batch) f64 log scale per sample (the SID scale, say) or NULL = 0;
 *   view    HOST pointer to vy0, vx0, vh, vw as in rdm_depth_frames; NULL = (0, 0, h, w);
 *   reject  outlier gate in log units, > 0; +inf = off.  A finite reject needs a prior;
 *   n_cells (batch,gy,gx) int32, s_cells (batch,gy,gx) f64: the outputs.
 * Per anchor:   r = (ln((double)a) - v) - prior_b;   the anchor is DROPPED when |r| > reject (a NaN r is never dropped).
 * Per cell:     n_c = the number of anchors kept;  s_c = the sum of their r in this order: pixel p = 0 .. ch * cw - 1 of the cell is
 *               (cy * cell + p / cw, cx * cell + p % cw), row-major in the cell;  lane l of the 64 (one wavefront owns the cell) adds the r of
 *               its kept pixels p = l, l + 64, l + 128, ... to 0.0 in ascending p;  the 64 lane sums t_l are then folded six times,
 *               t_l = t_l + t_(l + o) for l < o, o = 32, 16, 8, 4, 2, 1, and s_c = t_0.  A cell without a kept anchor has n_c = 0, s_c = 0.0.
 * Grid (ceil(gy * gx / 4), batch), 256 threads: four wavefronts, one cell each; no workgroup waits for another.  A pixel that is not an
 * anchor costs one load and no arithmetic, so a sparse frame is cheap.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): log_map, anchors, n_cells or s_cells NULL; log_map, prior or s_cells not 8-byte aligned, anchors
 * or n_cells not 4-byte aligned; batch, h or w not positive; batch above 65535; h * w beyond 2^31 - 1; cell < 1; min_depth < 0; max_depth NaN
 * or below min_depth; reject NaN or <= 0; a finite reject with prior NULL; a view value that is not finite; vh <= 0 or vw <= 0. */
int rdm_depth_anchor_cells(const double* log_map, const float* anchors, const double* prior, int32_t batch, int32_t h, int32_t w, const double* view,
                           int32_t cell, double min_depth, double max_depth, double reject, int32_t* n_cells, double* s_cells, rdm_stream_t stream);

/* Launch 2, fit and field: one workgroup per sample, the cell planes in LDS.
 *   n_cells, s_cells (batch,gy,gx): launch 1's;  prior (batch) f64 or NULL = 0: the one launch 1 was given;
 *   log_scale_out (batch) f64: ls_b;  count_out (batch) int32: n_b = the exact integer sum of n_c;
 *   field (batch,gy,gx) f64, or NULL: only the fit.
 * Fit:      RDM_ANCHOR_FIT_NONE     delta_b = 0.0
 *           RDM_ANCHOR_FIT_LOGMEAN  delta_b = S / (double)n_b,  S = the s_c added to 0.0 one by one, cells in row-major order;  0.0 when n_b = 0
 *           ls_b = prior_b + delta_b
 * Re-centre: s'_c = s_c - (double)n_c * delta_b                      (one multiplication, one subtraction)
 * Taps:     Rg = ceil(3 * sigma);  g[0] = 1.0 (set);  g[k] = exp(-((double)k * (double)k) / (2 * (sigma * sigma))), k = 1 .. Rg, formed ON THE HOST
 *           by the launcher with the C library's exp and passed by value: no device exponential enters the field.  sigma is in cells;
 *           sigma = 0 means Rg = 0: no smoothing.
 * Smoothing: a normalised convolution, separable, rows along x first and then along y.  For a plane P, with acc from 0.0 and k ascending from
 *           -Rg to Rg, taps beyond the border skipped:
 *               X(P)(cy, cx) = acc,  acc = acc + g[|k|] * P(cy, cx + k)      (one multiplication, one addition, no fma)
 *               Y(Q)(cy, cx) = acc,  acc = acc + g[|k|] * Q(cy + k, cx)
 *           N = Y(X(s')),  W = Y(X((double)n)).
 * Field:    C_c = N_c / (W_c + lambda), and 0.0 where W_c + lambda == 0.  lambda >= 0 is a regulariser in units of anchors: where there is
 *           little evidence the field tends to 0.  A sample without an anchor has ls_b = prior_b + 0.0 and a field of +0.0 throughout.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): n_cells, s_cells, log_scale_out or count_out NULL; s_cells, prior, log_scale_out or field not
 * 8-byte aligned, n_cells or count_out not 4-byte aligned; batch, gy or gx not positive; batch above 65535; gy * gx above
 * RDM_ANCHOR_MAX_CELLS (480x640 at cell = 8 is 4800); an unknown fit; sigma or lambda negative or not finite; ceil(3 * sigma) above
 * RDM_ANCHOR_MAX_RADIUS. */
int rdm_depth_anchor_field(const int32_t* n_cells, const double* s_cells, const double* prior, int32_t batch, int32_t gy, int32_t gx, int32_t fit,
                           double sigma, double lambda, double* log_scale_out, int32_t* count_out, double* field, rdm_stream_t stream);

/* Launch 3, corrected frames: rdm_depth_frames (rdm_depth.h; same kernel, same arguments, same grid and stores) with the field added in the
 * log domain.  log_scale is normally launch 2's log_scale_out and counts NULL, because the prior already carried the SID scale.
 *   field (batch,gy,gx) f64;  gy = ceil(h / cell), gx = ceil(w / cell);  cell >= 1: launch 1's.
 * Per pixel:    D = exp((v + ls_b) + c(y, x))          (ls_b as rdm_depth_frames forms it; two additions)
 * c is the bilinear interpolation of the field; cell i's centre sits at the pixel coordinate (i + 0.5) * cell - 0.5.  Per axis, in float64:
 *     u = ((double)y + 0.5) / (double)cell;  u = u - 0.5;  f = floor(u);  t = u - f;  i0 = clamp((int)f, 0, gy - 1),  i1 = clamp((int)f + 1, 0, gy - 1)
 * (j0, j1, tx from x, cell and gx likewise: indices are clamped at the border, where the field is therefore held constant), then
 *     top = fma(tx, F(i0, j1) - F(i0, j0), F(i0, j0));   bot = fma(tx, F(i1, j1) - F(i1, j0), F(i1, j0));   c = fma(ty, bot - top, top)
 * A field of zeros gives c = 0.0 and the bytes of rdm_depth_frames.  With outside == 0 a pixel outside the view stores 0.0f and 0 as before.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): whatever rdm_depth_frames refuses; field NULL or not 8-byte aligned; cell < 1; gy or gx not
 * ceil(h / cell), ceil(w / cell). */
int rdm_depth_frames_corrected(const double* log_map, const int64_t* counts, int32_t count_n, const double* log_scale, const double* sid, int32_t batch,
                               int32_t h, int32_t w, const double* view, int32_t outside, double unit, float* depth_f32, uint16_t* depth_u16,
                               double* scale_out, int32_t split, const double* field, int32_t gy, int32_t gx, int32_t cell, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_ANCHOR_H_ */
