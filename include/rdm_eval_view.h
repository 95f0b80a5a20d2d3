/* Standard-protocol depth evaluation against a ground-truth frame of which the network saw only a part: rdm_eval_standard_f64 (rdm_eval.h)
 * with the rectangle of the depth frame that the predicted map covers.  The loader's test transform is Resize(500) -> CenterCrop((480, 640))
 * -> Resize(size): of a raw 480x640 NYU frame the map covers rows 9.6 to 470.4 and columns 12.49 to 627.51, and scoring the raw depth with
 * the map stretched over the whole frame would compare pixels the network never saw.  A header of its own beside rdm_eval.h; the entry point
 * lives in the same library, runs the same kernel and follows the same conventions. */
#ifndef RDM_EVAL_VIEW_H_
#define RDM_EVAL_VIEW_H_
#include "rdm_eval.h"
#ifdef __cplusplus
extern "C" {
#endif

/* rdm_eval_standard_f64 with one more argument;  view: HOST pointer to vy0, vx0, vh, vw, the rectangle [vy0, vy0 + vh) x [vx0, vx0 + vw) of the
 * depth frame, in depth-pixel units (pixel (y, x) is the square [y, y + 1) x [x, x + 1)), that the 128x128 map covers; NULL = (0, 0, h, w).
 * The values may be fractional and the rectangle may reach outside the frame or be smaller than a pixel.
 * Only step 1 of rdm_eval_standard_f64's contract changes: p = exp(R_view(log_map)), where for depth pixel (y, x)
 *     real_y = fma(128 / vh, (y + 0.5) - vy0, -0.5),   real_x = fma(128 / vw, (x + 0.5) - vx0, -0.5)
 * and everything after that is the bicubic resize's own arithmetic (csrc/postproc_dev.h): index = min((long)floorf((float)real), 127),
 * t = min(max(real - index, 0), 1), the four taps index - 1 .. index + 2 clamped to [0, 127], the cubic coefficients of t and the fma order of
 * the two dot products.  A depth pixel outside the view therefore reads the map's replicated edge.  (For a |real| of 2^62 or more, or a
 * NaN from an overflowing 128 / vh, the float floor is clamped to +-2^62 before the conversion: every tap is then an edge.)
 * With view NULL or exactly (0, 0, h, w) the formula is rdm_resize_bicubic_f64's - 128 / h and (y + 0.5) - 0 are its operands - and rows and
 * pred_out are byte for byte what rdm_eval_standard_f64 writes, a 128x128 depth reading the map as it is included; under any other view a
 * 128x128 depth is resampled like every other size.  Steps 2 to 6, the workspace (rdm_eval_standard_workspace_bytes), the single launch, the
 * plain stores and the determinism (a repeated call gives the same bytes, a sample alone the row it gives inside a batch) are unchanged.
 * RDM_ERR_BAD_ARGUMENT (nothing is written): whatever rdm_eval_standard_f64 refuses; a view value that is not finite; vh <= 0 or vw <= 0. */
int rdm_eval_standard_view_f64(const double* log_map, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, int32_t align,
                               double min_depth, double max_depth, const int32_t* crop, const double* view, double* rows, void* pred_out,
                               void* workspace, size_t workspace_bytes, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_EVAL_VIEW_H_ */
