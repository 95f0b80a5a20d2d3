/* Guided depth refinement of librdm_hip.so: a (batch,h,w) float32 depth frame in metres (what rdm_depth_frames writes, or any sensor depth)
 * filtered by a joint (cross) bilateral filter under the colour frame it belongs to, as float32 and / or as the 16-bit plane of a depth PNG, in
 * ONE launch.  Neighbours whose colour differs get little weight, so depth edges that a resampling has smeared move back to the colour edges;
 * pixels without a measurement can be filled from their surroundings.  A header of its own beside rdm_hip.h; the entry point lives in the same
 * library and follows the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation, no
 * environment). */
#ifndef RDM_REFINE_H_
#define RDM_REFINE_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* depth   (batch,h,w) f32 metres;
 * guide   (batch,h,w,3) u8, the colour frame of the same geometry;
 * out_f32 / out_u16 (batch,h,w): either may be NULL, not both;  out_f32 must not be depth (taps read neighbours: not in place);
 * fill    0: a pixel whose own depth is not valid stays invalid;  1: it is filled from its valid taps;
 * unit    metres per step of out_u16, > 0 (0.001: millimetres).
 * A depth d is VALID iff d is finite and d > 0 (rdm_cloud.h's rule without the range limits).
 * Taps of the pixel (y, x): the pixels (y + j * step, x + i * step), j and i in [-radius, radius], visited with j outer and i inner, both
 * ascending.  A tap outside the frame is skipped (not clamped); so is a tap whose depth is not valid.
 * Tables, in IEEE float64:
 *     ws[k] = exp(-(sk * sk) / (2 * (sigma_space * sigma_space))),  sk = (double)(k * step),  k = 1..radius   (formed by the launcher on the host)
 *     E[k]  = exp(-(dk * dk) / (2 * (sigma_color * sigma_color))),  dk = (double)k,           k = 1..255      (formed by every workgroup with the
 *                                                                                                              device exp, once, into LDS)
 *     ws[0] = E[0] = 1.0 exactly (set, not computed).  A sigma of +inf makes its table exactly 1.0 throughout.
 * Weight of a tap q at the offset (j, i); dR, dG, dB the integer differences of the guide's bytes at q and at (y, x):
 *     w = (ws[|j|] * ws[|i|]) * ((E[|dR|] * E[|dG|]) * E[|dB|])
 * every operation one IEEE float64 operation in this order, without contraction.  Sums, from 0.0, in tap order:
 *     num = num + w * (double)d_q      (one multiplication and one addition, no fma)
 *     den = den + w
 *     D   = num / den
 * Result of the pixel:  its own depth valid: D (its own tap has the weight 1, so den >= 1);  not valid and fill == 0: invalid;  not valid and
 * fill == 1: D if den > 0, otherwise invalid.
 * Stores: an invalid pixel stores 0.0f and 0, the "no measurement" value of depth PNGs.  Otherwise
 *     out_f32 = (float)D
 *     out_u16: q = D / unit;  NaN -> 0;  q >= 65535 -> 65535;  otherwise rint(q), ties to even                 (rdm_depth_frames' rule)
 * Grid (tiles, batch): one workgroup per tile of 32 x 16 pixels of a sample; it stages the tile's depth and guide with a halo of radius * step
 * on every side into LDS once and reads every tap from there.  The output does not depend on how the frame is cut into tiles; a sample alone
 * gives the bytes it gives inside a batch; a repeated call gives the same bytes.  Plain stores only: no atomics, no memset, no workgroup waits
 * for another.  Any w and any alignment of the outputs is taken: a thread's two adjacent pixels leave as one 8-byte (float32) and one 4-byte
 * (uint16) store where that address is aligned, otherwise and at ragged row ends as scalars.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): depth or guide NULL; both outputs NULL; out_f32 == depth; batch, h or w not
 * positive; batch above 65535; h * w beyond 2^31 - 1; radius outside [1, 8]; step outside [1, 16]; radius * step > 24; a sigma that is NaN or
 * <= 0 (+inf is allowed); fill not 0 or 1; unit not finite or not positive. */
int rdm_depth_refine(const float* depth, const uint8_t* guide, int32_t batch, int32_t h, int32_t w, int32_t radius, int32_t step,
                     double sigma_space, double sigma_color, int32_t fill, double unit, float* out_f32, uint16_t* out_u16, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_REFINE_H_ */
