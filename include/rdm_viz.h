/* Depth-map rendering of librdm_hip.so: depth maps (and, optionally, the network input beside them) to packed 8-bit RGB images in ONE launch.
 * The counterpart of the reference's utils.py:71-91 (colored_depthmap, merge_into_row) followed by save_image's astype('uint8')
 * (utils.py:115-117).  A header of its own beside rdm_hip.h; the entry point lives in the same library and follows the same conventions
 * (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation). */
#ifndef RDM_VIZ_H_
#define RDM_VIZ_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out (batch, h, P*w, 3) uint8: per image a row of P = 1..3 panels, left to right [rgb | a | b], each h x w; P counts the panels given.
 *   rgb (batch,3,h,w) f32 NCHW or NULL: the network input, byte = (uint8) trunc(255.0f * x) in float32 (values outside [0,1] saturate, NaN -> 0);
 *   a   (batch,1,ha,wa) or NULL (the target), b (batch,1,hb,wb) required (the prediction): float64, or float32 widened on load when its
 *       *_is_f64 is 0.  A map whose size differs from (h, w) is resized bicubically in the kernel, bit for bit rdm_resize_bicubic_f64;
 *       a map of that size is read as it is.
 * Colour (IEEE float64, no contraction): x = (v - lo) / (hi - lo), xa = x * 256; index 0 if xa < 0, 255 if xa >= 256, else (int)xa; a NaN
 * xa gives black.  The pixel is entry `index` of matplotlib's 256-entry jet table, each component truncated to uint8 (255 * value).
 * lo / hi: the colour range; a NaN argument takes that end from the data: the minimum / maximum over the a and b panels of THAT image after
 * resizing (merge_into_row's shared range; colored_depthmap's own for one panel).  As with np.min, one NaN pixel makes that end NaN and
 * the image's colour panels black; a constant image (0 / 0) is black too.
 * split: workgroups per image, each storing its share of the rows (0 = the library's default; more than h is taken as h); the output does
 * not depend on it.  Plain stores only: no atomics, no memset; a repeated call gives the same bytes.
 * Any width and any alignment of out is taken (rows leave as aligned dwords, ragged ends as bytes).
 * RDM_ERR_BAD_ARGUMENT (nothing is written): b or out NULL, a non-positive size, split < 0, a plane or an output row beyond 2^31 - 1 elements. */
int rdm_viz_rows_u8(const float* rgb, const void* a, int32_t a_is_f64, int32_t ha, int32_t wa, const void* b, int32_t b_is_f64, int32_t hb, int32_t wb,
                    int32_t batch, int32_t h, int32_t w, double lo, double hi, uint8_t* out, int32_t split, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_VIZ_H_ */
