/* Point clouds of librdm_hip.so: a (batch,h,w) float32 depth frame in metres (what rdm_depth_frames writes, or any sensor depth) unprojected
 * through pinhole intrinsics to packed vertex records - position, optionally a unit normal facing the camera, optionally the pixel's colour -
 * with the invalid pixels dropped and the valid ones kept in row-major order, in ONE launch.  The records are the payload of a binary
 * little-endian PLY file.  A header of its own beside rdm_hip.h; the entry point lives in the same library and follows the same conventions
 * (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation, no environment). */
#ifndef RDM_CLOUD_H_
#define RDM_CLOUD_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* depth   (batch,h,w) f32 metres;
 * rgb     (batch,h,w,3) u8, or NULL: no colour in the record;
 * intr    HOST pointer to fx, fy, cx, cy.  Pixel (y, x) is at the integer coordinates (x, y), 0-based, at its centre; the camera's axes are x right,
 *         y down, z forward;
 * step    only the pixels with y % step == 0 and x % step == 0 are SAMPLED: sh = ceil(h / step) rows of sw = ceil(w / step);
 * normals 1: the record carries a normal;
 * records sample b's records start at records + b * sample_stride_bytes (any alignment);  count (batch) i32 receives the number written.
 * A pixel with depth d is VALID iff d is finite and d > 0 and (double)d >= min_depth and (double)d <= max_depth (max_depth = +inf: no upper
 * bound).  The output of a sample holds its valid sampled pixels in row-major order; bytes from count[b] * rec to the end of its region are not
 * touched.
 * Position, in IEEE float64 without contraction, each result rounded once to float32:
 *     Z = (double)d,   X = (((double)x - cx) * Z) / fx,   Y = (((double)y - cy) * Z) / fy
 * Normal (normals == 1): P(y, x) = (X, Y, Z) is the float64 point of a valid pixel; the neighbours are the pixels at +-1 of the FULL
 * resolution frame, whatever step is.  The horizontal difference a: both (y, x-1) and (y, x+1) valid: a = P(y, x+1) - P(y, x-1); only one
 * of them: a = P(y, x+1) - P(y, x) or a = P(y, x) - P(y, x-1); neither: the normal is (0, 0, 0).  The vertical difference b likewise from
 * (y-1, x) and (y+1, x).  Then, every operation one IEEE float64 operation in this order:
 *     n = cross(b, a):  nx = b.y * a.z - b.z * a.y,   ny = b.z * a.x - b.x * a.z,   nz = b.x * a.y - b.y * a.x
 *     s = (nx * X + ny * Y) + nz * Z;   s > 0: n = -n                                (the normal faces the camera)
 *     l = sqrt((nx * nx + ny * ny) + nz * nz);   l finite and l > 0: n = n / l (three divisions), otherwise n = (+0, +0, +0)
 * and each component is rounded once to float32.
 * Record, little-endian: x y z f32, then nx ny nz f32 if normals, then r g b u8 if rgb: rec = 12, 15, 24 or 27 bytes.
 * Grid (split, batch): split workgroups per sample (0 = the library's default; more than sh * sw is taken as sh * sw).  Workgroup r of a sample
 * owns the sampled pixels [r * sh * sw / split, (r + 1) * sh * sw / split) in row-major order (integer division); it counts the valid sampled
 * pixels ahead of its run itself, so no workgroup waits for another, then compacts its run through LDS.  The output bytes do not depend on
 * split; a sample alone gives the bytes it gives inside a batch; a repeated call gives the same bytes.  Plain stores only: no atomics, no
 * memset, no read-modify-write: a run leaves as aligned 16-byte stores with its ragged ends as byte stores, so a neighbouring run may own the
 * rest of a shared word.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): depth, intr, records or count NULL; batch, h, w or step not positive;
 * batch above 65535; h * w beyond 2^31 - 1; normals not 0 or 1; sample_stride_bytes below sh * sw * rec or beyond 2^31 - 1; an intr value that
 * is not finite, fx or fy equal to 0; min_depth negative or NaN; max_depth NaN or below min_depth; split < 0. */
int rdm_depth_cloud(const float* depth, const uint8_t* rgb, int32_t batch, int32_t h, int32_t w, const double* intr, double min_depth,
                    double max_depth, int32_t step, int32_t normals, uint8_t* records, int64_t sample_stride_bytes, int32_t* count,
                    int32_t split, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_CLOUD_H_ */
