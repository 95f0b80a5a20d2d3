/* Novel views of librdm_hip.so: a (batch,h,w) float32 depth frame in metres, with its colours, seen from ANOTHER pinhole camera - every valid
 * source pixel unprojected (rdm_cloud.h's float64 point), moved by a rigid pose, projected into a (th, tw) target grid and kept where it is the
 * nearest surface of its cell (a z-buffer), then optionally the empty cells of every row filled from the farther of their nearest neighbours.
 * The right eye of a stereo pair, a small camera move, or the depth of frame A in frame B's pixel grid.  A header of its own beside rdm_hip.h;
 * the entry points live in the same library and follow the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation,
 * no synchronisation, no environment). */
#ifndef RDM_WARP_H_
#define RDM_WARP_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* bytes of device workspace rdm_depth_warp needs: batch * th * tw * 8 (one 64-bit key per target cell); 0 for a batch, th or tw that
 * rdm_depth_warp would refuse. */
size_t rdm_depth_warp_workspace_bytes(int32_t batch, int32_t th, int32_t tw);

/* depth     (batch,h,w) f32 metres, the SOURCE frame;
 * rgb       (batch,h,w,3) u8 colours of the source frame, or NULL;
 * intr_src  HOST pointer to fx, fy, cx, cy of the source camera;  intr_dst  HOST pointer to fxd, fyd, cxd, cyd of the target camera.  Pixel
 *           (y, x) is at the integer coordinates (x, y), 0-based, at its centre; the cameras' axes are x right, y down, z forward (rdm_cloud.h);
 * poses     DEVICE pointer to float64 poses of twelve values each, row-major [R | t] = r00 r01 r02 t0  r10 r11 r12 t1  r20 r21 r22 t2, mapping
 *           source-camera coordinates to target-camera coordinates;  pose_stride 0: one pose for every sample; 12: sample b's pose is at
 *           poses + 12 * b.  R is used as given and is not re-orthogonalised;
 * th, tw    the target grid;  splat 1..4;  fill 0..64;
 * depth_out (batch,th,tw) f32;  rgb_out (batch,th,tw,3) u8 or NULL (needs rgb);  index_out (batch,th,tw) i32 or NULL;  mask_out (batch,th,tw)
 *           u8 or NULL;
 * workspace device memory of at least rdm_depth_warp_workspace_bytes(batch, th, tw) bytes, 8-byte aligned, written by the call and of no
 *           meaning afterwards; whatever bytes it holds on entry, the result is the same; two calls that may run at the same time need one each.
 * All arithmetic below is IEEE float64, one operation per step in the order written, without contraction, unless a cast says otherwise.
 * SOURCE VALIDITY (rdm_cloud.h's): a pixel with depth d takes part iff d is finite and d > 0 and (double)d >= min_depth and (double)d <=
 * max_depth (max_depth = +inf: no upper bound).
 * SOURCE POINT of pixel (y, x):  Z = (double)d,  X = (((double)x - cx) * Z) / fx,  Y = (((double)y - cy) * Z) / fy   (not rounded to float32).
 * POSE:  Qx = ((r00 * X + r01 * Y) + r02 * Z) + t0,  Qy = ((r10 * X + r11 * Y) + r12 * Z) + t1,  Qz = ((r20 * X + r21 * Y) + r22 * Z) + t2.
 * TARGET DEPTH:  zf = (float)Qz, rounded once to nearest-even.  The point is DROPPED unless Qz is finite and zf is finite and zf > 0.
 * PROJECTION:  u = (fxd * Qx) / Qz + cxd,  v = (fyd * Qy) / Qz + cyd.  The point is dropped if u or v is not finite.
 * FOOTPRINT (splat = s):  c0 = floor((u - (s - 1) * 0.5) + 0.5),  r0 = floor((v - (s - 1) * 0.5) + 0.5); the point covers the columns c0 <= c <
 * c0 + s and the rows r0 <= r < r0 + s, of which only the cells with 0 <= c < tw and 0 <= r < th are touched (the comparison is made in
 * float64, before any conversion to an integer).  s = 1: the nearest cell, a half rounding up.
 * DEPTH TEST.  Every touched cell is offered key = (uint64)bits(zf) << 32 | (uint32)(y * w + x) and keeps the MINIMUM of the keys offered to it:
 * the bits of positive finite floats are ordered as the floats are, so the nearest point wins, and of points with the same zf the one with the
 * smaller source index.  A cell offered nothing is EMPTY.
 * RESOLVE.  A cell with a key:  depth_out = zf,  rgb_out = the three bytes of source pixel (y, x),  index_out = y * w + x,  mask_out = 1.
 * An empty cell:  depth_out = +0,  rgb_out = 0 0 0,  index_out = -1,  mask_out = 0.
 * HOLE FILL (fill = F > 0), on the resolved planes: for an empty cell (r, c), L is the nearest cell (r, c - k), 1 <= k <= F, c - k >= 0, that
 * has a key, and G the nearest cell (r, c + k), 1 <= k <= F, c + k < tw, that has a key.  Neither exists: the cell stays as above.  One exists:
 * that one.  Both: the one with the larger zf (the background, as disocclusion filling does); equal zf: L.  The cell receives that cell's
 * depth, colour and index, and mask_out = 2.  Only cells with a key (mask 1) are ever copied from: a filled cell fills nothing.
 * At most three launches on the caller's stream: the keys are set to 0xFFFFFFFFFFFFFFFF (which no key equals: its upper half is a NaN's bits);
 * one thread per source pixel offers its key with a 64-bit unsigned atomic minimum at device scope (the minimum is associative and commutative,
 * so the winner does not depend on the order of arrival); one thread per target cell resolves and fills, reading the keys of its row segment and
 * F cells either side through LDS, and writes with plain stores.  The output bytes depend on no launch geometry; a sample alone gives the
 * bytes it gives inside a batch; a repeated call gives the same bytes.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): depth, intr_src, intr_dst, poses, depth_out or workspace NULL; rgb_out
 * without rgb; batch, h, w, th or tw not positive; batch above 65535; h * w or th * tw beyond 2^31 - 1; pose_stride neither 0 nor 12; splat
 * outside 1..4; fill outside 0..64; workspace_bytes below rdm_depth_warp_workspace_bytes(batch, th, tw); workspace not 8-byte aligned; an
 * intrinsics value that is not finite, fx, fy, fxd or fyd equal to 0; min_depth negative or NaN; max_depth NaN or below min_depth. */
int rdm_depth_warp(const float* depth, const uint8_t* rgb, int32_t batch, int32_t h, int32_t w, const double* intr_src, const double* intr_dst,
                   const double* poses, int32_t pose_stride, double min_depth, double max_depth, int32_t th, int32_t tw, int32_t splat,
                   int32_t fill, float* depth_out, uint8_t* rgb_out /* may be NULL */, int32_t* index_out /* may be NULL */,
                   uint8_t* mask_out /* may be NULL */, void* workspace, size_t workspace_bytes, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_WARP_H_ */
