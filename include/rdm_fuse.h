/* Multi-frame depth fusion of librdm_hip.so: (batch,h,w) float32 depth frames in metres (what rdm_depth_frames or rdm_depth_frames_corrected
 * writes, or any sensor depth), each with a rigid pose, integrated into ONE truncated signed distance (TSDF) volume in world coordinates - a
 * running weighted mean of the projective distance per voxel, with the colours alongside - and the volume's zero crossings read out as oriented
 * surface points in rdm_cloud.h's record layout, the payload of a binary little-endian PLY file.  A header of its own beside rdm_hip.h; the entry
 * points live in the same library and follow the same conventions (status codes, rdm_last_error_string, caller's stream, no allocation, no
 * synchronisation, no environment). */
#ifndef RDM_FUSE_H_
#define RDM_FUSE_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* THE VOLUME.  nx, ny, nz voxels;  geom  HOST pointer to five doubles ox, oy, oz, voxel, trunc in world metres, voxel > 0 and trunc > 0.  The
 * centre of voxel (k, j, i), 0 <= k < nz, 0 <= j < ny, 0 <= i < nx, is
 *     Px = ox + (double)i * voxel,   Py = oy + (double)j * voxel,   Pz = oz + (double)k * voxel.
 * Planes, x fastest:  tsdf (nz,ny,nx) f32, the distance T in units of trunc;  weight (nz,ny,nx) f32, W;  color (nz,ny,nx,3) f32, C, or NULL.
 * The caller initialises the planes (md_rdm_amd.fuse.Volume: T = 1, W = 0, C = 0).
 * All arithmetic below is IEEE float64, one operation per step in the order written, without contraction, unless a cast says otherwise.
 *
 * rdm_tsdf_integrate: ONE launch that updates the planes in place from the `batch` frames, taken IN ORDER b = 0 .. batch - 1.
 * depth     (batch,h,w) f32 metres;  rgb  (batch,h,w,3) u8 or NULL (read only when color is given);
 * intr      HOST pointer to fx, fy, cx, cy, the one camera of all the frames.  Pixel (y, x) is at the integer coordinates (x, y), 0-based, at
 *           its centre; the camera's axes are x right, y down, z forward (rdm_cloud.h);
 * poses     DEVICE pointer to float64 poses of twelve values each, row-major [R | t] = r00 r01 r02 t0  r10 r11 r12 t1  r20 r21 r22 t2 (rdm_warp.h's
 *           layout), mapping WORLD coordinates to the coordinates of frame b's camera;  pose_stride 0: one pose for every frame; 12: frame b's
 *           pose is at poses + 12 * b.  R is used as given and is not re-orthogonalised;
 * obs_weight  the weight of one observation, finite and > 0;  max_weight  the cap of W, >= obs_weight (+inf: no cap).
 * Per voxel (T, W, C its values) and frame b:
 * POSE (rdm_warp.h's, of P):  Qx = ((r00 * Px + r01 * Py) + r02 * Pz) + t0,  Qy = ((r10 * Px + r11 * Py) + r12 * Pz) + t1,
 *           Qz = ((r20 * Px + r21 * Py) + r22 * Pz) + t2.  The frame is SKIPPED unless Qz is finite and Qz > 0.
 * PROJECTION:  u = (fx * Qx) / Qz + cx,  v = (fy * Qy) / Qz + cy.  Skipped unless u and v are finite.
 * PIXEL:  c = floor(u + 0.5),  r = floor(v + 0.5), a half rounding up.  Skipped unless 0 <= c <= w - 1 and 0 <= r <= h - 1 (the comparison is
 *           made in float64, before any conversion to an integer).
 * DEPTH:  d = depth[b, r, c].  Skipped unless d is VALID by rdm_cloud.h's rule: d finite and d > 0 and (double)d >= min_depth and (double)d <=
 *           max_depth (max_depth = +inf: no upper bound).
 * DISTANCE:  sdf = (double)d - Qz, the projective distance along z.  Skipped if sdf < -trunc (the voxel is hidden behind the surface).
 *           s = sdf / trunc;  s > 1: s = 1.
 * UPDATE:  Wd = (double)W,  den = Wd + obs_weight,
 *           T' = (float)((Wd * (double)T + obs_weight * s) / den),
 *           per channel ch, if color is given:  C' = (float)((Wd * (double)C + obs_weight * (double)rgb[b, r, c, ch]) / den),
 *           W' = (float)(den > max_weight ? max_weight : den),
 *           each rounded once to nearest-even.  The ROUNDED float32 values T', W', C' are what frame b + 1 sees: one call with B frames gives the
 *           bytes of B calls with one frame each.
 * A voxel that every frame skips keeps its bytes (it is not stored to).  One thread reads and writes a voxel, with plain loads and plain
 * vector stores: no atomics, no memset; the frame loop runs inside the thread, so the volume is read once and written once per call whatever
 * batch is.  The output bytes depend on no launch geometry; a repeated call from the same planes gives the same bytes.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): depth, intr, poses, geom, tsdf or weight NULL; color without rgb; batch, h
 * or w not positive; batch above 65535; h * w beyond 2^31 - 1; an intr value that is not finite, fx or fy equal to 0; min_depth negative or
 * NaN; max_depth NaN or below min_depth; pose_stride neither 0 nor 12; nx, ny or nz not positive; nx * ny * nz beyond 2^31 - 1; a geom value that
 * is not finite, voxel or trunc not > 0; obs_weight not finite or not > 0; max_weight NaN or below obs_weight. */
int rdm_tsdf_integrate(const float* depth, const uint8_t* rgb /* may be NULL */, int32_t batch, int32_t h, int32_t w, const double* intr,
                       const double* poses, int32_t pose_stride, double min_depth, double max_depth, double obs_weight, double max_weight,
                       int32_t nx, int32_t ny, int32_t nz, const double* geom, float* tsdf, float* weight, float* color /* may be NULL */,
                       rdm_stream_t stream);

/* bytes of device workspace rdm_tsdf_extract needs: nz * ny * 8 (one 64-bit entry per row of nx voxels); 0 for dims that rdm_tsdf_extract
 * would refuse. */
size_t rdm_tsdf_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);

/* rdm_tsdf_extract: the surface of the volume as oriented points, in world coordinates.
 * tsdf, weight, color (may be NULL), nx, ny, nz, geom: THE VOLUME above;  normals 1: the record carries a normal;
 * records   the output, any alignment, or NULL: count only;  capacity  the records it has room for, >= 0;  count  DEVICE pointer to one int64;
 * workspace device memory of at least rdm_tsdf_extract_workspace_bytes(nx, ny, nz) bytes, 8-byte aligned, written by the call and of no meaning
 *           afterwards; whatever bytes it holds on entry, the result is the same; two calls that may run at the same time need one each.
 * A voxel is OBSERVED iff its T is finite and (double)W >= min_weight.
 * EDGES.  Voxel V0 = (k, j, i) owns three edges: +x to V1 = (k, j, i + 1), +y to (k, j + 1, i), +z to (k + 1, j, i), each where V1 is in the
 * grid.  With T0, T1 the values of T at V0 and V1, an edge CROSSES the surface iff V0 and V1 are observed and |T0| < 1 and |T1| < 1 and
 * (T0 < 0) != (T1 < 0).  (|T| < 1: a sign change against a voxel that was only ever seen as free space, T = 1, or against the far end of a
 * band, T = -1, is the back of the band and not a surface.)
 * Per crossing, one record:
 * POSITION:  a = (double)T0 / ((double)T0 - (double)T1).  Along the edge's axis (x, origin ox, index i; y: oy, j; z: oz, k):
 *           o + ((double)idx + a) * voxel;  the two other coordinates are V0's centre, o + (double)idx * voxel.  Each rounded once to float32.
 * COLOUR (color given), per channel:  ch = (double)C0 + a * ((double)C1 - (double)C0);  the byte is 0 if ch is NaN, otherwise q = floor(ch +
 *           0.5), 0 where q <= 0, 255 where q >= 255, else q.
 * NORMAL (normals == 1).  The gradient g(V) of T at a voxel V, per axis, from the neighbours V- and V+ at -1 and +1 along that axis, a
 *           neighbour counting iff it is in the grid and observed:  both count: ((double)T(V+) - (double)T(V-)) * 0.5;  only V+: (double)T(V+) -
 *           (double)T(V);  only V-: (double)T(V) - (double)T(V-);  neither: 0.  Then per component  n = g(V0) + a * (g(V1) - g(V0)),
 *           l = sqrt((nx * nx + ny * ny) + nz * nz);   l finite and l > 0: n = n / l (three divisions), otherwise n = (+0, +0, +0),
 *           and each component is rounded once to float32.  T grows toward free space: the normal points out of the surface.
 * Record, little-endian (rdm_cloud.h's): x y z f32, then nx ny nz f32 if normals, then r g b u8 if color: rec = 12, 15, 24 or 27 bytes.
 * ORDER: the voxels V0 in row-major (k, j, i) order; within a voxel the x edge, then y, then z.
 * count receives the TOTAL number of crossings whatever capacity is; only the records with an ordinal below capacity are written, and the
 * bytes of `records` from min(total, capacity) * rec on are not touched.
 * At most three launches on the caller's stream: the crossings of every row (k, j) counted into the workspace; an exclusive scan of that table
 * by one workgroup, which also writes count; the writer (not launched when records is NULL or capacity is 0), one workgroup per row at a time,
 * which ranks its crossings and compacts them through LDS.  No workgroup waits for another.  Plain stores only: no atomics, no memset, no
 * read-modify-write: a run of records leaves as aligned 16-byte stores with its ragged ends as byte stores (rdm_cloud.h), so a neighbouring
 * row may own the rest of a shared word.  The output bytes depend on no launch geometry; a repeated call gives the same bytes.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): tsdf, weight, geom, count or workspace NULL; nx, ny or nz not positive;
 * nx * ny * nz beyond 2^31 - 1; a geom value that is not finite, voxel or trunc not > 0; min_weight NaN; normals not 0 or 1; capacity negative;
 * workspace_bytes below rdm_tsdf_extract_workspace_bytes(nx, ny, nz); workspace not 8-byte aligned. */
int rdm_tsdf_extract(const float* tsdf, const float* weight, const float* color /* may be NULL */, int32_t nx, int32_t ny, int32_t nz,
                     const double* geom, double min_weight, int32_t normals, uint8_t* records /* may be NULL */, int64_t capacity, int64_t* count,
                     void* workspace, size_t workspace_bytes, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_FUSE_H_ */
