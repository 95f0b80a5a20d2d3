/* Triangle meshes of librdm_hip.so: the FACES of the surface a (batch,h,w) float32 depth frame in metres describes - the sampled pixel grid
 * triangulated, two triangles per cell, the triangles that span a depth discontinuity or touch a pixel without a measurement left out, and the
 * rest written in row-major cell order as vertex-index triples.  The VERTICES are not written here: they are the records rdm_depth_cloud
 * (rdm_cloud.h) writes for the same (depth, min_depth, max_depth, step), whose record number is the vertex index; that entry point is unchanged,
 * and this one takes no intrinsics.  Vertex records followed by the RDM_MESH_FACES_PLY records are the payload of a binary little-endian PLY
 * file with a face element.  A header of its own beside rdm_hip.h; the entry points live in the same library and follow the same conventions
 * (status codes, rdm_last_error_string, caller's stream, no allocation, no synchronisation, no environment). */
#ifndef RDM_MESH_H_
#define RDM_MESH_H_
#include "rdm_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

#define RDM_MESH_FACES_I32 0   /* 12 bytes: v0 v1 v2 as little-endian int32 */
#define RDM_MESH_FACES_PLY 1   /* 13 bytes: the byte 3, then v0 v1 v2 as little-endian int32 (PLY "list uchar int") */

/* bytes of device workspace rdm_depth_mesh needs for these arguments: >= 0; 0 for arguments rdm_depth_mesh would refuse.  (Two int32 tables
 * per sample: the valid sampled pixels of every sampled row and the faces of every cell row.) */
int64_t rdm_depth_mesh_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t step);

/* depth   (batch,h,w) f32 metres;
 * step    only the pixels with y % step == 0 and x % step == 0 are SAMPLED: sh = ceil(h / step) rows of sw = ceil(w / step);
 * layout  RDM_MESH_FACES_I32 or RDM_MESH_FACES_PLY: rec = 12 or 13 bytes per face;
 * faces   sample b's faces start at faces + b * sample_stride_bytes (any alignment);  face_count (batch) i32 receives the number written;
 *         bytes from face_count[b] * rec to the end of the sample's region are not touched;
 * vertex_count  (batch) i32 or NULL: receives the number of valid sampled pixels of the sample, which is rdm_depth_cloud's count[b];
 * workspace     device memory of at least rdm_depth_mesh_workspace_bytes(batch, h, w, step) bytes, 4-byte aligned, written by the call and
 *         of no meaning afterwards; two calls that may run at the same time need a workspace each.
 * VALIDITY and SAMPLING are those of rdm_cloud.h: a pixel with depth d is VALID iff d is finite and d > 0 and (double)d >= min_depth and
 * (double)d <= max_depth (max_depth = +inf: no upper bound).
 * VERTEX INDEX of a valid sampled pixel: the number of valid sampled pixels before it in row-major order - its record number in
 * rdm_depth_cloud's output for that sample.
 * CELLS.  Cell (i, j), 0 <= i < sh - 1, 0 <= j < sw - 1, has the corners A = (i, j), B = (i, j + 1), C = (i + 1, j), D = (i + 1, j + 1) of the
 * sampled grid (pixel (i * step, j * step) of the frame, and so on).  sh == 1 or sw == 1: no cells, 0 faces, not an error.
 * DIAGONAL.  AD iff A and D are both valid and either B and C are not both valid or fabs((double)dA - (double)dD) <= fabs((double)dB -
 * (double)dC) (a tie goes to AD); otherwise BC.  AD yields the candidates (A, C, D) then (A, D, B); BC yields (A, C, B) then (B, C, D).
 * With the camera's axes x right, y down, z forward and positive fx, fy (the unprojection of rdm_cloud.h) all four candidates are wound so that
 * cross(p1 - p0, p2 - p0) points at the camera: the side rdm_depth_cloud's normals face.
 * A candidate is EMITTED iff its three corners are valid and it passes the edge test: with lo and hi the minimum and maximum of its three
 * float32 depths, (double)hi <= (double)lo * edge_ratio, one IEEE float64 multiplication, no contraction.  edge_ratio = +inf rejects nothing.  A
 * cell with exactly three valid corners therefore yields at most the one triangle of those three.
 * ORDER.  The faces follow the cells in row-major order, within a cell the first candidate before the second.
 * Two launches on the caller's stream: the first fills the two tables of the workspace, one workgroup per sampled row; in the second one
 * workgroup per cell row sums the table entries ahead of its row itself, so no workgroup waits for another, numbers the corners along the row,
 * and compacts the row's faces through LDS.  Plain stores only: no atomics, no memset, no read-modify-write of output words: a row's faces
 * leave as aligned 16-byte stores with the ragged ends as byte stores, so a neighbouring row may own the rest of a shared word.  A sample alone
 * gives the bytes it gives inside a batch; a repeated call gives the same bytes; there is no launch-shape argument and the bytes depend on none.
 * RDM_ERR_BAD_ARGUMENT (nothing is written, no device call is made): depth, faces or face_count NULL; batch, h, w or step not positive; batch
 * above 65535; h * w beyond 2^31 - 1; min_depth negative or NaN; max_depth NaN or below min_depth; edge_ratio NaN or below 1; layout not 0 or 1;
 * sample_stride_bytes below 2 * (sh - 1) * (sw - 1) * rec or beyond 2^31 - 1; workspace_bytes below rdm_depth_mesh_workspace_bytes(batch, h, w,
 * step); workspace NULL while that is not 0. */
int rdm_depth_mesh(const float* depth, int32_t batch, int32_t h, int32_t w, double min_depth, double max_depth, int32_t step,
                   double edge_ratio, int32_t layout, uint8_t* faces, int64_t sample_stride_bytes, int32_t* face_count,
                   int32_t* vertex_count /* may be NULL */, void* workspace, int64_t workspace_bytes, rdm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RDM_MESH_H_ */
