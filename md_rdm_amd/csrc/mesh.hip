// Triangle faces of a depth frame (include/rdm_mesh.h): the sampled pixel grid triangulated, the triangles across a depth step or next to a pixel
// without a measurement left out, the rest compacted IN ORDER into 12- or 13-byte index records whose vertex numbers are the record numbers of
// rdm_depth_cloud (cloud.hip) for the same validity arguments.  Composed from single operators that is an exclusive scan of the mask, four
// shifted views of depth and index, the diagonal rule, two masks, a boolean index per triangle kind, an interleave, a cast and a cat - and a host
// synchronisation to size the outputs.
//
// Two quantities have to be known ahead of a cell row: the vertices in front of its two pixel rows and the faces in front of its cells.  cloud.hip
// lets every workgroup re-count the plane ahead of its run; here that would evaluate the four-load face predicate of half a sample per workgroup, so
// this is DESIGN.md 4.11's shape (b):
//   k_mesh_count, grid (sh, batch): workgroup i writes the valid sampled pixels of sampled row i and the faces of cell row i into two int32 tables;
//   k_mesh_faces, grid (max(sh - 1, 1), batch): workgroup i sums the (at most sh) table entries ahead of it itself - no workgroup waits for another,
//     no look-back, no ticket, no atomic - then walks its cell row in chunks of one cell per thread: the four corners, a ballot / popcount scan of
//     the two pixel rows' validity (the corners' vertex numbers) and of the two candidates (the faces' places), the records to an LDS stage, the
//     stage to memory by depthout_dev.h's stream-out, which cloud.hip uses too: the interior as aligned 16-byte stores, the ragged head and tail -
//     whose words a neighbouring row may own - as byte stores.  Nothing is read back.
// Both kernels decide validity (depthout_dev.h's depth_valid, cloud.hip's too: the vertex numbers are its record numbers), diagonal and edge
// test with the same function, so the table and the rows cannot disagree.
#include <cmath>

#include "rdm_common.h"
#include "depthout_dev.h"
#include "../../include/rdm_mesh.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int MS_THREADS = 256;
constexpr int MS_WAVES = MS_THREADS / 64;
constexpr int MS_MAX_REC = 13;
constexpr int MS_STAGE = (16 + 2 * MS_THREADS * MS_MAX_REC + 15) / 16 * 16;      // the residue in front, two faces per cell, whole 16-byte units

struct MsArgs {
  const float* depth;
  uint8_t* faces;
  int32_t* face_count;
  int32_t* vertex_count;
  int32_t* rows;                                     // workspace: per sample sh row counts, then sh face counts (the last one unused)
  int h, w, step, sh, sw, rec;
  long stride;
  double dmin, dmax, ratio;
};

__device__ __forceinline__ bool ms_edge_ok(float a, float b, float c, double ratio) {
#pragma clang fp contract(off)
  const float lo = fminf(a, fminf(b, c)), hi = fmaxf(a, fmaxf(b, c));
  return (double)hi <= (double)lo * ratio;
}

// the two candidates of a cell: bit 0 of the result: the first is emitted, bit 1: the second; ad: the diagonal
__device__ __forceinline__ int ms_cell(float dA, float dB, float dC, float dD, bool vA, bool vB, bool vC, bool vD, double ratio, bool& ad) {
#pragma clang fp contract(off)
  ad = vA && vD && (!(vB && vC) || fabs((double)dA - (double)dD) <= fabs((double)dB - (double)dC));
  int m = 0;
  if (ad) {
    if (vC && ms_edge_ok(dA, dC, dD, ratio)) m |= 1;                 // (A, C, D)
    if (vB && ms_edge_ok(dA, dD, dB, ratio)) m |= 2;                 // (A, D, B)
  } else {
    if (vA && vB && vC && ms_edge_ok(dA, dC, dB, ratio)) m |= 1;     // (A, C, B)
    if (vB && vC && vD && ms_edge_ok(dB, dC, dD, ratio)) m |= 2;     // (B, C, D)
  }
  return m;
}

// grid (sh, batch): the valid sampled pixels of sampled row i and the faces of cell row i
__global__ __launch_bounds__(MS_THREADS) void k_mesh_count(MsArgs a) {
  __shared__ int red[2 * MS_WAVES];
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const float* __restrict__ r0 = a.depth + (long)b * a.h * a.w + (long)i * a.step * a.w;
  const float* __restrict__ r1 = r0 + (long)a.step * a.w;          // read only where i + 1 < sh
  const bool cells = i + 1 < a.sh;
  int nv = 0, nf = 0;
  for (int j = tid; j < a.sw; j += MS_THREADS) {
    const float dA = r0[(long)j * a.step];
    const bool vA = depth_valid(dA, a.dmin, a.dmax);
    nv += vA;
    if (cells && j + 1 < a.sw) {
      const float dB = r0[(long)(j + 1) * a.step], dC = r1[(long)j * a.step], dD = r1[(long)(j + 1) * a.step];
      bool ad;
      const int m = ms_cell(dA, dB, dC, dD, vA, depth_valid(dB, a.dmin, a.dmax), depth_valid(dC, a.dmin, a.dmax), depth_valid(dD, a.dmin, a.dmax), a.ratio, ad);
      nf += (m & 1) + (m >> 1);
    }
  }
  block_sums_bcast<MS_WAVES>(red, nv, nf);
  if (tid == 0) {
    int32_t* t = a.rows + (long)b * 2 * a.sh;
    t[i] = nv, t[a.sh + i] = nf;
  }
}

// grid (max(sh - 1, 1), batch): the faces of cell row i, and from the last workgroup of a sample its two counts
__global__ __launch_bounds__(MS_THREADS) void k_mesh_faces(MsArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[MS_STAGE];
  __shared__ int red[2 * MS_WAVES];
  __shared__ int wsum[3][MS_WAVES];
  const int i = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int32_t* __restrict__ t = a.rows + (long)b * 2 * a.sh;
  uint8_t* __restrict__ out = a.faces + (long)b * a.stride;
  const int rec = a.rec, ply = rec == 13;

  int v0 = 0, written = 0;                           // vertices in front of sampled row i, faces in front of cell row i
  for (int k = tid; k < i; k += MS_THREADS) v0 += t[k], written += t[a.sh + k];
  block_sums_bcast<MS_WAVES>(red, v0, written);
  int v1 = v0 + t[i];                                // vertices in front of sampled row i + 1
  const int vtotal = v1 + (i + 1 < a.sh ? t[i + 1] : 0);           // of the sample, where this is its last workgroup: row i + 1 is its last row

  const int nc = i + 1 < a.sh ? a.sw - 1 : 0;        // cells of this row (sh == 1: the one workgroup has none)
  const float* __restrict__ r0 = a.depth + (long)b * a.h * a.w + (long)i * a.step * a.w;
  const float* __restrict__ r1 = r0 + (long)a.step * a.w;
  for (int c0 = 0; c0 < nc; c0 += MS_THREADS) {
    const int j = c0 + tid;
    bool vA = false, vC = false, ad = false;
    int m = 0;
    float dA = 0.0f, dB = 0.0f, dC = 0.0f, dD = 0.0f;
    bool vB = false, vD = false;
    if (j < nc) {
      dA = r0[(long)j * a.step], dB = r0[(long)(j + 1) * a.step], dC = r1[(long)j * a.step], dD = r1[(long)(j + 1) * a.step];
      vA = depth_valid(dA, a.dmin, a.dmax), vB = depth_valid(dB, a.dmin, a.dmax), vC = depth_valid(dC, a.dmin, a.dmax), vD = depth_valid(dD, a.dmin, a.dmax);
      m = ms_cell(dA, dB, dC, dD, vA, vB, vC, vD, a.ratio, ad);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    const unsigned long long bA = __ballot(vA), bC = __ballot(vC), b1 = __ballot(m & 1), b2 = __ballot(m & 2);
    __syncthreads();                                 // the previous chunk's readers of stage and wsum are done
    if (lane == 0) wsum[0][wv] = __popcll(bA), wsum[1][wv] = __popcll(bC), wsum[2][wv] = __popcll(b1) + __popcll(b2);
    __syncthreads();
    int iA = v0 + __popcll(bA & below), iC = v1 + __popcll(bC & below), rank = __popcll(b1 & below) + __popcll(b2 & below), total = 0;
    for (int k = 0; k < MS_WAVES; ++k) {
      if (k < wv) iA += wsum[0][k], iC += wsum[1][k], rank += wsum[2][k];
      v0 += wsum[0][k], v1 += wsum[1][k], total += wsum[2][k];
    }
    const int iB = iA + vA, iD = iC + vC;            // the next pixel of the row follows this one
    uint8_t* g0 = out + (long)written * rec;         // where the chunk's first face goes
    const int phase = (int)((uintptr_t)g0 & 15);     // stage byte k is memory byte (g0 - phase) + k
    int off = phase + rank * rec;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      if (!(m >> c & 1)) continue;
      int f[3];
      if (ad) f[0] = iA, f[1] = c ? iD : iC, f[2] = c ? iB : iD;
      else f[0] = c ? iB : iA, f[1] = iC, f[2] = c ? iD : iB;
      if (ply) stage[off] = 3;
      const int at = off + ply;
      if ((at & 3) == 0) {
        int* d = (int*)(stage + at);
        d[0] = f[0], d[1] = f[1], d[2] = f[2];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
#pragma unroll
          for (int q = 0; q < 4; ++q) stage[at + 4 * k + q] = (uint8_t)((unsigned)f[k] >> (8 * q));
        }
      }
      off += rec;
    }
    __syncthreads();
    stage_flush<MS_THREADS>(stage, g0, phase, phase + total * rec);      // stage bytes [phase, phase + total * rec) are the chunk
    written += total;
  }
  if (i == (int)gridDim.x - 1 && tid == 0) {
    a.face_count[b] = written;
    if (a.vertex_count) a.vertex_count[b] = vtotal;
  }
}

}  // namespace rdm

using namespace rdm;

extern "C" int64_t rdm_depth_mesh_workspace_bytes(int32_t batch, int32_t h, int32_t w, int32_t step) {
  if (!(frame_shape_ok(batch, h, w) && step > 0)) return 0;
  return (int64_t)batch * 2 * cdiv(h, step) * (int64_t)sizeof(int32_t);
}

extern "C" int rdm_depth_mesh(const float* depth, int32_t batch, int32_t h, int32_t w, double min_depth, double max_depth, int32_t step,
                              double edge_ratio, int32_t layout, uint8_t* faces, int64_t sample_stride_bytes, int32_t* face_count,
                              int32_t* vertex_count, void* workspace, int64_t workspace_bytes, rdm_stream_t stream) {
  RDM_CHECK_ARG(depth, "depth_mesh: depth must not be NULL");
  RDM_CHECK_ARG(faces, "depth_mesh: faces must not be NULL");
  RDM_CHECK_ARG(face_count, "depth_mesh: face_count must not be NULL");
  if (const int rc = check_frame_shape("depth_mesh", batch, h, w)) return rc;
  RDM_CHECK_ARG(step > 0, "depth_mesh: step must be positive (got %d)", (int)step);
  if (const int rc = check_depth_range("depth_mesh", min_depth, max_depth)) return rc;
  RDM_CHECK_ARG(edge_ratio >= 1, "depth_mesh: edge_ratio must be >= 1 and not NaN (got %g)", edge_ratio);
  RDM_CHECK_ARG(layout == RDM_MESH_FACES_I32 || layout == RDM_MESH_FACES_PLY, "depth_mesh: layout must be 0 (int32 triples) or 1 (PLY face records) (got %d)", (int)layout);
  const int rec = layout == RDM_MESH_FACES_PLY ? 13 : 12;
  const long sh = cdiv(h, step), sw = cdiv(w, step);
  RDM_CHECK_ARG(sample_stride_bytes >= 2 * (sh - 1) * (sw - 1) * rec && sample_stride_bytes <= 0x7fffffffL,
                "depth_mesh: sample_stride_bytes %lld must hold 2 x %ld x %ld faces of %d bytes and stay below 2^31", (long long)sample_stride_bytes, sh - 1, sw - 1, rec);
  const int64_t need = rdm_depth_mesh_workspace_bytes(batch, h, w, step);
  RDM_CHECK_ARG(workspace_bytes >= need, "depth_mesh: workspace_bytes %lld is below the %lld bytes rdm_depth_mesh_workspace_bytes asks for", (long long)workspace_bytes,
                (long long)need);
  RDM_CHECK_ARG(workspace || need == 0, "depth_mesh: workspace must not be NULL (%lld bytes are needed)", (long long)need);
  MsArgs a = {};
  a.depth = depth, a.faces = faces, a.face_count = face_count, a.vertex_count = vertex_count, a.rows = (int32_t*)workspace;
  a.h = h, a.w = w, a.step = step, a.sh = (int)sh, a.sw = (int)sw, a.rec = rec;
  a.stride = sample_stride_bytes;
  a.dmin = min_depth, a.dmax = max_depth, a.ratio = edge_ratio;
  hipLaunchKernelGGL(k_mesh_count, dim3((unsigned)sh, batch), dim3(MS_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  hipLaunchKernelGGL(k_mesh_faces, dim3((unsigned)std::max(sh - 1, 1L), batch), dim3(MS_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
