// Point clouds in ONE launch (include/rdm_cloud.h): a float32 depth frame unprojected through pinhole intrinsics, optional normals from the
// full-resolution +-1 neighbours, optional colour, and the valid sampled pixels compacted IN ORDER into packed records of 12, 15, 24 or 27 bytes -
// the payload of a binary PLY file.  Composed from single operators that is a meshgrid, three multiplies and divides, a mask, a boolean index
// per plane, a cat and a byte view, each with its intermediate.
//
// Grid (split, batch), 256 threads.  A workgroup owns a contiguous run of a sample's sampled pixels.  It first counts the valid sampled pixels
// AHEAD of its run itself (a predicate over a depth plane that sits in L2; float4 loads where step == 1), as every workgroup of depthframe.hip
// recomputes ls_b itself: no workgroup waits for another, there is no look-back, no ticket and no atomic.  Then it walks its run in chunks of one
// sampled pixel per thread: validity, the record in registers, a ballot / popcount scan over the workgroup, the records to an LDS stage, the
// stage to memory (depthout_dev.h's stream-out: aligned 16-byte stores, the ragged head and tail as bytes).  Nothing is read back.
// Validity and the unprojection are depthout_dev.h's, shared with mesh.hip (whose vertex numbers are these records' numbers) and warp.hip.
#include <cmath>

#include "rdm_common.h"
#include "depthout_dev.h"
#include "../../include/rdm_cloud.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int CL_THREADS = 256;
constexpr int CL_MAX_REC = 27;
constexpr int CL_STAGE = (16 + CL_THREADS * CL_MAX_REC + 15) / 16 * 16;      // the residue in front, whole 16-byte units

struct ClArgs {
  const float* depth;
  const uint8_t* rgb;
  uint8_t* records;
  int32_t* count;
  int h, w, step, normals, sw, ns, rec;              // sw: sampled columns; ns = sh * sw sampled pixels of a sample
  long stride;
  double fx, fy, cx, cy, dmin, dmax;
};

__device__ __forceinline__ DepthPoint cl_point(const ClArgs& a, int y, int x, float d) { return depth_unproject(y, x, d, a.fx, a.fy, a.cx, a.cy); }

__device__ __forceinline__ DepthPoint cl_sub(const DepthPoint& u, const DepthPoint& v) {
#pragma clang fp contract(off)
  return {u.x - v.x, u.y - v.y, u.z - v.z};
}

// the difference along one axis from the neighbours at -1 (lo) and +1 (hi); false: neither is valid
__device__ __forceinline__ bool cl_diff(const ClArgs& a, const float* __restrict__ p, const DepthPoint& P, int y, int x, int dy, int dx, DepthPoint& out) {
  const int yl = y - dy, xl = x - dx, yh = y + dy, xh = x + dx;
  float dl = 0.0f, dh = 0.0f;
  bool vl = false, vh = false;
  if (yl >= 0 && xl >= 0) dl = p[yl * a.w + xl], vl = depth_valid(dl, a.dmin, a.dmax);
  if (yh < a.h && xh < a.w) dh = p[yh * a.w + xh], vh = depth_valid(dh, a.dmin, a.dmax);
  if (vl && vh)
    out = cl_sub(cl_point(a, yh, xh, dh), cl_point(a, yl, xl, dl));
  else if (vh)
    out = cl_sub(cl_point(a, yh, xh, dh), P);
  else if (vl)
    out = cl_sub(P, cl_point(a, yl, xl, dl));
  return vl || vh;
}

__device__ __forceinline__ void cl_normal(const ClArgs& a, const float* __restrict__ p, const DepthPoint& P, int y, int x, float n[3]) {
#pragma clang fp contract(off)
  n[0] = n[1] = n[2] = 0.0f;
  DepthPoint da, db;
  const bool ha = cl_diff(a, p, P, y, x, 0, 1, da), hb = cl_diff(a, p, P, y, x, 1, 0, db);
  if (!(ha && hb)) return;
  double nx = db.y * da.z - db.z * da.y;
  double ny = db.z * da.x - db.x * da.z;
  double nz = db.x * da.y - db.y * da.x;
  const double s = (nx * P.x + ny * P.y) + nz * P.z;
  if (s > 0) nx = -nx, ny = -ny, nz = -nz;
  const double l = sqrt((nx * nx + ny * ny) + nz * nz);
  if (!(l > 0.0 && l < (double)INFINITY)) return;
  n[0] = (float)(nx / l), n[1] = (float)(ny / l), n[2] = (float)(nz / l);
}

// valid pixels among the sampled pixels [0, n) of the plane p, in row-major order
__device__ __forceinline__ int cl_count_ahead(const ClArgs& a, const float* __restrict__ p, int n, int* sh) {
  const int tid = threadIdx.x;
  int c = 0;
  if (a.step == 1) {                                 // the first n pixels of the plane: scalars up to a 16-byte boundary, float4, scalars
    const int head = min(n, (int)(((16 - ((uintptr_t)p & 15)) & 15) >> 2));
    if (tid < head) c += depth_valid(p[tid], a.dmin, a.dmax);
    const float4* __restrict__ q = (const float4*)(p + head);
    const int nv = (n - head) >> 2;
    for (int i = tid; i < nv; i += CL_THREADS) {
      const float4 v = q[i];
      c += (int)depth_valid(v.x, a.dmin, a.dmax) + (int)depth_valid(v.y, a.dmin, a.dmax) + (int)depth_valid(v.z, a.dmin, a.dmax) + (int)depth_valid(v.w, a.dmin, a.dmax);
    }
    const int t0 = head + nv * 4;                    // fewer than four are left
    if (t0 + tid < n) c += depth_valid(p[t0 + tid], a.dmin, a.dmax);
  } else {
    for (int i = tid; i < n; i += CL_THREADS) {
      const int ry = i / a.sw, rx = i - ry * a.sw;
      c += depth_valid(p[ry * a.step * a.w + rx * a.step], a.dmin, a.dmax);
    }
  }
  return block_sum_bcast<CL_THREADS / 64>(c, sh);
}

__global__ __launch_bounds__(CL_THREADS) void k_depth_cloud(ClArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[CL_STAGE];
  __shared__ int wsum[CL_THREADS / 64];
  const int b = blockIdx.y, part = blockIdx.x, split = gridDim.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* __restrict__ p = a.depth + (long)b * a.h * a.w;
  const uint8_t* __restrict__ rgb = a.rgb ? a.rgb + (long)b * a.h * a.w * 3 : nullptr;
  uint8_t* __restrict__ out = a.records + (long)b * a.stride;
  const int s0 = (int)((long)part * a.ns / split), s1 = (int)((long)(part + 1) * a.ns / split);
  const int nf = a.normals ? 6 : 3, rec = a.rec;

  int written = cl_count_ahead(a, p, s0, wsum);      // records of this sample in front of the run
  for (int c0 = s0; c0 < s1; c0 += CL_THREADS) {
    const int s = c0 + tid;
    bool ok = false;
    uint32_t r[7] = {0, 0, 0, 0, 0, 0, 0};           // the record: nf float words, then the colour in the low three bytes of word nf
    if (s < s1) {
      const int ry = s / a.sw, rx = s - ry * a.sw, y = ry * a.step, x = rx * a.step, at = y * a.w + x;
      const float d = p[at];
      ok = depth_valid(d, a.dmin, a.dmax);
      if (ok) {
        const DepthPoint P = cl_point(a, y, x, d);
        r[0] = __float_as_uint((float)P.x), r[1] = __float_as_uint((float)P.y), r[2] = __float_as_uint((float)P.z);
        if (a.normals) {
          float n[3];
          cl_normal(a, p, P, y, x, n);
          r[3] = __float_as_uint(n[0]), r[4] = __float_as_uint(n[1]), r[5] = __float_as_uint(n[2]);
        }
        if (rgb) {
          const uint8_t* c = rgb + (long)at * 3;
          const uint32_t col = (uint32_t)c[0] | (uint32_t)c[1] << 8 | (uint32_t)c[2] << 16;
          if (a.normals) r[6] = col; else r[3] = col;
        }
      }
    }
    const unsigned long long votes = __ballot(ok);
    const int rank = __popcll(votes & ((1ull << lane) - 1ull));
    __syncthreads();                                 // the previous chunk's readers of stage and wsum are done
    if (lane == 0) wsum[wv] = __popcll(votes);
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < CL_THREADS / 64; ++i) {
      before += i < wv ? wsum[i] : 0;
      total += wsum[i];
    }
    uint8_t* g0 = out + (long)written * rec;         // where the chunk's first record goes
    const int phase = (int)((uintptr_t)g0 & 15);     // stage byte k is memory byte (g0 - phase) + k
    if (ok) {
      const int off = phase + (before + rank) * rec;
      if ((off & 3) == 0) {
        uint32_t* d = (uint32_t*)(stage + off);
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if (k < nf) d[k] = r[k];
      } else {
#pragma unroll
        for (int k = 0; k < 6; ++k)
          if (k < nf) {
#pragma unroll
            for (int j = 0; j < 4; ++j) stage[off + 4 * k + j] = (uint8_t)(r[k] >> (8 * j));
          }
      }
      if (rgb) {
        const uint32_t col = a.normals ? r[6] : r[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) stage[off + 4 * nf + j] = (uint8_t)(col >> (8 * j));
      }
    }
    __syncthreads();
    stage_flush<CL_THREADS>(stage, g0, phase, phase + total * rec);      // stage bytes [phase, phase + total * rec) are the chunk
    written += total;
  }
  if (part == split - 1 && tid == 0) a.count[b] = written;
}

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_depth_cloud(const float* depth, const uint8_t* rgb, int32_t batch, int32_t h, int32_t w, const double* intr, double min_depth,
                               double max_depth, int32_t step, int32_t normals, uint8_t* records, int64_t sample_stride_bytes, int32_t* count,
                               int32_t split, rdm_stream_t stream) {
  RDM_CHECK_ARG(depth, "depth_cloud: depth must not be NULL");
  RDM_CHECK_ARG(intr, "depth_cloud: intr (fx, fy, cx, cy) must not be NULL");
  RDM_CHECK_ARG(records, "depth_cloud: records must not be NULL");
  RDM_CHECK_ARG(count, "depth_cloud: count must not be NULL");
  if (const int rc = check_frame_shape("depth_cloud", batch, h, w)) return rc;
  RDM_CHECK_ARG(step > 0, "depth_cloud: step must be positive (got %d)", (int)step);
  RDM_CHECK_ARG(normals == 0 || normals == 1, "depth_cloud: normals must be 0 or 1 (got %d)", (int)normals);
  const int rec = 12 + 12 * normals + (rgb ? 3 : 0);
  const long sh = cdiv(h, step), sw = cdiv(w, step);
  RDM_CHECK_ARG(sample_stride_bytes >= sh * sw * rec && sample_stride_bytes <= 0x7fffffffL,
                "depth_cloud: sample_stride_bytes %lld must hold %ld x %ld records of %d bytes and stay below 2^31", (long long)sample_stride_bytes, sh, sw, rec);
  if (const int rc = check_intrinsics("depth_cloud", "intr", intr)) return rc;
  if (const int rc = check_depth_range("depth_cloud", min_depth, max_depth)) return rc;
  RDM_CHECK_ARG(split >= 0, "depth_cloud: split must be >= 0 (got %d)", (int)split);
  ClArgs a = {};
  a.depth = depth, a.rgb = rgb, a.records = records, a.count = count;
  a.h = h, a.w = w, a.step = step, a.normals = normals, a.sw = (int)sw, a.ns = (int)(sh * sw), a.rec = rec;
  a.stride = sample_stride_bytes;
  a.fx = intr[0], a.fy = intr[1], a.cx = intr[2], a.cy = intr[3], a.dmin = min_depth, a.dmax = max_depth;
  // two workgroups per compute unit in all, and runs of at least 512 sampled pixels: every workgroup reads the plane ahead of its run, so more
  // workgroups per sample buy parallelism with re-read L2 traffic; tools/cloud_bench.py compares
  if (split == 0) split = std::max(1, std::min(cdiv(512, batch), cdiv(a.ns, 512)));
  split = std::min<int>(split, a.ns);
  hipLaunchKernelGGL(k_depth_cloud, dim3(split, batch), dim3(CL_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
