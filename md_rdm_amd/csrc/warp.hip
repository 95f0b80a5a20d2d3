// A depth frame and its colours seen from another camera (include/rdm_warp.h): a forward warp with a depth test.  Composed from single operators
// that is an unprojection, a matrix product, a projection, a rounding, a range mask, int64 keys, a scatter_reduce("amin") over a full-frame int64
// temporary, a decode, three gathers and a hole fill of shifted views: about a dozen launches.
//
// Three launches:
//   k_warp_init    the batch * th * tw keys of the workspace set to all ones, 8-byte stores, a grid-stride loop;
//   k_warp_splat   one thread per source pixel in row-major order - a wave's 64 lanes are 64 neighbouring columns of a source row, which a
//                  near-identity pose sends to neighbouring target cells, so each atomic wave-instruction covers a nearly contiguous run of
//                  8-byte keys - validity, the float64 point, pose and projection of the header, and for each of the splat^2 cells inside the
//                  target one no-return 64-bit unsigned atomicMin.  min is associative and commutative: the winner is the same for every order of
//                  arrival, so the result is reproducible bit for bit although atomics are used.  (A plain load that skips the atomic where the
//                  stored key is already smaller would not change the result; it was not built or measured.)
//   k_warp_resolve one thread per target cell, 256 consecutive cells of a row per workgroup: the keys of the segment and `fill` cells either side
//                  staged once in LDS, the cell resolved from its own key, an empty cell filled from the nearest keyed cell to its left and right
//                  (at most 2 * fill LDS reads), plain stores, consecutive lanes to consecutive addresses.
// The grids are capped and looped over, so no dimension of a frame meets a grid limit and the bytes depend on no launch geometry.
#include <cmath>

#include "rdm_common.h"
#include "depthout_dev.h"
#include "../../include/rdm_warp.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int WP_THREADS = 256;
constexpr int WP_MAX_FILL = 64;
constexpr int WP_MAX_SPLAT = 4;
constexpr long WP_MAX_GRID = 1L << 20;              // workgroups per sample and launch; the rest of the work is looped over
constexpr unsigned long long WP_EMPTY = 0xFFFFFFFFFFFFFFFFull;

struct WpArgs {
  const float* depth;
  const uint8_t* rgb;
  const double* poses;
  unsigned long long* keys;
  float* depth_out;
  uint8_t* rgb_out;
  int32_t* index_out;
  uint8_t* mask_out;
  int h, w, th, tw, pose_stride, splat, fill;
  double fx, fy, cx, cy, fxd, fyd, cxd, cyd, dmin, dmax;
};

__device__ __forceinline__ bool wp_finite(double v) { return fabs(v) < (double)INFINITY; }      // NaN fails

__global__ __launch_bounds__(WP_THREADS) void k_warp_init(unsigned long long* __restrict__ keys, long n) {
  for (long i = (long)blockIdx.x * WP_THREADS + threadIdx.x; i < n; i += (long)gridDim.x * WP_THREADS) keys[i] = WP_EMPTY;
}

// first cell of a footprint along one axis: false where no cell of [c0, c0 + s) lies in [0, n)
__device__ __forceinline__ bool wp_first(double u, int s, int n, int& c0) {
#pragma clang fp contract(off)
  const double f = floor((u - (double)(s - 1) * 0.5) + 0.5);
  if (!(f >= (double)(1 - s) && f <= (double)(n - 1))) return false;              // in float64, before the conversion: a huge u is not converted
  c0 = (int)f;
  return true;
}

// grid (chunks of 256 source pixels, capped; batch)
__global__ __launch_bounds__(WP_THREADS) void k_warp_splat(WpArgs a) {
#pragma clang fp contract(off)
  const int b = blockIdx.y;
  const long np = (long)a.h * a.w;
  const float* __restrict__ p = a.depth + (long)b * np;
  const double* __restrict__ T = a.poses + (long)b * a.pose_stride;
  unsigned long long* __restrict__ keys = a.keys + (long)b * a.th * a.tw;
  const double r00 = T[0], r01 = T[1], r02 = T[2], t0 = T[3], r10 = T[4], r11 = T[5], r12 = T[6], t1 = T[7], r20 = T[8], r21 = T[9], r22 = T[10], t2 = T[11];
  for (long i = (long)blockIdx.x * WP_THREADS + threadIdx.x; i < np; i += (long)gridDim.x * WP_THREADS) {
    const float d = p[i];
    if (!depth_valid(d, a.dmin, a.dmax)) continue;                     // depthout_dev.h: the pixels and the points of cloud.hip
    const int y = (int)(i / a.w), x = (int)(i - (long)y * a.w);
    const DepthPoint P = depth_unproject(y, x, d, a.fx, a.fy, a.cx, a.cy);
    const double Qx = ((r00 * P.x + r01 * P.y) + r02 * P.z) + t0;
    const double Qy = ((r10 * P.x + r11 * P.y) + r12 * P.z) + t1;
    const double Qz = ((r20 * P.x + r21 * P.y) + r22 * P.z) + t2;
    const float zf = (float)Qz;
    const unsigned zbits = __float_as_uint(zf);
    if (!(wp_finite(Qz) && zbits - 1u < 0x7f7fffffu)) continue;      // zf > 0 and finite, decided on its bits: 1 .. 0x7f7fffff, the smallest denormal included
    const double u = (a.fxd * Qx) / Qz + a.cxd;
    const double v = (a.fyd * Qy) / Qz + a.cyd;
    if (!(wp_finite(u) && wp_finite(v))) continue;
    int c0, r0;
    if (!wp_first(u, a.splat, a.tw, c0) || !wp_first(v, a.splat, a.th, r0)) continue;
    const unsigned long long key = (unsigned long long)zbits << 32 | (unsigned long long)(unsigned)i;
    const int c1 = min(c0 + a.splat, a.tw), r1 = min(r0 + a.splat, a.th);
    for (int r = max(r0, 0); r < r1; ++r)
      for (int c = max(c0, 0); c < c1; ++c) atomicMin(keys + (long)r * a.tw + c, key);      // 0 <= r < th, 0 <= c < tw: inside the sample's keys
  }
}

// grid (segments of 256 cells of a target row, all rows, capped; batch)
__global__ __launch_bounds__(WP_THREADS) void k_warp_resolve(WpArgs a) {
  __shared__ unsigned long long seg[WP_THREADS + 2 * WP_MAX_FILL];
  const int b = blockIdx.y, tid = threadIdx.x, F = a.fill;
  const long nt = (long)a.th * a.tw;
  const unsigned long long* __restrict__ keys = a.keys + (long)b * nt;
  const uint8_t* __restrict__ rgb = a.rgb ? a.rgb + (long)b * a.h * a.w * 3 : nullptr;
  const int per_row = (a.tw + WP_THREADS - 1) / WP_THREADS;
  const long items = (long)a.th * per_row;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const int r = (int)(it / per_row), x0 = (int)(it - (long)r * per_row) * WP_THREADS;
    const unsigned long long* __restrict__ row = keys + (long)r * a.tw;
    __syncthreads();                                 // the previous item's readers of seg are done
    for (int k = tid; k < WP_THREADS + 2 * F; k += WP_THREADS) {      // seg[k] is column x0 - F + k; outside the row: empty
      const int c = x0 - F + k;
      seg[k] = c >= 0 && c < a.tw ? row[c] : WP_EMPTY;
    }
    __syncthreads();
    const int c = x0 + tid;
    if (c < a.tw) {
      unsigned long long key = seg[F + tid];
      uint8_t mask = key != WP_EMPTY ? 1 : 0;
      if (!mask && F > 0) {
        unsigned long long kl = WP_EMPTY, kr = WP_EMPTY;
        for (int k = 1; k <= F && kl == WP_EMPTY; ++k) kl = seg[F + tid - k];
        for (int k = 1; k <= F && kr == WP_EMPTY; ++k) kr = seg[F + tid + k];
        if (kl != WP_EMPTY && kr != WP_EMPTY)
          key = (unsigned)(kr >> 32) > (unsigned)(kl >> 32) ? kr : kl;              // the larger zf (bit order = float order here); a tie: the left
        else
          key = kl != WP_EMPTY ? kl : kr;
        if (key != WP_EMPTY) mask = 2;
      }
      const long at = (long)b * nt + (long)r * a.tw + c;
      const unsigned src = (unsigned)key;
      a.depth_out[at] = mask ? __uint_as_float((unsigned)(key >> 32)) : 0.0f;
      if (a.index_out) a.index_out[at] = mask ? (int)src : -1;
      if (a.mask_out) a.mask_out[at] = mask;
      if (a.rgb_out) {
        uint8_t c0 = 0, c1 = 0, c2 = 0;
        if (mask) {
          const uint8_t* q = rgb + (long)src * 3;
          c0 = q[0], c1 = q[1], c2 = q[2];
        }
        uint8_t* o = a.rgb_out + at * 3;
        o[0] = c0, o[1] = c1, o[2] = c2;
      }
    }
  }
}

}  // namespace rdm

using namespace rdm;

extern "C" size_t rdm_depth_warp_workspace_bytes(int32_t batch, int32_t th, int32_t tw) {
  if (!frame_shape_ok(batch, th, tw)) return 0;
  return (size_t)batch * (size_t)th * (size_t)tw * 8;
}

extern "C" int rdm_depth_warp(const float* depth, const uint8_t* rgb, int32_t batch, int32_t h, int32_t w, const double* intr_src,
                              const double* intr_dst, const double* poses, int32_t pose_stride, double min_depth, double max_depth, int32_t th,
                              int32_t tw, int32_t splat, int32_t fill, float* depth_out, uint8_t* rgb_out, int32_t* index_out, uint8_t* mask_out,
                              void* workspace, size_t workspace_bytes, rdm_stream_t stream) {
  RDM_CHECK_ARG(depth, "depth_warp: depth must not be NULL");
  RDM_CHECK_ARG(intr_src, "depth_warp: intr_src (fx, fy, cx, cy) must not be NULL");
  RDM_CHECK_ARG(intr_dst, "depth_warp: intr_dst (fx, fy, cx, cy) must not be NULL");
  RDM_CHECK_ARG(poses, "depth_warp: poses must not be NULL");
  RDM_CHECK_ARG(depth_out, "depth_warp: depth_out must not be NULL");
  RDM_CHECK_ARG(workspace, "depth_warp: workspace must not be NULL");
  RDM_CHECK_ARG(rgb || !rgb_out, "depth_warp: rgb_out needs rgb, the source frame's colours");
  RDM_CHECK_ARG(batch > 0 && h > 0 && w > 0, "depth_warp: need batch, h, w > 0 (got %d, %d, %d)", (int)batch, (int)h, (int)w);
  RDM_CHECK_ARG(th > 0 && tw > 0, "depth_warp: need th, tw > 0 (got %d, %d)", (int)th, (int)tw);
  RDM_CHECK_ARG(batch <= 65535, "depth_warp: batch %d is beyond the grid limit 65535", (int)batch);
  RDM_CHECK_ARG((long)h * w <= 0x7fffffffL, "depth_warp: h * w (%d x %d) is beyond the key's 32-bit index", (int)h, (int)w);
  RDM_CHECK_ARG((long)th * tw <= 0x7fffffffL, "depth_warp: th * tw (%d x %d) is beyond the kernel's 32-bit index", (int)th, (int)tw);
  RDM_CHECK_ARG(pose_stride == 0 || pose_stride == 12, "depth_warp: pose_stride must be 0 (one pose) or 12 (one per sample) (got %d)", (int)pose_stride);
  RDM_CHECK_ARG(splat >= 1 && splat <= WP_MAX_SPLAT, "depth_warp: splat must be 1..%d (got %d)", WP_MAX_SPLAT, (int)splat);
  RDM_CHECK_ARG(fill >= 0 && fill <= WP_MAX_FILL, "depth_warp: fill must be 0..%d (got %d)", WP_MAX_FILL, (int)fill);
  const size_t need = rdm_depth_warp_workspace_bytes(batch, th, tw);
  RDM_CHECK_ARG(workspace_bytes >= need, "depth_warp: workspace_bytes %zu is below the %zu bytes rdm_depth_warp_workspace_bytes asks for", workspace_bytes, need);
  RDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "depth_warp: workspace must be 8-byte aligned");
  if (const int rc = check_intrinsics("depth_warp", "intr_src", intr_src)) return rc;
  if (const int rc = check_intrinsics("depth_warp", "intr_dst", intr_dst)) return rc;
  if (const int rc = check_depth_range("depth_warp", min_depth, max_depth)) return rc;
  WpArgs a = {};
  a.depth = depth, a.rgb = rgb, a.poses = poses, a.keys = (unsigned long long*)workspace;
  a.depth_out = depth_out, a.rgb_out = rgb_out, a.index_out = index_out, a.mask_out = mask_out;
  a.h = h, a.w = w, a.th = th, a.tw = tw, a.pose_stride = pose_stride, a.splat = splat, a.fill = fill;
  a.fx = intr_src[0], a.fy = intr_src[1], a.cx = intr_src[2], a.cy = intr_src[3];
  a.fxd = intr_dst[0], a.fyd = intr_dst[1], a.cxd = intr_dst[2], a.cyd = intr_dst[3];
  a.dmin = min_depth, a.dmax = max_depth;
  const long nt = (long)th * tw, np = (long)h * w, nkeys = (long)batch * nt;
  const auto blocks = [](long items) { return (unsigned)std::min((items + WP_THREADS - 1) / WP_THREADS, WP_MAX_GRID); };
  hipLaunchKernelGGL(k_warp_init, dim3(blocks(nkeys)), dim3(WP_THREADS), 0, (hipStream_t)stream, a.keys, nkeys);
  RDM_LAUNCH_OK();
  hipLaunchKernelGGL(k_warp_splat, dim3(blocks(np), batch), dim3(WP_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  const long items = (long)th * ((tw + WP_THREADS - 1) / WP_THREADS);
  hipLaunchKernelGGL(k_warp_resolve, dim3((unsigned)std::min(items, WP_MAX_GRID), batch), dim3(WP_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
