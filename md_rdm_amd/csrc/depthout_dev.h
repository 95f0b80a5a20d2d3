// What the kernels that consume or produce a depth frame share (depthframe.hip, refine.hip, cloud.hip, mesh.hip, warp.hip, viz.hip): which depth
// counts as a measurement, the pinhole unprojection, the 16-bit quantiser, the ordered workgroup sum, the stream-out of packed records, the
// wide-or-scalar pixel store and the host checks of a frame's arguments.  Two of them are contracts BETWEEN files and exist once for that
// reason: mesh.hip's vertex numbers are cloud.hip's record numbers only while both decide validity alike, and warp.hip's source points are
// cloud.hip's points only while both unprojections round alike.  Device code is __forceinline__; not part of the C ABI.
#pragma once
#include <cmath>

#include "rdm_common.h"

namespace rdm {

// Validity (include/rdm_cloud.h).  NaN fails d > 0.
// a measurement at all: what refine.hip stages, which has no depth range
__device__ __forceinline__ bool depth_measured(float d) { return d > 0.0f && d < INFINITY; }

// a measurement inside [dmin, dmax]: the pixels cloud.hip numbers, mesh.hip indexes and warp.hip moves
__device__ __forceinline__ bool depth_valid(float d, double dmin, double dmax) { return depth_measured(d) && (double)d >= dmin && (double)d <= dmax; }

// Pinhole unprojection of pixel (y, x) at depth d, float64, one IEEE operation per step: subtract, multiply by Z, divide
struct DepthPoint {
  double x, y, z;
};

__device__ __forceinline__ DepthPoint depth_unproject(int y, int x, float d, double fx, double fy, double cx, double cy) {
#pragma clang fp contract(off)
  DepthPoint p;
  p.z = (double)d;
  p.x = (((double)x - cx) * p.z) / fx;
  p.y = (((double)y - cy) * p.z) / fy;
  return p;
}

// The 16-bit plane of a depth PNG: D / unit in float64, rounded to nearest even, NaN -> 0, saturating at 65535
__device__ __forceinline__ uint16_t depth_quantise(double D, double unit) {
  const double q = D / unit;
  if (q != q) return 0;
  if (q >= 65535.0) return 65535;
  return (uint16_t)(int)rint(q);
}

// The sums of N per-thread values over the workgroup in a FIXED order - lanes by shuffle (32, 16, ... 1), then the wavefronts 0, 1, ... in
// sequence - broadcast to every thread, with one pair of barriers for all N.  WAVES: the workgroup's wavefronts at compile time, or 0 for
// blockDim.x / 64.  sh: N * waves elements; value k of wavefront i sits at sh[k * waves + i].
template <int WAVES>
__device__ __forceinline__ int block_waves() {
  return WAVES > 0 ? WAVES : (int)(blockDim.x >> 6);
}

template <int WAVES = 0, typename T, typename... V>
__device__ __forceinline__ void block_sums_bcast(T* sh, V&... v) {
  for (int o = 32; o > 0; o >>= 1) ((v += __shfl_down(v, o)), ...);
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0) {
    int k = 0;
    ((sh[k++ * block_waves<WAVES>() + wv] = v), ...);
  }
  __syncthreads();
  ((v = 0), ...);
  for (int i = 0; i < block_waves<WAVES>(); ++i) {
    int k = 0;
    ((v += sh[k++ * block_waves<WAVES>() + i]), ...);
  }
}

template <int WAVES = 0, typename T>
__device__ __forceinline__ T block_sum_bcast(T v, T* sh) {
  block_sums_bcast<WAVES>(sh, v);
  return v;
}

// Ordered stream-out of packed records (cloud.hip, mesh.hip).  A chunk's records are laid out in an LDS stage at the output address's own
// residue mod 16 (`phase`): stage byte k is memory byte (g0 - phase) + k, so the chunk leaves as aligned 16-byte stores straight from aligned
// 16-byte LDS reads.  Which record goes where (the ballot / popcount ranking) is the kernel's, and so is putting a record's words into the
// stage (one 32-bit store per word where the offset is a multiple of 4, bytes otherwise): as a shared function that compiled to other code
// in both kernels, and k_depth_cloud's 12-byte records measured up to 1.4 % slower with it.
// stage_flush: stage bytes [phase, end) to g0 - phase (16-byte aligned), by a workgroup of THREADS threads after a barrier: the 16-byte units wholly inside
// as uint4, the ragged head and tail - whose words the previous chunk, the next one or a neighbouring workgroup may own - as bytes.  Only
// [g0, g0 + end - phase) is stored to; nothing is read back.
template <int THREADS>
__device__ __forceinline__ void stage_flush(const uint8_t* stage, uint8_t* g0, int phase, int end) {
  uint8_t* gA = g0 - phase;
  for (int u = threadIdx.x; u < (end + 15) >> 4; u += THREADS) {
    const int lo = u * 16, hi = lo + 16;
    if (lo >= phase && hi <= end) {
      *(uint4*)(gA + lo) = *(const uint4*)(stage + lo);
    } else {
      for (int k = max(lo, phase); k < min(hi, end); ++k) gA[k] = stage[k];
    }
  }
}

// PX adjacent pixels of a plane (float32 or uint16) whose first is column x of a row of w pixels, at d: one store of PX * sizeof(T) bytes
// where the address is aligned to it and the row holds all PX, otherwise - and at the ragged end of a row - scalars.  I: int or unsigned, the
// type the kernel holds its coordinates in, so that what it has already proved about x (refine.hip: x < w, unsigned) still counts here.
template <typename T, int PX, typename I>
__device__ __forceinline__ void store_pixels(T* d, const T (&v)[PX], I x, I w) {
  typedef T Wide __attribute__((ext_vector_type(PX)));
  if (x + PX <= w && ((uintptr_t)d & (sizeof(Wide) - 1)) == 0) {
    Wide t;
#pragma unroll
    for (int p = 0; p < PX; ++p) t[p] = v[p];
    *(Wide*)d = t;
  } else {
#pragma unroll
    for (int p = 0; p < PX; ++p)
      if (x + p < w) d[p] = v[p];
  }
}

// Host: the argument checks every entry point of the family makes.  `who` is the entry point's name, the prefix of the message.
// frame_shape_ok: a (batch, h, w) frame one launch can take - batch is a grid dimension, a pixel's index is 32-bit
static inline bool frame_shape_ok(int32_t batch, int32_t h, int32_t w) { return batch > 0 && h > 0 && w > 0 && batch <= 65535 && (long)h * w <= 0x7fffffffL; }

static inline int check_frame_shape(const char* who, int32_t batch, int32_t h, int32_t w) {
  RDM_CHECK_ARG(batch > 0 && h > 0 && w > 0, "%s: need batch, h, w > 0 (got %d, %d, %d)", who, (int)batch, (int)h, (int)w);
  RDM_CHECK_ARG(batch <= 65535, "%s: batch %d is beyond the grid limit 65535", who, (int)batch);
  RDM_CHECK_ARG(frame_shape_ok(batch, h, w), "%s: h * w (%d x %d) is beyond the kernel's 32-bit index", who, (int)h, (int)w);
  return RDM_OK;
}

// (fx, fy, cx, cy), not NULL; `name` is the argument's
static inline int check_intrinsics(const char* who, const char* name, const double* intr) {
  RDM_CHECK_ARG(std::isfinite(intr[0]) && std::isfinite(intr[1]) && std::isfinite(intr[2]) && std::isfinite(intr[3]) && intr[0] != 0 && intr[1] != 0,
                "%s: %s (fx %g, fy %g, cx %g, cy %g) must be finite with fx and fy not 0", who, name, intr[0], intr[1], intr[2], intr[3]);
  return RDM_OK;
}

static inline int check_depth_range(const char* who, double min_depth, double max_depth) {
  RDM_CHECK_ARG(min_depth >= 0, "%s: min_depth must be >= 0 (got %g)", who, min_depth);
  RDM_CHECK_ARG(max_depth >= min_depth, "%s: max_depth (%g) must not be NaN or below min_depth (%g)", who, max_depth, min_depth);
  return RDM_OK;
}

static inline int check_depth_unit(const char* who, double unit) {
  RDM_CHECK_ARG(std::isfinite(unit) && unit > 0, "%s: unit must be finite and positive (got %g)", who, unit);
  return RDM_OK;
}

}  // namespace rdm
