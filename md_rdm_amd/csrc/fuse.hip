// Multi-frame depth fusion (include/rdm_fuse.h): depth frames with poses integrated into one TSDF volume, and the volume's zero crossings read
// out as oriented points in cloud.hip's record layout.  Composed from single operators the integration is, PER FRAME, a projection of the whole
// voxel grid, a rounding, a range mask, a gather of depth and colour, a handful of `where`s and a rewrite of every plane: a dozen passes over
// the volume for every frame.
//
//   k_tsdf_integrate  one thread per voxel, 256 consecutive voxels of a row (k, j) per workgroup, so the planes are read and written in whole
//                     lines.  The voxel's T, W and C live in registers while the thread walks the frames IN ORDER: one read and one write of the
//                     volume per call whatever batch is.  The poses are read at uniform addresses (scalar loads); intr and geom are kernel
//                     arguments.  What a voxel costs is the float64 pose, the two divisions of the projection and the divisions of the update per
//                     frame, not its bytes (not profiled).  A voxel no frame touches is not stored to.
//   k_tsdf_count      the crossings of every row (k, j) of nx voxels, summed in a fixed order, one 64-bit entry per row;
//   k_tsdf_scan       ONE workgroup: the exclusive scan of the row table in place, chunk by chunk with a carry, and the total to `count`;
//   k_tsdf_write      one workgroup per row at a time: 256 voxels per chunk, up to three records per voxel ranked by a scan over the workgroup,
//                     laid out in an LDS stage and streamed out (depthout_dev.h's stage_flush: aligned 16-byte stores, ragged ends as bytes).
// Rows start at the scanned offsets, so no workgroup waits for another and nothing is read back.  The grids are capped and looped over: the bytes
// depend on no launch geometry.
#include <cmath>

#include "rdm_common.h"
#include "depthout_dev.h"
#include "../../include/rdm_fuse.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int FU_THREADS = 256;
constexpr int FU_WAVES = FU_THREADS / 64;
constexpr long FU_MAX_GRID = 1L << 20;              // workgroups per launch; the rest of the work is looped over
constexpr int FU_MAX_REC = 27;
constexpr int FU_STAGE = (16 + 3 * FU_THREADS * FU_MAX_REC + 15) / 16 * 16;      // the residue in front, three records per voxel, whole 16-byte units

struct FuVolume {
  int nx, ny, nz;
  double ox, oy, oz, voxel, trunc;
};

struct FuArgs {
  const float* depth;
  const uint8_t* rgb;
  const double* poses;
  float* tsdf;
  float* weight;
  float* color;
  int batch, h, w, pose_stride;
  double fx, fy, cx, cy, dmin, dmax, obs_weight, max_weight;
  FuVolume v;
};

struct FxArgs {
  const float* tsdf;
  const float* weight;
  const float* color;
  uint8_t* records;
  long long* table;                                  // one entry per row (k, j): its crossings, then the crossings ahead of it
  long long* count;
  long long capacity;
  int normals, rec;
  double min_weight;
  FuVolume v;
};

__device__ __forceinline__ bool fu_finite(double v) { return fabs(v) < (double)INFINITY; }      // NaN fails

// nearest pixel along one axis, a half rounding up: false where it is outside [0, n)
__device__ __forceinline__ bool fu_pixel(double u, int n, int& c) {
#pragma clang fp contract(off)
  const double f = floor(u + 0.5);
  if (!(f >= 0.0 && f <= (double)(n - 1))) return false;              // in float64, before the conversion: a huge u is not converted
  c = (int)f;
  return true;
}

// grid: (row, segment of 256 voxels) items, capped
__global__ __launch_bounds__(FU_THREADS) void k_tsdf_integrate(FuArgs a) {
#pragma clang fp contract(off)
  const int per_row = (a.v.nx + FU_THREADS - 1) / FU_THREADS;
  const long rows = (long)a.v.nz * a.v.ny, items = rows * per_row;
  const long np = (long)a.h * a.w;
  const double* __restrict__ poses = a.poses;
  for (long it = blockIdx.x; it < items; it += gridDim.x) {
    const long row = it / per_row;
    const int i = (int)(it - row * per_row) * FU_THREADS + (int)threadIdx.x;
    if (i >= a.v.nx) continue;
    const int k = (int)(row / a.v.ny), j = (int)(row - (long)k * a.v.ny);
    const long at = row * a.v.nx + i;                // < 2^31: inside the planes
    const double Px = a.v.ox + (double)i * a.v.voxel, Py = a.v.oy + (double)j * a.v.voxel, Pz = a.v.oz + (double)k * a.v.voxel;
    float T = a.tsdf[at], W = a.weight[at], C[3] = {0.0f, 0.0f, 0.0f};
    if (a.color) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) C[ch] = a.color[at * 3 + ch];
    }
    bool touched = false;
    for (int b = 0; b < a.batch; ++b) {
      const double* __restrict__ R = poses + (long)b * a.pose_stride;          // uniform over the workgroup
      const double Qz = ((R[8] * Px + R[9] * Py) + R[10] * Pz) + R[11];
      if (!(fu_finite(Qz) && Qz > 0.0)) continue;
      const double Qx = ((R[0] * Px + R[1] * Py) + R[2] * Pz) + R[3];
      const double Qy = ((R[4] * Px + R[5] * Py) + R[6] * Pz) + R[7];
      const double u = (a.fx * Qx) / Qz + a.cx;
      const double v = (a.fy * Qy) / Qz + a.cy;
      if (!(fu_finite(u) && fu_finite(v))) continue;
      int c, r;
      if (!fu_pixel(u, a.w, c) || !fu_pixel(v, a.h, r)) continue;
      const long px = (long)b * np + (long)r * a.w + c;                        // 0 <= r < h, 0 <= c < w: inside frame b
      const float d = a.depth[px];
      if (!depth_valid(d, a.dmin, a.dmax)) continue;                           // depthout_dev.h: the pixels cloud.hip keeps
      const double sdf = (double)d - Qz;
      if (sdf < -a.v.trunc) continue;
      double s = sdf / a.v.trunc;
      if (s > 1.0) s = 1.0;
      const double Wd = (double)W, den = Wd + a.obs_weight;
      T = (float)((Wd * (double)T + a.obs_weight * s) / den);
      if (a.color) {
        const uint8_t* q = a.rgb + px * 3;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) C[ch] = (float)((Wd * (double)C[ch] + a.obs_weight * (double)q[ch]) / den);
      }
      W = (float)(den > a.max_weight ? a.max_weight : den);
      touched = true;
    }
    if (touched) {
      a.tsdf[at] = T;
      a.weight[at] = W;
      if (a.color) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) a.color[at * 3 + ch] = C[ch];
      }
    }
  }
}

// ---- extraction ------------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool fx_observed(const FxArgs& a, long at) {
  const float T = a.tsdf[at];
  return fabsf(T) < INFINITY && (double)a.weight[at] >= a.min_weight;          // NaN fails both
}

__device__ __forceinline__ bool fx_cross(float T0, float T1) { return fabsf(T0) < 1.0f && fabsf(T1) < 1.0f && ((T0 < 0.0f) != (T1 < 0.0f)); }

// the edges of voxel (k, j, i) that cross, bit 0: +x, 1: +y, 2: +z; `at` its index
__device__ __forceinline__ int fx_edges(const FxArgs& a, int k, int j, int i, long at) {
  if (!fx_observed(a, at)) return 0;
  const float T0 = a.tsdf[at];
  if (!(fabsf(T0) < 1.0f)) return 0;
  const long sy = a.v.nx, sz = (long)a.v.nx * a.v.ny;
  int m = 0;
  if (i + 1 < a.v.nx && fx_observed(a, at + 1) && fx_cross(T0, a.tsdf[at + 1])) m |= 1;
  if (j + 1 < a.v.ny && fx_observed(a, at + sy) && fx_cross(T0, a.tsdf[at + sy])) m |= 2;
  if (k + 1 < a.v.nz && fx_observed(a, at + sz) && fx_cross(T0, a.tsdf[at + sz])) m |= 4;
  return m;
}

// the gradient of T along one axis at the voxel `at` (index `idx` of `n` along it, `stride` elements apart), from the neighbours that count
__device__ __forceinline__ double fx_diff(const FxArgs& a, long at, int idx, int n, long stride) {
#pragma clang fp contract(off)
  const bool lo = idx > 0 && fx_observed(a, at - stride), hi = idx + 1 < n && fx_observed(a, at + stride);
  const double T = (double)a.tsdf[at];
  if (lo && hi) return ((double)a.tsdf[at + stride] - (double)a.tsdf[at - stride]) * 0.5;
  if (hi) return (double)a.tsdf[at + stride] - T;
  if (lo) return T - (double)a.tsdf[at - stride];
  return 0.0;
}

__device__ __forceinline__ void fx_grad(const FxArgs& a, int k, int j, int i, long at, double g[3]) {
  g[0] = fx_diff(a, at, i, a.v.nx, 1);
  g[1] = fx_diff(a, at, j, a.v.ny, a.v.nx);
  g[2] = fx_diff(a, at, k, a.v.nz, (long)a.v.nx * a.v.ny);
}

__device__ __forceinline__ uint32_t fx_byte(double ch) {
#pragma clang fp contract(off)
  if (ch != ch) return 0;
  const double q = floor(ch + 0.5);
  return q <= 0.0 ? 0u : q >= 255.0 ? 255u : (uint32_t)q;
}

// the record of the crossing on the edge of voxel (k, j, i) along `axis`: nf float words, then the colour in the low three bytes of word nf
__device__ __forceinline__ void fx_record(const FxArgs& a, int k, int j, int i, long at, int axis, uint32_t r[7]) {
#pragma clang fp contract(off)
  const long stride = axis == 0 ? 1 : axis == 1 ? (long)a.v.nx : (long)a.v.nx * a.v.ny;
  const long at1 = at + stride;
  const double T0 = (double)a.tsdf[at], T1 = (double)a.tsdf[at1];
  const double al = T0 / (T0 - T1);
  double p[3] = {a.v.ox + (double)i * a.v.voxel, a.v.oy + (double)j * a.v.voxel, a.v.oz + (double)k * a.v.voxel};
  if (axis == 0) p[0] = a.v.ox + ((double)i + al) * a.v.voxel;
  if (axis == 1) p[1] = a.v.oy + ((double)j + al) * a.v.voxel;
  if (axis == 2) p[2] = a.v.oz + ((double)k + al) * a.v.voxel;
  r[0] = __float_as_uint((float)p[0]), r[1] = __float_as_uint((float)p[1]), r[2] = __float_as_uint((float)p[2]);
  int nf = 3;
  if (a.normals) {
    double g0[3], g1[3], n[3];
    fx_grad(a, k, j, i, at, g0);
    fx_grad(a, k + (axis == 2), j + (axis == 1), i + (axis == 0), at1, g1);
#pragma unroll
    for (int c = 0; c < 3; ++c) n[c] = g0[c] + al * (g1[c] - g0[c]);
    const double l = sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    float f[3] = {0.0f, 0.0f, 0.0f};
    if (l > 0.0 && l < (double)INFINITY) f[0] = (float)(n[0] / l), f[1] = (float)(n[1] / l), f[2] = (float)(n[2] / l);
    r[3] = __float_as_uint(f[0]), r[4] = __float_as_uint(f[1]), r[5] = __float_as_uint(f[2]);
    nf = 6;
  }
  if (a.color) {
    uint32_t col = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double C0 = (double)a.color[at * 3 + c], C1 = (double)a.color[at1 * 3 + c];
      col |= fx_byte(C0 + al * (C1 - C0)) << (8 * c);
    }
    r[nf] = col;
  }
}

// grid: rows, capped
__global__ __launch_bounds__(FU_THREADS) void k_tsdf_count(FxArgs a) {
  __shared__ int sh[FU_WAVES];
  const long rows = (long)a.v.nz * a.v.ny;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = (int)(row / a.v.ny), j = (int)(row - (long)k * a.v.ny);
    int c = 0;
    for (int i = threadIdx.x; i < a.v.nx; i += FU_THREADS) c += __popc(fx_edges(a, k, j, i, row * a.v.nx + i));
    c = block_sum_bcast<FU_WAVES>(c, sh);            // an integer sum in a fixed order; its two barriers also fence sh between rows
    if (threadIdx.x == 0) a.table[row] = c;
  }
}

// the inclusive scan of v over the workgroup -> (v's inclusive prefix, the workgroup's total); sh: FU_WAVES elements, fenced by the barriers here
template <typename T>
__device__ __forceinline__ T fx_block_scan(T v, T* sh, T& total) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 1; o < 64; o <<= 1) {
    const T t = __shfl_up(v, o);
    if (lane >= o) v += t;
  }
  __syncthreads();                                   // the previous readers of sh are done
  if (lane == 63) sh[wv] = v;
  __syncthreads();
  T before = 0;
  total = 0;
  for (int i = 0; i < FU_WAVES; ++i) {
    before += i < wv ? sh[i] : (T)0;
    total += sh[i];
  }
  return before + v;
}

// ONE workgroup
__global__ __launch_bounds__(FU_THREADS) void k_tsdf_scan(long long* __restrict__ table, long rows, long long* __restrict__ count) {
  __shared__ long long sh[FU_WAVES];
  long long carry = 0;
  for (long c0 = 0; c0 < rows; c0 += FU_THREADS) {
    const long at = c0 + threadIdx.x;
    const long long v = at < rows ? table[at] : 0;
    long long total;
    const long long inc = fx_block_scan(v, sh, total);
    if (at < rows) table[at] = carry + (inc - v);
    carry += total;
  }
  if (threadIdx.x == 0) *count = carry;
}

// grid: rows, capped
__global__ __launch_bounds__(FU_THREADS) void k_tsdf_write(FxArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t stage[FU_STAGE];
  __shared__ int sh[FU_WAVES];
  const long rows = (long)a.v.nz * a.v.ny;
  const int nf = a.normals ? 6 : 3, rec = a.rec, tid = threadIdx.x;
  for (long row = blockIdx.x; row < rows; row += gridDim.x) {
    const int k = (int)(row / a.v.ny), j = (int)(row - (long)k * a.v.ny);
    long long written = a.table[row];                // the records in front of the row
    for (int x0 = 0; x0 < a.v.nx && written < a.capacity; x0 += FU_THREADS) {          // uniform over the workgroup
      const int i = x0 + tid;
      const long at = row * a.v.nx + i;
      const int m = i < a.v.nx ? fx_edges(a, k, j, i, at) : 0;
      const int mine = (int)__popc(m);
      int total;
      int ord = fx_block_scan(mine, sh, total) - mine;                   // the voxel's first record within the chunk
      const long long room = a.capacity - written;                       // > 0
      const int keep = (int)(room < (long long)total ? room : (long long)total);
      uint8_t* g0 = a.records + written * rec;       // where the chunk's first record goes
      const int phase = (int)((uintptr_t)g0 & 15);   // stage byte k is memory byte (g0 - phase) + k
      for (int axis = 0; axis < 3; ++axis) {
        if (!(m >> axis & 1)) continue;
        if (ord < keep) {
          uint32_t r[7] = {0, 0, 0, 0, 0, 0, 0};
          fx_record(a, k, j, i, at, axis, r);
          const int off = phase + ord * rec;
          if ((off & 3) == 0) {
            uint32_t* d = (uint32_t*)(stage + off);
#pragma unroll
            for (int q = 0; q < 6; ++q)
              if (q < nf) d[q] = r[q];
          } else {
#pragma unroll
            for (int q = 0; q < 6; ++q)
              if (q < nf) {
#pragma unroll
                for (int b = 0; b < 4; ++b) stage[off + 4 * q + b] = (uint8_t)(r[q] >> (8 * b));
              }
          }
          if (a.color) {
            const uint32_t col = a.normals ? r[6] : r[3];
#pragma unroll
            for (int b = 0; b < 3; ++b) stage[off + 4 * nf + b] = (uint8_t)(col >> (8 * b));
          }
        }
        ++ord;
      }
      __syncthreads();
      stage_flush<FU_THREADS>(stage, g0, phase, phase + keep * rec);      // only [g0, g0 + keep * rec) is stored to
      written += total;
      __syncthreads();                               // the stage is read out before the next chunk fills it
    }
  }
}

static int check_volume(const char* who, int32_t nx, int32_t ny, int32_t nz, const double* geom) {
  RDM_CHECK_ARG(nx > 0 && ny > 0 && nz > 0, "%s: need nx, ny, nz > 0 (got %d, %d, %d)", who, (int)nx, (int)ny, (int)nz);
  RDM_CHECK_ARG((long)nx * ny <= 0x7fffffffL && (long)nx * ny * nz <= 0x7fffffffL, "%s: nx * ny * nz (%d x %d x %d) is beyond the kernel's 32-bit index", who,
                (int)nx, (int)ny, (int)nz);
  RDM_CHECK_ARG(std::isfinite(geom[0]) && std::isfinite(geom[1]) && std::isfinite(geom[2]) && std::isfinite(geom[3]) && std::isfinite(geom[4]) && geom[3] > 0 &&
                    geom[4] > 0,
                "%s: geom (ox %g, oy %g, oz %g, voxel %g, trunc %g) must be finite with voxel and trunc > 0", who, geom[0], geom[1], geom[2], geom[3], geom[4]);
  return RDM_OK;
}

static bool volume_dims_ok(int32_t nx, int32_t ny, int32_t nz) {
  return nx > 0 && ny > 0 && nz > 0 && (long)nx * ny <= 0x7fffffffL && (long)nx * ny * nz <= 0x7fffffffL;
}

static FuVolume volume_of(int32_t nx, int32_t ny, int32_t nz, const double* geom) {
  FuVolume v;
  v.nx = nx, v.ny = ny, v.nz = nz, v.ox = geom[0], v.oy = geom[1], v.oz = geom[2], v.voxel = geom[3], v.trunc = geom[4];
  return v;
}

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_tsdf_integrate(const float* depth, const uint8_t* rgb, int32_t batch, int32_t h, int32_t w, const double* intr, const double* poses,
                                  int32_t pose_stride, double min_depth, double max_depth, double obs_weight, double max_weight, int32_t nx, int32_t ny,
                                  int32_t nz, const double* geom, float* tsdf, float* weight, float* color, rdm_stream_t stream) {
  RDM_CHECK_ARG(depth, "tsdf_integrate: depth must not be NULL");
  RDM_CHECK_ARG(intr, "tsdf_integrate: intr (fx, fy, cx, cy) must not be NULL");
  RDM_CHECK_ARG(poses, "tsdf_integrate: poses must not be NULL");
  RDM_CHECK_ARG(geom, "tsdf_integrate: geom (ox, oy, oz, voxel, trunc) must not be NULL");
  RDM_CHECK_ARG(tsdf, "tsdf_integrate: tsdf must not be NULL");
  RDM_CHECK_ARG(weight, "tsdf_integrate: weight must not be NULL");
  RDM_CHECK_ARG(rgb || !color, "tsdf_integrate: color needs rgb, the frames' colours");
  if (const int rc = check_frame_shape("tsdf_integrate", batch, h, w)) return rc;
  if (const int rc = check_intrinsics("tsdf_integrate", "intr", intr)) return rc;
  if (const int rc = check_depth_range("tsdf_integrate", min_depth, max_depth)) return rc;
  RDM_CHECK_ARG(pose_stride == 0 || pose_stride == 12, "tsdf_integrate: pose_stride must be 0 (one pose) or 12 (one per frame) (got %d)", (int)pose_stride);
  if (const int rc = check_volume("tsdf_integrate", nx, ny, nz, geom)) return rc;
  RDM_CHECK_ARG(std::isfinite(obs_weight) && obs_weight > 0, "tsdf_integrate: obs_weight must be finite and > 0 (got %g)", obs_weight);
  RDM_CHECK_ARG(max_weight >= obs_weight, "tsdf_integrate: max_weight (%g) must not be NaN or below obs_weight (%g)", max_weight, obs_weight);
  FuArgs a = {};
  a.depth = depth, a.rgb = rgb, a.poses = poses, a.tsdf = tsdf, a.weight = weight, a.color = color;
  a.batch = batch, a.h = h, a.w = w, a.pose_stride = pose_stride;
  a.fx = intr[0], a.fy = intr[1], a.cx = intr[2], a.cy = intr[3], a.dmin = min_depth, a.dmax = max_depth, a.obs_weight = obs_weight, a.max_weight = max_weight;
  a.v = volume_of(nx, ny, nz, geom);
  const long items = (long)nz * ny * ((nx + FU_THREADS - 1) / FU_THREADS);
  hipLaunchKernelGGL(k_tsdf_integrate, dim3((unsigned)std::min(items, FU_MAX_GRID)), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" size_t rdm_tsdf_extract_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
  if (!volume_dims_ok(nx, ny, nz)) return 0;
  return (size_t)nz * (size_t)ny * 8;
}

extern "C" int rdm_tsdf_extract(const float* tsdf, const float* weight, const float* color, int32_t nx, int32_t ny, int32_t nz, const double* geom,
                                double min_weight, int32_t normals, uint8_t* records, int64_t capacity, int64_t* count, void* workspace,
                                size_t workspace_bytes, rdm_stream_t stream) {
  RDM_CHECK_ARG(tsdf, "tsdf_extract: tsdf must not be NULL");
  RDM_CHECK_ARG(weight, "tsdf_extract: weight must not be NULL");
  RDM_CHECK_ARG(geom, "tsdf_extract: geom (ox, oy, oz, voxel, trunc) must not be NULL");
  RDM_CHECK_ARG(count, "tsdf_extract: count must not be NULL");
  RDM_CHECK_ARG(workspace, "tsdf_extract: workspace must not be NULL");
  if (const int rc = check_volume("tsdf_extract", nx, ny, nz, geom)) return rc;
  RDM_CHECK_ARG(min_weight == min_weight, "tsdf_extract: min_weight must not be NaN");
  RDM_CHECK_ARG(normals == 0 || normals == 1, "tsdf_extract: normals must be 0 or 1 (got %d)", (int)normals);
  RDM_CHECK_ARG(capacity >= 0, "tsdf_extract: capacity must be >= 0 (got %lld)", (long long)capacity);
  const size_t need = rdm_tsdf_extract_workspace_bytes(nx, ny, nz);
  RDM_CHECK_ARG(workspace_bytes >= need, "tsdf_extract: workspace_bytes %zu is below the %zu bytes rdm_tsdf_extract_workspace_bytes asks for", workspace_bytes, need);
  RDM_CHECK_ARG(((uintptr_t)workspace & 7) == 0, "tsdf_extract: workspace must be 8-byte aligned");
  FxArgs a = {};
  a.tsdf = tsdf, a.weight = weight, a.color = color, a.records = records, a.table = (long long*)workspace, a.count = (long long*)count;
  a.capacity = capacity, a.normals = normals, a.rec = 12 + 12 * normals + (color ? 3 : 0), a.min_weight = min_weight;
  a.v = volume_of(nx, ny, nz, geom);
  const long rows = (long)nz * ny;
  const unsigned grid = (unsigned)std::min(rows, FU_MAX_GRID);
  hipLaunchKernelGGL(k_tsdf_count, dim3(grid), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  hipLaunchKernelGGL(k_tsdf_scan, dim3(1), dim3(FU_THREADS), 0, (hipStream_t)stream, a.table, rows, a.count);
  RDM_LAUNCH_OK();
  if (records && capacity > 0) {
    hipLaunchKernelGGL(k_tsdf_write, dim3(grid), dim3(FU_THREADS), 0, (hipStream_t)stream, a);
    RDM_LAUNCH_OK();
  }
  return RDM_OK;
}
