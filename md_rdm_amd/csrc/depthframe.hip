// Metric depth frames in ONE launch (include/rdm_depth.h): the 128x128 log map resampled over the view of the (h, w) frame (bicubic_at_view's
// arithmetic, postproc_dev.h), shifted by the sample's log scale - the mean SID log depth of its DORN counts plus the caller's own - then
// exp, the float32 plane and the quantised 16-bit plane of a depth PNG.  Composed from single operators that is a resize to a float64
// (batch,h,w) intermediate, an add, an exp, a cast, a divide and a round with clamp.
//
// Grid (split, batch), one workgroup of 64..256 threads (the quads of a row, rounded up to whole wavefronts) per share of a sample's rows.  Every
// workgroup sums the sample's counts itself (an integer sum: exact in any order; block_sum_bcast's fixed order all the same), so no workgroup
// waits for another.  A thread owns FOUR adjacent columns (a quad) at a time and walks down the workgroup's rows: its column taps and weights stay
// in registers; the row taps of a chunk of DF_ROWS rows are computed once by a few threads and shared through LDS.  Along x first, then along
// y, as bicubic_taps does: the four x-interpolated map rows of a pixel depend on the output row only through WHICH map rows they are, and
// an enlarged frame keeps them for several output rows (480 rows over 128: three to four), so they are kept and recomputed - with the same
// operations, hence the same bits - only when the row taps move.  What is then left per pixel is one dot4, the add, the float64 exp and the
// two conversions.  The map itself (128 KiB per sample) is read through the caches: 16 loads per pixel when the taps move, none otherwise.
// Stores (depthout_dev.h's store_pixels): the quad's float32 as one 16-byte store and its uint16 as one 8-byte store where the address is
// aligned (always, for a w that is a multiple of 4 in an aligned allocation), otherwise and at the ragged end of a row as scalars.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "rdm_common.h"
#include "postproc_dev.h"
#include "../../include/rdm_anchor.h"               // rdm_depth.h and the corrected call

namespace rdm {

constexpr int DF_THREADS = 256;
constexpr int DF_ROWS = 32;                         // rows per chunk: one LDS table of row taps
constexpr int DF_SIDE = 128;
constexpr int DF_PX = 4;                            // adjacent pixels per thread

struct DfArgs {
  const double* map;
  const int64_t* counts;
  const double* log_scale;
  int count_n, h, w, outside;
  double A, Bc, K, offset;                          // S_b = A + Bc * (sum / count_n + offset) / K
  double sy, sx, vy0, vx0, vy1, vx1;                // 128 / vh, 128 / vw; the view [vy0, vy1) x [vx0, vx1), vy1 = vy0 + vh
  double unit;
  float* f32;
  uint16_t* u16;
  double* scale_out;
};

// rdm_depth_frames_corrected (include/rdm_anchor.h): the same kernel with a correction field, bilinear between the cell centres, added in the
// log domain.  A type of its own, so that the plain call's kernel argument - and with it its code - stays what it was.
struct DfFieldArgs : DfArgs {
  const double* field;
  int gy, gx, cell;
};

struct DfLerp {                          // one output coordinate between two cells of the field: the clamped cell indices and the weight of the second
  double t;
  int i0, i1;
};

__device__ __forceinline__ void df_lerp_axis(int i, int cell, int n, DfLerp& l) {
#pragma clang fp contract(off)
  double u = ((double)i + 0.5) / (double)cell;
  u = u - 0.5;
  const double f = floor(u);                         // >= -1 and < n: the conversion is exact
  l.t = u - f;
  l.i0 = min(max((int)f, 0), n - 1);
  l.i1 = min(max((int)f + 1, 0), n - 1);
}

struct DfTaps : CubicAxis {             // the taps of one output coordinate (postproc_dev.h) and whether its centre is inside the view
  int inside, pad;
};

__device__ __forceinline__ double df_log_scale(const DfArgs& a, int b, long long* sh) {
#pragma clang fp contract(off)
  double S = 0.0;
  if (a.counts) {                                    // uniform over the grid
    const int64_t* c = a.counts + (long)b * a.count_n;
    long long s = 0;
    for (int i = threadIdx.x; i < a.count_n; i += blockDim.x) s += c[i];
    s = block_sum_bcast(s, sh);
    double x = (double)s / (double)a.count_n;
    x = x + a.offset;
    x = a.Bc * x;
    x = x / a.K;
    S = a.A + x;
  }
  return S + (a.log_scale ? a.log_scale[b] : 0.0);
}

template <class Args>
__global__ __launch_bounds__(DF_THREADS) void k_depth_frames(Args a) {
  constexpr bool FIELD = std::is_same<Args, DfFieldArgs>::value;
  __shared__ DfTaps rowtab[DF_ROWS];
  __shared__ DfLerp rowlerp[FIELD ? DF_ROWS : 1];
  __shared__ long long red[DF_THREADS / 64];
  const int b = blockIdx.y, part = blockIdx.x, split = gridDim.x, tid = threadIdx.x;
  const int h = a.h, w = a.w;

  const double ls = df_log_scale(a, b, red);
  if (part == 0 && tid == 0 && a.scale_out) a.scale_out[b] = ls;

  const double* __restrict__ map = a.map + (long)b * DF_SIDE * DF_SIDE;
  float* __restrict__ f32 = a.f32 ? a.f32 + (long)b * h * w : nullptr;
  uint16_t* __restrict__ u16 = a.u16 ? a.u16 + (long)b * h * w : nullptr;
  const bool edge = a.outside != 0;
  const int r0 = (int)((long)part * h / split), r1 = (int)((long)(part + 1) * h / split);
  const int quads = (w + DF_PX - 1) / DF_PX;

  for (int rc = r0; rc < r1; rc += DF_ROWS) {
    const int nr = min(DF_ROWS, r1 - rc);
    __syncthreads();                                 // the previous chunk's readers of rowtab are done
    if (tid < nr) rowtab[tid].inside = cubic_axis_view(rc + tid, a.sy, a.vy0, a.vy1, DF_SIDE, DF_SIDE, rowtab[tid]);
    if constexpr (FIELD)
      if (tid < nr) df_lerp_axis(rc + tid, a.cell, a.gy, rowlerp[tid]);
    __syncthreads();
    for (int q = tid; q < quads; q += blockDim.x) {
      const int x0 = q * DF_PX;
      DfTaps cx[DF_PX];                              // columns past the end of a ragged row get taps too (clamped: valid reads), and are not stored
#pragma unroll
      for (int p = 0; p < DF_PX; ++p) cx[p].inside = cubic_axis_view(x0 + p, a.sx, a.vx0, a.vx1, DF_SIDE, 1, cx[p]);
      DfLerp lx[FIELD ? DF_PX : 1];
      if constexpr (FIELD) {
#pragma unroll
        for (int p = 0; p < DF_PX; ++p) df_lerp_axis(min(x0 + p, w - 1), a.cell, a.gx, lx[p]);
      }
      double hrow[DF_PX][4];                         // the x-interpolated map rows ro[0..3] of the quad's pixels
      int ro[4] = {-1, -1, -1, -1};
      for (int r = 0; r < nr; ++r) {
        const DfTaps ry = rowtab[r];
        const int y = rc + r;
        float vf[DF_PX];
        uint16_t vu[DF_PX];
        if (edge || ry.inside) {
          if (ry.o[0] != ro[0] || ry.o[1] != ro[1] || ry.o[2] != ro[2] || ry.o[3] != ro[3]) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              ro[i] = ry.o[i];
#pragma unroll
              for (int p = 0; p < DF_PX; ++p) {
                double v[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) v[j] = map[ry.o[i] + cx[p].o[j]];
                hrow[p][i] = dot4(v, cx[p].c);
              }
            }
          }
#pragma unroll
          for (int p = 0; p < DF_PX; ++p) {
            if (edge || cx[p].inside) {
              double e = dot4(hrow[p], ry.c) + ls;
              if constexpr (FIELD) {
                const DfLerp ly = rowlerp[r];
                const double* __restrict__ f0 = a.field + ((long)b * a.gy + ly.i0) * a.gx;
                const double* __restrict__ f1 = a.field + ((long)b * a.gy + ly.i1) * a.gx;
                const double a0 = f0[lx[p].i0], a1 = f1[lx[p].i0];
                const double top = __builtin_fma(lx[p].t, f0[lx[p].i1] - a0, a0), bot = __builtin_fma(lx[p].t, f1[lx[p].i1] - a1, a1);
                e = e + __builtin_fma(ly.t, bot - top, top);
              }
              const double D = exp(e);
              vf[p] = (float)D;
              vu[p] = depth_quantise(D, a.unit);
            } else {
              vf[p] = 0.0f, vu[p] = 0;
            }
          }
        } else {
#pragma unroll
          for (int p = 0; p < DF_PX; ++p) vf[p] = 0.0f, vu[p] = 0;
        }
        const long at = (long)y * w + x0;
        if (f32) store_pixels(f32 + at, vf, x0, w);
        if (u16) store_pixels(u16 + at, vu, x0, w);
      }
    }
  }
}

}  // namespace rdm

using namespace rdm;

// the checks and the launch of both entry points; A: DfArgs, or DfFieldArgs with its own members already set and checked
template <class A>
static int depth_frames_launch(A a, const double* log_map, const int64_t* counts, int32_t count_n, const double* log_scale, const double* sid, int32_t batch,
                               int32_t h, int32_t w, const double* view, int32_t outside, double unit, float* depth_f32, uint16_t* depth_u16,
                               double* scale_out, int32_t split, rdm_stream_t stream) {
  RDM_CHECK_ARG(log_map, "depth_frames: log_map must not be NULL");
  RDM_CHECK_ARG(depth_f32 || depth_u16, "depth_frames: depth_f32 and depth_u16 must not both be NULL");
  if (const int rc = check_frame_shape("depth_frames", batch, h, w)) return rc;
  RDM_CHECK_ARG(!counts || count_n >= 1, "depth_frames: counts need count_n >= 1 (got %d)", (int)count_n);
  RDM_CHECK_ARG(!counts || sid, "depth_frames: counts need sid (alpha, beta, K, offset)");
  if (counts) {
    RDM_CHECK_ARG(std::isfinite(sid[0]) && std::isfinite(sid[1]) && std::isfinite(sid[2]) && std::isfinite(sid[3]) && sid[0] > 0 && sid[1] > sid[0] && sid[2] > 0,
                  "depth_frames: sid (alpha %g, beta %g, K %g, offset %g) must be finite with 0 < alpha < beta and K > 0", sid[0], sid[1], sid[2], sid[3]);
    a.A = std::log(sid[0]), a.Bc = std::log(sid[1] / sid[0]), a.K = sid[2], a.offset = sid[3];
  }
  if (const int rc = check_depth_unit("depth_frames", unit)) return rc;
  RDM_CHECK_ARG(outside == 0 || outside == 1, "depth_frames: outside must be 0 (invalid) or 1 (replicated edge) (got %d)", (int)outside);
  RDM_CHECK_ARG(split >= 0, "depth_frames: split must be >= 0 (got %d)", (int)split);
  RDM_CHECK_ARG(!view || (std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2]) && std::isfinite(view[3]) && view[2] > 0 && view[3] > 0),
                "depth_frames: view (%g, %g, %g, %g) must be finite with vh > 0 and vw > 0", view ? view[0] : 0.0, view ? view[1] : 0.0, view ? view[2] : 0.0,
                view ? view[3] : 0.0);
  const double vy0 = view ? view[0] : 0.0, vx0 = view ? view[1] : 0.0, vh = view ? view[2] : (double)h, vw = view ? view[3] : (double)w;
  a.map = log_map, a.counts = counts, a.log_scale = log_scale;
  a.count_n = count_n, a.h = h, a.w = w, a.outside = outside;
  a.sy = (double)DF_SIDE / vh, a.sx = (double)DF_SIDE / vw, a.vy0 = vy0, a.vx0 = vx0, a.vy1 = vy0 + vh, a.vx1 = vx0 + vw;
  a.unit = unit, a.f32 = depth_f32, a.u16 = depth_u16, a.scale_out = scale_out;
  if (split == 0) split = cdiv(1024, batch);            // four workgroups per compute unit in all; tools/depthframe_bench.py compares
  split = std::min<int>(split, h);
  const int quads = cdiv(w, DF_PX);
  const int threads = std::min(DF_THREADS, std::max(64, cdiv(quads, 64) * 64));
  hipLaunchKernelGGL(k_depth_frames<A>, dim3(split, batch), dim3(threads), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_depth_frames(const double* log_map, const int64_t* counts, int32_t count_n, const double* log_scale, const double* sid, int32_t batch,
                                int32_t h, int32_t w, const double* view, int32_t outside, double unit, float* depth_f32, uint16_t* depth_u16,
                                double* scale_out, int32_t split, rdm_stream_t stream) {
  return depth_frames_launch(DfArgs{}, log_map, counts, count_n, log_scale, sid, batch, h, w, view, outside, unit, depth_f32, depth_u16, scale_out, split, stream);
}

extern "C" int rdm_depth_frames_corrected(const double* log_map, const int64_t* counts, int32_t count_n, const double* log_scale, const double* sid,
                                          int32_t batch, int32_t h, int32_t w, const double* view, int32_t outside, double unit, float* depth_f32,
                                          uint16_t* depth_u16, double* scale_out, int32_t split, const double* field, int32_t gy, int32_t gx, int32_t cell,
                                          rdm_stream_t stream) {
  RDM_CHECK_ARG(field && ((uintptr_t)field & 7) == 0, "depth_frames: field must not be NULL and must be 8-byte aligned");
  RDM_CHECK_ARG(cell >= 1, "depth_frames: cell must be >= 1 (got %d)", (int)cell);
  RDM_CHECK_ARG(h <= 0 || w <= 0 || (gy == cdiv(h, cell) && gx == cdiv(w, cell)), "depth_frames: the field's gy x gx (%d x %d) is not ceil(h / cell) x ceil(w / cell) (%d x %d)",
                (int)gy, (int)gx, cdiv(std::max(h, 1), cell), cdiv(std::max(w, 1), cell));
  DfFieldArgs a = {};
  a.field = field, a.gy = gy, a.gx = gx, a.cell = cell;
  return depth_frames_launch(a, log_map, counts, count_n, log_scale, sid, batch, h, w, view, outside, unit, depth_f32, depth_u16, scale_out, split, stream);
}
