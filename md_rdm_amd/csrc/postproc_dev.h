// Device arithmetic of the DORN head and the float64 post-processing, shared by the single-purpose kernels (dorn.hip, postproc.hip) and the
// fused kernels (predict.hip: the predict tail; evalmetrics.hip: the evaluation target + metrics) so that all compute bit for bit the same
// values.  Device code only; not part of the C ABI.
#pragma once
#include "rdm_common.h"
#include "depthout_dev.h"                          // block_sum_bcast

namespace rdm {

// ---------------------------------------------------------------------------------------------
// DORN pair (RDM_Net.py:313-345): clamp in f32, two-way softmax in f64, P = probability of the second logit
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dorn_clamp(float x) { return fminf(fmaxf(x, 1e-8f), 1e4f); }

__device__ __forceinline__ double dorn_pair_prob(float xa, float xb) {
  const double a = (double)dorn_clamp(xa), bb = (double)dorn_clamp(xb);
  const double m = fmax(a, bb);
  const double ea = exp(a - m), eb = exp(bb - m);
  return eb / (ea + eb);
}

// The decision `dorn_pair_prob(xa, xb) > 0.5` without the two f64 exponentials: it equals `clamp(xb) > clamp(xa)`, exactly.
//   b > a:  eb = exp(0) = 1 and ea = exp(a - b) with b - a >= one f32 ulp at 1e-8 = 2^-50, so ea <= 1 - 8 * 2^-53 (the exponential is
//           accurate to 1 ulp: at least 7 ulps below 1), 1 + ea < 2 after rounding and P = 1 / (1 + ea) rounds to a double above 0.5;
//   b < a:  ea = 1, eb <= 1 - 7 * 2^-53 and eb / (1 + eb) <= 0.5 - 1.5 * 2^-52, eight representable doubles below 0.5;
//   b == a: P = 1 / 2 exactly, not above 0.5.
// tests/test_gpu_predict.py holds the two forms against each other on neighbouring floats across the whole clamp range.
__device__ __forceinline__ bool dorn_pair_above_half(float xa, float xb) { return dorn_clamp(xb) > dorn_clamp(xa); }

// ---------------------------------------------------------------------------------------------
// Bicubic resize, BIT-EXACT with the float64 CPU path of the reference's `F.interpolate(mode='bicubic',
// align_corners=False)` (computations.py:308-311; third party: torch 2.10 ATen, UpSampleKernel.cpp
// `cpu_upsample_generic` + UpSample.h `get_cubic_upsample_coefficients` / `guard_index_and_lambda`).
// The exact rounding sequence of that build (which mul+add pairs its compiler contracted into FMAs) was
// pinned against the library itself (oracle/bicubic_aten.c restates it; tests/test_oracle_ops.py holds it
// to the reference-generated fixtures with assert_array_equal, 3 318 further outputs were compared while
// deriving it).  Every operation below is therefore explicit: contraction is OFF, fused steps are fma().
//   real  = fma(scale, i + 0.5, -0.5), scale = in / out
//   index = min((long)floorf((float)real), in - 1)           (float floor, as ATen writes it)
//   t     = min(max(real - index, 0), 1)
//   c2(x) = fma(fma(A, x, -5A), x, 8A) * x - 4A              (outer taps, x = t + 1 and (1 - t) + 1)
//   c1(x) = fma(A + 2, x, -(A + 3)) * x * x + 1              (inner taps, x = t and 1 - t)
//   dot4  = fma(v3, w3, fma(v2, w2, fma(v0, w0, v1 * w1)))   (rows along x first, then the 4 rows along y)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void cubic_coeffs(double t, double (&c)[4]) {
#pragma clang fp contract(off)
  const double A = -0.75;
  const double x2 = 1.0 - t;
  const double xa = t + 1.0, xb = x2 + 1.0;
  c[0] = __builtin_fma(__builtin_fma(A, xa, -5.0 * A), xa, 8.0 * A) * xa - 4.0 * A;
  c[1] = __builtin_fma(A + 2.0, t, -(A + 3.0)) * t * t + 1.0;
  c[2] = __builtin_fma(A + 2.0, x2, -(A + 3.0)) * x2 * x2 + 1.0;
  c[3] = __builtin_fma(__builtin_fma(A, xb, -5.0 * A), xb, 8.0 * A) * xb - 4.0 * A;
}

__device__ __forceinline__ int cubic_index(int i, int n_in, int n_out, double& t) {
#pragma clang fp contract(off)
  const double scale = (double)n_in / (double)n_out;
  const double real = __builtin_fma(scale, (double)i + 0.5, -0.5);
  const long idx = min((long)floorf((float)real), (long)n_in - 1);
  t = fmin(fmax(real - (double)idx, 0.0), 1.0);
  return (int)idx;
}

__device__ __forceinline__ double dot4(const double (&v)[4], const double (&w)[4]) {
#pragma clang fp contract(off)
  double acc = v[1] * w[1];
  acc = __builtin_fma(v[0], w[0], acc);
  acc = __builtin_fma(v[2], w[2], acc);
  return __builtin_fma(v[3], w[3], acc);
}

// cubic_index for an output grid that covers only a VIEW of the source: output sample i of a grid whose samples [v0, v0 + vn) span the n_in
// source samples sits at real = fma(scale, pos, -0.5) with scale = n_in / vn and pos = (i + 0.5) - v0, both formed by the caller.  v0 = 0 and
// vn = n_out make scale and pos the two operands of cubic_index's fma, so the result is cubic_index's bit for bit.  real may lie far outside
// [0, n_in) (a sample outside the view): the float floor is held inside the range of a long before the conversion (a NaN becomes the lower
// end), which changes nothing for a |real| below 2^62; the caller clamps the taps.
__device__ __forceinline__ long cubic_index_view(double scale, double pos, int n_in, double& t) {
#pragma clang fp contract(off)
  const double real = __builtin_fma(scale, pos, -0.5);
  const float fl = fminf(fmaxf(floorf((float)real), -0x1p62f), 0x1p62f);
  const long idx = min((long)fl, (long)n_in - 1);
  t = fmin(fmax(real - (double)idx, 0.0), 1.0);
  return idx;
}

// the 4x4 taps around (iy, ix), border indices clamped: rows along x first, then the 4 rows along y
template <typename T>
__device__ __forceinline__ double bicubic_taps(const T* __restrict__ src, int h, int w, int iy, double ty, int ix, double tx) {
  double cy[4], cx[4], rows[4];
  cubic_coeffs(ty, cy);
  cubic_coeffs(tx, cx);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int y = min(max(iy - 1 + i, 0), h - 1);
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = (double)src[y * w + min(max(ix - 1 + j, 0), w - 1)];
    rows[i] = dot4(v, cx);
  }
  return dot4(rows, cy);
}

// align_corners=False, no antialias, border indices clamped.  T = double, or float widened on load (exact): the arithmetic is float64 either way
template <typename T>
__device__ __forceinline__ double bicubic_at(const T* __restrict__ src, int h, int w, int oh, int ow, int oy, int ox) {
  double ty, tx;
  const int iy = cubic_index(oy, h, oh, ty), ix = cubic_index(ox, w, ow, tx);
  return bicubic_taps(src, h, w, iy, ty, ix, tx);
}

// bicubic_at for an output frame of which the source covers only the view (vy0, vx0, h / sy, w / sx): py = (oy + 0.5) - vy0, px likewise
// (cubic_index_view).  An index below -3 has all four taps on the source's first row / column, as -3 has: held there, the int arithmetic of
// the taps cannot overflow, and t keeps the value formed from the real index.  Outside the view the source's edge is replicated.
template <typename T>
__device__ __forceinline__ double bicubic_at_view(const T* __restrict__ src, int h, int w, double sy, double sx, double py, double px) {
  double ty, tx;
  const long iy = cubic_index_view(sy, py, h, ty), ix = cubic_index_view(sx, px, w, tx);
  return bicubic_taps(src, h, w, (int)max(iy, -3L), ty, (int)max(ix, -3L), tx);
}

// The four taps of one output coordinate, precomputed for a kernel that keeps a row or a column fixed while it walks the other axis: the
// weights and the clamped source offsets (elements, times `stride`).  cubic_axis is bicubic_at's index and taps (viz.hip), cubic_axis_view
// bicubic_at_view's for output sample i of a grid whose view starts at v0 (depthframe.hip); it returns whether the sample's centre lies inside
// the view [v0, v1).  The two index functions stay distinct, as in bicubic_at and bicubic_at_view.
struct CubicAxis {
  double c[4];
  int o[4];
};

__device__ __forceinline__ void cubic_axis_taps(int i0, double t, int n_in, int stride, CubicAxis& ax) {
  cubic_coeffs(t, ax.c);
#pragma unroll
  for (int k = 0; k < 4; ++k) ax.o[k] = min(max(i0 - 1 + k, 0), n_in - 1) * stride;
}

__device__ __forceinline__ void cubic_axis(int i, int n_in, int n_out, int stride, CubicAxis& ax) {
  double t;
  const int i0 = cubic_index(i, n_in, n_out, t);
  cubic_axis_taps(i0, t, n_in, stride, ax);
}

__device__ __forceinline__ bool cubic_axis_view(int i, double scale, double v0, double v1, int n_in, int stride, CubicAxis& ax) {
#pragma clang fp contract(off)
  const double centre = (double)i + 0.5;
  double t;
  const int i0 = (int)max(cubic_index_view(scale, centre - v0, n_in, t), -3L);
  cubic_axis_taps(i0, t, n_in, stride, ax);
  return centre >= v0 && centre < v1;
}

// the sum over the workgroup in a FIXED order, broadcast to every thread: block_sum_bcast (depthout_dev.h), for double with the wavefront count
// from blockDim; postproc.hip, predict.hip, evalmetrics.hip and evalstd.hip depend on its bits
//
// block_sum_bcast of the FIRST `waves` wavefronts of a larger workgroup (every thread calls it; the others' `v` is ignored): the same
// order of additions as block_sum_bcast in a workgroup of `waves` wavefronts, so a wide kernel can restate a narrow kernel's sum bit for bit
__device__ __forceinline__ double head_waves_sum_bcast(double v, double* sh, int waves) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  __syncthreads();
  if (l == 0 && wv < waves) sh[wv] = v;
  __syncthreads();
  double r = 0;
  for (int i = 0; i < waves; ++i) r += sh[i];
  return r;
}

// One pixel of the validation metrics (metrics.py:48-128): skipped unless target > 0, pred clamped to >= 1e-7; acc = the ten sums of
// rdm_depth_metrics_f64 (include/rdm_hip.h)
__device__ __forceinline__ void depth_metric_terms(double pred, double t, double (&acc)[10]) {
  if (!(t > 0)) return;
  const double p = fmax(pred, 1e-7);
  const double r = fmax(p / t, t / p), d = p - t;
  acc[0] += 1;
  acc[1] += r < 1.25 ? 1 : 0;
  acc[2] += r < 1.25 * 1.25 ? 1 : 0;
  acc[3] += r < 1.25 * 1.25 * 1.25 ? 1 : 0;
  acc[4] += d * d;
  acc[5] += fabs(d);
  acc[6] += fabs(log10(p) - log10(t));
  acc[7] += fabs(d) / t;
  acc[8] += d * d / t;
  acc[9] += sqrt(d * d / t);
}

// first element of level k in a packed pyramid [d_0 (1x1) | F_1 (2x2) | ...]
__host__ __device__ __forceinline__ long level_off(int k) { return ((1L << (2 * k)) - 1) / 3; }

// y_hat_k = float(log F_k) * w_k   (single-candidate make_pred: A^T.float() @ w.float())
__device__ __forceinline__ float fine_detail_value(double level, float w) { return (float)log(level) * w; }

}  // namespace rdm
