// Batched evaluation, target and metric side in ONE launch: raw depth (B,1,H,W) + predicted map (B,1,128,128) -> ten metric sums per sample.
// It restates, with the device functions of postproc_dev.h and in the order of the single-purpose kernels, what harness.prepare_target
// (rdm_resize_bicubic_f64 + four ATen mask ops, module.py:68,75-78) -> harness.normalize (rdm_gm_normalize_f64, module.py:145-149) ->
// rdm_depth_metrics_f64 (a memset + a launch with atomics, metrics.py:48-128) compute per sample over eight launches.
//
// Grid (B): one workgroup of 1024 threads per sample, so the geometric mean needs no exchange between workgroups.  Thread (q, v) =
// (tid / 256, tid % 256) owns the 16 pixels v + 256 * (16 q + k): the 64 pixels that thread v of k_gm_normalize sums, split in order among
// four threads.  Targets and their logarithms stay in registers; the four threads of a column chain their partial sums through LDS in the
// order q = 0..3, which is k_gm_normalize's order of additions, and the 256 column sums are reduced as its workgroup reduces them: gm and
// the normalised target are bit-identical to the composed path.  The metric sums meet in LDS in a fixed order and leave with plain stores:
// no atomics, no memset, a repeated call gives the same bits.
#include "rdm_common.h"
#include "postproc_dev.h"

namespace rdm {

constexpr int EM_SIDE = 128;                      // module.py:68: the target is compared at 128x128
constexpr int EM_PIX = EM_SIDE * EM_SIDE;
constexpr int EM_THREADS = 1024;
constexpr int EM_COLS = 256;                      // threads of k_gm_normalize, whose summation order is kept
constexpr int EM_Q = EM_THREADS / EM_COLS;        // threads that share one of its columns
constexpr int EM_PER = EM_PIX / EM_THREADS;       // pixels per thread
constexpr int EM_WAVES = EM_THREADS / 64;

// harness.prepare_target on one resized pixel (module.py:75-78): (y * (y > 0)) + ((y <= 0) + 1e-4).  `(y <= 0) + 1e-4` is a FLOAT32 tensor in
// torch (bool + Python scalar), so a valid pixel gets (double)(float)1e-4 and a non-positive one (double)(1.0f + 1e-4f); y * false is +-0.
__device__ __forceinline__ double masked_target(double y) {
#pragma clang fp contract(off)
  const float m2 = (y <= 0 ? 1.0f : 0.0f) + 1e-4f;
  return y * (y > 0 ? 1.0 : 0.0) + (double)m2;
}

template <typename T>
__global__ __launch_bounds__(EM_THREADS) void k_eval_target_metrics(const double* __restrict__ pred, const T* __restrict__ depth, int h, int w,
                                                                    double* __restrict__ rows, double* __restrict__ target_out, double* __restrict__ gm_out,
                                                                    int exp_pred, double e) {
  __shared__ double sh[EM_COLS / 64];
  __shared__ double part[EM_COLS];
  __shared__ double red[10][EM_WAVES];
  const int tid = threadIdx.x, v = tid & (EM_COLS - 1), q = tid / EM_COLS, b = blockIdx.x;
  const T* src = depth + (long)b * h * w;

  // 1. resize (k_resize_bicubic), mask (prepare_target), log
  double t[EM_PER], lg[EM_PER];
#pragma unroll
  for (int k = 0; k < EM_PER; ++k) {
    const int i = v + EM_COLS * (EM_PER * q + k);
    t[k] = masked_target(bicubic_at(src, h, w, EM_SIDE, EM_SIDE, i / EM_SIDE, i % EM_SIDE));
    lg[k] = log(t[k]);
  }

  // 2. geometric mean in k_gm_normalize's order: column v adds its 64 logarithms front to back (thread q continues thread q-1's sum), then
  //    the 256 column sums are reduced like a workgroup of four wavefronts
  for (int ph = 0; ph < EM_Q; ++ph) {
    if (q == ph) {
      double acc = ph == 0 ? 0.0 : part[v];
#pragma unroll
      for (int k = 0; k < EM_PER; ++k) acc += lg[k];
      part[v] = acc;
    }
    __syncthreads();
  }
  const double gm = exp(e * head_waves_sum_bcast(part[v], sh, EM_COLS / 64));
  if (gm_out && tid == 0) gm_out[b] = gm;

  // 3. normalised target and the ten sums of k_depth_metrics
  const double* pb = pred + (long)b * EM_PIX;
  double* tb = target_out ? target_out + (long)b * EM_PIX : nullptr;
  double acc[10];
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = 0;
#pragma unroll
  for (int k = 0; k < EM_PER; ++k) {
    const int i = v + EM_COLS * (EM_PER * q + k);
    const double tn = t[k] / gm;
    if (tb) tb[i] = tn;
    const double p = pb[i];
    depth_metric_terms(exp_pred ? exp(p) : p, tn, acc);
  }

  // 4. lanes by shuffle, then the sixteen wavefronts in sequence: a fixed order
  const int wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < 10; ++k) {
    double r = acc[k];
    for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
    if ((tid & 63) == 0) red[k][wv] = r;
  }
  __syncthreads();
  if (tid < 10) {
    double r = 0;
    for (int i = 0; i < EM_WAVES; ++i) r += red[tid][i];
    rows[(long)b * 10 + tid] = r;
  }
}

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_eval_target_metrics_f64(const double* pred, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, double* rows,
                                           double* target_out, double* gm_out, int32_t flags, rdm_stream_t stream) {
  RDM_CHECK_ARG(pred && depth && rows, "eval_target_metrics: pred, depth and rows must not be NULL");
  RDM_CHECK_ARG(batch > 0 && h > 0 && w > 0, "eval_target_metrics: need batch, h, w > 0 (got %d, %d, %d)", (int)batch, (int)h, (int)w);
  RDM_CHECK_ARG((long)h * w <= 0x7fffffffL, "eval_target_metrics: a %dx%d depth plane is beyond the kernel's 32-bit pixel index", (int)h, (int)w);
  RDM_CHECK_ARG((flags & ~RDM_EVAL_EXP_PRED) == 0, "eval_target_metrics: unknown flags 0x%x", (unsigned)flags);
  const double e = 1.0 / (double)EM_PIX;                  // harness.normalize: exponent 1 / 128^2
  const int exp_pred = (flags & RDM_EVAL_EXP_PRED) ? 1 : 0;
  if (depth_is_f64)
    hipLaunchKernelGGL(k_eval_target_metrics<double>, dim3(batch), dim3(EM_THREADS), 0, (hipStream_t)stream, pred, (const double*)depth, h, w, rows, target_out,
                       gm_out, exp_pred, e);
  else
    hipLaunchKernelGGL(k_eval_target_metrics<float>, dim3(batch), dim3(EM_THREADS), 0, (hipStream_t)stream, pred, (const float*)depth, h, w, rows, target_out,
                       gm_out, exp_pred, e);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
