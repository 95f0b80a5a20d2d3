// Optimiser-side gradient kernels (include/rdm_optim.h), all HBM-bound sweeps over ranges of the flat gradient buffer:
//   k_grad_accumulate  acc = g / acc += g between the micro-batches of an accumulation window (and g += acc when the window closes)
//   k_grad_sumsq       sum g^2 of a range in float64, a partial per workgroup; k_grad_sumsq_final adds the partials in workgroup order
//   k_adamw_clip       k_adamw with clip_grad_norm_'s coefficient folded into the gradient scale: every thread forms it from the few slots
//   k_adamw_ema        either step with the weight average advanced in the same sweep; k_ema_swap exchanges two buffers (include/rdm_ema.h)
// Plain global loads and stores throughout (no buffer-descriptor stores with a scalar offset: rdm_common.h), no floating-point atomics, no
// counter shared between workgroups: the partials cross from the first launch to the second through the launch boundary.
#include <math.h>
#include <algorithm>
#include "rdm_common.h"
#include "adamw_dev.h"
#include "../../include/rdm_optim.h"
#include "../../include/rdm_ema.h"

namespace rdm {

constexpr int OPT_THREADS = 256;
constexpr int OPT_WAVES = OPT_THREADS / 64;
constexpr int ACC_MAX_BLOCKS = 2048;              // one trip covers 2048 x 256 quads, as k_adamw's grid
constexpr int SUMSQ_MAX_BLOCKS = 1024;            // partials the one-workgroup second launch adds: 4 per thread

static inline int sweep_grid(long n4, int cap) { return (int)std::min<long>(std::max<long>(cdiv(n4, OPT_THREADS), 1), cap); }

template <int MODE>
__global__ __launch_bounds__(OPT_THREADS) void k_grad_accumulate(float* __restrict__ dst, const float* __restrict__ src, long n4, long n) {
  for (long i = (long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_THREADS) {
    float4 s = *reinterpret_cast<const float4*>(src + i * 4);
    if (MODE == RDM_GRAD_ACC_ADD) {
      const float4 d = *reinterpret_cast<const float4*>(dst + i * 4);
      s.x = d.x + s.x; s.y = d.y + s.y; s.z = d.z + s.z; s.w = d.w + s.w;
    }
    *reinterpret_cast<float4*>(dst + i * 4) = s;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                      // tail (n not a multiple of 4)
    const long i = n4 * 4 + threadIdx.x;
    dst[i] = MODE == RDM_GRAD_ACC_ADD ? dst[i] + src[i] : src[i];
  }
}

// the workgroup's sum of one double per thread, in a fixed order: lanes by shuffle, wavefronts in sequence; valid on thread 0
__device__ __forceinline__ double opt_block_sum(double r, double* wave_sum) {
  for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
  if ((threadIdx.x & 63) == 0) wave_sum[threadIdx.x >> 6] = r;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0)
    for (int w = 0; w < OPT_WAVES; ++w) t += wave_sum[w];
  return t;
}

__global__ __launch_bounds__(OPT_THREADS) void k_grad_sumsq(const float* __restrict__ g, long n4, long n, double* __restrict__ partial) {
  __shared__ double wave_sum[OPT_WAVES];
  double acc = 0.0;
  for (long i = (long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_THREADS) {
    const float4 v = *reinterpret_cast<const float4*>(g + i * 4);
    acc += (double)v.x * (double)v.x;
    acc += (double)v.y * (double)v.y;
    acc += (double)v.z * (double)v.z;
    acc += (double)v.w * (double)v.w;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                      // the tail holds the highest indices: added last
    const double x = (double)g[n4 * 4 + threadIdx.x];
    acc += x * x;
  }
  const double t = opt_block_sum(acc, wave_sum);
  if (threadIdx.x == 0) partial[blockIdx.x] = t;
}

// one workgroup: thread t adds the partials [t per, (t + 1) per) by rising index, then the fixed combine above
__global__ __launch_bounds__(OPT_THREADS) void k_grad_sumsq_final(const double* __restrict__ partial, int count, double* __restrict__ out) {
  __shared__ double wave_sum[OPT_WAVES];
  const int per = (count + OPT_THREADS - 1) / OPT_THREADS;
  double acc = 0.0;
  for (int k = 0; k < per; ++k) {
    const int i = (int)threadIdx.x * per + k;
    if (i < count) acc += partial[i];
  }
  const double t = opt_block_sum(acc, wave_sum);
  if (threadIdx.x == 0) *out = t;
}

// clip_grad_norm_'s coefficient for the gradient scaled by gscale, from the slots of squared norms (rdm_optim.h states the arithmetic)
__device__ __forceinline__ float clip_coef(const double* __restrict__ sumsq, int n_slots, float max_norm, float gscale) {
#pragma clang fp contract(off)
  double total = sumsq[0];
  for (int i = 1; i < n_slots; ++i) total += sumsq[i];
  const double q = (double)max_norm / (sqrt(total) * fabs((double)gscale) + 1e-6);
  return (float)(q > 1.0 ? 1.0 : q);
}

__global__ __launch_bounds__(256) void k_adamw_clip(float* p, const float* g, float* m, float* v, long n4, long n, float lr, float b1, float b2,
                                                    float eps, float wd, float bc1, float rsqrt_bc2, float gscale, const double* sumsq, int n_slots,
                                                    float max_norm, float* coef_out) {
  const float c = clip_coef(sumsq, n_slots, max_norm, gscale);
  if (coef_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *coef_out = c;
  adamw_sweep(p, g, m, v, n4, n, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale * c);
}

// the plain (CLIP false: sumsq, n_slots, max_norm and coef_out unused) or the clipped step, and the average e in the same sweep
template <bool CLIP>
__global__ __launch_bounds__(256) void k_adamw_ema(float* p, const float* g, float* m, float* v, float* e, long n4, long n, float lr, float b1,
                                                   float b2, float eps, float wd, float bc1, float rsqrt_bc2, float gscale, const double* sumsq,
                                                   int n_slots, float max_norm, float* coef_out, float omd) {
  if (CLIP) {
    const float c = clip_coef(sumsq, n_slots, max_norm, gscale);
    if (coef_out != nullptr && blockIdx.x == 0 && threadIdx.x == 0) *coef_out = c;
    adamw_sweep_ema(p, g, m, v, e, n4, n, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale * c, omd);
  } else {
    adamw_sweep_ema(p, g, m, v, e, n4, n, lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale, omd);
  }
}

// a <-> b: a quad (and a tail element) is read and written by the one thread that owns it
__global__ __launch_bounds__(OPT_THREADS) void k_ema_swap(float* __restrict__ a, float* __restrict__ b, long n4, long n) {
  for (long i = (long)blockIdx.x * OPT_THREADS + threadIdx.x; i < n4; i += (long)gridDim.x * OPT_THREADS) {
    const float4 x = *reinterpret_cast<const float4*>(a + i * 4), y = *reinterpret_cast<const float4*>(b + i * 4);
    *reinterpret_cast<float4*>(a + i * 4) = y;
    *reinterpret_cast<float4*>(b + i * 4) = x;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                      // tail (n not a multiple of 4)
    const long i = n4 * 4 + threadIdx.x;
    const float x = a[i], y = b[i];
    a[i] = y;
    b[i] = x;
  }
}

// do the n-element float ranges at x and y share a byte?
static inline bool ranges_overlap(const float* x, const float* y, int64_t n) {
  const uintptr_t a = (uintptr_t)x, b = (uintptr_t)y, bytes = (uintptr_t)n * 4;
  return a < b + bytes && b < a + bytes;
}

}  // namespace rdm

using namespace rdm;

static int sumsq_blocks(int64_t n) { return sweep_grid(n / 4, SUMSQ_MAX_BLOCKS); }

extern "C" int rdm_grad_accumulate_f32(float* dst, const float* src, int64_t n, int32_t mode, rdm_stream_t stream) {
  RDM_CHECK_ARG(dst && src, "grad_accumulate: dst and src must not be NULL");
  RDM_CHECK_ARG((((uintptr_t)dst | (uintptr_t)src) & 15) == 0, "grad_accumulate: buffers must be 16-byte aligned");
  RDM_CHECK_ARG(n >= 0, "grad_accumulate: n = %lld is negative", (long long)n);
  RDM_CHECK_ARG(mode == RDM_GRAD_ACC_COPY || mode == RDM_GRAD_ACC_ADD, "grad_accumulate: unknown mode %d (0 copy, 1 add)", (int)mode);
  if (n == 0) return RDM_OK;
  const long n4 = n / 4;
  const dim3 grid(sweep_grid(n4, ACC_MAX_BLOCKS));
  if (mode == RDM_GRAD_ACC_ADD)
    hipLaunchKernelGGL(k_grad_accumulate<RDM_GRAD_ACC_ADD>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, dst, src, n4, (long)n);
  else
    hipLaunchKernelGGL(k_grad_accumulate<RDM_GRAD_ACC_COPY>, grid, dim3(OPT_THREADS), 0, (hipStream_t)stream, dst, src, n4, (long)n);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" size_t rdm_grad_sumsq_workspace_bytes(int64_t n) { return n < 0 ? 0 : (size_t)sumsq_blocks(n) * sizeof(double); }

extern "C" int rdm_grad_sumsq_f64(const float* grad, int64_t n, double* out_slot, void* ws, size_t ws_bytes, rdm_stream_t stream) {
  RDM_CHECK_ARG(grad && out_slot && ws, "grad_sumsq: grad, out_slot and ws must not be NULL");
  RDM_CHECK_ARG(((uintptr_t)grad & 15) == 0, "grad_sumsq: grad must be 16-byte aligned");
  RDM_CHECK_ARG((((uintptr_t)out_slot | (uintptr_t)ws) & 7) == 0, "grad_sumsq: out_slot and ws must be 8-byte aligned");
  RDM_CHECK_ARG(n >= 0, "grad_sumsq: n = %lld is negative", (long long)n);
  RDM_CHECK_ARG(ws_bytes >= rdm_grad_sumsq_workspace_bytes(n), "grad_sumsq: workspace of %zu bytes, %zu needed", ws_bytes, rdm_grad_sumsq_workspace_bytes(n));
  const int blocks = sumsq_blocks(n);
  hipLaunchKernelGGL(k_grad_sumsq, dim3(blocks), dim3(OPT_THREADS), 0, (hipStream_t)stream, grad, (long)(n / 4), (long)n, (double*)ws);
  RDM_LAUNCH_OK();
  hipLaunchKernelGGL(k_grad_sumsq_final, dim3(1), dim3(OPT_THREADS), 0, (hipStream_t)stream, (const double*)ws, blocks, out_slot);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_adamw_fused_clip(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float lr, float beta1, float beta2,
                                    float eps, float weight_decay, int32_t step, float grad_scale, const double* sumsq, int32_t n_slots,
                                    float max_norm, float* coef_out, rdm_stream_t stream) {
  RDM_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, "adamw_fused_clip: bad argument");
  RDM_CHECK_ARG((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0, "adamw_fused_clip: buffers must be 16-byte aligned");
  RDM_CHECK_ARG(sumsq && ((uintptr_t)sumsq & 7) == 0, "adamw_fused_clip: sumsq must be an 8-byte aligned device pointer");
  RDM_CHECK_ARG(n_slots >= 1 && n_slots <= RDM_CLIP_MAX_SLOTS, "adamw_fused_clip: n_slots = %d outside 1..%d", (int)n_slots, RDM_CLIP_MAX_SLOTS);
  RDM_CHECK_ARG(max_norm >= 0.f, "adamw_fused_clip: max_norm must be non-negative (got %g)", (double)max_norm);
  RDM_CHECK_ARG(((uintptr_t)coef_out & 3) == 0, "adamw_fused_clip: coef_out must be 4-byte aligned");
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);      // as launch_adamw (elementwise.hip)
  const long n4 = n / 4;
  hipLaunchKernelGGL(k_adamw_clip, dim3(adamw_grid(n4)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n4, (long)n, lr, beta1,
                     beta2, eps, weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)), grad_scale, sumsq, (int)n_slots, max_norm, coef_out);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_adamw_fused_ema(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float* ema, int64_t n, float lr, float beta1,
                                   float beta2, float eps, float weight_decay, int32_t step, float grad_scale, const double* sumsq, int32_t n_slots,
                                   float max_norm, float* coef_out, float ema_decay, rdm_stream_t stream) {
  RDM_CHECK_ARG(param && grad && exp_avg && exp_avg_sq && n >= 0 && step >= 1, "adamw_fused_ema: bad argument");
  RDM_CHECK_ARG((((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) == 0, "adamw_fused_ema: buffers must be 16-byte aligned");
  RDM_CHECK_ARG(ema && ((uintptr_t)ema & 15) == 0, "adamw_fused_ema: ema must be a 16-byte aligned device pointer");
  RDM_CHECK_ARG(!ranges_overlap(param, ema, n), "adamw_fused_ema: ema overlaps param");
  RDM_CHECK_ARG(ema_decay >= 0.f && ema_decay <= 1.f, "adamw_fused_ema: ema_decay must lie in [0, 1] (got %g)", (double)ema_decay);
  RDM_CHECK_ARG((sumsq == nullptr) == (n_slots == 0), "adamw_fused_ema: sumsq and n_slots must be NULL and 0 (unclipped) or both set (got %s, n_slots = %d)",
                sumsq ? "a pointer" : "NULL", (int)n_slots);
  const bool clipped = sumsq != nullptr;
  if (clipped) {                                                                                  // as rdm_adamw_fused_clip
    RDM_CHECK_ARG(((uintptr_t)sumsq & 7) == 0, "adamw_fused_ema: sumsq must be an 8-byte aligned device pointer");
    RDM_CHECK_ARG(n_slots >= 1 && n_slots <= RDM_CLIP_MAX_SLOTS, "adamw_fused_ema: n_slots = %d outside 1..%d", (int)n_slots, RDM_CLIP_MAX_SLOTS);
    RDM_CHECK_ARG(max_norm >= 0.f, "adamw_fused_ema: max_norm must be non-negative (got %g)", (double)max_norm);
    RDM_CHECK_ARG(((uintptr_t)coef_out & 3) == 0, "adamw_fused_ema: coef_out must be 4-byte aligned");
  }
  if (n == 0) return RDM_OK;
  const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);      // as launch_adamw (elementwise.hip)
  const long n4 = n / 4;
  const float omd = 1.f - ema_decay;
  const dim3 grid(adamw_grid(n4));
  if (clipped)
    hipLaunchKernelGGL(k_adamw_ema<true>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, ema, n4, (long)n, lr, beta1, beta2,
                       eps, weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)), grad_scale, sumsq, (int)n_slots, max_norm, coef_out, omd);
  else
    hipLaunchKernelGGL(k_adamw_ema<false>, grid, dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, ema, n4, (long)n, lr, beta1, beta2,
                       eps, weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)), grad_scale, (const double*)nullptr, 0, 0.f, (float*)nullptr, omd);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_ema_swap_f32(float* a, float* b, int64_t n, rdm_stream_t stream) {
  RDM_CHECK_ARG(a && b, "ema_swap: a and b must not be NULL");
  RDM_CHECK_ARG((((uintptr_t)a | (uintptr_t)b) & 15) == 0, "ema_swap: buffers must be 16-byte aligned");
  RDM_CHECK_ARG(n >= 0, "ema_swap: n = %lld is negative", (long long)n);
  RDM_CHECK_ARG(!ranges_overlap(a, b, n), "ema_swap: the two ranges overlap");
  if (n == 0) return RDM_OK;
  const long n4 = n / 4;
  hipLaunchKernelGGL(k_ema_swap, dim3(sweep_grid(n4, ACC_MAX_BLOCKS)), dim3(OPT_THREADS), 0, (hipStream_t)stream, a, b, n4, (long)n);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
