// THE AdamW update body (torch.optim.AdamW, decoupled weight decay, no amsgrad; network/module.py:41), shared by k_adamw (elementwise.hip),
// k_adamw_clip and k_adamw_ema (optim.hip) so that the clipped step differs from the plain one in the value of `gscale` alone and agrees with it bit for bit
// when that value is the same.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace rdm {

__device__ __forceinline__ void adamw_elem(float& p, float g, float& m, float& v, float lr, float b1, float b2, float eps, float wd, float bc1,
                                           float rsqrt_bc2, float gscale) {
  const float gr = g * gscale;
  float w = p * (1.f - lr * wd);
  m = b1 * m + (1.f - b1) * gr;
  v = b2 * v + (1.f - b2) * gr * gr;
  const float denom = sqrtf(v) * rsqrt_bc2 + eps;
  w -= (lr / bc1) * (m / denom);
  p = w;
}

// one workgroup's share of the sweep over n elements: n4 = n / 4 quads grid-strided in 128-bit accesses, the n % 4 tail on block 0
__device__ __forceinline__ void adamw_sweep(float* p, const float* g, float* m, float* v, long n4, long n, float lr, float b1, float b2, float eps,
                                            float wd, float bc1, float rsqrt_bc2, float gscale) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pp = *reinterpret_cast<const float4*>(p + i * 4), gg = *reinterpret_cast<const float4*>(g + i * 4);
    float4 mm = *reinterpret_cast<const float4*>(m + i * 4), vv = *reinterpret_cast<const float4*>(v + i * 4);
    float* P = &pp.x; float* Gv = &gg.x; float* Mv = &mm.x; float* Vv = &vv.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) adamw_elem(P[k], Gv[k], Mv[k], Vv[k], lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale);
    *reinterpret_cast<float4*>(p + i * 4) = pp; *reinterpret_cast<float4*>(m + i * 4) = mm; *reinterpret_cast<float4*>(v + i * 4) = vv;
  }
  // tail (n not a multiple of 4).  Kept in the form it has always had, through memory: the compiler contracts this form differently from
  // adamw_elem's (one product and sum stay apart here), and the bytes rdm_adamw_fused gives for a tail element must not move
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = n4 * 4 + threadIdx.x;
    const float gr = g[i] * gscale;
    float w = p[i] * (1.f - lr * wd);
    m[i] = b1 * m[i] + (1.f - b1) * gr;
    v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
    w -= (lr / bc1) * (m[i] / (sqrtf(v[i]) * rsqrt_bc2 + eps));
    p[i] = w;
  }
}

// the weight average's update from the weight the step has just formed: e + omd (w - e) with omd = 1 - decay rounded once on the host.
// omd == 0 (decay 1) hands e back as it is, so that -0 and NaN payloads survive too
__device__ __forceinline__ float ema_elem(float e, float w, float omd) { return omd == 0.f ? e : e + omd * (w - e); }

// adamw_sweep with the average e advanced in the same pass (k_adamw_ema, optim.hip): the quad loop shares adamw_elem, and the tail repeats
// adamw_sweep's text word for word so that p, m and v get the bytes adamw_sweep gives them; e costs one more 128-bit load and store per quad
__device__ __forceinline__ void adamw_sweep_ema(float* p, const float* g, float* m, float* v, float* e, long n4, long n, float lr, float b1,
                                                float b2, float eps, float wd, float bc1, float rsqrt_bc2, float gscale, float omd) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
    float4 pp = *reinterpret_cast<const float4*>(p + i * 4), gg = *reinterpret_cast<const float4*>(g + i * 4);
    float4 mm = *reinterpret_cast<const float4*>(m + i * 4), vv = *reinterpret_cast<const float4*>(v + i * 4);
    float4 ee = *reinterpret_cast<const float4*>(e + i * 4);
    float* P = &pp.x; float* Gv = &gg.x; float* Mv = &mm.x; float* Vv = &vv.x; float* Ev = &ee.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      adamw_elem(P[k], Gv[k], Mv[k], Vv[k], lr, b1, b2, eps, wd, bc1, rsqrt_bc2, gscale);
      Ev[k] = ema_elem(Ev[k], P[k], omd);
    }
    *reinterpret_cast<float4*>(p + i * 4) = pp; *reinterpret_cast<float4*>(m + i * 4) = mm; *reinterpret_cast<float4*>(v + i * 4) = vv;
    *reinterpret_cast<float4*>(e + i * 4) = ee;
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {                      // adamw_sweep's tail, through memory, then the average
    const long i = n4 * 4 + threadIdx.x;
    const float gr = g[i] * gscale;
    float w = p[i] * (1.f - lr * wd);
    m[i] = b1 * m[i] + (1.f - b1) * gr;
    v[i] = b2 * v[i] + (1.f - b2) * gr * gr;
    w -= (lr / bc1) * (m[i] / (sqrtf(v[i]) * rsqrt_bc2 + eps));
    p[i] = w;
    e[i] = ema_elem(e[i], w, omd);
  }
}

// blocks of 256 threads for a sweep over n4 quads (one trip up to 2048 x 256 quads, grid-strided beyond)
static inline int adamw_grid(long n4) { return (int)(n4 <= 256 ? 1 : n4 >= 2048L * 256 ? 2048 : (n4 + 255) / 256); }

}  // namespace rdm
