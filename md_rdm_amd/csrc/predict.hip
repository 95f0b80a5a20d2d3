// The inference tail in ONE launch: d_1 logits -> log relative depth map (RDM_Net.py:113-133 + computations.py:394-421 for the ordinal-only
// model with a square power-of-two head).  It restates, with the device functions of postproc_dev.h and in the order of the single-purpose
// kernels, what rdm_dorn_fwd -> rdm_gm_normalize_f64 -> (float32 round, RDM_Net.py:117) -> rdm_decompose_f64 -> rdm_fine_detail_pred_f32 ->
// rdm_recombine_f64 compute over six launches and three casts; the (B,K,s,s) float64 ordinal probabilities are never formed.
//
// Grid (split, B): every workgroup of an image redundantly reads its 2K*s*s logits (46 KB at 8x8, coalesced along the pixels of a channel),
// counts, normalises and builds the pyramid (341 doubles at most) in LDS, then stores its 1/split of the output rows with 16-byte stores.
// No atomics, no inter-workgroup traffic; sums run in the fixed order of block_sum_bcast, so the result does not depend on `split`.
#include "rdm_common.h"
#include "postproc_dev.h"
#include "predict.h"

namespace rdm {

constexpr int PT_THREADS = 256;
constexpr int PT_MAX_N = 4;                       // head side 2^n <= 16: s*s <= PT_THREADS pixels, pyramid level_off(5) = 341 values
constexpr int PT_PYR = 341;
constexpr int PT_CHUNK = 8;                       // ordinal pairs whose 2 logits are in flight per thread before the first compare

__global__ __launch_bounds__(PT_THREADS) void k_predict_tail(const float* __restrict__ logits, const float* __restrict__ w, double* __restrict__ log_map,
                                                             long long* __restrict__ decode, float* __restrict__ lin_map, int K, int n, int n_out, double e) {
  __shared__ double sh[PT_THREADS / 64];
  __shared__ int part[PT_THREADS];
  __shared__ double cnt[PT_THREADS];
  __shared__ double L[PT_PYR];
  __shared__ float Y[PT_PYR];
  __shared__ double V[PT_THREADS];
  __shared__ float E[PT_THREADS];
  const int tid = threadIdx.x, b = blockIdx.y;
  const int s = 1 << n, hw = s * s;

  // 1. DORN counts: thread = (pair group g, pixel p); a wavefront reads 64 contiguous pixels of one channel
  {
    const int G = PT_THREADS / hw, p = tid & (hw - 1), g = tid >> (2 * n);
    const float* xb = logits + (long)b * 2 * K * hw + p;
    int c = 0;
    for (int k0 = g; k0 < K; k0 += G * PT_CHUNK) {
      float va[PT_CHUNK], vb[PT_CHUNK];
#pragma unroll
      for (int j = 0; j < PT_CHUNK; ++j) {
        const int k = k0 + j * G;
        const bool in = k < K;
        va[j] = in ? xb[(long)(2 * k) * hw] : 0.f;
        vb[j] = in ? xb[(long)(2 * k + 1) * hw] : 0.f;
      }
#pragma unroll
      for (int j = 0; j < PT_CHUNK; ++j) c += dorn_pair_above_half(va[j], vb[j]) ? 1 : 0;        // out-of-range pairs are (0, 0): a tie, not counted
    }
    part[tid] = c;
    __syncthreads();
    if (tid < hw) {
      int t = 0;
      for (int j = 0; j < G; ++j) t += part[j * hw + tid];
      cnt[tid] = (double)t;
      if (decode && blockIdx.x == 0) decode[(long)b * hw + tid] = t;
    }
    __syncthreads();
  }

  // 2. geometric-mean normalisation (k_gm_normalize), rounded to float32 as DepthEstimationNet.forward hands it on
  double* top = L + level_off(n);
  {
    double acc = 0;
    for (int i = tid; i < hw; i += PT_THREADS) acc += log(cnt[i]);
    const double gm = exp(e * block_sum_bcast(acc, sh));
    for (int i = tid; i < hw; i += PT_THREADS) top[i] = (double)(float)(cnt[i] / gm);
    __syncthreads();
  }

  // 3. pyramid and ratio levels (k_decompose): slot_k holds d_k, then is divided in place by the nearest-upsampled d_{k-1}
  for (int k = n; k >= 1; --k) {
    const int sk = 1 << k, h = sk >> 1;
    double* cur = L + level_off(k);
    double* low = L + level_off(k - 1);
    for (int i = tid; i < h * h; i += PT_THREADS) low[i] = bicubic_at(cur, sk, sk, h, h, i / h, i % h);
    __syncthreads();
    for (int i = tid; i < sk * sk; i += PT_THREADS) cur[i] = cur[i] / low[((i / sk) >> 1) * h + ((i % sk) >> 1)];
    __syncthreads();
  }

  // 4. weighted logs (k_fine_detail_pred)
  for (int i = tid; i < (int)level_off(n + 1); i += PT_THREADS) {
    int k = 0;
    while (level_off(k + 1) <= i) ++k;
    Y[i] = fine_detail_value(L[i], w[k]);
  }
  __syncthreads();

  // 5. the sum of k_recombine (levels 1..n ascending, then d_0 + r), once per pixel of the finest level: the nearest upsampling only repeats it
  if (tid < hw) {
    const int yy = tid >> n, xx = tid & (s - 1);
    double r = 0.0;
    bool have = false;
    for (int k = 1; k <= n; ++k) {
      const double v = (double)Y[level_off(k) + ((yy >> (n - k)) << k) + (xx >> (n - k))];
      r = have ? r + v : v;
      have = true;
    }
    const double d0 = (double)Y[0];
    r = have ? d0 + r : d0;
    V[tid] = r;
    if (lin_map) E[tid] = (float)exp(r);
  }
  __syncthreads();

  // 6. this workgroup's rows, two neighbouring pixels per store
  const int So = 1 << n_out, pr = So >> 1, up = n_out - n;
  const int rows = So / (int)gridDim.x, row0 = (int)blockIdx.x * rows;
  double* ob = log_map + ((long)b << (2 * n_out));
  float* lb = lin_map ? lin_map + ((long)b << (2 * n_out)) : nullptr;
  for (int i = tid; i < rows * pr; i += PT_THREADS) {
    const int y = row0 + i / pr, x = (i % pr) * 2;
    const int base = (y >> up) << n;
    const int i0 = base + (x >> up), i1 = base + ((x + 1) >> up);
    const long o = (long)y * So + x;
    *reinterpret_cast<double2*>(ob + o) = make_double2(V[i0], V[i1]);
    if (lb) *reinterpret_cast<float2*>(lb + o) = make_float2(E[i0], E[i1]);
  }
}

int predict_tail_default_split(int batch, int n_out) {
  // tools/predict_bench.py sweeps S at B = 1, 8, 16; 8 until that sweep has been run: 16 rows = 16 KB of stores per workgroup
  int split = 8;
  (void)batch;
  while (split > (1 << n_out)) split >>= 1;
  return split;
}

int launch_predict_tail(const float* logits, const float* w, double* log_map, int64_t* decode, float* lin_map, int B, int K, int n, int n_out, int split,
                        hipStream_t stream) {
  static_assert(((1L << (2 * (PT_MAX_N + 1))) - 1) / 3 == PT_PYR && (1 << (2 * PT_MAX_N)) <= PT_THREADS, "LDS arrays are sized for side 2^PT_MAX_N");
  if (n < 0 || n > PT_MAX_N) { set_error("predict_tail: head side 2^%d is outside the kernel's range (side <= %d)", n, 1 << PT_MAX_N); return RDM_ERR_BAD_ARGUMENT; }
  const double e = 1.0 / (double)(1 << (2 * n));
  hipLaunchKernelGGL(k_predict_tail, dim3(split, B), dim3(PT_THREADS), 0, stream, logits, w, log_map, reinterpret_cast<long long*>(decode), lin_map, K, n, n_out, e);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

}  // namespace rdm
