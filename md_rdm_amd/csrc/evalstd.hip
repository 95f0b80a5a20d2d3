// Standard-protocol evaluation in ONE launch (include/rdm_eval.h): the predicted log map (B,1,128,128) + the loader's raw depth (B,1,h,w) ->
// sixteen figures per sample: the Eigen et al. error sums over the valid pixels at the depth's own resolution, after a per-image scale
// alignment.  Composed from single operators it is a resize, an exp, a mask, a sort (or two) per sample and a dozen reductions, with several
// full-resolution float64 intermediates and a host decision per sample.
//
// Grid (B): one workgroup of 1024 threads per sample, so nothing is exchanged between workgroups.  Thread t owns the pixels t, t + 1024, ...
// in EVERY pass, so what it stored to the workspace in the first pass it reads back itself.  Passes over the sample:
//   A  p = exp(bicubic(map)) -> workspace (the map covers a VIEW of the depth frame, the whole frame unless the caller says otherwise); valid count, any non-finite p, sum ln d, sum ln p
//   M  median alignment only: an exact radix select of the middle order statistic of d_valid and of p_valid at once.  The bit patterns of
//      non-negative doubles sort like the doubles: eight passes of 8-bit digits from the top, an integer histogram per array in LDS (integer
//      atomics: the counts do not depend on the order), a scan of the 256 bins, the bin that holds the wanted rank extends the key prefix.
//      For an even count the upper middle element is the same value when the last bin holds more than the wanted rank, else the smallest
//      key above it: one more pass with an integer minimum.
//   B  q = clamp(s * p) -> pred_out; the sums, in a fixed order (a thread's pixels front to back, lanes by shuffle, wavefronts in sequence)
// Plain stores only, no floating-point atomics: a repeated call gives the same bytes, a sample alone the row it gives inside a batch.
#include <cmath>

#include "rdm_common.h"
#include "postproc_dev.h"
#include "../../include/rdm_eval.h"
#include "../../include/rdm_eval_view.h"

namespace rdm {

constexpr int ES_SIDE = 128;                      // the predicted map
constexpr int ES_THREADS = 1024;
constexpr int ES_WAVES = ES_THREADS / 64;
constexpr int ES_BINS = 256;                      // 8-bit digits
constexpr int ES_SUMS = 12;                       // columns 0-10 and 14
constexpr int ES_COLS = RDM_EVAL_STANDARD_COLS;

struct EsArgs {
  const double* map;
  const void* depth;
  double* rows;
  double* pred_out;
  double* ws;
  int h, w, align, has_crop;
  int y0, x0, y1, x1;
  double lo, hi;
  // the view: the map's rows cover the depth rows [vy0, vy0 + 128 / sy), its columns [vx0, vx0 + 128 / sx); the full frame is (0, 0, 128 / h, 128 / w),
  // whose sy and (y + 0.5) - 0 are the operands of cubic_index(y, 128, h).  identity: a 128x128 frame under the full view reads the map as it is
  double sy, sx, vy0, vx0;
  int identity;
};

struct EsState {
  unsigned hist[2][ES_BINS];
  unsigned wave_total[2][ES_BINS / 64];
  unsigned long long key[2];                      // the selected key's digits so far
  unsigned rank[2], equal[2];                     // wanted rank among the keys with that prefix; keys in the chosen bin
  unsigned long long wave_min[2][ES_WAVES];
  double sum[ES_WAVES];
  double red[ES_SUMS][ES_WAVES];
};

template <typename T>
__device__ __forceinline__ bool es_valid(const T* __restrict__ d, long i, const EsArgs& a, double& dv) {
  dv = (double)d[i];
  bool ok = dv > a.lo && dv < a.hi && __builtin_isfinite(dv);
  if (a.has_crop) {
    const int y = (int)((unsigned)i / (unsigned)a.w), x = (int)((unsigned)i - (unsigned)y * (unsigned)a.w);
    ok = ok && y >= a.y0 && y < a.y1 && x >= a.x0 && x < a.x1;
  }
  return ok;
}

// one count into hist[digit] for every lane with `on`; EVERY lane of the wavefront calls it.  When all of them name one bin (the top digits of
// depths within a few octaves) a single lane adds the population count instead of 64 atomics queueing on one address.
__device__ __forceinline__ void es_hist_add(unsigned* hist, bool on, unsigned digit) {
  const unsigned long long m = __ballot(on);
  if (m == 0) return;
  const int leader = __ffsll((long long)m) - 1;
  const unsigned d0 = (unsigned)__shfl((int)digit, leader);
  if (__ballot(on && digit != d0) == 0) {
    if ((int)(threadIdx.x & 63) == leader) atomicAdd(&hist[d0], (unsigned)__popcll(m));
  } else if (on) {
    atomicAdd(&hist[digit], 1u);
  }
}

// Exact order statistics of the valid d (array 0) and of their p (array 1): returns the medians as numpy forms them.  n >= 1 valid pixels.
template <typename T>
__device__ __forceinline__ void es_medians(EsState& S, const T* __restrict__ d, const double* __restrict__ wp, long P, const EsArgs& a, unsigned n,
                                           double& med_d, double& med_p) {
  const int tid = threadIdx.x;
  if (tid < 2) S.key[tid] = 0, S.rank[tid] = (n - 1) / 2;
  for (int s = 56; s >= 0; s -= 8) {
    if (tid < 2 * ES_BINS) (&S.hist[0][0])[tid] = 0;
    __syncthreads();
    const unsigned long long k0 = S.key[0], k1 = S.key[1];
    for (long i0 = 0; i0 < P; i0 += ES_THREADS) {                    // uniform trip count: es_hist_add is a wavefront-wide call
      const long i = i0 + tid;
      double dv = 0;
      const bool ok = i < P && es_valid(d, i, a, dv);
      const unsigned long long kd = (unsigned long long)__double_as_longlong(dv), kp = ok ? (unsigned long long)__double_as_longlong(wp[i]) : 0ull;
      const bool top = s == 56;                                      // (a shift by 64 is undefined)
      es_hist_add(S.hist[0], ok && (top || (kd >> (s + 8)) == (k0 >> (s + 8))), (unsigned)(kd >> s) & 255u);
      es_hist_add(S.hist[1], ok && (top || (kp >> (s + 8)) == (k1 >> (s + 8))), (unsigned)(kp >> s) & 255u);
    }
    __syncthreads();
    // threads 0-255 scan array 0's bins, 256-511 array 1's: inclusive scan inside a wavefront, then the four wavefront totals
    const int arr = (tid >> 8) & 1, bin = tid & (ES_BINS - 1), wv = (tid >> 6) & 3, lane = tid & 63;
    const bool scans = tid < 2 * ES_BINS;
    const unsigned c = scans ? S.hist[arr][bin] : 0u;
    unsigned incl = c;
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned up = (unsigned)__shfl_up((int)incl, o);
      if (lane >= o) incl += up;
    }
    const unsigned want = S.rank[arr];
    if (scans && lane == 63) S.wave_total[arr][wv] = incl;
    __syncthreads();
    if (scans) {
      unsigned before = incl - c;
      for (int k = 0; k < wv; ++k) before += S.wave_total[arr][k];
      if (before <= want && want < before + c) {                     // exactly one bin per array
        S.key[arr] |= (unsigned long long)bin << s;
        S.rank[arr] = want - before;
        S.equal[arr] = c;
      }
    }
    __syncthreads();
  }
  const unsigned long long k0 = S.key[0], k1 = S.key[1];
  unsigned long long up0 = k0, up1 = k1;                             // the element of rank (n - 1) / 2 + 1, for an even n
  if ((n & 1) == 0) {
    const bool next0 = S.rank[0] + 1 >= S.equal[0], next1 = S.rank[1] + 1 >= S.equal[1];
    if (next0 || next1) {                                            // uniform over the workgroup
      unsigned long long m0 = ~0ull, m1 = ~0ull;
      for (long i = tid; i < P; i += ES_THREADS) {
        double dv;
        if (es_valid(d, i, a, dv)) {
          const unsigned long long kd = (unsigned long long)__double_as_longlong(dv), kp = (unsigned long long)__double_as_longlong(wp[i]);
          if (kd > k0 && kd < m0) m0 = kd;
          if (kp > k1 && kp < m1) m1 = kp;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long o0 = __shfl_down(m0, o), o1 = __shfl_down(m1, o);
        m0 = o0 < m0 ? o0 : m0;
        m1 = o1 < m1 ? o1 : m1;
      }
      if ((tid & 63) == 0) S.wave_min[0][tid >> 6] = m0, S.wave_min[1][tid >> 6] = m1;
      __syncthreads();
      m0 = S.wave_min[0][0], m1 = S.wave_min[1][0];
      for (int k = 1; k < ES_WAVES; ++k) {
        m0 = S.wave_min[0][k] < m0 ? S.wave_min[0][k] : m0;
        m1 = S.wave_min[1][k] < m1 ? S.wave_min[1][k] : m1;
      }
      if (next0) up0 = m0;
      if (next1) up1 = m1;
    }
  }
  const double a0 = __longlong_as_double((long long)k0), a1 = __longlong_as_double((long long)k1);
  med_d = (n & 1) ? a0 : (a0 + __longlong_as_double((long long)up0)) / 2.0;
  med_p = (n & 1) ? a1 : (a1 + __longlong_as_double((long long)up1)) / 2.0;
}

template <typename T>
__global__ __launch_bounds__(ES_THREADS) void k_eval_standard(EsArgs a) {
#pragma clang fp contract(off)
  __shared__ EsState S;
  const int tid = threadIdx.x, b = blockIdx.x;
  const long P = (long)a.h * a.w;
  const T* d = (const T*)a.depth + (long)b * P;
  const double* map = a.map + (long)b * ES_SIDE * ES_SIDE;
  double* wp = a.ws + (long)b * P;
  double* row = a.rows + (long)b * ES_COLS;

  // A. the prediction at the depth's resolution; what the alignment needs of the valid pixels
  double cnt = 0, sld = 0, slp = 0;
  int bad = 0;
  for (long i = tid; i < P; i += ES_THREADS) {
    const int oy = (int)((unsigned)i / (unsigned)a.w), ox = (int)((unsigned)i - (unsigned)oy * (unsigned)a.w);
    const double p = exp(a.identity ? map[i] : bicubic_at_view(map, ES_SIDE, ES_SIDE, a.sy, a.sx, ((double)oy + 0.5) - a.vy0, ((double)ox + 0.5) - a.vx0));
    wp[i] = p;
    double dv;
    if (es_valid(d, i, a, dv)) {
      cnt += 1;
      if (!__builtin_isfinite(p)) bad = 1;
      if (a.align == RDM_EVAL_ALIGN_LOGMEAN) sld += log(dv), slp += log(p);
    }
  }
  const double n = block_sum_bcast(cnt, S.sum);                       // an integer below 2^31: exact
  bad = __syncthreads_or(bad);
  const bool score = n > 0 && !bad;

  // the scale
  double s = 1.0, stat_d = 0.0, stat_p = 0.0;
  if (score && a.align == RDM_EVAL_ALIGN_LOGMEAN) {
    stat_d = block_sum_bcast(sld, S.sum) / n;
    stat_p = block_sum_bcast(slp, S.sum) / n;
    s = exp(stat_d - stat_p);
  } else if (score && a.align == RDM_EVAL_ALIGN_MEDIAN) {
    es_medians(S, d, wp, P, a, (unsigned)n, stat_d, stat_p);
    s = stat_d / stat_p;
  }

  // B. clamp, pred_out, the sums
  double* po = a.pred_out ? a.pred_out + (long)b * P : nullptr;
  double acc[ES_SUMS];
#pragma unroll
  for (int k = 0; k < ES_SUMS; ++k) acc[k] = 0;
  if (score || po) {
    for (long i = tid; i < P; i += ES_THREADS) {
      const double sp = s * wp[i];
      const double q = sp < a.lo ? a.lo : sp > a.hi ? a.hi : sp;
      if (po) po[i] = q;
      double dv;
      if (score && es_valid(d, i, a, dv)) {
        const double r = fmax(q / dv, dv / q), e = q - dv, l = log(q) - log(dv);
        acc[0] += 1;
        acc[1] += r < 1.25 ? 1 : 0;
        acc[2] += r < 1.25 * 1.25 ? 1 : 0;
        acc[3] += r < 1.25 * 1.25 * 1.25 ? 1 : 0;
        acc[4] += fabs(e) / dv;
        acc[5] += e * e / dv;
        acc[6] += e * e;
        acc[7] += l * l;
        acc[8] += l;
        acc[9] += fabs(log10(q) - log10(dv));
        acc[10] += fabs(e);
        acc[11] += (sp < a.lo || sp > a.hi) ? 1 : 0;
      }
    }
  }
  if (!score) {                                                        // uniform: no valid pixel -> zeros; a non-finite p -> NaN
    if (tid < ES_COLS) row[tid] = n > 0 ? (tid == 0 ? n : tid < 14 ? __builtin_nan("") : 0.0) : 0.0;
    return;
  }
  const int wv = tid >> 6;
#pragma unroll
  for (int k = 0; k < ES_SUMS; ++k) {
    double r = acc[k];
    for (int o = 32; o > 0; o >>= 1) r += __shfl_down(r, o);
    if ((tid & 63) == 0) S.red[k][wv] = r;
  }
  __syncthreads();
  if (tid < ES_SUMS) {
    double r = 0;
    for (int i = 0; i < ES_WAVES; ++i) r += S.red[tid][i];
    row[tid < 11 ? tid : 14] = r;
  } else if (tid < ES_COLS) {                                          // threads 12, 13, 14, 15 -> columns 11, 12, 13, 15
    const int c = tid == 15 ? 15 : tid - 1;
    row[c] = c == 11 ? s : c == 12 ? stat_d : c == 13 ? stat_p : 0.0;
  }
}

}  // namespace rdm

using namespace rdm;

static bool es_plane_ok(int32_t batch, int32_t h, int32_t w) { return batch > 0 && h > 0 && w > 0 && (long)h * w <= 0x7fffffffL; }

extern "C" size_t rdm_eval_standard_workspace_bytes(int32_t batch, int32_t h, int32_t w) {
  return es_plane_ok(batch, h, w) ? (size_t)batch * (size_t)h * (size_t)w * sizeof(double) : 0;
}

// both entry points: the checks, then the one launch.  view NULL = the full frame (0, 0, h, w)
static int es_run(const double* log_map, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, int32_t align, double min_depth,
                  double max_depth, const int32_t* crop, const double* view, double* rows, void* pred_out, void* workspace, size_t workspace_bytes,
                  rdm_stream_t stream) {
  RDM_CHECK_ARG(log_map && depth && rows && workspace, "eval_standard: log_map, depth, rows and workspace must not be NULL");
  RDM_CHECK_ARG(((uintptr_t)log_map | (uintptr_t)rows | (uintptr_t)workspace | (uintptr_t)pred_out) % sizeof(double) == 0 &&
                    (uintptr_t)depth % (depth_is_f64 ? sizeof(double) : sizeof(float)) == 0,
                "eval_standard: log_map, rows, workspace and pred_out must be 8-byte aligned, depth aligned to its element");
  RDM_CHECK_ARG(batch > 0 && h > 0 && w > 0, "eval_standard: need batch, h, w > 0 (got %d, %d, %d)", (int)batch, (int)h, (int)w);
  RDM_CHECK_ARG(es_plane_ok(batch, h, w), "eval_standard: a %dx%d depth plane is beyond the kernel's 32-bit pixel index", (int)h, (int)w);
  RDM_CHECK_ARG(align == RDM_EVAL_ALIGN_NONE || align == RDM_EVAL_ALIGN_MEDIAN || align == RDM_EVAL_ALIGN_LOGMEAN, "eval_standard: unknown align %d", (int)align);
  RDM_CHECK_ARG(min_depth >= 0 && min_depth < max_depth, "eval_standard: need 0 <= min_depth < max_depth (got %g, %g)", min_depth, max_depth);
  RDM_CHECK_ARG(!crop || (crop[0] >= 0 && crop[1] >= 0 && crop[0] < crop[2] && crop[1] < crop[3] && crop[2] <= h && crop[3] <= w),
                "eval_standard: crop [%d, %d) x [%d, %d) is empty or outside the %dx%d frame", crop ? (int)crop[0] : 0, crop ? (int)crop[2] : 0,
                crop ? (int)crop[1] : 0, crop ? (int)crop[3] : 0, (int)h, (int)w);
  RDM_CHECK_ARG(workspace_bytes >= rdm_eval_standard_workspace_bytes(batch, h, w), "eval_standard: workspace of %zu bytes, %zu needed", workspace_bytes,
                rdm_eval_standard_workspace_bytes(batch, h, w));
  RDM_CHECK_ARG(!view || (std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2]) && std::isfinite(view[3]) && view[2] > 0 && view[3] > 0),
                "eval_standard: view (%g, %g, %g, %g) must be finite with vh > 0 and vw > 0", view ? view[0] : 0.0, view ? view[1] : 0.0, view ? view[2] : 0.0,
                view ? view[3] : 0.0);
  const double vy0 = view ? view[0] : 0.0, vx0 = view ? view[1] : 0.0, vh = view ? view[2] : (double)h, vw = view ? view[3] : (double)w;
  EsArgs a;
  a.map = log_map, a.depth = depth, a.rows = rows, a.pred_out = (double*)pred_out, a.ws = (double*)workspace;
  a.h = h, a.w = w, a.align = align, a.has_crop = crop ? 1 : 0;
  a.y0 = crop ? crop[0] : 0, a.x0 = crop ? crop[1] : 0, a.y1 = crop ? crop[2] : h, a.x1 = crop ? crop[3] : w;
  a.lo = min_depth, a.hi = max_depth;
  a.sy = (double)ES_SIDE / vh, a.sx = (double)ES_SIDE / vw, a.vy0 = vy0, a.vx0 = vx0;
  a.identity = h == ES_SIDE && w == ES_SIDE && vy0 == 0.0 && vx0 == 0.0 && vh == (double)h && vw == (double)w;
  if (depth_is_f64)
    hipLaunchKernelGGL(k_eval_standard<double>, dim3(batch), dim3(ES_THREADS), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(k_eval_standard<float>, dim3(batch), dim3(ES_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_eval_standard_f64(const double* log_map, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, int32_t align,
                                     double min_depth, double max_depth, const int32_t* crop, double* rows, void* pred_out, void* workspace,
                                     size_t workspace_bytes, rdm_stream_t stream) {
  return es_run(log_map, depth, depth_is_f64, batch, h, w, align, min_depth, max_depth, crop, nullptr, rows, pred_out, workspace, workspace_bytes, stream);
}

extern "C" int rdm_eval_standard_view_f64(const double* log_map, const void* depth, int32_t depth_is_f64, int32_t batch, int32_t h, int32_t w, int32_t align,
                                          double min_depth, double max_depth, const int32_t* crop, const double* view, double* rows, void* pred_out,
                                          void* workspace, size_t workspace_bytes, rdm_stream_t stream) {
  return es_run(log_map, depth, depth_is_f64, batch, h, w, align, min_depth, max_depth, crop, view, rows, pred_out, workspace, workspace_bytes, stream);
}
