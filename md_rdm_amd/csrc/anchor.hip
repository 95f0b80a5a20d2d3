// Anchored metric depth, launches 1 and 2 of include/rdm_anchor.h (launch 3, the corrected frames, is depthframe.hip's kernel with a field).
//
// k_anchor_cells: the log residuals of the anchors against the view-resampled map, summed per square cell.  Grid (cells / 4, batch), four
// wavefronts per workgroup, ONE WAVEFRONT PER CELL: no barrier, no LDS, and the order of a cell's sum is the wavefront's own (a lane adds its
// pixels p = l, l + 64, ... in sequence, then the lane tree 32, 16, ... 1 by shuffle) - it depends on nothing but the cell, so a sample alone,
// another batch size or another grid give the same bits.  A pixel costs one float32 load; only an anchor (valid, inside the view) pays for the
// bicubic taps (bicubic_at_view's arithmetic through cubic_axis_view, 16 map loads through the caches, five dot4) and the float64 log, so a
// sparse frame (a fraction of a percent of the pixels) is a stream over the anchor plane.  480x640 at cell 16 is 1200 cells: 300 workgroups
// per sample, against the one workgroup per sample of evalstd.hip.
//
// k_anchor_field: one workgroup per sample.  The cell planes (s as float64, n as int32) are staged in LDS; thread 0 adds the s_c in row-major
// order for the fit (the header's order: a chain of gy * gx dependent float64 additions, 1200 at the default cell), every thread re-centres its
// cells, and the two passes of the separable normalised convolution go LDS -> LDS (along x) and LDS -> registers -> the field (along y).  The
// tap weights come from the launcher (host exp) by value and are copied to LDS once (a read of the kernel-argument segment: no private copy).
// LDS: 28 bytes per cell, RDM_ANCHOR_MAX_CELLS = 5120 cells: 140 KiB of the compute unit's 160 KiB.
#include <cmath>

#include "rdm_common.h"
#include "postproc_dev.h"
#include "../../include/rdm_anchor.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int AC_THREADS = 256;
constexpr int AC_WAVES = AC_THREADS / 64;           // cells per workgroup
constexpr int AC_SIDE = 128;
constexpr int AF_THREADS = 512;
constexpr int AF_CELLS = RDM_ANCHOR_MAX_CELLS;
constexpr int AF_TAPS = RDM_ANCHOR_MAX_RADIUS + 1;

struct AcArgs {
  const double* map;
  const float* anchors;
  const double* prior;
  int h, w, cell, gy, gx;
  double sy, sx, vy0, vx0, vy1, vx1;                // 128 / vh, 128 / vw; the view [vy0, vy1) x [vx0, vx1), as depthframe.hip forms them
  double dmin, dmax, reject;
  int* n;
  double* s;
};

__global__ __launch_bounds__(AC_THREADS) void k_anchor_cells(AcArgs a) {
  const int b = blockIdx.y, lane = threadIdx.x & 63;
  const int c = blockIdx.x * AC_WAVES + (threadIdx.x >> 6);
  if (c >= a.gy * a.gx) return;                     // the whole wavefront: the kernel has no barrier
  const int cy = c / a.gx, cx = c - cy * a.gx;
  const int y0 = cy * a.cell, x0 = cx * a.cell;     // < h, < w: no overflow for any cell
  const unsigned cw = (unsigned)min(a.cell, a.w - x0), np = (unsigned)min(a.cell, a.h - y0) * cw;       // <= h * w < 2^31
  const double* __restrict__ map = a.map + (long)b * AC_SIDE * AC_SIDE;
  const float* __restrict__ anchors = a.anchors + (long)b * a.h * a.w;
  const double prior = a.prior ? a.prior[b] : 0.0;

  double acc = 0.0;
  int n = 0;
  for (unsigned p = lane; p < np; p += 64) {
    const unsigned py = p / cw;
    const int y = y0 + (int)py, x = x0 + (int)(p - py * cw);
    const float d = anchors[(long)y * a.w + x];
    if (!depth_valid(d, a.dmin, a.dmax)) continue;
    const double ccy = (double)y + 0.5, ccx = (double)x + 0.5;
    if (!(ccy >= a.vy0 && ccy < a.vy1 && ccx >= a.vx0 && ccx < a.vx1)) continue;
    CubicAxis ay, ax;
    cubic_axis_view(y, a.sy, a.vy0, a.vy1, AC_SIDE, AC_SIDE, ay);
    cubic_axis_view(x, a.sx, a.vx0, a.vx1, AC_SIDE, 1, ax);
    double rows[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      double v[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = map[ay.o[i] + ax.o[j]];
      rows[i] = dot4(v, ax.c);
    }
    const double v = dot4(rows, ay.c);
    double r = log((double)d) - v;
    r = r - prior;
    if (fabs(r) > a.reject) continue;               // false for a NaN r and for reject = +inf
    acc = acc + r;
    ++n;
  }
  for (int o = 32; o > 0; o >>= 1) {
    acc = acc + __shfl_down(acc, o);
    n += __shfl_down(n, o);
  }
  if (lane == 0) {
    const long at = ((long)b * a.gy + cy) * a.gx + cx;
    a.n[at] = n;
    a.s[at] = acc;
  }
}

struct AfArgs {
  const int* n;
  const double* s;
  const double* prior;
  int gy, gx, fit, rg;
  double lambda;
  double* ls;
  int* count;
  double* field;
  double g[AF_TAPS];
};

__global__ __launch_bounds__(AF_THREADS) void k_anchor_field(AfArgs a) {
  __shared__ double S[AF_CELLS], SX[AF_CELLS], WX[AF_CELLS];
  __shared__ int N[AF_CELLS];
  __shared__ double G[AF_TAPS];
  __shared__ long long red[AF_THREADS / 64];
  __shared__ double sh_delta;
  const int b = blockIdx.x, tid = threadIdx.x;
  const int gx = a.gx, gy = a.gy, cells = gy * gx, rg = a.rg;
  const int* __restrict__ nc = a.n + (long)b * cells;
  const double* __restrict__ sc = a.s + (long)b * cells;

  if (tid <= rg) G[tid] = a.g[tid];                  // a load from the kernel-argument segment at a register index: no private copy of the table
  long long cnt = 0;
  for (int c = tid; c < cells; c += AF_THREADS) {
    const int n = nc[c];
    N[c] = n;
    S[c] = sc[c];
    cnt += n;
  }
  cnt = block_sum_bcast<AF_THREADS / 64>(cnt, red);  // its barriers also publish S, N and G
  if (tid == 0) {
    double delta = 0.0;
    if (a.fit == RDM_ANCHOR_FIT_LOGMEAN && cnt > 0) {
      double sum = 0.0;
      for (int c = 0; c < cells; ++c) sum = sum + S[c];
      delta = sum / (double)cnt;
    }
    sh_delta = delta;
    a.ls[b] = (a.prior ? a.prior[b] : 0.0) + delta;
    a.count[b] = (int)cnt;
  }
  if (!a.field) return;                              // uniform over the grid
  __syncthreads();
  const double delta = sh_delta;
  for (int c = tid; c < cells; c += AF_THREADS) {    // a thread re-centres the cells it staged itself
    const double m = (double)N[c] * delta;
    S[c] = S[c] - m;
  }
  __syncthreads();
  for (int c = tid; c < cells; c += AF_THREADS) {    // along x
    const int cy = c / gx, cx = c - cy * gx;
    const int k0 = max(-rg, -cx), k1 = min(rg, gx - 1 - cx);
    double as = 0.0, aw = 0.0;
    for (int k = k0; k <= k1; ++k) {
      const double g = G[abs(k)];
      const double ps = g * S[c + k], pw = g * (double)N[c + k];
      as = as + ps;
      aw = aw + pw;
    }
    SX[c] = as;
    WX[c] = aw;
  }
  __syncthreads();
  double* __restrict__ field = a.field + (long)b * cells;
  for (int c = tid; c < cells; c += AF_THREADS) {    // along y
    const int cy = c / gx;
    const int k0 = max(-rg, -cy), k1 = min(rg, gy - 1 - cy);
    double as = 0.0, aw = 0.0;
    for (int k = k0; k <= k1; ++k) {
      const double g = G[abs(k)];
      const double ps = g * SX[c + k * gx], pw = g * WX[c + k * gx];
      as = as + ps;
      aw = aw + pw;
    }
    const double den = aw + a.lambda;
    field[c] = den == 0.0 ? 0.0 : as / den;
  }
}

static inline bool aligned_to(const void* p, size_t n) { return ((uintptr_t)p & (n - 1)) == 0; }

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_depth_anchor_cells(const double* log_map, const float* anchors, const double* prior, int32_t batch, int32_t h, int32_t w,
                                      const double* view, int32_t cell, double min_depth, double max_depth, double reject, int32_t* n_cells,
                                      double* s_cells, rdm_stream_t stream) {
  RDM_CHECK_ARG(log_map && anchors, "depth_anchor_cells: log_map and anchors must not be NULL");
  RDM_CHECK_ARG(n_cells && s_cells, "depth_anchor_cells: n_cells and s_cells must not be NULL");
  RDM_CHECK_ARG(aligned_to(log_map, 8) && aligned_to(prior, 8) && aligned_to(s_cells, 8), "depth_anchor_cells: log_map, prior and s_cells must be 8-byte aligned");
  RDM_CHECK_ARG(aligned_to(anchors, 4) && aligned_to(n_cells, 4), "depth_anchor_cells: anchors and n_cells must be 4-byte aligned");
  if (const int rc = check_frame_shape("depth_anchor_cells", batch, h, w)) return rc;
  RDM_CHECK_ARG(cell >= 1, "depth_anchor_cells: cell must be >= 1 (got %d)", (int)cell);
  if (const int rc = check_depth_range("depth_anchor_cells", min_depth, max_depth)) return rc;
  RDM_CHECK_ARG(reject > 0, "depth_anchor_cells: reject must be > 0 and not NaN, +inf = off (got %g)", reject);
  RDM_CHECK_ARG(prior || !std::isfinite(reject), "depth_anchor_cells: a finite reject (%g) needs a prior to gate against", reject);
  RDM_CHECK_ARG(!view || (std::isfinite(view[0]) && std::isfinite(view[1]) && std::isfinite(view[2]) && std::isfinite(view[3]) && view[2] > 0 && view[3] > 0),
                "depth_anchor_cells: view (%g, %g, %g, %g) must be finite with vh > 0 and vw > 0", view ? view[0] : 0.0, view ? view[1] : 0.0,
                view ? view[2] : 0.0, view ? view[3] : 0.0);
  const double vy0 = view ? view[0] : 0.0, vx0 = view ? view[1] : 0.0, vh = view ? view[2] : (double)h, vw = view ? view[3] : (double)w;
  AcArgs a = {};
  a.map = log_map, a.anchors = anchors, a.prior = prior;
  a.h = h, a.w = w, a.cell = cell, a.gy = cdiv(h, cell), a.gx = cdiv(w, cell);
  a.sy = (double)AC_SIDE / vh, a.sx = (double)AC_SIDE / vw, a.vy0 = vy0, a.vx0 = vx0, a.vy1 = vy0 + vh, a.vx1 = vx0 + vw;
  a.dmin = min_depth, a.dmax = max_depth, a.reject = reject;
  a.n = n_cells, a.s = s_cells;
  hipLaunchKernelGGL(k_anchor_cells, dim3(cdiv((long)a.gy * a.gx, AC_WAVES), batch), dim3(AC_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

extern "C" int rdm_depth_anchor_field(const int32_t* n_cells, const double* s_cells, const double* prior, int32_t batch, int32_t gy, int32_t gx,
                                      int32_t fit, double sigma, double lambda, double* log_scale_out, int32_t* count_out, double* field,
                                      rdm_stream_t stream) {
  RDM_CHECK_ARG(n_cells && s_cells, "depth_anchor_field: n_cells and s_cells must not be NULL");
  RDM_CHECK_ARG(log_scale_out && count_out, "depth_anchor_field: log_scale_out and count_out must not be NULL");
  RDM_CHECK_ARG(aligned_to(s_cells, 8) && aligned_to(prior, 8) && aligned_to(log_scale_out, 8) && aligned_to(field, 8),
                "depth_anchor_field: s_cells, prior, log_scale_out and field must be 8-byte aligned");
  RDM_CHECK_ARG(aligned_to(n_cells, 4) && aligned_to(count_out, 4), "depth_anchor_field: n_cells and count_out must be 4-byte aligned");
  RDM_CHECK_ARG(batch > 0 && gy > 0 && gx > 0, "depth_anchor_field: need batch, gy, gx > 0 (got %d, %d, %d)", (int)batch, (int)gy, (int)gx);
  RDM_CHECK_ARG(batch <= 65535, "depth_anchor_field: batch %d is beyond the grid limit 65535", (int)batch);
  RDM_CHECK_ARG((long)gy * gx <= AF_CELLS, "depth_anchor_field: gy * gx (%d x %d) cells is beyond the %d whose planes fit the LDS; use a larger cell", (int)gy,
                (int)gx, AF_CELLS);
  RDM_CHECK_ARG(fit == RDM_ANCHOR_FIT_NONE || fit == RDM_ANCHOR_FIT_LOGMEAN, "depth_anchor_field: fit must be 0 (none) or 1 (logmean) (got %d)", (int)fit);
  RDM_CHECK_ARG(std::isfinite(sigma) && sigma >= 0, "depth_anchor_field: sigma must be finite and >= 0 (got %g)", sigma);
  RDM_CHECK_ARG(std::isfinite(lambda) && lambda >= 0, "depth_anchor_field: lambda must be finite and >= 0 (got %g)", lambda);
  RDM_CHECK_ARG(std::ceil(3.0 * sigma) <= RDM_ANCHOR_MAX_RADIUS, "depth_anchor_field: sigma %g gives a tap radius ceil(3 * sigma) above %d", sigma,
                RDM_ANCHOR_MAX_RADIUS);
  AfArgs a = {};
  a.n = n_cells, a.s = s_cells, a.prior = prior;
  a.gy = gy, a.gx = gx, a.fit = fit, a.rg = (int)std::ceil(3.0 * sigma);
  a.lambda = lambda, a.ls = log_scale_out, a.count = count_out, a.field = field;
  a.g[0] = 1.0;
  const double two_s2 = 2.0 * (sigma * sigma);
  for (int k = 1; k <= a.rg; ++k) a.g[k] = std::exp(-((double)k * (double)k) / two_s2);
  hipLaunchKernelGGL(k_anchor_field, dim3(batch), dim3(AF_THREADS), 0, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
