// Guided depth refinement in ONE launch (include/rdm_refine.h): a joint bilateral filter of a float32 depth frame under its uint8 colour frame,
// dilated taps, float64 weights from two small tables, optional filling of the pixels without a measurement, the float32 plane and the quantised
// 16-bit plane of a depth PNG.  Composed from single operators that is an unfold of depth and guide to (B, taps, h, w) intermediates, the
// weights, two sums over the taps, a divide, a cast and a round with clamp.
//
// Grid (tiles, batch), 256 threads, one workgroup per 32 x 16 tile of a sample.  The tile's cells with a halo of radius * step on every side
// are staged once into LDS by coalesced loads as two planes of one 32-bit word per pixel: the depth (0.0f where the depth is not valid or the
// cell is outside the frame, so the tap loop tests d > 0 and needs no bounds) and the three guide bytes packed into one word.  The 256-entry
// colour table E (float64, the device exp) and the spatial table ws sit in front of them.  LDS: 2128 + 8 * (16 + 2 halo) * (33 + 2 halo) bytes:
// 7.0 KiB at halo 1, 19.9 KiB at the default halo 12 (eight workgroups per CU, the wave limit too), 42.6 KiB at the largest halo 24 (three).
// A thread owns TWO adjacent pixels and walks the taps j outer, i inner; per tap and pixel one ds_read_b32 brings the depth, one more the
// guide if the depth is valid, and three ds_read_b64 the E entries.  Bank conflicts: all lanes of a wave read the SAME tap at a time, so step
// shifts every lane's address alike and never puts two lanes on one bank; what could is the lanes' own layout.  A 32-lane group (the unit
// that shares the 32 banks of a ds_read_b32) is two tile rows of 16 threads, 2 words apart: one row takes the 16 banks of one parity, and the
// row pitch is kept ODD in words so that the other row takes the other 16: the plane reads are conflict-free for every step.  (Depth and
// guide interleaved in one 8-byte cell put the threads of a row 4 words apart: 2-way conflicts in the 32-bit reads the compiler makes of it.)
// The E reads are indexed by colour differences: lanes with equal differences share an address (a broadcast), the others may collide; that
// is data, not layout.
// Stores (depthout_dev.h's store_pixels): the pair's float32 as one 8-byte store and its uint16 as one 4-byte store where the address is
// aligned, otherwise and at the ragged end of a row as scalars.
#include <cmath>

#include "rdm_common.h"
#include "depthout_dev.h"
#include "../../include/rdm_refine.h"

#pragma clang fp contract(off)                      // the float64 arithmetic is the header's, one IEEE operation per step

namespace rdm {

constexpr int RF_THREADS = 256;
constexpr int RF_TW = 32, RF_TH = 16;               // the tile
constexpr int RF_PX = 2;                            // adjacent pixels per thread: RF_TW / RF_PX * RF_TH threads
constexpr int RF_MAX_RADIUS = 8, RF_MAX_STEP = 16, RF_MAX_HALO = 24;
constexpr int RF_TABLE = 256 + RF_MAX_RADIUS + 2;   // doubles in front of the cells: E, then ws (padded to a 16-byte boundary)

struct RfArgs {
  const float* depth;
  const uint8_t* guide;
  float* f32;
  uint16_t* u16;
  int h, w, radius, step, fill;
  int halo, lw, lh, sw;                             // lh rows of sw staged cells at a pitch of lw (odd) words; sw = RF_TW + 2 * halo
  int tiles_x;
  double c2;                                        // 2 * sigma_color^2
  double unit;
  double ws[RF_MAX_RADIUS + 1];
};

__global__ __launch_bounds__(RF_THREADS) void k_depth_refine(RfArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rf_lds[];
  double* __restrict__ E = (double*)rf_lds;
  double* __restrict__ ws = E + 256;
  float* __restrict__ dcell = (float*)(E + RF_TABLE);
  uint32_t* __restrict__ gcell = (uint32_t*)(dcell + a.lh * a.lw);
  const int tid = threadIdx.x, b = blockIdx.y;
  const int ty = blockIdx.x / a.tiles_x, tx = blockIdx.x - ty * a.tiles_x;
  const unsigned y0 = (unsigned)ty * RF_TH, x0 = (unsigned)tx * RF_TW;
  const int h = a.h, w = a.w, halo = a.halo, lw = a.lw;
  const float* __restrict__ depth = a.depth + (long)b * h * w;
  const uint8_t* __restrict__ guide = a.guide + (long)b * h * w * 3;

  // the tables
  {
    const double k = (double)tid;
    E[tid] = tid == 0 ? 1.0 : exp(-(k * k) / a.c2);
#pragma unroll
    for (int k2 = 0; k2 <= RF_MAX_RADIUS; ++k2)
      if (tid == k2) ws[k2] = a.ws[k2];
  }
  // the cells: consecutive threads take consecutive cells of a staged row
  const int ncell = a.lh * a.sw;
  for (int c = tid; c < ncell; c += RF_THREADS) {
    const int cy = c / a.sw, cx = c - cy * a.sw;
    const unsigned gy = y0 - (unsigned)halo + (unsigned)cy, gx = x0 - (unsigned)halo + (unsigned)cx;      // wraps below 0: fails the test
    float cd = 0.0f;
    uint32_t cg = 0u;
    if (gy < (unsigned)h && gx < (unsigned)w) {
      const long at = (long)gy * w + gx;
      const float d = depth[at];
      const uint8_t* g = guide + at * 3;
      cd = depth_measured(d) ? d : 0.0f;                                                                   // no depth range here, unlike depth_valid
      cg = (uint32_t)g[0] | (uint32_t)g[1] << 8 | (uint32_t)g[2] << 16;
    }
    dcell[cy * lw + cx] = cd;
    gcell[cy * lw + cx] = cg;
  }
  __syncthreads();

  const int ly = tid >> 4, lx = (tid & 15) * RF_PX;
  const unsigned y = y0 + (unsigned)ly, x = x0 + (unsigned)lx;
  if (y >= (unsigned)h || x >= (unsigned)w) return;                              // nothing to store; no barrier follows

  const int centre = (ly + halo) * lw + lx + halo;
  int cR[RF_PX], cG[RF_PX], cB[RF_PX];
  bool cvalid[RF_PX];
  double num[RF_PX], den[RF_PX];
#pragma unroll
  for (int p = 0; p < RF_PX; ++p) {
    const uint32_t c = gcell[centre + p];
    cvalid[p] = dcell[centre + p] > 0.0f;
    cR[p] = (int)(c & 255u), cG[p] = (int)((c >> 8) & 255u), cB[p] = (int)((c >> 16) & 255u);
    num[p] = 0.0, den[p] = 0.0;
  }
  const int r = a.radius, step = a.step;
  for (int j = -r; j <= r; ++j) {
    const double wj = ws[abs(j)];
    const int row = centre + j * step * lw;
    for (int i = -r; i <= r; ++i) {
      const double wsp = wj * ws[abs(i)];
      const int at = row + i * step;
#pragma unroll
      for (int p = 0; p < RF_PX; ++p) {
        const float d = dcell[at + p];
        if (d > 0.0f) {
          const uint32_t q = gcell[at + p];
          const int dR = abs((int)(q & 255u) - cR[p]), dG = abs((int)((q >> 8) & 255u) - cG[p]), dB = abs((int)((q >> 16) & 255u) - cB[p]);
          const double wc = (E[dR] * E[dG]) * E[dB];
          const double wt = wsp * wc;
          const double t = wt * (double)d;
          num[p] = num[p] + t;
          den[p] = den[p] + wt;
        }
      }
    }
  }

  float vf[RF_PX];
  uint16_t vu[RF_PX];
#pragma unroll
  for (int p = 0; p < RF_PX; ++p) {
    const bool ok = cvalid[p] || (a.fill != 0 && den[p] > 0.0);
    vf[p] = 0.0f, vu[p] = 0;
    if (ok) {
      const double D = num[p] / den[p];
      vf[p] = (float)D;
      vu[p] = depth_quantise(D, a.unit);
    }
  }
  const long at = (long)b * h * w + (long)y * w + x;
  if (a.f32) store_pixels(a.f32 + at, vf, x, (unsigned)w);
  if (a.u16) store_pixels(a.u16 + at, vu, x, (unsigned)w);
}

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_depth_refine(const float* depth, const uint8_t* guide, int32_t batch, int32_t h, int32_t w, int32_t radius, int32_t step,
                                double sigma_space, double sigma_color, int32_t fill, double unit, float* out_f32, uint16_t* out_u16,
                                rdm_stream_t stream) {
  RDM_CHECK_ARG(depth, "depth_refine: depth must not be NULL");
  RDM_CHECK_ARG(guide, "depth_refine: guide must not be NULL");
  RDM_CHECK_ARG(out_f32 || out_u16, "depth_refine: out_f32 and out_u16 must not both be NULL");
  RDM_CHECK_ARG(out_f32 != depth, "depth_refine: out_f32 must not be depth: the taps read neighbours, in place is not supported");
  if (const int rc = check_frame_shape("depth_refine", batch, h, w)) return rc;
  RDM_CHECK_ARG(radius >= 1 && radius <= RF_MAX_RADIUS, "depth_refine: radius must be in [1, %d] (got %d)", RF_MAX_RADIUS, (int)radius);
  RDM_CHECK_ARG(step >= 1 && step <= RF_MAX_STEP, "depth_refine: step must be in [1, %d] (got %d)", RF_MAX_STEP, (int)step);
  RDM_CHECK_ARG(radius * step <= RF_MAX_HALO, "depth_refine: radius * step must not exceed %d (got %d * %d)", RF_MAX_HALO, (int)radius, (int)step);
  RDM_CHECK_ARG(sigma_space > 0, "depth_refine: sigma_space must be positive, +inf allowed (got %g)", sigma_space);        // NaN fails
  RDM_CHECK_ARG(sigma_color > 0, "depth_refine: sigma_color must be positive, +inf allowed (got %g)", sigma_color);
  RDM_CHECK_ARG(fill == 0 || fill == 1, "depth_refine: fill must be 0 or 1 (got %d)", (int)fill);
  if (const int rc = check_depth_unit("depth_refine", unit)) return rc;
  RfArgs a = {};
  a.depth = depth, a.guide = guide, a.f32 = out_f32, a.u16 = out_u16;
  a.h = h, a.w = w, a.radius = radius, a.step = step, a.fill = fill;
  a.halo = radius * step;
  a.sw = RF_TW + 2 * a.halo, a.lh = RF_TH + 2 * a.halo;
  a.lw = a.sw | 1;                                      // an odd pitch: see the bank note at the top
  a.tiles_x = cdiv(w, RF_TW);
  {
#pragma clang fp contract(off)
    a.c2 = 2.0 * (sigma_color * sigma_color);
    const double s2 = 2.0 * (sigma_space * sigma_space);
    a.ws[0] = 1.0;
    for (int k = 1; k <= radius; ++k) {
      const double sk = (double)(k * step);
      a.ws[k] = std::exp(-(sk * sk) / s2);
    }
  }
  a.unit = unit;
  const long tiles = (long)a.tiles_x * cdiv(h, RF_TH);    // at most 2^31 / 512 + a row and a column of ragged tiles
  const size_t lds = sizeof(double) * RF_TABLE + 2 * sizeof(uint32_t) * (size_t)a.lh * a.lw;
  hipLaunchKernelGGL(k_depth_refine, dim3((unsigned)tiles, batch), dim3(RF_THREADS), lds, (hipStream_t)stream, a);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
