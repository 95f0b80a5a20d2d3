// Depth-map rendering in ONE launch (include/rdm_viz.h): up to three panels per image - network input | target | prediction - to one packed uint8
// RGB image.  It restates utils.py:71-91 (colored_depthmap, merge_into_row) + save_image's astype('uint8') on the device: bicubic resize of
// each map to the output size (the arithmetic of postproc_dev.h, so bit for bit rdm_resize_bicubic_f64), the per-image colour range, the jet
// table and the byte packing, which composed from single operators is a resize, two reductions, a normalisation, a gather and a cast per batch
// with two full-resolution float64 intermediates.
//
// Grid (batch * split): `split` workgroups of 256 threads per image.  The range of an image is needed by every workgroup that colours it, and one
// launch without atomics or a grid barrier leaves no way to exchange it: every workgroup of an image takes the minimum and maximum over ALL of
// the image's resized pixels itself (minimum and maximum do not depend on the order, so all of them arrive at the same bits), then colours its
// own rows.  With a fixed range the first sweep is skipped.
//
// Both sweeps walk the image the same way.  The panels side by side form a "merged row" of M = P*w pixels; a thread owns ONE merged column at a time
// (tile of 256 columns), so its panel and its horizontal cubic taps are fixed while it walks down the rows: they stay in registers.  The vertical
// taps of a chunk of VZ_ROWS rows are computed once per chunk by a few threads and shared through LDS.  What is left per pixel is the 16
// loads and 20 fused multiply-adds of the two dot4 stages.  Colouring writes 3 bytes per pixel into an LDS image of the tile (VZ_ROWS x 768
// bytes), each row shifted by its destination address mod 4, so that it leaves as aligned dwords, consecutive lanes to consecutive
// addresses.  Any width and any alignment of `out` is taken: the first and last dword of a row segment, where they are shared with a
// neighbouring segment (another tile, row, workgroup or the caller's bytes around `out`), leave as single bytes of this segment only.
#include "rdm_common.h"
#include "postproc_dev.h"
#include "../../include/rdm_viz.h"

namespace rdm {

constexpr int VZ_THREADS = 256;
constexpr int VZ_ROWS = 8;                          // rows per chunk: one LDS table of vertical taps, one LDS image of VZ_ROWS x 768 bytes
constexpr int VZ_TILE_DWORDS = VZ_THREADS * 3 / 4 + 1;     // 768 bytes + up to 3 of shift

// matplotlib's jet, 256 entries: (uint8) trunc(255 * component), r g b (tests/golden/viz_goldens.npz `lut8` pins it)
__constant__ uint8_t VZ_JET[768] = {
    0, 0, 127, 0, 0, 132, 0, 0, 136, 0, 0, 141, 0, 0, 145, 0, 0, 150, 0, 0, 154, 0, 0, 159, 0, 0, 163, 0, 0, 168, 0, 0, 172, 0, 0, 177, 0, 0, 182, 0, 0, 186, 0, 0, 191, 0, 0, 195,
    0, 0, 200, 0, 0, 204, 0, 0, 209, 0, 0, 213, 0, 0, 218, 0, 0, 222, 0, 0, 227, 0, 0, 232, 0, 0, 236, 0, 0, 241, 0, 0, 245, 0, 0, 250, 0, 0, 254, 0, 0, 255, 0, 0, 255, 0, 0, 255,
    0, 0, 255, 0, 4, 255, 0, 8, 255, 0, 12, 255, 0, 16, 255, 0, 20, 255, 0, 24, 255, 0, 28, 255, 0, 32, 255, 0, 36, 255, 0, 40, 255, 0, 44, 255, 0, 48, 255, 0, 52, 255, 0, 56, 255, 0, 60, 255,
    0, 64, 255, 0, 68, 255, 0, 72, 255, 0, 76, 255, 0, 80, 255, 0, 84, 255, 0, 88, 255, 0, 92, 255, 0, 96, 255, 0, 100, 255, 0, 104, 255, 0, 108, 255, 0, 112, 255, 0, 116, 255, 0, 120, 255, 0, 124, 255,
    0, 128, 255, 0, 132, 255, 0, 136, 255, 0, 140, 255, 0, 144, 255, 0, 148, 255, 0, 152, 255, 0, 156, 255, 0, 160, 255, 0, 164, 255, 0, 168, 255, 0, 172, 255, 0, 176, 255, 0, 180, 255, 0, 184, 255, 0, 188, 255,
    0, 192, 255, 0, 196, 255, 0, 200, 255, 0, 204, 255, 0, 208, 255, 0, 212, 255, 0, 216, 255, 0, 220, 254, 0, 224, 250, 0, 228, 247, 2, 232, 244, 5, 236, 241, 8, 240, 237, 12, 244, 234, 15, 248, 231, 18, 252, 228,
    21, 255, 225, 24, 255, 221, 28, 255, 218, 31, 255, 215, 34, 255, 212, 37, 255, 208, 41, 255, 205, 44, 255, 202, 47, 255, 199, 50, 255, 195, 54, 255, 192, 57, 255, 189, 60, 255, 186, 63, 255, 183, 66, 255, 179, 70, 255, 176,
    73, 255, 173, 76, 255, 170, 79, 255, 166, 83, 255, 163, 86, 255, 160, 89, 255, 157, 92, 255, 154, 95, 255, 150, 99, 255, 147, 102, 255, 144, 105, 255, 141, 108, 255, 137, 112, 255, 134, 115, 255, 131, 118, 255, 128, 121, 255, 125,
    124, 255, 121, 128, 255, 118, 131, 255, 115, 134, 255, 112, 137, 255, 108, 141, 255, 105, 144, 255, 102, 147, 255, 99, 150, 255, 95, 154, 255, 92, 157, 255, 89, 160, 255, 86, 163, 255, 83, 166, 255, 79, 170, 255, 76, 173, 255, 73,
    176, 255, 70, 179, 255, 66, 183, 255, 63, 186, 255, 60, 189, 255, 57, 192, 255, 54, 195, 255, 50, 199, 255, 47, 202, 255, 44, 205, 255, 41, 208, 255, 37, 212, 255, 34, 215, 255, 31, 218, 255, 28, 221, 255, 24, 224, 255, 21,
    228, 255, 18, 231, 255, 15, 234, 255, 12, 237, 255, 8, 241, 252, 5, 244, 248, 2, 247, 244, 0, 250, 240, 0, 254, 237, 0, 255, 233, 0, 255, 229, 0, 255, 226, 0, 255, 222, 0, 255, 218, 0, 255, 215, 0, 255, 211, 0,
    255, 207, 0, 255, 203, 0, 255, 200, 0, 255, 196, 0, 255, 192, 0, 255, 189, 0, 255, 185, 0, 255, 181, 0, 255, 177, 0, 255, 174, 0, 255, 170, 0, 255, 166, 0, 255, 163, 0, 255, 159, 0, 255, 155, 0, 255, 152, 0,
    255, 148, 0, 255, 144, 0, 255, 140, 0, 255, 137, 0, 255, 133, 0, 255, 129, 0, 255, 126, 0, 255, 122, 0, 255, 118, 0, 255, 115, 0, 255, 111, 0, 255, 107, 0, 255, 103, 0, 255, 100, 0, 255, 96, 0, 255, 92, 0,
    255, 89, 0, 255, 85, 0, 255, 81, 0, 255, 77, 0, 255, 74, 0, 255, 70, 0, 255, 66, 0, 255, 63, 0, 255, 59, 0, 255, 55, 0, 255, 52, 0, 255, 48, 0, 255, 44, 0, 255, 40, 0, 255, 37, 0, 255, 33, 0,
    255, 29, 0, 255, 26, 0, 255, 22, 0, 254, 18, 0, 250, 15, 0, 245, 11, 0, 241, 7, 0, 236, 3, 0, 232, 0, 0, 227, 0, 0, 222, 0, 0, 218, 0, 0, 213, 0, 0, 209, 0, 0, 204, 0, 0, 200, 0, 0,
    195, 0, 0, 191, 0, 0, 186, 0, 0, 182, 0, 0, 177, 0, 0, 172, 0, 0, 168, 0, 0, 163, 0, 0, 159, 0, 0, 154, 0, 0, 150, 0, 0, 145, 0, 0, 141, 0, 0, 136, 0, 0, 132, 0, 0, 127, 0, 0,
};

struct VizMap {            // one depth panel
  const void* p;           // (batch,1,h,w), NULL = panel absent
  int is_f64, h, w;
  int resize;              // (h, w) differs from the output size
};

__device__ __forceinline__ double viz_load(const void* p, int is_f64, long i) { return is_f64 ? ((const double*)p)[i] : (double)((const float*)p)[i]; }

// bicubic_at (postproc_dev.h) with the taps precomputed: rows along x first, then the four rows along y
__device__ __forceinline__ double viz_sample(const void* p, int is_f64, const CubicAxis& ry, const CubicAxis& cx) {
  double rows[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = viz_load(p, is_f64, ry.o[i] + cx.o[j]);
    rows[i] = dot4(v, cx.c);
  }
  return dot4(rows, ry.c);
}

// matplotlib Colormap.__call__ on a float64 array, then 255 * rgb and astype('uint8'): r | g << 8 | b << 16
__device__ __forceinline__ uint32_t viz_colour(double v, double lo, double hi) {
#pragma clang fp contract(off)
  const double x = (v - lo) / (hi - lo);
  const double xa = x * 256.0;
  if (xa != xa) return 0;
  const int idx = xa < 0 ? 0 : xa >= 256.0 ? 255 : (int)xa;
  return (uint32_t)VZ_JET[3 * idx] | (uint32_t)VZ_JET[3 * idx + 1] << 8 | (uint32_t)VZ_JET[3 * idx + 2] << 16;
}

__device__ __forceinline__ uint32_t viz_byte(float x) {
  const float s = 255.0f * x;
  return s >= 255.0f ? 255u : s > 0.0f ? (uint32_t)s : 0u;       // (uint8) trunc inside [0, 255]; saturates outside, NaN -> 0
}

struct VizState {
  __attribute__((aligned(16))) CubicAxis rowtab[2][VZ_ROWS];
  uint32_t stage[VZ_ROWS][VZ_TILE_DWORDS];
  double red[2][VZ_THREADS / 64];
};

// One sweep over rows [r0, r1) of image `img`.  STORE = false: minimum / maximum / any-NaN of the depth panels' pixels into (mn, mx, nan),
// per thread.  STORE = true: colour with (lo, hi) and store the rows.
template <bool STORE>
__device__ __forceinline__ void viz_sweep(VizState& S, const float* __restrict__ rgb, const VizMap (&maps)[2], int first_depth, int H, int W, int M, int img,
                                          int r0, int r1, double lo, double hi, uint8_t* __restrict__ out, double& mn, double& mx, bool& nan) {
  const int tid = threadIdx.x;
  const void* base[2];
#pragma unroll
  for (int k = 0; k < 2; ++k)
    base[k] = !maps[k].p ? nullptr
              : maps[k].is_f64 ? (const void*)((const double*)maps[k].p + (long)img * maps[k].h * maps[k].w)
                               : (const void*)((const float*)maps[k].p + (long)img * maps[k].h * maps[k].w);
  const float* rgb_img = rgb ? rgb + (long)img * 3 * H * W : nullptr;
  const long row_bytes = (long)M * 3;
  uint8_t* stage8 = (uint8_t*)&S.stage[0][0];

  for (int rc = r0; rc < r1; rc += VZ_ROWS) {
    const int nr = min(VZ_ROWS, r1 - rc);
    __syncthreads();                                   // the previous chunk's readers of rowtab are done
    if (tid < 2 * VZ_ROWS) {
      const int k = tid / VZ_ROWS, r = tid % VZ_ROWS;
      const VizMap mk = k == 0 ? maps[0] : maps[1];
      if (r < nr && mk.p && mk.resize) cubic_axis(rc + r, mk.h, H, mk.w, S.rowtab[k][r]);
    }
    __syncthreads();
    for (int m0 = 0; m0 < M; m0 += VZ_THREADS) {
      const int m = m0 + tid;
      const int slot = m < M ? m / W : -1, ox = m < M ? m % W : 0;
      // slot -> what this merged column shows: 2 = nothing (past the row), -1 = rgb, 0 / 1 = maps[0] / maps[1]
      const int kind = slot < 0 ? 2 : slot < first_depth ? -1 : (maps[0].p ? slot - first_depth : 1);
      const bool depth = kind == 0 || kind == 1;
      const VizMap mp = kind == 0 ? maps[0] : maps[1];
      const void* bp = kind == 0 ? base[0] : base[1];
      CubicAxis cx;
      if (depth && mp.resize) cubic_axis(ox, mp.w, W, 1, cx);
      if (STORE || depth) {
        for (int r = 0; r < nr; ++r) {
          const int oy = rc + r;
          uint32_t px = 0;
          if (depth) {
            double v;
            if (mp.resize) {
              const CubicAxis ry = S.rowtab[kind][r];
              v = viz_sample(bp, mp.is_f64, ry, cx);
            } else {
              v = viz_load(bp, mp.is_f64, (long)oy * W + ox);
            }
            if (STORE) {
              px = viz_colour(v, lo, hi);
            } else if (v != v) {
              nan = true;
            } else {
              mn = fmin(mn, v);
              mx = fmax(mx, v);
            }
          } else if (STORE && kind == -1) {
            const long i = (long)oy * W + ox, plane = (long)H * W;
            px = viz_byte(rgb_img[i]) | viz_byte(rgb_img[plane + i]) << 8 | viz_byte(rgb_img[2 * plane + i]) << 16;
          }
          if (STORE) {
            const int shift = (int)(((uintptr_t)out + ((long)img * H + oy) * row_bytes + (long)m0 * 3) & 3);
            uint8_t* d = stage8 + r * (VZ_TILE_DWORDS * 4) + shift + tid * 3;
            d[0] = (uint8_t)px, d[1] = (uint8_t)(px >> 8), d[2] = (uint8_t)(px >> 16);
          }
        }
      }
      if (STORE) {
        __syncthreads();
        const int nb = min(VZ_THREADS, M - m0) * 3;                    // bytes of this tile per row
        for (int i = tid; i < nr * VZ_TILE_DWORDS; i += VZ_THREADS) {
          const int r = i / VZ_TILE_DWORDS, d = i % VZ_TILE_DWORDS;
          uint8_t* seg = out + ((long)img * H + rc + r) * row_bytes + (long)m0 * 3;      // first byte of the row segment
          const int shift = (int)((uintptr_t)seg & 3);
          const int b0 = max(4 * d, shift), b1 = min(4 * d + 4, shift + nb);            // this dword's bytes that belong to the segment
          uint8_t* g = seg - shift + 4 * d;                                              // 4-byte aligned
          if (b1 - b0 == 4)
            *(uint32_t*)g = S.stage[r][d];
          else
            for (int k = b0; k < b1; ++k) g[k - 4 * d] = stage8[r * (VZ_TILE_DWORDS * 4) + k];
        }
        __syncthreads();                                // the LDS image is free again
      }
    }
  }
}

__global__ __launch_bounds__(VZ_THREADS) void k_viz_rows(const float* __restrict__ rgb, VizMap a, VizMap b, int H, int W, int panels, double lo, double hi,
                                                         uint8_t* __restrict__ out, int split) {
  __shared__ VizState S;
  const int img = blockIdx.x / split, part = blockIdx.x % split;
  const VizMap maps[2] = {a, b};
  const int first_depth = rgb ? 1 : 0, M = panels * W;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  bool nan = false;

  if (lo != lo || hi != hi) {                                                  // a NaN end comes from the data
    viz_sweep<false>(S, rgb, maps, first_depth, H, W, M, img, 0, H, 0.0, 0.0, nullptr, mn, mx, nan);
    for (int o = 32; o > 0; o >>= 1) {
      mn = fmin(mn, __shfl_down(mn, o));
      mx = fmax(mx, __shfl_down(mx, o));
    }
    const int any_nan = __syncthreads_or(nan ? 1 : 0);
    if ((threadIdx.x & 63) == 0) S.red[0][threadIdx.x >> 6] = mn, S.red[1][threadIdx.x >> 6] = mx;
    __syncthreads();
    mn = S.red[0][0], mx = S.red[1][0];
    for (int i = 1; i < VZ_THREADS / 64; ++i) mn = fmin(mn, S.red[0][i]), mx = fmax(mx, S.red[1][i]);
    const double qnan = __builtin_nan("");
    if (lo != lo) lo = any_nan ? qnan : mn;                                    // np.min / np.max propagate a NaN pixel
    if (hi != hi) hi = any_nan ? qnan : mx;
  }
  const int r0 = (int)((long)part * H / split), r1 = (int)((long)(part + 1) * H / split);
  viz_sweep<true>(S, rgb, maps, first_depth, H, W, M, img, r0, r1, lo, hi, out, mn, mx, nan);
}

}  // namespace rdm

using namespace rdm;

extern "C" int rdm_viz_rows_u8(const float* rgb, const void* a, int32_t a_is_f64, int32_t ha, int32_t wa, const void* b, int32_t b_is_f64, int32_t hb, int32_t wb,
                               int32_t batch, int32_t h, int32_t w, double lo, double hi, uint8_t* out, int32_t split, rdm_stream_t stream) {
  RDM_CHECK_ARG(b && out, "viz_rows: b (the prediction) and out must not be NULL");
  RDM_CHECK_ARG(batch > 0 && h > 0 && w > 0, "viz_rows: need batch, h, w > 0 (got %d, %d, %d)", (int)batch, (int)h, (int)w);
  RDM_CHECK_ARG(hb > 0 && wb > 0 && (!a || (ha > 0 && wa > 0)), "viz_rows: need positive map sizes (a %dx%d, b %dx%d)", (int)ha, (int)wa, (int)hb, (int)wb);
  RDM_CHECK_ARG(split >= 0, "viz_rows: split must be >= 0 (got %d)", (int)split);
  const int panels = (rgb ? 1 : 0) + (a ? 1 : 0) + 1;
  const long M = (long)panels * w;
  RDM_CHECK_ARG(M * 3 <= 0x7fffffffL && (long)h * w <= 0x7fffffffL && (long)hb * wb <= 0x7fffffffL && (!a || (long)ha * wa <= 0x7fffffffL),
                "viz_rows: a plane or an output row is beyond the kernel's 32-bit index");
  if (split == 0) split = cdiv(512, batch);             // two workgroups per compute unit in all; tools/viz_bench.py --split compares
  split = std::min<int>(split, h);
  RDM_CHECK_ARG((long)batch * split <= 0x7fffffffL, "viz_rows: batch * split is beyond the grid limit");
  const VizMap ma = {a, a_is_f64 ? 1 : 0, a ? ha : 1, a ? wa : 1, a && (ha != h || wa != w) ? 1 : 0};
  const VizMap mb = {b, b_is_f64 ? 1 : 0, hb, wb, (hb != h || wb != w) ? 1 : 0};
  hipLaunchKernelGGL(k_viz_rows, dim3(batch * split), dim3(VZ_THREADS), 0, (hipStream_t)stream, rgb, ma, mb, h, w, panels, lo, hi, out, split);
  RDM_LAUNCH_OK();
  return RDM_OK;
}
