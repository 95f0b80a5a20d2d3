// The relative decoders d_6..d_10 (reference network/RDM_Net.py:137-162) on the bf16 inference path:
//   dense block (24 layers, the d_1 block's shape: the same kernels as rdm_net_forward_bf16, dense_block_bf16 in net.hip)
//   -> WSM chain (WSMLayer.forward, RDM_Net.py:163-236) -> conv1 1x1 -> 1 channel + bias (:156-157), f32 (B,1,S,S).
//
// Every conv of the WSM chain is ONE implicit-GEMM kernel family (wsm_conv_bf16_kernel): NHWC bf16 activations, bf16 weights packed
// once per weight update ([n][tap][k], k zero-padded to a multiple of 32 per tap), v_mfma_f32_16x16x32_bf16 with f32 accumulation,
// round-to-nearest-even on output, no atomics and no K split (the same launch gives the same bits).  Operand roles as in bf16.hip:
// the WEIGHT fragment is the MFMA A operand, the ACTIVATION fragment the B operand, so a lane holds 4 consecutive output channels of
// one pixel.  The activation address of (pixel (b,y,x), tap (dy,dx), k) is
//     b*sb + (y+dy-ph)*sy + (x+dx-pw)*sx + (k / cq)*sq + k % cq + xoff         (zero outside the image)
// which covers plain kxk "same" convs (cq = K per tap) and the WSM strip convs as rows-as-pixels GEMMs: the (3,S)/(1,S) conv after
// ZeroPad2d((0,0,1,1)) is a 3-tap conv over the rows of the map (pixel = row, k = (column, channel)); the (S,3)/(S,1) conv after
// ZeroPad2d((1,1,0,0)) is the same over the columns (pixel = column, k = (row, channel): sq = one row of the map).
// The epilogue routes column ranges ("segments") of the GEMM to their destinations:
//   WSM_PLAIN     bf16 into a channel slice (off, ld) of an NHWC buffer (the five 1x1 convs write conv1_1 straight into its slot of the
//                 layer's output and the other four into one scratch tensor)
//   WSM_SHUFFLE   ConvTranspose2d(k2,s2) as a 1x1 to 4 phases x Cp outputs, stored through the pixel shuffle into (B,2H,2W,C)
//   WSM_BCAST_*   the strip convs' one value per row (column) broadcast along the row (column) into its slot: the reference's `repeat`
//                 (:223-224) without an expand / cat pass
//   WSM_F32       f32 (conv1: the one-channel map the relative head consumes)
// so a WSM layer writes its (B,S,S,C) output once, in the reference's cat order (:234): out1_1, out2_1, out2_2, completion_vertical,
// completion_horizontal.
#include <algorithm>
#include <vector>

#include "rdm_common.h"
#include "elementwise.h"
#include "bf16.h"

namespace rdm {

enum { WSM_PLAIN = 0, WSM_SHUFFLE = 1, WSM_BCAST_ROWS = 2, WSM_BCAST_COLS = 3, WSM_F32 = 4 };

struct WsmSeg {
  void* dst; int n0, n1;      // GEMM columns [n0, n1) of this segment
  int nstore;                 // columns stored (from n0; SHUFFLE: channels per phase); the rest of the range is padding
  int ld, off, mode;          // destination pixel stride and channel offset (elements)
};

struct WsmConvArgs {
  const unsigned short* X; unsigned x_bytes;    // bf16 activations; x_bytes bounds every read (the buffer descriptor returns 0 beyond)
  long sb, sy, sx, sq; int cq, xoff;            // addressing (elements), see the header comment
  int B, H, W, kh, kw, ph, pw, kc, K;           // output grid == input grid; kc = K per tap (multiple of 32), K = kh*kw*kc
  const unsigned short* Wt; unsigned w_bytes; int N;   // bf16 [N rows (>= N, multiple of 64 allocated)][K]
  const float* bias; int nbias;                 // optional f32, bias[n] for n < nbias (0 beyond)
  int nseg; WsmSeg seg[4];
  int S;                                        // BCAST: broadcast length
};

// 4 consecutive channels of one pixel: one 8-byte store when all four are stored and 8-byte aligned, else 2-byte stores
__device__ __forceinline__ void st4(unsigned short* p, float v0, float v1, float v2, float v3, int cnt) {
  if (cnt >= 4 && (((uintptr_t)p & 7) == 0)) {
    *reinterpret_cast<uint2*>(p) = make_uint2(pack2_scalar(v0, v1), pack2_scalar(v2, v3));
    return;
  }
  if (cnt > 0) p[0] = bf1(v0);
  if (cnt > 1) p[1] = bf1(v1);
  if (cnt > 2) p[2] = bf1(v2);
  if (cnt > 3) p[3] = bf1(v3);
}

// Block = 4 wave64s (2 x 2), wave tile (MT*16 pixels) x (NT*16 outputs), K walked in 64-deep steps (2 MFMA k-steps);
// global -> registers (the next step's loads in flight under this step's MFMAs) -> swizzled LDS, 2 buffers, 1 barrier per step.
template <int MT, int NT>
__global__ __launch_bounds__(256, 2) void wsm_conv_bf16_kernel(WsmConvArgs p) {
  constexpr int BK = 64, BM = MT * 32, BN = NT * 32;
  constexpr int CH = BK / 8, RP = 256 / CH;
  constexpr int XL = BM / RP, WL = BN / RP;
  __shared__ __attribute__((aligned(16))) unsigned short lds[2 * (BM + BN) * BK];
  unsigned short* const Xs0 = lds;
  unsigned short* const Ws0 = lds + 2 * BM * BK;
  auto swz = [](int row) { return (row >> 1) & 7; };       // 128-byte rows: conflict-free ds_read_b128 (bf16.hip)

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int wrow = (wave >> 1) * MT * 16, wcol = (wave & 1) * NT * 16;
  const int n0 = blockIdx.x * BN, m0 = blockIdx.y * BM;
  const int HW = p.H * p.W, M = p.B * HW;
  const __amdgpu_buffer_rsrc_t srdX = make_srd(p.X, p.x_bytes), srdW = make_srd(p.Wt, p.w_bytes);

  const int ch = tid % CH, r0 = tid / CH;
  long xbase[XL];
  int xy[XL], xx[XL];
#pragma unroll
  for (int i = 0; i < XL; ++i) {
    const int m = m0 + r0 + RP * i;
    if (m < M) {
      const int b = m / HW, rem = m - b * HW, y = rem / p.W, x = rem - y * p.W;
      xbase[i] = b * p.sb + y * p.sy + x * p.sx + p.xoff;
      xy[i] = y; xx[i] = x;
    } else {
      xbase[i] = 0; xy[i] = -1000000; xx[i] = 0;           // never inside the image
    }
  }
  unsigned woff[WL];
#pragma unroll
  for (int i = 0; i < WL; ++i) {
    const int n = n0 + r0 + RP * i;
    woff[i] = n < p.N ? (unsigned)n * (unsigned)(p.K * 2) + (unsigned)(ch * 16) : OOB;
  }
  struct Stage { uint4 rx[XL]; uint4 rw[WL]; };
  Stage S[2];
  auto load_step = [&](int kt, Stage& St) {
    const int k = kt * BK + ch * 8;
    const bool kok = k < p.K;                                 // K is a multiple of 8: a chunk is all in or all out
    const int tap = kok ? k / p.kc : 0, kk = k - tap * p.kc;
    const int dy = tap / p.kw, dx = tap - dy * p.kw;
    const int q = kk / p.cq, c = kk - q * p.cq;
    const long koff = (long)(dy - p.ph) * p.sy + (long)(dx - p.pw) * p.sx + q * p.sq + c;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int y = xy[i] + dy - p.ph, x = xx[i] + dx - p.pw;
      const bool ok = kok && y >= 0 && y < p.H && x >= 0 && x < p.W;
      St.rx[i] = bld_u4(srdX, ok ? (unsigned)((xbase[i] + koff) * 2) : OOB);
    }
    const unsigned kb = (unsigned)(kt * BK * 2);
#pragma unroll
    for (int i = 0; i < WL; ++i) St.rw[i] = bld_u4(srdW, (kok && woff[i] != OOB) ? woff[i] + kb : OOB);
  };
  auto store_step = [&](int buf, const Stage& St) {
    unsigned short* Xs = Xs0 + buf * BM * BK;
    unsigned short* Ws = Ws0 + buf * BN * BK;
#pragma unroll
    for (int i = 0; i < XL; ++i) {
      const int r = r0 + RP * i;
      *reinterpret_cast<uint4*>(Xs + r * BK + ((ch ^ swz(r)) << 3)) = St.rx[i];
    }
#pragma unroll
    for (int i = 0; i < WL; ++i) {
      const int r = r0 + RP * i;
      *reinterpret_cast<uint4*>(Ws + r * BK + ((ch ^ swz(r)) << 3)) = St.rw[i];
    }
  };

  f32x4 acc[MT][NT];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int nk = (p.K + BK - 1) / BK;
  const int sw = swz(l16);
  auto mma_step = [&](int buf) {
    const unsigned short* Xs = Xs0 + buf * BM * BK;
    const unsigned short* Ws = Ws0 + buf * BN * BK;
#pragma unroll
    for (int ks = 0; ks < BK / 32; ++ks) {
      const int co = ((ks * 4 + g) ^ sw) << 3;
      bf16x8 wf[NT], xf[MT];
#pragma unroll
      for (int j = 0; j < NT; ++j) wf[j] = *reinterpret_cast<const bf16x8*>(Ws + (wcol + j * 16 + l16) * BK + co);
#pragma unroll
      for (int i = 0; i < MT; ++i) xf[i] = *reinterpret_cast<const bf16x8*>(Xs + (wrow + i * 16 + l16) * BK + co);
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j], xf[i], acc[i][j], 0, 0, 0);
    }
  };
  load_step(0, S[0]);
  if (nk > 1) load_step(1, S[1]);
  store_step(0, S[0]);
  if (nk > 2) load_step(2, S[0]);
  __syncthreads();
  for (int k = 0; k < nk; ++k) {                              // step k: LDS buffer k & 1; step k+1 in S[(k+1)&1], k+2 loading into S[k&1]
    mma_step(k & 1);
    if (k + 1 < nk) {
      store_step((k + 1) & 1, S[(k + 1) & 1]);
      if (k + 3 < nk) load_step(k + 3, S[(k + 1) & 1]);
    }
    __syncthreads();
  }

  // D[row = output 4g+r of the n-tile][col = pixel l16 of the m-tile]
#pragma unroll
  for (int j = 0; j < NT; ++j) {
    const int n = n0 + wcol + j * 16 + g * 4;
    if (n >= p.N) continue;
    int s = 0;
    while (s + 1 < p.nseg && n >= p.seg[s].n1) ++s;
    const WsmSeg& sg = p.seg[s];
    if (n < sg.n0 || n >= sg.n1) continue;
    const int jn = n - sg.n0;
    float b4[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) b4[r] = (p.bias && n + r < p.nbias) ? p.bias[n + r] : 0.f;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const int m = m0 + wrow + i * 16 + l16;
      if (m >= M) continue;
      const float v0 = acc[i][j][0] + b4[0], v1 = acc[i][j][1] + b4[1], v2 = acc[i][j][2] + b4[2], v3 = acc[i][j][3] + b4[3];
      if (sg.mode == WSM_F32) {
        float* d = static_cast<float*>(sg.dst) + (long)m * sg.ld + sg.off + jn;
        const int cnt = sg.nstore - jn;
        if (cnt > 0) d[0] = v0;
        if (cnt > 1) d[1] = v1;
        if (cnt > 2) d[2] = v2;
        if (cnt > 3) d[3] = v3;
        continue;
      }
      unsigned short* dst = static_cast<unsigned short*>(sg.dst);
      if (sg.mode == WSM_PLAIN) {
        st4(dst + (long)m * sg.ld + sg.off + jn, v0, v1, v2, v3, sg.nstore - jn);
      } else if (sg.mode == WSM_SHUFFLE) {                    // column jn = phase * cp + channel; phase (r, s) -> output pixel (2y+r, 2x+s)
        const int cp = (sg.n1 - sg.n0) >> 2, ph = jn / cp, co = jn - ph * cp;
        const int b = m / HW, rem = m - b * HW, y = rem / p.W, x = rem - y * p.W;
        const long pix = ((long)b * 2 * p.H + 2 * y + (ph >> 1)) * (2 * p.W) + 2 * x + (ph & 1);
        st4(dst + pix * sg.ld + sg.off + co, v0, v1, v2, v3, sg.nstore - co);
      } else {                                                // strip: m = b*S + t, t = row (BCAST_ROWS) or column (BCAST_COLS)
        const int b = m / p.S, t = m - b * p.S;
        const long step = sg.mode == WSM_BCAST_ROWS ? 1 : p.S;
        const long first = sg.mode == WSM_BCAST_ROWS ? (long)t * p.S : t;
        unsigned short* d = dst + ((long)b * p.S * p.S + first) * sg.ld + sg.off + jn;
        for (int u = 0; u < p.S; ++u) st4(d + u * step * sg.ld, v0, v1, v2, v3, sg.nstore - jn);
      }
    }
  }
}

__global__ __launch_bounds__(256) void k_wsm_pack_bf16(const float* __restrict__ src, unsigned short* __restrict__ dst, int O, int row_off, int K, int kc,
                                                       int T, int Q, int cq, int creal, long so, long sc, long sq, long st) {
  // dst[(row_off + o) * K + t*kc + q*cq + c] = bf16(src[o*so + c*sc + q*sq + t*st]) for c < creal (everything else stays as the caller zeroed it)
  const long total = (long)O * T * Q * creal;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % creal);
    long r = i / creal;
    const int q = (int)(r % Q); r /= Q;
    const int t = (int)(r % T);
    const int o = (int)(r / T);
    dst[(long)(row_off + o) * K + (long)t * kc + (long)q * cq + c] = bf1(src[o * so + c * sc + q * sq + t * st]);
  }
}

__global__ __launch_bounds__(256) void k_nchw_f32_to_nhwc_bf16(const float* __restrict__ x, unsigned short* __restrict__ y, int ldy, int B, int C, int HW) {
  const long total = (long)B * C * HW;
  for (long i = blockIdx.x * 256L + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int c = (int)(i % C);
    const long pix = i / C;
    const int b = (int)(pix / HW), s = (int)(pix % HW);
    y[pix * ldy + c] = bf1(x[((long)b * C + c) * HW + s]);
  }
}

static int pack_w(const float* src, void* dst, int O, int row_off, int K, int kc, int T, int Q, int cq, int creal, long so, long sc, long sq, long st,
                  hipStream_t s) {
  const long total = (long)O * T * Q * creal;
  if (total <= 0) return RDM_OK;
  const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
  k_wsm_pack_bf16<<<blocks, 256, 0, s>>>(src, static_cast<unsigned short*>(dst), O, row_off, K, kc, T, Q, cq, creal, so, sc, sq, st);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

int launch_wsm_conv_bf16(const WsmConvArgs& a, hipStream_t s) {
  RDM_CHECK_ARG(a.X && a.Wt && a.nseg >= 1 && a.nseg <= 4, "wsm conv: bad arguments");
  RDM_CHECK_ARG(a.K > 0 && a.K % 8 == 0 && a.kc % 8 == 0 && a.cq % 8 == 0 && a.xoff % 8 == 0 && a.sx % 8 == 0 && a.sy % 8 == 0 && a.sb % 8 == 0 && a.sq % 8 == 0,
                "wsm conv: K, K per tap, channel groups, offsets and strides must be multiples of 8");
  RDM_CHECK_ARG(((uintptr_t)a.X & 15) == 0 && ((uintptr_t)a.Wt & 15) == 0, "wsm conv: operands must be 16-byte aligned");
  RDM_CHECK_ARG(a.B > 0 && a.H > 0 && a.W > 0 && a.N > 0, "wsm conv: empty geometry");
  for (int i = 0; i < a.nseg; ++i) {
    const WsmSeg& g = a.seg[i];
    RDM_CHECK_ARG(g.dst && g.n0 % 4 == 0 && g.n1 % 4 == 0 && g.n0 < g.n1 && g.ld > 0 && g.off >= 0 && g.mode >= 0 && g.mode <= WSM_F32, "wsm conv: bad segment %d", i);
    RDM_CHECK_ARG(g.mode != WSM_SHUFFLE || (g.n1 - g.n0) % 16 == 0, "wsm conv: pixel-shuffle segment width must be 4 phases x a multiple of 4");
    RDM_CHECK_ARG((g.mode != WSM_BCAST_ROWS && g.mode != WSM_BCAST_COLS) || (a.W == 1 && a.H == a.S), "wsm conv: strip launches are (B, S, 1) images");
  }
  const long M = (long)a.B * a.H * a.W;
  const long tiles128 = ((M + 127) / 128) * ((a.N + 63) / 64);
  if (tiles128 >= 512) {
    dim3 grid((a.N + 63) / 64, (unsigned)((M + 127) / 128));
    wsm_conv_bf16_kernel<4, 2><<<grid, 256, 0, s>>>(a);
  } else {
    dim3 grid((a.N + 63) / 64, (unsigned)((M + 63) / 64));
    wsm_conv_bf16_kernel<2, 2><<<grid, 256, 0, s>>>(a);
  }
  RDM_LAUNCH_OK();
  return RDM_OK;
}

static WsmSeg seg(void* dst, int n0, int n1, int nstore, int ld, int off, int mode) { return WsmSeg{dst, n0, n1, nstore, ld, off, mode}; }
static int pad32(int c) { return (c + 31) / 32 * 32; }
static bool fits32(long elems) { return elems < (1L << 30); }       // bf16 elements the 32-bit byte offsets of a buffer load can address
static int pad64(int c) { return (c + 63) / 64 * 64; }

// a "same" kxk conv over an NHWC map (plain addressing)
static WsmConvArgs conv_args(const void* x, long x_elems, int ldx, int xoff, int cin, int B, int H, int W, int k, const void* w, int N, const float* bias, int nbias) {
  WsmConvArgs a{};
  a.X = static_cast<const unsigned short*>(x); a.x_bytes = (unsigned)(x_elems * 2);
  a.sx = ldx; a.sy = (long)W * ldx; a.sb = (long)H * W * ldx; a.xoff = xoff;
  a.kc = pad32(cin); a.cq = a.kc; a.sq = 0;
  a.B = B; a.H = H; a.W = W; a.kh = a.kw = k; a.ph = a.pw = k / 2; a.K = k * k * a.kc;
  a.Wt = static_cast<const unsigned short*>(w); a.w_bytes = (unsigned)((size_t)pad64(N) * a.K * 2); a.N = N;
  a.bias = bias; a.nbias = nbias;
  return a;
}
// the WSM strip conv over a (B,S,S) map with channels [xoff, xoff + cw) of pixel stride ldx (cw = its padded width):
// columns = false: the (3,S)/(1,S) conv -> one value per row;  columns = true: the (S,3)/(S,1) conv -> one value per column
static WsmConvArgs strip_args(const void* x, long x_elems, int ldx, int xoff, int cw, int B, int S, bool columns, const void* w, int N, const float* bias, int nbias) {
  WsmConvArgs a{};
  a.X = static_cast<const unsigned short*>(x); a.x_bytes = (unsigned)(x_elems * 2);
  a.sb = (long)S * S * ldx; a.xoff = xoff; a.cq = cw;
  a.sy = columns ? ldx : (long)S * ldx;                       // pixel = a row (columns = 0) or a column of the map
  a.sq = columns ? (long)S * ldx : ldx;                       // k = (position along it, channel)
  a.sx = 8;                                                   // W == 1: never stepped
  a.B = B; a.H = S; a.W = 1; a.kh = 3; a.kw = 1; a.ph = 1; a.pw = 0; a.kc = S * cw; a.K = 3 * a.kc;
  a.Wt = static_cast<const unsigned short*>(w); a.w_bytes = (unsigned)((size_t)pad64(N) * a.K * 2); a.N = N;
  a.bias = bias; a.nbias = nbias; a.S = S;
  return a;
}

// =============================================================================================
// per-decoder plan: prepared-weight layout and workspace layout
// =============================================================================================
static constexpr int kGrowth = 48, kLayers = 24, kCin0 = 1056, kCtot = 2208, kCb = 384;
static const int kWsmC[4] = {1664, 832, 416, 208};
static const int kWsmS[4] = {16, 32, 64, 128};

struct RelWsm {                  // one WSM layer
  int C, S, raw, ki, wi, cp, kip, wip, nf, kraw;
  size_t ia_w, ia_b, dc_w, dc_b, f5_w, f5_b, c3_w, c3_b, c5_w, c5_b, sv_w, sv_b, sh_w, sh_b;   // weight buffer (bytes)
  size_t t, out1, T, out;                                                                        // workspace (bytes)
};
struct RelPlan {
  int id, nw, B, cf, sf;
  size_t dw1[kLayers], dw3[kLayers], dbn1[kLayers], dbn2[kLayers];
  RelWsm L[4];
  size_t c1_w, c1_b, wbytes = 0;
  size_t blk, Y, partial, partial_floats, wsbytes = 0;
  size_t bst, yst, aff1, aff2, stats, stats_floats, train_wsbytes = 0;    // training form (plan_rel_train): behind the eval layout
};

static size_t take(size_t& off, size_t bytes) {
  const size_t o = off;
  off = (off + bytes + 255) & ~(size_t)255;
  return o;
}

static void plan_rel(int id, int B, RelPlan& P) {
  P.id = id; P.nw = id - 6; P.B = B;
  size_t w = 0, a = 0;
  for (int i = 0; i < kLayers; ++i) {
    const int cin = kCin0 + i * kGrowth;
    P.dw1[i] = take(w, (size_t)kCb * cin * 2);
    P.dw3[i] = take(w, (size_t)9 * kGrowth * kCb * 2);
    P.dbn1[i] = take(w, (size_t)4 * cin * 4);
    P.dbn2[i] = take(w, (size_t)4 * kCb * 4);
  }
  const int M8 = B * 64;
  P.blk = take(a, (size_t)M8 * kCtot * 2);
  P.Y = take(a, (size_t)M8 * kCb * 2);
  P.partial_floats = std::max((size_t)8 * M8 * kCb, (size_t)16 * M8 * kGrowth);
  P.partial = take(a, P.partial_floats * 4);
  int raw = kCtot;
  for (int l = 0; l < P.nw; ++l) {
    RelWsm& R = P.L[l];
    R.C = kWsmC[l]; R.S = kWsmS[l]; R.raw = raw; R.ki = R.C / 4; R.wi = R.C / 8;
    R.cp = pad32(R.C); R.kip = pad32(R.ki); R.wip = pad32(R.wi); R.kraw = pad32(raw);
    R.nf = 3 * R.kip + 2 * R.wip;
    const int h = R.S / 2;
    R.ia_w = take(w, (size_t)pad64(R.cp) * R.kraw * 2);       R.ia_b = take(w, (size_t)pad64(R.cp) * 4);
    R.dc_w = take(w, (size_t)pad64(4 * R.cp) * R.cp * 2);     R.dc_b = take(w, (size_t)pad64(4 * R.cp) * 4);
    R.f5_w = take(w, (size_t)pad64(R.nf) * R.cp * 2);         R.f5_b = take(w, (size_t)pad64(R.nf) * 4);
    R.c3_w = take(w, (size_t)pad64(R.kip) * 9 * R.kip * 2);   R.c3_b = take(w, (size_t)pad64(R.kip) * 4);
    R.c5_w = take(w, (size_t)pad64(R.kip) * 25 * R.kip * 2);  R.c5_b = take(w, (size_t)pad64(R.kip) * 4);
    R.sv_w = take(w, (size_t)pad64(R.wip) * 3 * R.S * R.wip * 2); R.sv_b = take(w, (size_t)pad64(R.wip) * 4);
    R.sh_w = take(w, (size_t)pad64(R.wip) * 3 * R.S * R.wip * 2); R.sh_b = take(w, (size_t)pad64(R.wip) * 4);
    R.t = take(a, (size_t)B * h * h * R.cp * 2);
    R.out1 = take(a, (size_t)B * R.S * R.S * R.cp * 2);
    R.T = take(a, (size_t)B * R.S * R.S * (R.nf - R.kip) * 2);
    R.out = take(a, (size_t)B * R.S * R.S * R.C * 2);
    raw = R.C;
  }
  P.cf = raw; P.sf = P.nw ? kWsmS[P.nw - 1] : 8;
  P.c1_w = take(w, (size_t)64 * pad32(P.cf) * 2);
  P.c1_b = take(w, 64 * 4);
  P.wbytes = w;
  P.wsbytes = a;
}

// the training forward's extra workspace, appended to the eval layout (which stays as it is): block / bottleneck statistics (f64),
// BatchNorm affines, the statistics epilogues' f32 scratch
static void plan_rel_train(RelPlan& P) {
  size_t a = P.wsbytes;
  const int M8 = P.B * 64;
  P.bst = take(a, (size_t)2 * kCtot * 8);
  P.yst = take(a, (size_t)2 * kCb * 8);
  P.aff1 = take(a, (size_t)4 * kCtot * 4);
  P.aff2 = take(a, (size_t)4 * kCb * 4);
  P.stats_floats = bf16_stats_floats(M8, kCb);
  P.stats = take(a, P.stats_floats * 4);
  P.train_wsbytes = a;
}

template <class T> static T* at(void* base, size_t off) { return reinterpret_cast<T*>(static_cast<char*>(base) + off); }
static const float* Fp(void* const* T, int i) { return static_cast<const float*>(T[i]); }

// state_dict order of a Decoder (RDM_Net.py:137-148): dense_layer.denselayer1..24 (norm1 w b rm rv nbt, conv1, norm2 w b rm rv nbt, conv2),
// wsm_block.WSM_k (deconv1.0 w b, conv1_1..conv1_5 w b, conv2_1 w b, conv2_2 w b, wsm_wx3.1 w b, wsm_3xh.1 w b, input_adjustment_layer w b),
// conv1 w b, conv2 w b
static int rel_num_tensors(int id) { return 12 * kLayers + 22 * (id - 6) + 4; }

// WSM chain + conv1 of a relative decoder (RDM_Net.py:151-157) from the finished dense block in the workspace: no BatchNorm, so the eval
// and the training forward enqueue the same launches
static int rel_wsm_chain(const RelPlan& P, int batch, void* wb, void* ws, float* out_map, hipStream_t s) {
  int rc;
  const int M8 = batch * 64;
  unsigned short* blk = at<unsigned short>(ws, P.blk);
  const void* x = blk;
  long x_elems = (long)M8 * kCtot;
  int ldx = kCtot;
  for (int l = 0; l < P.nw; ++l) {
    const RelWsm& R = P.L[l];
    const int h = R.S / 2, S = R.S, C = R.C;
    const long Mo = (long)batch * S * S;
    unsigned short* t = at<unsigned short>(ws, R.t);
    unsigned short* out1 = at<unsigned short>(ws, R.out1);
    unsigned short* Tt = at<unsigned short>(ws, R.T);
    unsigned short* out = at<unsigned short>(ws, R.out);
    const int ldT = R.nf - R.kip;
    {  // input_adjustment_layer: 1x1 raw -> C (+bias), all cp columns (the pad columns are exact zeros)
      WsmConvArgs a = conv_args(x, x_elems, ldx, 0, R.raw, batch, h, h, 1, at<char>(wb, R.ia_w), R.cp, at<float>(wb, R.ia_b), R.cp);
      a.nseg = 1; a.seg[0] = seg(t, 0, R.cp, R.cp, R.cp, 0, WSM_PLAIN);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // deconv1: 1x1 to 4 phases x cp, stored through the pixel shuffle
      WsmConvArgs a = conv_args(t, (long)batch * h * h * R.cp, R.cp, 0, R.cp, batch, h, h, 1, at<char>(wb, R.dc_w), 4 * R.cp, at<float>(wb, R.dc_b), 4 * R.cp);
      a.nseg = 1; a.seg[0] = seg(out1, 0, 4 * R.cp, R.cp, R.cp, 0, WSM_SHUFFLE);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // conv1_1..conv1_5 as ONE GEMM: conv1_1 -> its slot of the output, the other four -> the scratch T
      WsmConvArgs a = conv_args(out1, Mo * R.cp, R.cp, 0, R.cp, batch, S, S, 1, at<char>(wb, R.f5_w), R.nf, at<float>(wb, R.f5_b), R.nf);
      a.nseg = 2;
      a.seg[0] = seg(out, 0, R.kip, R.ki, C, 0, WSM_PLAIN);
      a.seg[1] = seg(Tt, R.kip, R.nf, ldT, ldT, 0, WSM_PLAIN);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // conv2_1 3x3 p1 on out1_2 -> slot 1
      WsmConvArgs a = conv_args(Tt, Mo * ldT, ldT, 0, R.kip, batch, S, S, 3, at<char>(wb, R.c3_w), R.ki, at<float>(wb, R.c3_b), R.ki);
      a.nseg = 1; a.seg[0] = seg(out, 0, R.kip, R.ki, C, R.ki, WSM_PLAIN);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // conv2_2 5x5 p2 on out1_3 -> slot 2
      WsmConvArgs a = conv_args(Tt, Mo * ldT, ldT, R.kip, R.kip, batch, S, S, 5, at<char>(wb, R.c5_w), R.ki, at<float>(wb, R.c5_b), R.ki);
      a.nseg = 1; a.seg[0] = seg(out, 0, R.kip, R.ki, C, 2 * R.ki, WSM_PLAIN);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // wsm_3xh on out1_5: one value per COLUMN, repeated along H -> completion_vertical, slot 3
      WsmConvArgs a = strip_args(Tt, Mo * ldT, ldT, 2 * R.kip + R.wip, R.wip, batch, S, true, at<char>(wb, R.sh_w), R.wi, at<float>(wb, R.sh_b), R.wi);
      a.nseg = 1; a.seg[0] = seg(out, 0, R.wip, R.wi, C, 3 * R.ki, WSM_BCAST_COLS);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    {  // wsm_wx3 on out1_4: one value per ROW, repeated along W -> completion_horizontal, slot 4
      WsmConvArgs a = strip_args(Tt, Mo * ldT, ldT, 2 * R.kip, R.wip, batch, S, false, at<char>(wb, R.sv_w), R.wi, at<float>(wb, R.sv_b), R.wi);
      a.nseg = 1; a.seg[0] = seg(out, 0, R.wip, R.wi, C, 3 * R.ki + R.wi, WSM_BCAST_ROWS);
      if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
    }
    x = out; x_elems = Mo * C; ldx = C;
  }
  {  // conv1: 1x1 -> 1 channel + bias, f32 (B,1,S,S) (NCHW with one channel == NHWC)
    WsmConvArgs a = conv_args(x, x_elems, ldx, 0, P.cf, batch, P.sf, P.sf, 1, at<char>(wb, P.c1_w), 1, at<float>(wb, P.c1_b), 1);
    a.nseg = 1; a.seg[0] = seg(out_map, 0, 4, 1, 1, 0, WSM_F32);
    if ((rc = launch_wsm_conv_bf16(a, s))) return rc;
  }
  return RDM_OK;
}

}  // namespace rdm

using namespace rdm;

extern "C" {

int rdm_rel_num_tensors(int32_t id) { return (id >= 6 && id <= 10) ? rel_num_tensors(id) : RDM_ERR_BAD_ARGUMENT; }

size_t rdm_rel_bf16_weight_bytes(int32_t id) {
  if (id < 6 || id > 10) return 0;
  RelPlan P;
  plan_rel(id, 1, P);
  return P.wbytes;
}

size_t rdm_rel_bf16_workspace_bytes(int32_t id, int32_t batch) {
  if (id < 6 || id > 10 || batch <= 0) return 0;
  RelPlan P;
  plan_rel(id, batch, P);
  return P.wsbytes;
}

int rdm_rel_bf16_prepare(int32_t id, void* const* T, void* wbuf, size_t wbuf_bytes, rdm_stream_t stream) {
  RDM_CHECK_ARG(id >= 6 && id <= 10, "relative decoder id must be 6..10, got %d", id);
  RDM_CHECK_ARG(T && wbuf, "NULL argument");
  RDM_CHECK_ARG(((uintptr_t)wbuf & 255) == 0, "bf16 weight buffer must be 256-byte aligned");
  RelPlan P;
  plan_rel(id, 1, P);
  if (wbuf_bytes < P.wbytes) { set_error("relative decoder weight buffer too small: %zu < %zu", wbuf_bytes, P.wbytes); return RDM_ERR_WORKSPACE_TOO_SMALL; }
  const int nt = rel_num_tensors(id);
  for (int i = 0; i < nt; ++i) RDM_CHECK_ARG(T[i] != nullptr, "tensor %d is NULL", i);
  hipStream_t s = stream;
  int rc;
  RDM_HIP_OK(hipMemsetAsync(wbuf, 0, P.wbytes, s));          // padded rows / columns / biases are zeros
  for (int i = 0; i < kLayers; ++i) {                          // the dense block: the layout rdm_net_bf16_prepare gives d_1's block
    const int b = 12 * i, cin = kCin0 + i * kGrowth;
    if ((rc = launch_f32_to_bf16_rows(Fp(T, b + 5), cin, at<char>(wbuf, P.dw1[i]), cin, kCb, cin, cin, s))) return rc;
    if ((rc = launch_pack_w_bf16(Fp(T, b + 11), at<char>(wbuf, P.dw3[i]), kGrowth, kCb, kCb, 9, s))) return rc;
    // eval-mode affines of norm1 (tensors b .. b + 4) and norm2 (b + 6 .. b + 10): no sums, no batch counted
    if ((rc = launch_bn_finalize(StatPair(), 1.0, BnParams(T, BnIdx{b, b + 1, b + 2, b + 3, b + 4}, false), BnAffine(at<float>(wbuf, P.dbn1[i]), cin), cin, 0, s))) return rc;
    if ((rc = launch_bn_finalize(StatPair(), 1.0, BnParams(T, BnIdx{b + 6, b + 7, b + 8, b + 9, b + 10}, false), BnAffine(at<float>(wbuf, P.dbn2[i]), kCb), kCb, 0, s))) return rc;
  }
  auto bias = [&](size_t off, int idx, int n) -> int {
    RDM_HIP_OK(hipMemcpyAsync(at<char>(wbuf, off), T[idx], (size_t)n * 4, hipMemcpyDeviceToDevice, s));
    return RDM_OK;
  };
  for (int l = 0; l < P.nw; ++l) {
    const RelWsm& R = P.L[l];
    const int b = 12 * kLayers + 22 * l, C = R.C, S = R.S;
    // input_adjustment_layer (C, raw, 1, 1)
    if ((rc = pack_w(Fp(T, b + 20), at<char>(wbuf, R.ia_w), C, 0, R.kraw, R.kraw, 1, 1, R.kraw, R.raw, R.raw, 1, 0, 0, s))) return rc;
    if ((rc = bias(R.ia_b, b + 21, C))) return rc;
    // deconv1.0: ConvTranspose2d weight (Cin, Cout, 2, 2) -> row phase*cp + co, phase = 2r + s, k = ci
    for (int ph = 0; ph < 4; ++ph) {
      if ((rc = pack_w(Fp(T, b) + ph, at<char>(wbuf, R.dc_w), C, ph * R.cp, R.cp, R.cp, 1, 1, R.cp, C, 4, 4L * C, 0, 0, s))) return rc;
      RDM_HIP_OK(hipMemcpyAsync(at<char>(wbuf, R.dc_b + (size_t)ph * R.cp * 4), T[b + 1], (size_t)C * 4, hipMemcpyDeviceToDevice, s));
    }
    // conv1_1..conv1_5 (out, C, 1, 1) concatenated: rows [0,kip) [kip,2kip) [2kip,3kip) [3kip,3kip+wip) [3kip+wip, nf)
    const int r0[5] = {0, R.kip, 2 * R.kip, 3 * R.kip, 3 * R.kip + R.wip};
    const int no[5] = {R.ki, R.ki, R.ki, R.wi, R.wi};
    for (int c = 0; c < 5; ++c) {
      if ((rc = pack_w(Fp(T, b + 2 + 2 * c), at<char>(wbuf, R.f5_w), no[c], r0[c], R.cp, R.cp, 1, 1, R.cp, C, C, 1, 0, 0, s))) return rc;
      RDM_HIP_OK(hipMemcpyAsync(at<char>(wbuf, R.f5_b + (size_t)r0[c] * 4), T[b + 3 + 2 * c], (size_t)no[c] * 4, hipMemcpyDeviceToDevice, s));
    }
    // conv2_1 3x3 / conv2_2 5x5 (ki, ki, k, k): k = tap*kip + ci
    if ((rc = pack_w(Fp(T, b + 12), at<char>(wbuf, R.c3_w), R.ki, 0, 9 * R.kip, R.kip, 9, 1, R.kip, R.ki, 9L * R.ki, 9, 0, 1, s))) return rc;
    if ((rc = bias(R.c3_b, b + 13, R.ki))) return rc;
    if ((rc = pack_w(Fp(T, b + 14), at<char>(wbuf, R.c5_w), R.ki, 0, 25 * R.kip, R.kip, 25, 1, R.kip, R.ki, 25L * R.ki, 25, 0, 1, s))) return rc;
    if ((rc = bias(R.c5_b, b + 15, R.ki))) return rc;
    // wsm_wx3 (wi, wi, 3, S): tap dy, k = w*wip + ci        wsm_3xh (wi, wi, S, 3): tap dx, k = h*wip + ci
    if ((rc = pack_w(Fp(T, b + 16), at<char>(wbuf, R.sv_w), R.wi, 0, 3 * S * R.wip, S * R.wip, 3, S, R.wip, R.wi, 3L * S * R.wi, 3L * S, 1, S, s))) return rc;
    if ((rc = bias(R.sv_b, b + 17, R.wi))) return rc;
    if ((rc = pack_w(Fp(T, b + 18), at<char>(wbuf, R.sh_w), R.wi, 0, 3 * S * R.wip, S * R.wip, 3, S, R.wip, R.wi, 3L * S * R.wi, 3L * S, 3, 1, s))) return rc;
    if ((rc = bias(R.sh_b, b + 19, R.wi))) return rc;
  }
  const int bc = 12 * kLayers + 22 * P.nw;
  if ((rc = pack_w(Fp(T, bc), at<char>(wbuf, P.c1_w), 1, 0, pad32(P.cf), pad32(P.cf), 1, 1, pad32(P.cf), P.cf, P.cf, 1, 0, 0, s))) return rc;
  if ((rc = bias(P.c1_b, bc + 1, 1))) return rc;
  return RDM_OK;
}

int rdm_rel_forward_bf16(int32_t id, const void* enc, int32_t ld_enc, int32_t batch, const void* wbuf, void* ws, size_t ws_bytes, float* out_map,
                         rdm_stream_t stream) {
  RDM_CHECK_ARG(id >= 6 && id <= 10, "relative decoder id must be 6..10, got %d", id);
  RDM_CHECK_ARG(enc && wbuf && ws && out_map, "NULL argument");
  RDM_CHECK_ARG(batch > 0 && batch <= 256 && ld_enc >= kCin0, "batch must be 1..256 (32-bit buffer offsets) and ld_enc >= 1056");
  RDM_CHECK_ARG((((uintptr_t)ws | (uintptr_t)wbuf) & 255) == 0, "workspace and weight buffer must be 256-byte aligned");
  RelPlan P;
  plan_rel(id, batch, P);
  if (ws_bytes < P.wsbytes) { set_error("relative decoder workspace too small: %zu < %zu", ws_bytes, P.wsbytes); return RDM_ERR_WORKSPACE_TOO_SMALL; }
  hipStream_t s = stream;
  void* wb = const_cast<void*>(wbuf);
  int rc;
  const int M8 = batch * 64;
  unsigned short* blk = at<unsigned short>(ws, P.blk);
  RDM_HIP_OK(hipMemcpy2DAsync(blk, (size_t)kCtot * 2, enc, (size_t)ld_enc * 2, (size_t)kCin0 * 2, M8, hipMemcpyDeviceToDevice, s));
  {
    DenseBf16Block d{};
    d.blk = blk; d.B = batch; d.H = 8; d.W = 8; d.M = M8; d.ctot = kCtot; d.cin0 = kCin0; d.layers = kLayers; d.cbp = kCb; d.act3 = false;
    d.Y = at<char>(ws, P.Y); d.partial = at<float>(ws, P.partial); d.partial_floats = P.partial_floats;
    for (int i = 0; i < kLayers; ++i) {
      d.w1[i] = at<char>(wb, P.dw1[i]); d.w3[i] = at<char>(wb, P.dw3[i]);
      d.bn1[i] = at<float>(wb, P.dbn1[i]); d.bn2[i] = at<float>(wb, P.dbn2[i]);
    }
    if ((rc = dense_block_bf16(d, s))) return rc;
  }
  return rel_wsm_chain(P, batch, wb, ws, out_map, s);
}

size_t rdm_rel_bf16_train_workspace_bytes(int32_t id, int32_t batch) {
  if (id < 6 || id > 10 || batch <= 0) return 0;
  RelPlan P;
  plan_rel(id, batch, P);
  plan_rel_train(P);
  return P.train_wsbytes;
}

int rdm_rel_forward_bf16_train(int32_t id, const void* enc, int32_t ld_enc, const double* enc_stats, int32_t batch, void* const* T, const void* wbuf, void* ws,
                               size_t ws_bytes, float* out_map, rdm_stream_t stream) {
  RDM_CHECK_ARG(id >= 6 && id <= 10, "relative decoder id must be 6..10, got %d", id);
  RDM_CHECK_ARG(enc && T && wbuf && ws && out_map, "NULL argument");
  RDM_CHECK_ARG(batch > 0 && batch <= 256 && ld_enc >= kCin0 && ld_enc % 8 == 0, "batch must be 1..256 (32-bit buffer offsets), ld_enc >= 1056 and a multiple of 8");
  RDM_CHECK_ARG((((uintptr_t)ws | (uintptr_t)wbuf) & 255) == 0 && ((uintptr_t)enc & 15) == 0, "workspace and weight buffer must be 256-byte aligned, enc 16-byte aligned");
  RelPlan P;
  plan_rel(id, batch, P);
  plan_rel_train(P);
  if (ws_bytes < P.train_wsbytes) { set_error("relative decoder training workspace too small: %zu < %zu", ws_bytes, P.train_wsbytes); return RDM_ERR_WORKSPACE_TOO_SMALL; }
  for (int i = 0; i < 12 * kLayers; ++i) RDM_CHECK_ARG(T[i] != nullptr, "tensor %d is NULL", i);
  hipStream_t s = stream;
  void* wb = const_cast<void*>(wbuf);
  int rc;
  const int M8 = batch * 64;
  unsigned short* blk = at<unsigned short>(ws, P.blk);
  double* bst = at<double>(ws, P.bst);
  RDM_HIP_OK(hipMemcpy2DAsync(blk, (size_t)kCtot * 2, enc, (size_t)ld_enc * 2, (size_t)kCin0 * 2, M8, hipMemcpyDeviceToDevice, s));
  if (enc_stats) {                                                   // [sum 1056 | sq 1056], shared by the decoders of one forward
    RDM_HIP_OK(hipMemcpyAsync(bst, enc_stats, (size_t)kCin0 * 8, hipMemcpyDeviceToDevice, s));
    RDM_HIP_OK(hipMemcpyAsync(bst + kCtot, enc_stats + kCin0, (size_t)kCin0 * 8, hipMemcpyDeviceToDevice, s));
  } else if ((rc = launch_colstats_bf16(enc, ld_enc, M8, kCin0, bst, bst + kCtot, s))) {
    return rc;
  }
  {
    DenseBf16TrainBlock d{};
    d.blk = blk; d.B = batch; d.H = 8; d.W = 8; d.M = M8; d.ctot = kCtot; d.cin0 = kCin0; d.layers = kLayers; d.cb = kCb;
    d.Y = at<char>(ws, P.Y); d.partial = at<float>(ws, P.partial); d.partial_floats = P.partial_floats;
    d.stats = at<float>(ws, P.stats); d.stats_floats = P.stats_floats;
    d.bsum = bst; d.bsq = bst + kCtot;
    d.ysum = at<double>(ws, P.yst); d.ysq = d.ysum + kCb;
    d.aff1 = at<float>(ws, P.aff1); d.aff2 = at<float>(ws, P.aff2);
    for (int i = 0; i < kLayers; ++i) {
      const int b = 12 * i;                                          // norm1 w b rm rv nbt, conv1, norm2 w b rm rv nbt, conv2
      d.w1[i] = at<char>(wb, P.dw1[i]); d.w3[i] = at<char>(wb, P.dw3[i]);
      d.p1[i] = BnParams(T, BnIdx{b, b + 1, b + 2, b + 3, b + 4}); d.p2[i] = BnParams(T, BnIdx{b + 6, b + 7, b + 8, b + 9, b + 10});
    }
    if ((rc = dense_block_bf16_train(d, s))) return rc;
  }
  return rel_wsm_chain(P, batch, wb, ws, out_map, s);
}

int rdm_colstats_bf16(const void* x, int32_t ldx, int32_t m, int32_t c, double* sum, double* sumsq, rdm_stream_t stream) {
  return launch_colstats_bf16(x, ldx, m, c, sum, sumsq, stream);
}

int rdm_rel_bf16_input_nchw(const float* x_nchw, int32_t batch, void* enc, int32_t ld_enc, rdm_stream_t stream) {
  RDM_CHECK_ARG(x_nchw && enc && batch > 0 && ld_enc >= kCin0, "bad argument");
  const long total = (long)batch * kCin0 * 64;
  k_nchw_f32_to_nhwc_bf16<<<(int)std::min<long>((total + 255) / 256, 4096), 256, 0, stream>>>(x_nchw, static_cast<unsigned short*>(enc), ld_enc, batch, kCin0, 64);
  RDM_LAUNCH_OK();
  return RDM_OK;
}

/* operator entries: one per epilogue mode (tests; the decoder forward enqueues the same launches).  Weights: bf16 [rows][K] as
 * rdm_rel_bf16_prepare packs them (k = tap * pad32(cin) + ci), rows allocated up to a multiple of 64. */
int rdm_wsm_conv_bf16(const void* x, int32_t ldx, int32_t xoff, int32_t cin, const void* w, const float* bias, int32_t n, void* out, int32_t ldc, int32_t coff,
                      int32_t batch, int32_t h, int32_t wd, int32_t k, rdm_stream_t stream) {
  RDM_CHECK_ARG(x && w && out, "NULL argument");
  RDM_CHECK_ARG(k == 1 || k == 3 || k == 5, "kernel size must be 1, 3 or 5");
  RDM_CHECK_ARG(cin > 0 && n > 0 && ldx >= xoff + cin && ldc >= coff + n && batch > 0 && h > 0 && wd > 0, "bad geometry");
  RDM_CHECK_ARG(fits32((long)batch * h * wd * std::max(ldx, ldc)), "tensor too large for 32-bit buffer offsets");
  WsmConvArgs a = conv_args(x, (long)batch * h * wd * ldx, ldx, xoff, cin, batch, h, wd, k, w, n, bias, bias ? n : 0);
  a.nseg = 1; a.seg[0] = seg(out, 0, (n + 3) / 4 * 4, n, ldc, coff, WSM_PLAIN);
  return launch_wsm_conv_bf16(a, stream);
}

int rdm_wsm_deconv_bf16(const void* x, int32_t ldx, int32_t cin, const void* w, const float* bias, int32_t c, void* out, int32_t ldc, int32_t batch, int32_t h,
                        int32_t wd, rdm_stream_t stream) {
  RDM_CHECK_ARG(x && w && out, "NULL argument");
  RDM_CHECK_ARG(cin > 0 && c > 0 && ldx >= cin && ldc >= c && batch > 0 && h > 0 && wd > 0, "bad geometry");
  RDM_CHECK_ARG(fits32(4L * batch * h * wd * std::max(ldx, ldc)), "tensor too large for 32-bit buffer offsets");
  const int cp = pad32(c);
  WsmConvArgs a = conv_args(x, (long)batch * h * wd * ldx, ldx, 0, cin, batch, h, wd, 1, w, 4 * cp, bias, bias ? 4 * cp : 0);
  a.nseg = 1; a.seg[0] = seg(out, 0, 4 * cp, c, ldc, 0, WSM_SHUFFLE);
  return launch_wsm_conv_bf16(a, stream);
}

int rdm_wsm_strip_bf16(const void* x, int32_t ldx, int32_t xoff, int32_t cin, const void* w, const float* bias, int32_t n, void* out, int32_t ldc, int32_t coff,
                       int32_t batch, int32_t s, int32_t columns, rdm_stream_t stream) {
  RDM_CHECK_ARG(x && w && out, "NULL argument");
  RDM_CHECK_ARG(cin > 0 && cin % 32 == 0 && n > 0 && ldx >= xoff + cin && ldc >= coff + n && batch > 0 && s > 0, "bad geometry (cin: the padded channel width, a multiple of 32)");
  RDM_CHECK_ARG(fits32((long)batch * s * s * std::max(ldx, ldc)), "tensor too large for 32-bit buffer offsets");
  WsmConvArgs a = strip_args(x, (long)batch * s * s * ldx, ldx, xoff, cin, batch, s, columns != 0, w, n, bias, bias ? n : 0);
  a.nseg = 1; a.seg[0] = seg(out, 0, (n + 3) / 4 * 4, n, ldc, coff, columns ? WSM_BCAST_COLS : WSM_BCAST_ROWS);
  return launch_wsm_conv_bf16(a, stream);
}

int rdm_wsm_conv1x1_f32(const void* x, int32_t ldx, int32_t cin, const void* w, const float* bias, float* out, int32_t batch, int32_t h, int32_t wd,
                        rdm_stream_t stream) {
  RDM_CHECK_ARG(x && w && out, "NULL argument");
  RDM_CHECK_ARG(cin > 0 && ldx >= cin && batch > 0 && h > 0 && wd > 0, "bad geometry");
  RDM_CHECK_ARG(fits32((long)batch * h * wd * ldx), "tensor too large for 32-bit buffer offsets");
  WsmConvArgs a = conv_args(x, (long)batch * h * wd * ldx, ldx, 0, cin, batch, h, wd, 1, w, 1, bias, bias ? 1 : 0);
  a.nseg = 1; a.seg[0] = seg(out, 0, 4, 1, 1, 0, WSM_F32);
  return launch_wsm_conv_bf16(a, stream);
}

}  // extern "C"
