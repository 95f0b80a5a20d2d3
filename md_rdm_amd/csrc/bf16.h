// internal declarations of the bf16 forward kernels (bf16.hip); not part of the C ABI
#pragma once
#include <hip/hip_runtime.h>
#include "plan_views.h"
namespace rdm {

struct GemmBf16Args {        // out[m][n] = bias[n] + sum_k f(X[m][k]) * W[n][k],  f = relu(x*scale[k]+shift[k]) when scale != NULL
  const void* X; int ldx; int K;           // bf16 activations [M][ldx] (k-contiguous), contracted extent (multiple of 8)
  const float* scale; const float* shift;  // optional eval-mode BatchNorm affine + ReLU over k
  const void* W; int ldw;                  // bf16 weights [N][ldw]
  void* out; int ldc; int M, N;            // bf16 (or f32) [M][ldc]
  const float* bias;                       // optional f32[N]
  const float* oscale; const float* oshift; // optional f32[N]: out = relu(out*oscale[n] + oshift[n]) before the bf16 rounding (the CONSUMER's eval-mode BatchNorm + ReLU)
  float* partial; size_t partial_floats;   // optional f32 scratch for a K-split ([split][M][N] partial sums + one tiny reduction launch)
  unsigned x_bytes, w_bytes, p_bytes, o_bytes;   // set by the launcher (buffer descriptors)
  // training-mode statistics epilogue (osum != NULL; gemm_bf16_kernel<..., STATS = true>, no panel kernel, no oscale): per-channel sum and sum of
  // squares of the STORED (bf16-rounded) outputs - f32 per wave row tile into `stats` ([tile][sum N | sq N]), combined in f64 in tile order
  double* osum; double* osq;
  float* stats; size_t stats_floats;       // >= bf16_stats_floats(M, N)
};

struct Conv3Bf16Args {       // out[m][n] = sum_{tap,c} relu(Y[pix(m,tap)][c]*scale[c]+shift[c]) * Wt[tap][n][c], zero padding, n < 48
  const void* Y; int ldy; int C;           // bf16 [M][ldy], C multiple of 8
  const float* scale; const float* shift;
  const void* Wt; long wtap; int ldw;      // bf16 [9][48][ldw]
  unsigned short* out; int ldc;            // bf16 [M][ldc] (a 48-channel slice of the block buffer)
  int B, H, W, M;
  float* partial; size_t partial_floats;   // optional f32 scratch for the K-split: [split][M][48] partial sums, reduced by a second (tiny) launch
  int split;                               // set by the launcher
  int slots;                               // set by the launcher: zero-padded LDS image slots (pixels) the kernel may use, multiple of 8
  unsigned y_bytes, w_bytes, p_bytes;
  // training-mode statistics epilogue (osum != NULL; conv3x3_bf16_kernel<..., STATS = true>): as GemmBf16Args, over the 48 outputs
  double* osum; double* osq;
  float* stats; size_t stats_floats;       // >= bf16_stats_floats(M, 48)
};

struct Conv3ActArgs {        // out[m][n] = sum_{tap,c} Y[pix(m,tap)][c] * w[n][c][tap] on an ALREADY ACTIVATED input, zero padding, n < 48
  const void* Y; int ldy; int C;           // bf16 [B*H*W][ldy]; C multiple of 32 (pad channels: finite values, their weights are zero)
  const void* Wimg;                        // fragment-order weight image (launch_pack_w3_frag_bf16): C/32 slabs of 27 KiB
  unsigned short* out; int ldc;            // bf16 [B*H*W][ldc]
  int B, H, W;
  float* partial; size_t partial_floats;   // optional f32 scratch for the K-split ([tile][split][BM][48])
  unsigned* counters; int n_counters;      // one per tile, ZERO on entry, left zero (needed when partial != NULL)
  int split, slots, tiles_per_img, rect;   // set by the launcher (rect: 64-column rectangular tiles for rows too wide for whole-row tiles)
  unsigned y_bytes, w_bytes;
};

int launch_gemm_bf16(const GemmBf16Args& a, bool out_f32, hipStream_t s);
// f32 scratch the statistics epilogues need for M rows x N channels (tiles of >= 8 rows, two values per channel and tile)
inline size_t bf16_stats_floats(long M, int N) { return (size_t)2 * N * ((M + 7) / 8 + 4); }
// per-channel f64 sum / sum of squares of x[0, M) x [0, C) bf16 (row stride ldx; C, ldx multiples of 8): f32 per thread, f64 in a fixed order
int launch_colstats_bf16(const void* x, int ldx, int M, int C, double* sum, double* sq, hipStream_t s);
int launch_conv3x3_act_bf16(const Conv3ActArgs& a, hipStream_t s);      // RDM_ERR_UNSUPPORTED when the geometry does not fit the LDS (nothing launched)
size_t conv3x3_act_partial_floats(int C, int B, int H, int W);          // scratch the heuristic would like
int conv3x3_act_tiles(int B, int H, int W);                             // upper bound of the tile count (counters needed)
bool conv3x3_act_fits(int B, int H, int W);                             // a tile's padded rows fit the LDS image
int launch_pack_w3_frag_bf16(const float* w, void* img, int C, int Cpad, int packed, hipStream_t s);
int launch_conv3x3_bf16(const Conv3Bf16Args& a, hipStream_t s);
int launch_f32_to_bf16_rows(const float* src, int ld_src, void* dst, int ld_dst, long rows, int cols, int cols_pad, hipStream_t s);
int launch_pack_w_bf16(const float* w_oihw, void* w_packed, int O, int I, int ld, int T, hipStream_t s);
int launch_im2col_stem_bf16(const float* x, void* patches, int B, int H, int W, hipStream_t s);
int launch_maxpool3s2_bf16(const void* X, void* Y, int ldy, int B, int H, int W, int C, hipStream_t s);
// one dense block of the bf16 forward (net.hip): per layer BN-ReLU -> 1x1 (cin -> cbp, the 3x3's BN-ReLU in the epilogue) -> 3x3 (cbp -> 48)
// written in place behind the block's channels.  rdm_net_forward_bf16 runs its four blocks through it, the relative decoders their own.
struct DenseBf16Block {
  unsigned short* blk; int B, H, W, M, ctot, cin0, layers, cbp; bool act3;
  void* Y; float* partial; size_t partial_floats; unsigned* counters; int n_counters;
  const void* w1[48]; const void* w3[48]; const float* bn1[48]; const float* bn2[48];
};
int dense_block_bf16(const DenseBf16Block& d, hipStream_t s);
// the same block in TRAINING mode (net.hip): BatchNorm from batch statistics, running statistics updated like nn.BatchNorm2d.  Per layer:
// finalize norm1 over [0, cin) -> 1x1 with the norm1 BN-ReLU prologue, raw Y + its statistics -> finalize norm2 -> 3x3 with the norm2 BN-ReLU
// prologue into the block + the statistics of its 48 channels (norm1 of every later layer).  bsum / bsq [ctot] f64 hold the statistics of
// channels [0, cin0) on entry; gamma / beta / running buffers are the live tensors (nbt: int64 num_batches_tracked).
struct DenseBf16TrainBlock {
  unsigned short* blk; int B, H, W, M, ctot, cin0, layers, cb;
  void* Y; float* partial; size_t partial_floats; float* stats; size_t stats_floats;
  double* bsum; double* bsq; double* ysum; double* ysq; float* aff1; float* aff2;     // aff1 [4][ctot] / aff2 [4][cb] f32: scale | shift | mean | rstd
  const void* w1[48]; const void* w3[48];
  BnParams p1[48], p2[48];                 // norm1 / norm2 of each layer
};
int dense_block_bf16_train(const DenseBf16TrainBlock& d, hipStream_t s);
int launch_trans_pool_bf16(const void* X, int ldx, const float* sc, const float* sh, void* P, int B, int H, int W, int C, hipStream_t s);

}  // namespace rdm
