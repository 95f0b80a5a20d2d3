// Device primitives shared by every kernel file of the library (and of the measurement kernels under bench/): the vector types, buffer
// descriptors and their out-of-range convention, the 16-byte buffer load and LDS-DMA piece, bf16 packing and the XCD-aware block order.
// A kernel file declares none of these itself: a fix to one of them lands here, once.  Not part of the C ABI.
#pragma once
#include <hip/hip_runtime.h>

namespace rdm {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef short s16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---------------------------------------------------------------------------------------------
// Global operands are read through buffer descriptors (SRD): 32-bit byte offsets instead of 64-bit
// pointer arithmetic, and the hardware range check returns 0 for an out-of-range offset - so zero
// padding, ragged tile edges and the K tail cost one v_cndmask (offset := OOB) instead of a
// divergent branch per load.  Every operand extent is < 4 GiB (checked by the launchers).
// ---------------------------------------------------------------------------------------------
constexpr unsigned OOB = 0xFFFFFFFFu;

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_srd(const void* p, unsigned bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, (int)bytes, 0x00020000);
}
// 16-byte buffer loads at a byte offset (OOB: zeros)
__device__ __forceinline__ uint4 bld_u4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ float4 bld_f4(__amdgpu_buffer_rsrc_t r, unsigned off) {
  const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(r, (int)off, 0, 0);
  return make_float4(__uint_as_float(v.x), __uint_as_float(v.y), __uint_as_float(v.z), __uint_as_float(v.w));
}
// one 1-KiB LDS-DMA piece: lane l's 16 bytes at (voff + soff) land at lds_dst + 16*l (lds_dst wave-uniform: it goes to M0)
__device__ __forceinline__ void lds_dma16(__amdgpu_buffer_rsrc_t rsrc, unsigned voff, unsigned soff, void* lds_dst) {
#if defined(__HIP_DEVICE_COMPILE__)      // (the host pass cannot type-check the gfx950 builtin and would silently drop the kernel's stub)
  __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)lds_dst, 16, (int)voff, (int)soff, 0, 0);
#endif
}

// two packed bf16 (low half first) <-> float
__device__ __forceinline__ float bf_lo(unsigned u) { return __uint_as_float(u << 16); }
__device__ __forceinline__ float bf_hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
__device__ __forceinline__ unsigned short bf1(float a) { return __builtin_bit_cast(unsigned short, (__bf16)a); }      // one value, same rounding
__device__ __forceinline__ unsigned pack2(float a, float b) {
  const bf16x2 r = {(__bf16)a, (__bf16)b};                  // v_cvt_pk_bf16_f32: round to nearest even, NaN stays NaN
  return __builtin_bit_cast(unsigned, r);
}
// the same pair from two scalar conversions and an or: what wsm_bf16.hip's store path was compiled with.  Same bits as pack2; the packed
// convert there changes the kernel's register allocation, so the site keeps its arithmetic until someone measures the other form
__device__ __forceinline__ unsigned pack2_scalar(float a, float b) { return (unsigned)bf1(a) | ((unsigned)bf1(b) << 16); }

// ---------------------------------------------------------------------------------------------
// XCD-aware block order.  Workgroups are dealt round-robin over the 8 XCDs in dispatch order
// (x fastest), and each XCD has its own 4 MB L2: with the plain order the gx column tiles that
// share one A row-tile land on 8 different L2s and the tile is pulled over the fabric up to 8 times
// (the 1x1 dgrad of dense_e2 read 3.5x its operand bytes).  Remapped, XCD x works through the
// contiguous range [x*total/8, (x+1)*total/8) of the logical (x fastest) order, so blocks that are
// adjacent in time on one XCD are adjacent column tiles of the same row-tile.  A bijection for any
// grid size; placement only affects speed, never results.  A/B on dense_e2: 1x1 dgrad 116.6 vs 109.7 TFLOP/s.
// ---------------------------------------------------------------------------------------------
// dispatch index L of `total` workgroups -> position Lp in the logical order; the caller unflattens Lp over its own grid
__device__ __forceinline__ unsigned xcd_logical(unsigned L, unsigned total) {
  const unsigned x = L & 7u, seq = L >> 3, q = total >> 3, r = total & 7u;
  return x * q + (x < r ? x : r) + seq;
}

}  // namespace rdm
