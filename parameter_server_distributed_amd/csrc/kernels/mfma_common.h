// Device helpers shared by the MFMA kernel families (gemm.hip, convn.hip, convw.hip): buffer
// descriptors for the LDS-DMA staging, the swizzled K-major LDS image, counted waits, the XCD-aware
// block order and the in-register exchanges of the epilogues.
#pragma once
#include "common.h"

namespace psd {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) s16x4 lds_s16x4;

// Buffer-descriptor LDS-DMA staging: per piece the lane's byte offset = (scalar tile/k origin) +
// (per-lane part, loop-invariant); rows past the operand's end fall outside the descriptor's range
// and load zeros (only garbage rows/cols of C, never stored, depend on them), so no per-lane clamp.
typedef __amdgpu_buffer_rsrc_t rsrc_t;
__device__ __forceinline__ rsrc_t make_rsrc(const void* p, uint32_t bytes) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), (short)0, (int)bytes, 0x00020000);
}
constexpr uint32_t kOOB = 0xFFFFFFF0u;  // past every descriptor's range: the load returns zeros

__device__ __forceinline__ int kmaj_off(int row, int kc) {  // byte offset in a [rows][64] bf16 tile
  return row * 128 + ((kc ^ ((row >> 1) & 7)) << 4);
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
  // bijective: blocks with equal bid % 8 (one XCD under round-robin dispatch) get a contiguous range
  const int q = nwg / 8, r = nwg % 8, xcd = bid % 8;
  return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + bid / 8;
}

template <int CTRL>
__device__ __forceinline__ float dpp_q(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_mov_dpp(__builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
// 4x4 transpose inside a lane quad: in v[r] = C[row r][col L]; out w[c] = C[row L][col c]
__device__ __forceinline__ void quad_t4(const f32x4 v, int L, float (&w)[4]) {
  const bool o1 = L & 1, o2 = (L >> 1) & 1;
  const float r0 = dpp_q<0xB1>(o1 ? v[0] : v[1]);  // quad_perm [1,0,3,2]: partner L^1
  const float r1 = dpp_q<0xB1>(o1 ? v[2] : v[3]);
  const float a0 = o1 ? r0 : v[0], a1 = o1 ? v[1] : r0;  // row L&1,     cols (L&~1, L|1)
  const float b0 = o1 ? r1 : v[2], b1 = o1 ? v[3] : r1;  // row (L&1)+2, same cols
  const float q0 = dpp_q<0x4E>(o2 ? a0 : b0);            // quad_perm [2,3,0,1]: partner L^2
  const float q1 = dpp_q<0x4E>(o2 ? a1 : b1);
  w[0] = o2 ? q0 : a0;
  w[1] = o2 ? q1 : a1;
  w[2] = o2 ? b0 : q0;
  w[3] = o2 ? b1 : q1;
}
// two bf16 from separate conversions, OR-ed: the 8-phase epilogues are scheduled around this form
// (common.h pack_bf16x2_rne, the paired convert, compiles to different code there)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
  return (uint32_t)f32_to_bf16(lo) | ((uint32_t)f32_to_bf16(hi) << 16);
}

// x[lane ^ 16] / x[lane ^ 32] through the gfx950 half-row / half-wave swaps (VALU, no LDS round
// trip: the statistics reduction of a one-K-tile convolution is on its critical path)
__device__ __forceinline__ float xor16(float x, int lane) {
  const auto r = __builtin_amdgcn_permlane16_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float((lane & 16) ? r[0] : r[1]);
}
__device__ __forceinline__ float xor32(float x, int lane) {
  const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(x), __float_as_uint(x), false, false);
  return __uint_as_float((lane & 32) ? r[0] : r[1]);
}

}  // namespace psd
