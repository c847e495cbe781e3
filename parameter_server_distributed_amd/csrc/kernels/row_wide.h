// Device helpers of the one-workgroup-per-row kernels (rmsnorm_wide.hip, layernorm_wide.hip): a row of H bf16
// elements is H / 8 chunks of 8 consecutive columns (16 bytes), lane t of 256 owning chunks t + 256 s, s < S =
// ceil(H / 2048). Included after the including file's `#pragma clang fp contract(off)`.
#pragma once
#include "common.h"
#include "mx_common.h"
#include "row_common.h"

namespace psd {
namespace {
__device__ __forceinline__ u32x4 ld16(const uint16_t* p) { return *reinterpret_cast<const u32x4*>(p); }

__device__ __forceinline__ void unpack8(const u32x4& w, float (&v)[8]) {
  const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(ws[i] << 16);
    v[2 * i + 1] = __uint_as_float(ws[i] & 0xffff0000u);
  }
}

// whether chunk t + 256 s of a row of nch chunks exists: only the last slab can be partly filled
template <int S>
__device__ __forceinline__ bool has_chunk(int s, int t, int nch) {
  return s < S - 1 || t + 256 * s < nch;
}

// the row's sum over the workgroup: the same bits on every lane. red: [2][4], slot alternating by round
__device__ __forceinline__ float row_sum(float v, float (*red)[4], int slot, int lane, int wv) {
  v = wave_sum(v);
  if (lane == 0) red[slot][wv] = v;
  __syncthreads();
  return (red[slot][0] + red[slot][1]) + (red[slot][2] + red[slot][3]);
}

// the MX copy of a chunk (t: as about to be / just stored in bf16) at element offset off, block scale row srow
template <bool E5>
__device__ __forceinline__ void mx_chunk_store(float (&t)[8], uint8_t* __restrict__ q8, uint8_t* __restrict__ sc8,
                                               int64_t off) {
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = bf16_to_f32(f32_to_bf16(t[e]));  // as stored
  uint2 qb;
  const int eb = mx_quant8<E5>(t, qb);
  *reinterpret_cast<uint2*>(q8 + off) = qb;
  if ((off & 31) == 0) sc8[off >> 5] = (uint8_t)eb;  // H % 32 == 0: off / 32 = row * (H / 32) + block in row
}
}  // namespace

// the slab count S of hidden size H as a template argument of LAUNCH
#define PSD_WIDE_S(H, LAUNCH) \
  do {                        \
    if ((H) <= 2048) LAUNCH(1);      \
    else if ((H) <= 4096) LAUNCH(2); \
    else if ((H) <= 6144) LAUNCH(3); \
    else LAUNCH(4);                  \
  } while (0)

}  // namespace psd
