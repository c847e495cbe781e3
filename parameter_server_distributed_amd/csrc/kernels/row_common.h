// Device helpers of the one-wave-per-row kernels (layernorm.hip, rmsnorm.hip): a row of H = 64*E bf16
// elements, lane l owning columns [l*E, l*E + E), 8-byte loads / stores, wave butterfly reductions and
// the dropout keep flags of a lane's E columns.
#pragma once
#include "common.h"

namespace psd {

// the lane's E keep flags (common.h drop_keep's mask: 16 bits of one hash per element pair; off is
// even -- a lane's E columns start at an even index -- so each pair's hash is computed once here)
template <int E>
__device__ __forceinline__ void keep_flags(uint32_t key, int64_t off, uint32_t thresh, bool (&kp)[E]) {
  const uint32_t t16 = thresh >> 16;
#pragma unroll
  for (int j = 0; j < E / 2; ++j) {
    const uint32_t hb = drop_pair_bits(key, (uint64_t)(off + 2 * j));
    kp[2 * j] = (hb & 0xffffu) >= t16;
    kp[2 * j + 1] = (hb >> 16) >= t16;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

template <int E>
__device__ __forceinline__ void load_e(const uint16_t* p, float v[E]) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i) {
    const uint2 w = *reinterpret_cast<const uint2*>(p + 4 * i);
    v[4 * i + 0] = __uint_as_float(w.x << 16);
    v[4 * i + 1] = __uint_as_float(w.x & 0xffff0000u);
    v[4 * i + 2] = __uint_as_float(w.y << 16);
    v[4 * i + 3] = __uint_as_float(w.y & 0xffff0000u);
  }
}

template <int E>
__device__ __forceinline__ void store_e(uint16_t* p, const float v[E]) {
#pragma unroll
  for (int i = 0; i < E / 4; ++i)
    *reinterpret_cast<uint2*>(p + 4 * i) = make_uint2(pack_bf16x2_rne(v[4 * i], v[4 * i + 1]),
                                                      pack_bf16x2_rne(v[4 * i + 2], v[4 * i + 3]));
}

__device__ __forceinline__ uint32_t dropout_key(uint32_t seed, const int64_t* step) {
  return drop_mix32(seed * 0x27d4eb2fu ^ (uint32_t)(step ? *step : 0) * 0x165667b1u);
}

// the 32-bit keep threshold of dropout probability p (0: no dropout)
inline uint32_t keep_thresh(float p) {
  if (p <= 0.f) return 0u;
  const double t = (double)p * 4294967296.0;
  return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

}  // namespace psd
