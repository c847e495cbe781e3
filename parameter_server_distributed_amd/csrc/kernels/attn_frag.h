// MFMA fragment, dropout-hash and length helpers shared by the fused attention kernels: the
// whole-head-in-LDS family (attention.hip, S <= 128) and the streaming one (attention_long.hip,
// 128 < S <= 4096). Device code only; include after common.h and launchers_attn.h.
#pragma once

#include "common.h"
#include "launchers_attn.h"

namespace psd {

namespace {

typedef __bf16 abf16x8 __attribute__((ext_vector_type(8)));
typedef short as16x4 __attribute__((ext_vector_type(4)));
typedef float af32x16 __attribute__((ext_vector_type(16)));
typedef __attribute__((address_space(3))) as16x4 alds_s16x4;

constexpr int D = 64;                 // head dim
constexpr int LDT = D + 8;            // Q/K/V/dO tile row stride (elements): 144 B

// (common.h drop_keep: one hash per element pair, 16 bits each; fwd and bwd index elements alike)
// keep flags of the element pair (idx, idx + 1), idx even, from ONE hash -- drop_keep's mask bit for bit.
// (Calling drop_keep per element hashed every pair twice: dropout cost the forward 57 % of its
// time, 48.6 -> 76.2 us per BERT layer, tools/attn_bench.py.)
__device__ __forceinline__ void akeep2(uint32_t key, uint64_t idx, uint32_t thresh, bool& k0, bool& k1) {
  const uint32_t h = drop_pair_bits(key, idx);
  k0 = (h & 0xffffu) >= (thresh >> 16);
  k1 = (h >> 16) >= (thresh >> 16);
}
__device__ __forceinline__ uint32_t attn_key(uint32_t seed, const int64_t* step) {
  return drop_mix32(seed * 0x27d4eb2fu ^ (uint32_t)(step ? *step : 0) * 0x165667b1u);
}

// A/B fragment whose 8 k-values are contiguous in LDS: lane -> row r0 + lane%32, k = k0 + 8*(lane/32) + e
__device__ __forceinline__ abf16x8 rowfrag(const uint8_t* base, int stride_b, int r0, int k0) {
  const int lane = threadIdx.x & 63;
  const u32x4 w = *reinterpret_cast<const u32x4*>(base + (r0 + (lane & 31)) * stride_b + (k0 + 8 * (lane >> 5)) * 2);
  return __builtin_bit_cast(abf16x8, w);
}
// Same fragment from a [k][col] tile (col contiguous): ds_read_b64_tr_b16 transposes within 16 lanes.
// lane -> col c0 + lane%32, k = k0 + 8*(lane/32) + e
__device__ __forceinline__ abf16x8 trfrag(const uint8_t* base, int stride_b, int k0, int c0) {
  const int lane = threadIdx.x & 63;
  const int G = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int k = k0 + 8 * (G >> 1) + q;
  const int col = c0 + 16 * (G & 1) + 4 * p;
  const as16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((alds_s16x4*)(base + k * stride_b + col * 2));
  const as16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((alds_s16x4*)(base + (k + 4) * stride_b + col * 2));
  as16x4 both[2] = {lo, hi};
  return __builtin_bit_cast(abf16x8, both);
}

// trfrag with the key order of a 32x32 accumulator's rows: k-slot e of lane half hh is key
// kb + 8*(e/4) + 4*hh + e%4 -- exactly the keys acc_row(8*ks2 + e, hh) a lane holds in registers, so the
// softmax probabilities feed the P V MFMA as its B operand straight from the S^T accumulators
// (the k sum is order-free; A = V^T is read in the same permuted order)
__device__ __forceinline__ abf16x8 trfrag_accrows(const uint8_t* base, int stride_b, int kb, int c0) {
  const int lane = threadIdx.x & 63;
  const int G = lane >> 4, i16 = lane & 15, q = i16 >> 2, p = i16 & 3;
  const int k = kb + 4 * (G >> 1) + q;
  const int col = c0 + 16 * (G & 1) + 4 * p;
  const as16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((alds_s16x4*)(base + k * stride_b + col * 2));
  const as16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((alds_s16x4*)(base + (k + 8) * stride_b + col * 2));
  as16x4 both[2] = {lo, hi};
  return __builtin_bit_cast(abf16x8, both);
}

__device__ __forceinline__ af32x16 mfma(abf16x8 a, abf16x8 b, af32x16 c) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ af32x16 zero16() {
  af32x16 z;
#pragma unroll
  for (int i = 0; i < 16; ++i) z[i] = 0.f;
  return z;
}
// accumulator element i of a 32x32 tile: row (i&3) + 8*(i>>2) + 4*(lane/32), col lane%32
__device__ __forceinline__ int acc_row(int i, int hh) { return (i & 3) + 8 * (i >> 2) + 4 * hh; }

// valid rows of sequence b: S without lengths; else lens[b] clamped to [0, S] here, on the device (the
// host never reads lens, so a replayed graph sees the current values)
// The causal copies always run the length-aware code and are launched with or without lengths: only
// they test a.lens for null (L = S then).
template <bool VARLEN, bool CAUSAL = false>
__device__ __forceinline__ int item_len(const AttnArgs& a, int b, int S) {
  if constexpr (VARLEN) {
    if constexpr (CAUSAL) {
      if (!a.lens) return S;
    }
    return min(max(a.lens[b], 0), S);
  } else {
    return S;
  }
}
__device__ __forceinline__ u32x4 zero4() { return u32x4{0u, 0u, 0u, 0u}; }

// packed documents (DOCS copies, a.doc given; always causal): first token of the document of token t of
// sequence b, clamped to [0, t] here on the device. The value is only ever compared with key and query
// indices, never used as an address; callers pass t < L only, so entries past a length are never read.
template <bool DOCS>
__device__ __forceinline__ int doc_of(const AttnArgs& a, int b, int S, int t) {
  if constexpr (DOCS) {
    return min(max(a.doc[(int64_t)b * S + t], 0), t);
  } else {
    return 0;
  }
}

// first key that token t of sequence b may see. DOCS copies: its document's start. WINDOW copies (a.window
// = W >= 1, a.doc given or null -- only they test it): max(doc, t - W + 1, 0). Like a document start it is
// <= t, non-decreasing in t, only compared, and asked for t < L only; unlike one it is not a fixed point
// (lb(lb(t)) < lb(t) in general), so nothing may assume that the key lb(t) has itself as its lower bound.
template <bool DOCS, bool WINDOW = false>
__device__ __forceinline__ int lb_of(const AttnArgs& a, int b, int S, int t) {
  if constexpr (WINDOW) {
    const int d = a.doc ? min(max(a.doc[(int64_t)b * S + t], 0), t) : 0;
    return max(d, t - a.window + 1);  // 1 <= W <= INT32_MAX, t >= 0: no overflow; d >= 0 holds the floor
  } else {
    return doc_of<DOCS>(a, b, S, t);
  }
}

}  // namespace

}  // namespace psd
