// Per-element optimizer update and multi-source gradient load shared by the flat apply kernel
// (optim.hip) and the segmented layer-wise kernels (optim_lw.hip): one definition, so the two
// produce the same bits for the same inputs.
#pragma once
#include "common.h"
#include "launchers.h"
#include "mx_common.h"

namespace psd {

template <int KIND>
__device__ __forceinline__ void opt_update(const OptimHyper& h, float lr, float bc1, float bc2_sqrt,
                                           bool first, float& p, float g, float& s1, float& s2) {
  if (h.maximize) g = -g;
  if (KIND == OPT_SGD) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    p = fmaf(-lr, g, p);
  } else if (KIND == OPT_MOMENTUM) {
    if (h.weight_decay != 0.f) g = fmaf(h.weight_decay, p, g);
    float buf = first ? g : fmaf(h.momentum, s1, (1.f - h.dampening) * g);
    s1 = buf;
    float d = h.nesterov ? fmaf(h.momentum, buf, g) : buf;
    p = fmaf(-lr, d, p);
  } else {  // ADAM / ADAMW
    if (KIND == OPT_ADAMW) {
      p = p * (1.f - lr * h.weight_decay);
    } else if (h.weight_decay != 0.f) {
      g = fmaf(h.weight_decay, p, g);
    }
    float m = fmaf(h.beta1, s1, (1.f - h.beta1) * g);
    float v = fmaf(h.beta2, s2, (1.f - h.beta2) * g * g);
    s1 = m;
    s2 = v;
    float denom = __fsqrt_rn(v) / bc2_sqrt + h.eps;
    p = p - (lr / bc1) * (m / denom);
  }
}

// Per-source scales (SourceList::scale, the gradient-clipping coefficients of the pushes): thread 0
// reads the K device scalars once into LDS and every lane takes them from there. The unscaled
// instantiation declares no LDS and returns null.
template <bool SCALED>
__device__ __forceinline__ const float* stage_scales(const SourceList& g) {
  if constexpr (SCALED) {
    __shared__ float sc[kMaxSources];
    if (threadIdx.x == 0)
      for (int k = 0; k < g.count; ++k) sc[k] = *g.scale[k];
    __syncthreads();
    return sc;
  } else {
    return nullptr;
  }
}

// 8 elements of an MX source (DT_MX8) at i (a multiple of 8): 8 e4m3 payload bytes and the E8M0 byte
// of their 32-element block, dequantised as dequant_mx does: q * 2^(byte - 127) in fp32, exact (and
// exactly representable in bf16) for normal-range values.
__device__ __forceinline__ void load8_mx(const uint8_t* __restrict__ q, const uint8_t* __restrict__ sc, int64_t i,
                                         float t[8]) {
  const uint2 b = *reinterpret_cast<const uint2*>(q + i);
  const float s = __uint_as_float((uint32_t)sc[i >> 5] << 23);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    t[e] = e4m3_to_f32((uint8_t)(b.x >> (8 * e))) * s;
    t[e + 4] = e4m3_to_f32((uint8_t)(b.y >> (8 * e))) * s;
  }
}

// out = scale * sum_k src_k[i..i+8), or with SCALED scale * sum_k sc[k] * src_k (one fma per source
// element, in source order; sc[k] == 1 gives the unscaled bits)
template <int SRC_DT, bool SCALED = false>
__device__ __forceinline__ void load_sources8(const SourceList& g, int64_t i, float scale, float out[8],
                                              const float* sc = nullptr) {
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] = 0.f;
  for (int k = 0; k < g.count; ++k) {
    float t[8];
    if constexpr (SRC_DT == DT_MX8)
      load8_mx(static_cast<const uint8_t*>(g.ptr[k]), g.mx_scale[k], i, t);
    else if (SRC_DT == DT_BF16)
      load8_bf16(static_cast<const uint16_t*>(g.ptr[k]) + i, t);
    else
      load8_f32(static_cast<const float*>(g.ptr[k]) + i, t);
    if (SCALED) {
      const float c = sc[k];
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] = fmaf(c, t[e], out[e]);
    } else {
#pragma unroll
      for (int e = 0; e < 8; ++e) out[e] += t[e];
    }
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) out[e] *= scale;
}

}  // namespace psd
