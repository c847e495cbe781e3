// Segmented (per-tensor) parameter-server apply for gfx950: LARS, LAMB and per-tensor weight-decay
// exclusion for the flat optimizers.
//
// The flat apply (optim.hip) knows nothing about tensor boundaries. Here the buffer comes with a
// layer table (launchers_optim_lw.h): segments, one per tensor, cut into chunks of <= 8192 elements
// numbered from the segment's start. Three launches per step for the layer-wise kinds:
//
//   norm pass   one read of the K gradient sources (summed in registers like the flat kernel) and
//               of the master; per chunk sum w^2 and sum g^2 (LARS), or the Adam moments updated
//               and stored plus sum w^2 and sum u^2 (LAMB stage 1). Each chunk writes its own two
//               floats: no atomics, nothing to zero between steps.
//   finalize    one wave per segment adds the segment's chunk partials in a fixed order -> ratio[t]
//   apply       ratio[t] / wd_mult[t] through the chunk's segment id; master, state and the bf16
//               shadow written in one pass. LARS reads the sources again; LAMB stage 2 recomputes u
//               from the stored m, v, w with the very expression of stage 1 (no gradient read, no
//               scratch buffer).
//
// SGD / momentum / Adam / AdamW with decay exclusion run the apply alone, with the flat kernel's
// opt_update (optim_update.h) and weight_decay * wd_mult[t].
//
// Regime and rules as optim.hip: HBM streaming, 256-thread blocks, 16-byte vector accesses, no LDS
// staging of data (the only LDS is the 8-float exchange of the block reduction, and in the SCALED
// instantiations the K per-source clipping scalars; both LARS reads of the sources are scaled). A
// workgroup owns a whole chunk (4 vectors of 8 per lane) and walks the chunk table with a grid-stride loop, and
// every sum has a fixed order (lane-sequential, xor butterfly, waves 0..3, chunks in lane order),
// so the result does not depend on the grid, on grid_cap, or on where the buffer is cut into shards
// as long as the cuts are tensor starts.
#include "block_sum.h"
#include "common.h"
#include "launchers_optim_lw.h"
#include "optim_update.h"

namespace psd {

namespace {

struct LwChunk {
  int seg;
  int64_t off;   // first element
  int nvec;      // 8-element vectors in the chunk
};

__device__ __forceinline__ LwChunk lw_chunk(const LwTable& t, int c) {
  LwChunk k;
  k.seg = t.chunk_seg[c];
  k.off = t.chunk_off[c];
  const int64_t left = t.seg_start[k.seg + 1] - k.off;
  k.nvec = (int)((left < kLwChunk ? left : kLwChunk) >> 3);
  return k;
}

// LAMB update direction; stage 1 (norms) and stage 2 (apply) must agree bit for bit, so every
// operation is spelled out (nothing left for the compiler to contract one way here and another there)
__device__ __forceinline__ float lamb_u(float m, float v, float w, float bc1, float bc2_sqrt, float eps, float wd) {
  const float q = (m / bc1) / (__fsqrt_rn(v) / bc2_sqrt + eps);
  return fmaf(wd, w, q);
}

}  // namespace

template <int SRC_DT, bool LAMB, bool SCALED = false>
__global__ __launch_bounds__(256) void lw_norm_kernel(OptimHyper h, const OptimDyn* __restrict__ dyn,
                                                      const float* __restrict__ master, SourceList g,
                                                      float* __restrict__ s1, float* __restrict__ s2, LwTable t) {
  __shared__ float red[8];
  const float* sc = stage_scales<SCALED>(g);
  const float gs = dyn->grad_scale;
  const float bc1 = dyn->bc1;
  const float bc2s = sqrtf(dyn->bc2);
  for (int c = blockIdx.x; c < t.n_chunks; c += gridDim.x) {
    const LwChunk ck = lw_chunk(t, c);
    const float wd = h.weight_decay * t.wd_mult[ck.seg];
    float aw = 0.f, ab = 0.f;
    for (int v = threadIdx.x; v < ck.nvec; v += 256) {
      const int64_t i = ck.off + ((int64_t)v << 3);
      float gr[8], p[8];
      load_sources8<SRC_DT, SCALED>(g, i, gs, gr, sc);
      load8_f32(master + i, p);
      if (LAMB) {
        float a[8], b[8];
        load8_f32(s1 + i, a);
        load8_f32(s2 + i, b);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float ge = h.maximize ? -gr[e] : gr[e];
          a[e] = fmaf(h.beta1, a[e], (1.f - h.beta1) * ge);
          b[e] = fmaf(h.beta2, b[e], (1.f - h.beta2) * ge * ge);
          const float u = lamb_u(a[e], b[e], p[e], bc1, bc2s, h.eps, wd);
          aw = fmaf(p[e], p[e], aw);
          ab = fmaf(u, u, ab);
        }
        store8_f32(s1 + i, a);
        store8_f32(s2 + i, b);
      } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          aw = fmaf(p[e], p[e], aw);
          ab = fmaf(gr[e], gr[e], ab);
        }
      }
    }
    block_sum2_store(aw, ab, red, t.partials + 2 * (int64_t)c);
  }
}

// one wave per segment: lane l adds chunks l, l + 64, ... of the segment in order, then the butterfly
template <bool LAMB>
__global__ __launch_bounds__(64) void lw_finalize_kernel(OptimHyper h, LwTable t) {
  for (int s = blockIdx.x; s < t.n_seg; s += gridDim.x) {
    const int c0 = t.seg_chunk[s], c1 = t.seg_chunk[s + 1];
    float aw = 0.f, ab = 0.f;
    for (int c = c0 + threadIdx.x; c < c1; c += kWave) {
      aw += t.partials[2 * (int64_t)c];
      ab += t.partials[2 * (int64_t)c + 1];
    }
    aw = wave_sum(aw);
    ab = wave_sum(ab);
    if (threadIdx.x == 0) {
      const float wn = __fsqrt_rn(aw), bn = __fsqrt_rn(ab);
      float r = 1.f;
      if (t.adapt[s] && wn > 0.f && bn > 0.f) {
        if (LAMB) {
          r = wn / bn;
        } else {
          const float wd = h.weight_decay * t.wd_mult[s];
          r = t.trust_coef * wn / (bn + wd * wn + h.eps);
        }
      }
      t.ratio[s] = r;
    }
  }
}

template <int KIND, int SRC_DT, bool SCALED = false>
__global__ __launch_bounds__(256) void lw_apply_kernel(OptimHyper h, const OptimDyn* __restrict__ dyn,
                                                       float* __restrict__ master, SourceList g,
                                                       float* __restrict__ s1, float* __restrict__ s2,
                                                       uint16_t* __restrict__ shadow, LwTable t) {
  const float lr = dyn->lr;
  const float gs = dyn->grad_scale;
  const float bc1 = dyn->bc1;
  const float bc2s = sqrtf(dyn->bc2);
  const bool first = dyn->step <= 1;
  const bool has_state = (KIND != OPT_SGD);
  const bool two_state = (KIND == OPT_ADAM || KIND == OPT_ADAMW || KIND == OPT_LAMB);
  const bool layerwise = (KIND == OPT_LARS || KIND == OPT_LAMB);
  const float* sc = stage_scales<(SCALED && KIND != OPT_LAMB)>(g);

  for (int c = blockIdx.x; c < t.n_chunks; c += gridDim.x) {
    const LwChunk ck = lw_chunk(t, c);
    const float wd = h.weight_decay * t.wd_mult[ck.seg];
    const float r = layerwise ? t.ratio[ck.seg] : 1.f;
    OptimHyper hs = h;  // this segment's hyper-parameters for the flat update
    hs.weight_decay = (KIND == OPT_LARS) ? 0.f : wd;
    if (KIND == OPT_LARS) hs.maximize = 0;
    for (int v = threadIdx.x; v < ck.nvec; v += 256) {
      const int64_t i = ck.off + ((int64_t)v << 3);
      float gr[8], p[8], a[8], b[8];
      if (KIND != OPT_LAMB) load_sources8<SRC_DT, SCALED>(g, i, gs, gr, sc);
      load8_f32(master + i, p);
      if (has_state) load8_f32(s1 + i, a);
      if (two_state) load8_f32(s2 + i, b);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        if (KIND == OPT_LAMB) {
          const float u = lamb_u(a[e], b[e], p[e], bc1, bc2s, h.eps, wd);
          p[e] = fmaf(-(lr * r), u, p[e]);
        } else if (KIND == OPT_LARS) {
          float ge = h.maximize ? -gr[e] : gr[e];
          if (wd != 0.f) ge = fmaf(wd, p[e], ge);
          opt_update<OPT_MOMENTUM>(hs, lr, bc1, bc2s, first, p[e], r * ge, a[e], b[e]);
        } else {
          opt_update<KIND>(hs, lr, bc1, bc2s, first, p[e], gr[e], a[e], b[e]);
        }
      }
      store8_f32(master + i, p);
      if (has_state && KIND != OPT_LAMB) store8_f32(s1 + i, a);
      if (two_state && KIND != OPT_LAMB) store8_f32(s2 + i, b);
      if (shadow) store8_bf16(shadow + i, p);
    }
  }
}

namespace {

inline int lw_grid(int64_t items, int grid_cap) {
  int64_t g = items < 1 ? 1 : items;
  if (g > 2048) g = 2048;
  if (grid_cap > 0 && g > grid_cap) g = grid_cap;
  return (int)g;
}

inline bool lw_table_ok(const LwTable& t) {
  return t.n_seg >= 1 && t.n_chunks >= 1 && t.seg_start && t.seg_chunk && t.wd_mult && t.adapt && t.chunk_seg &&
         t.chunk_off && t.partials && t.ratio;
}

// bf16 / fp32 sources, or MX sources with their scale bytes (a layer table's range is a multiple of 8
// elements and MX sources are whole 32-element blocks: the host entry point checks the length)
inline bool lw_src_ok(const SourceList& g) {
  if (g.dtype == DT_MX8) return source_mx_ok(g, 0);
  return g.dtype == DT_BF16 || g.dtype == DT_F32;
}

template <int KIND>
void lw_apply_src(const OptimHyper& h, const OptimDyn* dyn, float* master, const SourceList& g, float* s1, float* s2,
                  uint16_t* shadow, const LwTable& t, hipStream_t st, int grid) {
  // LAMB stage 2 reads no gradient: one instantiation, scales or not
  const bool scaled = KIND != OPT_LAMB && source_scale_mode(g) == 1;
#define PSD_LW_APPLY(DT, SC)                                                                                        \
  hipLaunchKernelGGL((lw_apply_kernel<KIND, DT, SC>), dim3(grid), dim3(256), 0, st, h, dyn, master, g, s1, s2, shadow, t)
  if (g.dtype == DT_MX8) {
    if (scaled) PSD_LW_APPLY(DT_MX8, true);
    else PSD_LW_APPLY(DT_MX8, false);
  } else if (g.dtype == DT_BF16) {
    if (scaled) PSD_LW_APPLY(DT_BF16, true);
    else PSD_LW_APPLY(DT_BF16, false);
  } else {
    if (scaled) PSD_LW_APPLY(DT_F32, true);
    else PSD_LW_APPLY(DT_F32, false);
  }
#undef PSD_LW_APPLY
}

}  // namespace

hipError_t launch_lw_norms(const OptimHyper& h, const OptimDyn* dyn, const float* master, const SourceList& g,
                           float* s1, float* s2, const LwTable& t, hipStream_t st, int grid_cap) {
  if (!lw_table_ok(t) || g.count < 1 || g.count > kMaxSources) return hipErrorInvalidValue;
  if (!lw_src_ok(g)) return hipErrorInvalidValue;
  const int mode = source_scale_mode(g);
  if (mode < 0) return hipErrorInvalidValue;
  const int grid = lw_grid(t.n_chunks, grid_cap);
  const bool bf = g.dtype == DT_BF16, mx = g.dtype == DT_MX8;
#define PSD_LW_NORM(DT, LAMB)                                                                                          \
  do {                                                                                                                 \
    if (mode == 1)                                                                                                     \
      hipLaunchKernelGGL((lw_norm_kernel<DT, LAMB, true>), dim3(grid), dim3(256), 0, st, h, dyn, master, g, s1, s2, t); \
    else                                                                                                               \
      hipLaunchKernelGGL((lw_norm_kernel<DT, LAMB, false>), dim3(grid), dim3(256), 0, st, h, dyn, master, g, s1, s2, t); \
  } while (0)
  if (h.kind == OPT_LARS) {
    if (mx) PSD_LW_NORM(DT_MX8, false);
    else if (bf) PSD_LW_NORM(DT_BF16, false);
    else PSD_LW_NORM(DT_F32, false);
  } else if (h.kind == OPT_LAMB) {
    if (!s1 || !s2) return hipErrorInvalidValue;
    if (mx) PSD_LW_NORM(DT_MX8, true);
    else if (bf) PSD_LW_NORM(DT_BF16, true);
    else PSD_LW_NORM(DT_F32, true);
  } else {
    return hipErrorInvalidValue;
  }
#undef PSD_LW_NORM
  return hipGetLastError();
}

hipError_t launch_lw_finalize(const OptimHyper& h, const LwTable& t, hipStream_t st, int grid_cap) {
  if (!lw_table_ok(t)) return hipErrorInvalidValue;
  const int grid = lw_grid(t.n_seg, grid_cap);
  if (h.kind == OPT_LARS)
    hipLaunchKernelGGL((lw_finalize_kernel<false>), dim3(grid), dim3(kWave), 0, st, h, t);
  else if (h.kind == OPT_LAMB)
    hipLaunchKernelGGL((lw_finalize_kernel<true>), dim3(grid), dim3(kWave), 0, st, h, t);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_lw_apply(const OptimHyper& h, const OptimDyn* dyn, float* master, const SourceList& g, float* s1,
                           float* s2, uint16_t* shadow, const LwTable& t, hipStream_t st, int grid_cap) {
  if (!lw_table_ok(t)) return hipErrorInvalidValue;
  if (h.kind != OPT_LAMB && (g.count < 1 || g.count > kMaxSources)) return hipErrorInvalidValue;
  if (!lw_src_ok(g)) return hipErrorInvalidValue;
  if (h.kind != OPT_LAMB && source_scale_mode(g) < 0) return hipErrorInvalidValue;
  const int grid = lw_grid(t.n_chunks, grid_cap);
  switch (h.kind) {
    case OPT_SGD: lw_apply_src<OPT_SGD>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    case OPT_MOMENTUM: lw_apply_src<OPT_MOMENTUM>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    case OPT_ADAM: lw_apply_src<OPT_ADAM>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    case OPT_ADAMW: lw_apply_src<OPT_ADAMW>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    case OPT_LARS: lw_apply_src<OPT_LARS>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    case OPT_LAMB: lw_apply_src<OPT_LAMB>(h, dyn, master, g, s1, s2, shadow, t, st, grid); break;
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace psd
