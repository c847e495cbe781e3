// Gated SiLU activation (SwiGLU) between the two GEMMs of a Llama-style FFN for gfx950. The packed
// gate/up tensor gu [T, 2F] bf16 (gate g = columns [0, F), up u = columns [F, 2F): a checkpoint's gate_proj
// and up_proj concatenated) is read in place, no split copies.
//
//   forward   a  = bf16(silu(g) * u),  silu(g) = g * sig,  sig = 1 / (1 + exp(-g))
//   backward  dg = bf16(da * u * sig * (1 + g * (1 - sig))),  du = bf16(da * g * sig)
// fp32 math, one rounding; the backward recomputes sig from gu, nothing else is saved.
//
// Work item: 8 consecutive columns of one row: two 16-byte loads (g, u) and one 16-byte store forward,
// three loads and two stores backward. Items are numbered row-major and walked by a grid-stride loop of
// 256-lane workgroups (<= 2048); a lane keeps (row, item in row) and advances them by the stride's
// precomputed (rows, items) split, so the loop has no division; row and element offsets are 64-bit.
//
// Regime: pure streaming (guide Appendix B, element-wise): 6 bytes per element forward, 10 backward.
// Plain stores: the next GEMM reads a (and the gate/up GEMM's backward reads dgu) at once. The exponential
// is one v_exp_f32 (__expf) and the division one v_rcp_f32: both within ~1 ulp, so sig is within a few
// fp32 ulps -- far inside the 2^-9 relative the bf16 rounding leaves -- and the VALU work per 16-byte item
// stays below what the loads take. exp(-g) = inf for g < -88 gives sig = 0 and a = dg = du = 0, the limits.
// No LDS, no atomics, nothing summed: each output is a function of its own inputs, so the bits do not
// depend on the grid and two runs are equal.
#include "common.h"
#include "launchers_swiglu.h"

namespace psd {

namespace {
__device__ __forceinline__ float sigmoid_f32(float g) { return __builtin_amdgcn_rcpf(1.f + __expf(-g)); }

// the grid-stride walk over (row, item in row): L items per row, the stride split into srow rows + srem items
struct ItemWalk {
  int64_t row;
  uint32_t c;
};
__device__ __forceinline__ ItemWalk walk_start(uint32_t L) {
  const uint32_t idx0 = blockIdx.x * 256u + threadIdx.x;  // < 2048 * 256
  const uint32_t row0 = idx0 / L;
  return {(int64_t)row0, idx0 - row0 * L};
}
__device__ __forceinline__ void walk_next(ItemWalk& w, uint32_t L, int64_t srow, uint32_t srem) {
  w.c += srem;  // < 2 L <= 2^29
  if (w.c >= L) {
    w.c -= L;
    ++w.row;
  }
  w.row += srow;
}
}  // namespace

__global__ __launch_bounds__(256) void swiglu_fwd_kernel(SwigluArgs a, uint32_t L, int64_t srow, uint32_t srem) {
  const int64_t F = a.F;
  for (ItemWalk w = walk_start(L); w.row < a.T; walk_next(w, L, srow, srem)) {
    const uint16_t* p = a.gu + w.row * 2 * F + (int64_t)w.c * 8;
    float g[8], u[8], o[8];
    load8_bf16(p, g);
    load8_bf16(p + F, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (g[e] * sigmoid_f32(g[e])) * u[e];
    store8_bf16(a.a + w.row * F + (int64_t)w.c * 8, o);
  }
}

__global__ __launch_bounds__(256) void swiglu_bwd_kernel(SwigluArgs a, uint32_t L, int64_t srow, uint32_t srem) {
  const int64_t F = a.F;
  for (ItemWalk w = walk_start(L); w.row < a.T; walk_next(w, L, srow, srem)) {
    const int64_t off2 = w.row * 2 * F + (int64_t)w.c * 8;
    float g[8], u[8], d[8], dg[8], du[8];
    load8_bf16(a.gu + off2, g);
    load8_bf16(a.gu + off2 + F, u);
    load8_bf16(a.da + w.row * F + (int64_t)w.c * 8, d);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sig = sigmoid_f32(g[e]);
      const float ds = d[e] * sig;
      dg[e] = (ds * u[e]) * fmaf(g[e], 1.f - sig, 1.f);
      du[e] = ds * g[e];
    }
    store8_bf16(a.dgu + off2, dg);
    store8_bf16(a.dgu + off2 + F, du);
  }
}

namespace {
template <typename K>
hipError_t launch_swiglu(K kernel, const SwigluArgs& a, hipStream_t st) {
  // L < 2^28 keeps the 32-bit item-in-row arithmetic of the walk exact
  if (a.T < 0 || a.F < 0 || a.F % 8 != 0 || a.F / 8 >= (1 << 28) || a.blocks < 0) return hipErrorInvalidValue;
  if (a.T == 0 || a.F == 0) return hipSuccess;
  const int64_t L = a.F / 8;
  if (a.T > INT64_MAX / L) return hipErrorInvalidValue;
  int64_t grid = stream_grid(a.T * L, 256);
  if (a.blocks > 0 && grid > a.blocks) grid = a.blocks;
  const int64_t stride = grid * 256;
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, st, a, (uint32_t)L, stride / L, (uint32_t)(stride % L));
  return hipGetLastError();
}
}  // namespace

hipError_t launch_swiglu_fwd(const SwigluArgs& a, hipStream_t st) {
  if (a.T > 0 && a.F > 0 && (!a.gu || !a.a)) return hipErrorInvalidValue;
  return launch_swiglu(swiglu_fwd_kernel, a, st);
}

hipError_t launch_swiglu_bwd(const SwigluArgs& a, hipStream_t st) {
  if (a.T > 0 && a.F > 0 && (!a.gu || !a.da || !a.dgu)) return hipErrorInvalidValue;
  return launch_swiglu(swiglu_bwd_kernel, a, st);
}

}  // namespace psd
