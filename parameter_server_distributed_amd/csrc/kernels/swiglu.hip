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
//
// MX side outputs (template MX, SwigluArgs q8 / sc8; the fp8 Llama block): the forward also writes the MX
// e4m3 copy of a [T, F] -- the down Linear's forward operand -- and the backward the MX e5m2 copy of dgu
// [T, 2F] -- the gate/up Linear's bwd-data operand: fp8 payload plus one E8M0 byte per 32 columns, bitwise
// quant_mx_kernel (fp8.hip) of the bf16 tensor the same launch stores, from the registers that hold it. A
// lane's item is 8 consecutive columns, so a 32-column MX block is the 4 items of one aligned lane quad and
// mx_quant8 (mx_common.h: two quad-permute DPPs for the amax) applies as in the stand-alone pass; one 8-byte
// payload store per lane and half, the quad's first lane stores the scale byte.
// Why the quad exchange is valid -- the variant requires F % 32 == 0 (checked by the launcher):
//   * L = F / 8 is then a multiple of 4. Lanes 4q .. 4q+3 start at the consecutive item numbers idx0 =
//     4k .. 4k+3; row0 = idx0 / L is the same for the four (a multiple of 4 divides their common base), and
//     c = idx0 - row0 L = 4m .. 4m+3: one row, one block, in element order.
//   * the grid-stride is gridDim * 256, a multiple of 4, so srem = stride % L is a multiple of 4 and
//     srow is common: walk_next adds the same srem to the four c, the sums are again 4m' .. 4m'+3, and L % 4
//     == 0 makes `c >= L` one decision for the quad. By induction the quad stays in one row and one block.
//   * the loop condition row < T is therefore also one decision per quad: a quad is wholly inside the
//     tensor or has wholly left the loop, so the DPP reads only lanes that hold this block's items.
#include "common.h"
#include "launchers_swiglu.h"
#include "mx_common.h"

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

// t -> the values its bf16 store keeps (what the MX copy is the quantisation of)
__device__ __forceinline__ void round8_bf16(float (&t)[8]) {
#pragma unroll
  for (int e = 0; e < 8; ++e) t[e] = bf16_to_f32(f32_to_bf16(t[e]));
}

// The quad's MX block of 32 columns starting at element offset `off` (a multiple of 8; the quad's first lane
// has off % 32 == 0) of a contiguous tensor whose rows are whole blocks: payload at q8 + off, scale byte at
// sc8[off / 32]. All four lanes of the quad call it together.
template <bool E5>
__device__ __forceinline__ void mx_store8(float (&t)[8], uint8_t* __restrict__ q8, uint8_t* __restrict__ sc8,
                                          int64_t off) {
  round8_bf16(t);
  uint2 qb;
  const int eb = mx_quant8<E5>(t, qb);
  *reinterpret_cast<uint2*>(q8 + off) = qb;
  if ((off & 31) == 0) sc8[off >> 5] = (uint8_t)eb;
}
}  // namespace

template <bool MX>
__global__ __launch_bounds__(256) void swiglu_fwd_kernel(SwigluArgs a, uint32_t L, int64_t srow, uint32_t srem) {
  const int64_t F = a.F;
  for (ItemWalk w = walk_start(L); w.row < a.T; walk_next(w, L, srow, srem)) {
    const uint16_t* p = a.gu + w.row * 2 * F + (int64_t)w.c * 8;
    float g[8], u[8], o[8];
    load8_bf16(p, g);
    load8_bf16(p + F, u);
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (g[e] * sigmoid_f32(g[e])) * u[e];
    const int64_t off = w.row * F + (int64_t)w.c * 8;
    store8_bf16(a.a + off, o);
    if constexpr (MX) mx_store8<false>(o, a.q8, a.sc8, off);
  }
}

template <bool MX>
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
    if constexpr (MX) {  // F % 32 == 0: off2 + F is block-aligned where off2 is
      mx_store8<true>(dg, a.q8, a.sc8, off2);
      mx_store8<true>(du, a.q8, a.sc8, off2 + F);
    }
  }
}

namespace {
template <typename K>
hipError_t launch_swiglu(K kernel, const SwigluArgs& a, hipStream_t st) {
  // L < 2^28 keeps the 32-bit item-in-row arithmetic of the walk exact
  if (a.T < 0 || a.F < 0 || a.F % 8 != 0 || a.F / 8 >= (1 << 28) || a.blocks < 0) return hipErrorInvalidValue;
  // the MX variants: both pointers, and rows of whole 32-column blocks (the quad argument in the header)
  if ((a.q8 == nullptr) != (a.sc8 == nullptr) || (a.q8 != nullptr && a.F % 32 != 0)) return hipErrorInvalidValue;
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
  return a.q8 ? launch_swiglu(swiglu_fwd_kernel<true>, a, st) : launch_swiglu(swiglu_fwd_kernel<false>, a, st);
}

hipError_t launch_swiglu_bwd(const SwigluArgs& a, hipStream_t st) {
  if (a.T > 0 && a.F > 0 && (!a.gu || !a.da || !a.dgu)) return hipErrorInvalidValue;
  return a.q8 ? launch_swiglu(swiglu_bwd_kernel<true>, a, st) : launch_swiglu(swiglu_bwd_kernel<false>, a, st);
}

}  // namespace psd
