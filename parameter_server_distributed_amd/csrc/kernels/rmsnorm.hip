// The pre-norm residual step of a Llama-style block for gfx950: r_new = r + dropout(h), y = r_new * rstd *
// gamma with rstd = rsqrt(mean(r_new^2) + eps), and the matching backward (RMSNorm backward + the gradient
// arriving at the residual stream + dropout backward), bf16 in/out, fp32 math. No beta, no mean.
//
// One pass each way: forward reads r and h once and writes r_new, y and one fp32 rstd per row; backward
// reads dy, r_new, rstd (and dr_new) once and writes dr (and dh). The statistics come from the bf16-rounded
// r_new, the value that is stored, so the backward recomputes xh = r_new * rstd from what it is given.
//
// Layout: layernorm.hip's (row_common.h): one wave per row of H = 64*E elements, lane l owning columns
// [l*E, l*E + E), 8-byte loads / stores, wave butterfly reductions, the next row's loads issued before this
// row's reduction. The dropout keep flags are LayerNorm's for the same (seed, step, element); the step is
// read from device memory. dgamma: per-lane column partials over the rows a wave visits -> block partials
// [blk][H] (the four waves summed in a fixed order) -> layernorm.hip's fixed-order finalize with one partial
// row. No atomics; nothing crosses workgroups but through that finalize; every other output element is a
// function of its own row, so the bits do not depend on the grid. Row and element offsets are 64-bit.
#include "common.h"
#include "launchers_ln.h"
#include "launchers_rmsnorm.h"
#include "row_common.h"

namespace psd {

// ADD: with the branch h (r_new is written); without it r_new is r and only y / rstd are written
template <int E, bool ADD>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const uint16_t* __restrict__ r_in, const uint16_t* __restrict__ h,
                                                      const uint16_t* __restrict__ gamma, uint16_t* __restrict__ r_new,
                                                      uint16_t* __restrict__ y, float* __restrict__ rstd_out,
                                                      int64_t rows, float eps, uint32_t seed,
                                                      const int64_t* __restrict__ step, uint32_t thresh, float scale) {
  constexpr int H = 64 * E;
  const int lane = threadIdx.x & 63;
  const int c0 = lane * E;
  float g[E];
  load_e<E>(gamma + c0, g);
  const uint32_t key = ADD ? dropout_key(seed, step) : 0u;
  const int64_t wstride = (int64_t)gridDim.x * (blockDim.x >> 6);
  int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  float nxv[E], nhv[E];
  if (r < rows) {
    load_e<E>(r_in + r * H + c0, nxv);
    if constexpr (ADD) load_e<E>(h + r * H + c0, nhv);
  }
  for (; r < rows; r += wstride) {
    const int64_t off = r * H + c0;
    float xv[E], hv[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      xv[i] = nxv[i];
      if constexpr (ADD) hv[i] = nhv[i];
    }
    const int64_t rn = r + wstride;
    if (rn < rows) {
      load_e<E>(r_in + rn * H + c0, nxv);
      if constexpr (ADD) load_e<E>(h + rn * H + c0, nhv);
    }
    if constexpr (ADD) {
      bool kp[E];
      if (thresh != 0u) keep_flags<E>(key, off, thresh, kp);
#pragma unroll
      for (int i = 0; i < E; ++i) {
        const float d = (thresh == 0u || kp[i]) ? hv[i] * scale : 0.f;
        xv[i] = bf16_to_f32(f32_to_bf16(xv[i] + d));  // r_new, rounded as stored (the norm's input)
      }
      store_e<E>(r_new + off, xv);
    }
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) sq = fmaf(xv[i], xv[i], sq);
    const float rstd = rsqrtf(wave_sum(sq) * (1.f / H) + eps);
#pragma unroll
    for (int i = 0; i < E; ++i) xv[i] = (xv[i] * rstd) * g[i];
    store_e<E>(y + off, xv);
    if (lane == 0) rstd_out[r] = rstd;
  }
}

// DRN: the gradient dr_new arriving at the residual stream is added (else it counts as zero and is not
// read). DH: the pre-dropout gradient dh is written too (p > 0 with a branch; at p == 0 dh is dr itself)
template <int E, bool DRN, bool DH>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ drn,
                                                      const uint16_t* __restrict__ rnew,
                                                      const float* __restrict__ rstd_in,
                                                      const uint16_t* __restrict__ gamma, uint16_t* __restrict__ dr,
                                                      uint16_t* __restrict__ dh, float* __restrict__ part, int64_t rows,
                                                      uint32_t seed, const int64_t* __restrict__ step, uint32_t thresh,
                                                      float scale) {
  constexpr int H = 64 * E;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int c0 = lane * E;
  float g[E], pg[E];
  load_e<E>(gamma + c0, g);
#pragma unroll
  for (int i = 0; i < E; ++i) pg[i] = 0.f;
  const uint32_t key = DH ? dropout_key(seed, step) : 0u;
  const int64_t wstride = (int64_t)gridDim.x * (blockDim.x >> 6);
  int64_t r = (int64_t)blockIdx.x * (blockDim.x >> 6) + wv;
  float ndv[E], nxv[E], nrv[E], nrstd = 0.f;
  if (r < rows) {
    load_e<E>(dy + r * H + c0, ndv);
    load_e<E>(rnew + r * H + c0, nxv);
    if constexpr (DRN) load_e<E>(drn + r * H + c0, nrv);
    nrstd = rstd_in[r];
  }
  for (; r < rows; r += wstride) {
    const int64_t off = r * H + c0;
    float dv[E], xh[E], rv[E];
#pragma unroll
    for (int i = 0; i < E; ++i) {
      dv[i] = ndv[i];
      xh[i] = nxv[i];
      if constexpr (DRN) rv[i] = nrv[i];
    }
    const float rstd = nrstd;
    const int64_t rn = r + wstride;
    if (rn < rows) {
      load_e<E>(dy + rn * H + c0, ndv);
      load_e<E>(rnew + rn * H + c0, nxv);
      if constexpr (DRN) load_e<E>(drn + rn * H + c0, nrv);
      nrstd = rstd_in[rn];
    }
    float b = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      xh[i] *= rstd;
      pg[i] = fmaf(dv[i], xh[i], pg[i]);
      dv[i] *= g[i];
      b = fmaf(dv[i], xh[i], b);
    }
    b = wave_sum(b) * (1.f / H);
#pragma unroll
    for (int i = 0; i < E; ++i) {
      dv[i] = rstd * (dv[i] - xh[i] * b);
      if constexpr (DRN) dv[i] += rv[i];
    }
    store_e<E>(dr + off, dv);
    if constexpr (DH) {
      bool kp[E];
      keep_flags<E>(key, off, thresh, kp);
#pragma unroll
      for (int i = 0; i < E; ++i) dv[i] = kp[i] ? dv[i] * scale : 0.f;  // from the fp32 dr, before its rounding
      store_e<E>(dh + off, dv);
    }
  }
  // block partials of dgamma: [blk][H], waves summed in a fixed order
  __shared__ float red[4][H];
#pragma unroll
  for (int i = 0; i < E; ++i) red[wv][c0 + i] = pg[i];
  __syncthreads();
  for (int c = threadIdx.x; c < H; c += blockDim.x)
    part[(int64_t)blockIdx.x * H + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

bool rms_supported(int H) { return H == 768 || H == 1024; }

// one row per wave, four waves per workgroup, <= 2048 workgroups: past 8192 rows the waves take further rows
int rms_fwd_blocks(int64_t rows) {
  const int64_t want = (rows + 3) / 4;
  return (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

// >= 8 rows per wave, <= 512 workgroups (two per CU): at most 512 dgamma partial rows for the finalize
int rms_bwd_blocks(int64_t rows) {
  const int64_t want = (rows + 4 * 8 - 1) / (4 * 8);
  return (int)(want < 1 ? 1 : (want > 512 ? 512 : want));
}

hipError_t launch_rms_fwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  const int blocks = rms_fwd_blocks(a.rows);
  const bool add = a.h != nullptr;
  const uint32_t th = add ? keep_thresh(a.p) : 0u;
  const float sc = (add && a.p > 0.f) ? 1.f / (1.f - a.p) : 1.f;
#define PSD_RMSF(E, ADD)                                                                                        \
  hipLaunchKernelGGL((rms_fwd_kernel<E, ADD>), dim3(blocks), dim3(256), 0, st, a.r, a.h, a.gamma, a.r_new, a.y, \
                     a.rstd, a.rows, a.eps, a.seed, a.step, th, sc)
  if (a.H == 768) {
    if (add) PSD_RMSF(12, true);
    else PSD_RMSF(12, false);
  } else {
    if (add) PSD_RMSF(16, true);
    else PSD_RMSF(16, false);
  }
#undef PSD_RMSF
  return hipGetLastError();
}

hipError_t launch_rms_bwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  const int blocks = rms_bwd_blocks(a.rows);
  const uint32_t th = keep_thresh(a.p);
  const bool drn = a.dr_new != nullptr;
  const bool dh = a.dh != nullptr;  // null at p == 0: dh is dr, written once
  const float sc = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
#define PSD_RMSB(E, DRN, DH)                                                                                      \
  hipLaunchKernelGGL((rms_bwd_kernel<E, DRN, DH>), dim3(blocks), dim3(256), 0, st, a.dy, a.dr_new, a.rn, a.rstd_in, \
                     a.gamma, a.dr, a.dh, a.part, a.rows, a.seed, a.step, th, sc)
#define PSD_RMSB_E(E)                      \
  do {                                     \
    if (drn && dh) PSD_RMSB(E, true, true); \
    else if (drn) PSD_RMSB(E, true, false); \
    else if (dh) PSD_RMSB(E, false, true);  \
    else PSD_RMSB(E, false, false);         \
  } while (0)
  if (a.H == 768) PSD_RMSB_E(12);
  else PSD_RMSB_E(16);
#undef PSD_RMSB_E
#undef PSD_RMSB
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_ln_param_grad(a.part, blocks, a.H, 1, a.dgamma, nullptr, nullptr, st);
}

}  // namespace psd
