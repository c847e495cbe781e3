// The pre-norm residual step of rmsnorm.hip -- r_new = r + dropout(h), y = r_new * rstd * gamma, and its
// backward -- for the wide hidden sizes H = 512 n, n = 3 .. 16 (1536 .. 8192). Same semantics, same outputs,
// same contracts as rmsnorm.hip (its header and launchers_rmsnorm.h spell them out); another row layout,
// because one wave per row with the row in fp32 registers twice over stops fitting past H = 1024.
//
// Work split: one 256-lane workgroup per row per round, grid-stride over rows (64-bit offsets). A row is
// H / 8 = 64 n chunks of 8 consecutive columns (16 bytes of bf16); lane t owns chunks j = t + 256 s, s < S =
// ceil(H / 2048) (template, 1 .. 4): slab s is 2048 consecutive columns read by 256 consecutive 16-byte
// accesses. A chunk exists when j < 64 n. A wave's 64 chunks of a slab start at a multiple of 64, so the test is
// one decision per wave: a partly filled last slab (H = 1536, 2560, ...) idles whole waves, never lanes.
//
// Registers: the current row in fp32, 8 S <= 32 values per lane per tensor. The next row's 16-byte loads are
// issued before this row's reduction and stay packed as loaded (4 VGPRs per slab per tensor) until they
// become current. gamma stays packed too. The backward's dr_new is not needed before the reduction: it is
// loaded for the current row at the top of the round and used after the barrier, so it is never held twice.
//
// Row reduction (sum x^2 forward, b = mean(g xh) backward; rstd is given there): wave butterfly, the four wave
// sums through LDS, added by every lane in one fixed order. Two LDS slots alternate by round: a wave that
// writes slot k in round k + 2 has passed round k + 1's barrier, which every reader of round k reached after
// reading. One barrier per row. Idle waves add 0 and take the barriers.
//
// dgamma: a column belongs to one lane of the workgroup, so its partial over the rows the workgroup visits
// accumulates in that lane's registers and goes straight to part[blk][H] -- no LDS, no cross-wave add -- and
// layernorm.hip's fixed-order finalize sums the block partials. The result is a function of rows and
// rms_bwd_blocks(rows, H) only.
//
// Grid: forward min(rows, 2048) workgroups, the narrow kernels' cap. Backward min(ceil(rows / 8), 1024): at
// least 8 rows per workgroup, so the partials are at most 1 / 4 of one activation tensor's bytes (4 H bytes per
// 8 rows of 2 H), and at most 1024 partial rows: four workgroups per CU, what fits at the S = 1, 2 register
// counts, and two rounds of residents at S = 3, 4.
//
// Measured (profiles/rmsnorm_wide.md, 16,384 rows): 5.3 - 6.3 TB/s forward, 4.4 - 5.1 TB/s backward at H = 2048 /
// 4096 / 8192. The S = 1 backward is the slowest per byte, and with the e5m2 side output it only ties the plain
// launch + quant_mx_kernel at H = 2048, so ops/rmsnorm.py does not ask for that output at H <= 2048.
//
// MX side outputs: a lane's chunk is a quarter of a 32-column block and the block is the aligned lane quad
// (256 s and 64 n are multiples of 4; a wave is wholly in or out), so mx_quant8 (mx_common.h) applies as in
// swiglu.hip: one 8-byte payload store per chunk, the quad's first lane writes the scale byte. Quantised from
// the bf16-rounded values the same launch stores, after the bf16 stores; the file is built without packed fp32
// instructions and without contraction (every intended FMA is an fmaf), so all variants of a kernel run one
// arithmetic and the bf16 outputs keep their bits. No atomics; every output but dgamma is a function of its own
// row; the step is read on the device.
#include "common.h"
#include "launchers_ln.h"
#include "launchers_rmsnorm.h"
#include "mx_common.h"
#include "row_common.h"

#pragma clang fp contract(off)

#include "row_wide.h"

namespace psd {

// ADD / MX as rms_fwd_kernel
template <int S, bool ADD, bool MX>
__global__ __launch_bounds__(256) void rms_wide_fwd_kernel(const uint16_t* __restrict__ r_in,
                                                           const uint16_t* __restrict__ h,
                                                           const uint16_t* __restrict__ gamma,
                                                           uint16_t* __restrict__ r_new, uint16_t* __restrict__ y,
                                                           float* __restrict__ rstd_out, int64_t rows, int H, float eps,
                                                           uint32_t seed, const int64_t* __restrict__ step,
                                                           uint32_t thresh, float scale, uint8_t* __restrict__ q8,
                                                           uint8_t* __restrict__ sc8) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = H >> 3;
  const float inv_h = 1.f / (float)H;
  u32x4 gp[S], nx[S], nh[S];
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (has_chunk<S>(s, t, nch)) gp[s] = ld16(gamma + 8 * (t + 256 * s));
  const uint32_t key = ADD ? dropout_key(seed, step) : 0u;
  int64_t r = blockIdx.x;
  if (r < rows) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        nx[s] = ld16(r_in + r * H + 8 * (t + 256 * s));
        if constexpr (ADD) nh[s] = ld16(h + r * H + 8 * (t + 256 * s));
      }
  }
  for (int slot = 0; r < rows; r += gridDim.x, slot ^= 1) {
    float xv[S][8];
    float sq = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
        unpack8(nx[s], xv[s]);
        if constexpr (ADD) {
          float hv[8];
          bool kp[8];
          unpack8(nh[s], hv);
          if (thresh != 0u) keep_flags<8>(key, off, thresh, kp);
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const float d = (thresh == 0u || kp[i]) ? hv[i] * scale : 0.f;
            xv[s][i] = bf16_to_f32(f32_to_bf16(xv[s][i] + d));  // r_new, rounded as stored (the norm's input)
          }
          store8_bf16(r_new + off, xv[s]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) sq = fmaf(xv[s][i], xv[s][i], sq);
      }
    const int64_t rn = r + gridDim.x;  // the next row's loads, in flight over the reduction
    if (rn < rows) {
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (has_chunk<S>(s, t, nch)) {
          nx[s] = ld16(r_in + rn * H + 8 * (t + 256 * s));
          if constexpr (ADD) nh[s] = ld16(h + rn * H + 8 * (t + 256 * s));
        }
    }
    const float rstd = rsqrtf(row_sum(sq, red, slot, lane, wv) * inv_h + eps);
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
        float g[8];
        unpack8(gp[s], g);
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[s][i] = (xv[s][i] * rstd) * g[i];
        store8_bf16(y + off, xv[s]);
        if constexpr (MX) mx_chunk_store<false>(xv[s], q8, sc8, off);
      }
    if (t == 0) rstd_out[r] = rstd;
  }
}

// DRN / DH / MXG as rms_bwd_kernel
template <int S, bool DRN, bool DH, bool MXG>
__global__ __launch_bounds__(256) void rms_wide_bwd_kernel(const uint16_t* __restrict__ dy,
                                                           const uint16_t* __restrict__ drn,
                                                           const uint16_t* __restrict__ rnew,
                                                           const float* __restrict__ rstd_in,
                                                           const uint16_t* __restrict__ gamma, uint16_t* __restrict__ dr,
                                                           uint16_t* __restrict__ dh, float* __restrict__ part,
                                                           int64_t rows, int H, uint32_t seed,
                                                           const int64_t* __restrict__ step, uint32_t thresh, float scale,
                                                           uint8_t* __restrict__ q8, uint8_t* __restrict__ sc8) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = H >> 3;
  const float inv_h = 1.f / (float)H;
  u32x4 gp[S], nd[S], nx[S], cr[S];
  float pg[S][8];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (has_chunk<S>(s, t, nch)) gp[s] = ld16(gamma + 8 * (t + 256 * s));
#pragma unroll
    for (int i = 0; i < 8; ++i) pg[s][i] = 0.f;
  }
  const uint32_t key = DH ? dropout_key(seed, step) : 0u;
  int64_t r = blockIdx.x;
  float nrstd = 0.f;
  if (r < rows) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        nd[s] = ld16(dy + r * H + 8 * (t + 256 * s));
        nx[s] = ld16(rnew + r * H + 8 * (t + 256 * s));
      }
    nrstd = rstd_in[r];
  }
  for (int slot = 0; r < rows; r += gridDim.x, slot ^= 1) {
    const float rstd = nrstd;
    float dv[S][8], xh[S][8];
    float b = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        float g[8];
        unpack8(nd[s], dv[s]);
        unpack8(nx[s], xh[s]);
        unpack8(gp[s], g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xh[s][i] *= rstd;
          pg[s][i] = fmaf(dv[s][i], xh[s][i], pg[s][i]);
          dv[s][i] *= g[i];
          b = fmaf(dv[s][i], xh[s][i], b);
        }
      }
    // this row's dr_new (used after the barrier) and the next row's dy / r_new / rstd
    const int64_t rn = r + gridDim.x;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        if constexpr (DRN) cr[s] = ld16(drn + r * H + 8 * (t + 256 * s));
        if (rn < rows) {
          nd[s] = ld16(dy + rn * H + 8 * (t + 256 * s));
          nx[s] = ld16(rnew + rn * H + 8 * (t + 256 * s));
        }
      }
    if (rn < rows) nrstd = rstd_in[rn];
    b = row_sum(b, red, slot, lane, wv) * inv_h;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
#pragma unroll
        for (int i = 0; i < 8; ++i) dv[s][i] = rstd * (dv[s][i] - xh[s][i] * b);
        if constexpr (DRN) {
          float rv[8];
          unpack8(cr[s], rv);
#pragma unroll
          for (int i = 0; i < 8; ++i) dv[s][i] += rv[i];
        }
        store8_bf16(dr + off, dv[s]);
        if constexpr (DH) {
          bool kp[8];
          keep_flags<8>(key, off, thresh, kp);
#pragma unroll
          for (int i = 0; i < 8; ++i) dv[s][i] = kp[i] ? dv[s][i] * scale : 0.f;  // from the fp32 dr
          store8_bf16(dh + off, dv[s]);
        }
        if constexpr (MXG) mx_chunk_store<true>(dv[s], q8, sc8, off);
      }
  }
  // this workgroup's dgamma partial row: each column from the one lane that owns it
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (has_chunk<S>(s, t, nch)) store8_f32(part + (int64_t)blockIdx.x * H + 8 * (t + 256 * s), pg[s]);
}

bool rms_wide(int H) { return H >= 1536 && H <= 8192 && H % 512 == 0; }

int rms_wide_fwd_blocks(int64_t rows) { return (int)(rows < 1 ? 1 : (rows > 2048 ? 2048 : rows)); }

int rms_wide_bwd_blocks(int64_t rows) {
  const int64_t want = (rows + 7) / 8;
  return (int)(want < 1 ? 1 : (want > 1024 ? 1024 : want));
}

hipError_t launch_rms_wide_fwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_wide(a.H) || a.rows < 0) return hipErrorInvalidValue;
  if ((a.q8 == nullptr) != (a.sc8 == nullptr)) return hipErrorInvalidValue;
  const int blocks = rms_wide_fwd_blocks(a.rows);
  const bool add = a.h != nullptr, mx = a.q8 != nullptr;
  const uint32_t th = add ? keep_thresh(a.p) : 0u;
  const float sc = (add && a.p > 0.f) ? 1.f / (1.f - a.p) : 1.f;
#define PSD_RMSWF(S, ADD, MX)                                                                                      \
  hipLaunchKernelGGL((rms_wide_fwd_kernel<S, ADD, MX>), dim3(blocks), dim3(256), 0, st, a.r, a.h, a.gamma, a.r_new, \
                     a.y, a.rstd, a.rows, a.H, a.eps, a.seed, a.step, th, sc, a.q8, a.sc8)
#define PSD_RMSWF_S(S)                        \
  do {                                        \
    if (add && mx) PSD_RMSWF(S, true, true);  \
    else if (add) PSD_RMSWF(S, true, false);  \
    else if (mx) PSD_RMSWF(S, false, true);   \
    else PSD_RMSWF(S, false, false);          \
  } while (0)
  PSD_WIDE_S(a.H, PSD_RMSWF_S);
#undef PSD_RMSWF_S
#undef PSD_RMSWF
  return hipGetLastError();
}

hipError_t launch_rms_wide_bwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_wide(a.H) || a.rows < 0) return hipErrorInvalidValue;
  if ((a.dq8 == nullptr) != (a.dsc8 == nullptr)) return hipErrorInvalidValue;
  const int blocks = rms_wide_bwd_blocks(a.rows);
  const uint32_t th = keep_thresh(a.p);
  const bool drn = a.dr_new != nullptr, mx = a.dq8 != nullptr;
  const bool dh = a.dh != nullptr;  // null at p == 0: dh is dr, written once
  const float sc = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
#define PSD_RMSWB(S, DRN, DH, MXG)                                                                                 \
  hipLaunchKernelGGL((rms_wide_bwd_kernel<S, DRN, DH, MXG>), dim3(blocks), dim3(256), 0, st, a.dy, a.dr_new, a.rn, \
                     a.rstd_in, a.gamma, a.dr, a.dh, a.part, a.rows, a.H, a.seed, a.step, th, sc, a.dq8, a.dsc8)
#define PSD_RMSWB_M(S, MXG)                        \
  do {                                             \
    if (drn && dh) PSD_RMSWB(S, true, true, MXG);  \
    else if (drn) PSD_RMSWB(S, true, false, MXG);  \
    else if (dh) PSD_RMSWB(S, false, true, MXG);   \
    else PSD_RMSWB(S, false, false, MXG);          \
  } while (0)
#define PSD_RMSWB_S(S)            \
  do {                            \
    if (mx) PSD_RMSWB_M(S, true); \
    else PSD_RMSWB_M(S, false);   \
  } while (0)
  PSD_WIDE_S(a.H, PSD_RMSWB_S);
#undef PSD_RMSWB_S
#undef PSD_RMSWB_M
#undef PSD_RMSWB
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_ln_param_grad(a.part, blocks, a.H, 1, a.dgamma, nullptr, nullptr, st);
}

}  // namespace psd
