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
//
// MX side outputs (the fp8 Llama block, ops/linear.py fp8="mx"): the forward can also write the MX e4m3 copy
// of y -- the consumer Linear's forward operand -- and the backward the MX e5m2 copy of the tensor it returns
// as dh -- the bwd-data operand of the Linear that produced h. Payload q8 [rows, H] and one E8M0 byte per 32
// columns sc8 [rows, H/32], quantised from the bf16-rounded values the same launch stores: bitwise
// quant_mx_kernel (fp8.hip) of that tensor, from registers, so the stand-alone pass's read of [rows, H] bf16
// is saved. The bf16 outputs keep the bits of the variants without it (same arithmetic, stores added after).
#include "common.h"
#include "launchers_ln.h"
#include "launchers_rmsnorm.h"
#include "mx_common.h"
#include "row_common.h"

namespace psd {

namespace {
// The MX copy of one row held as v (fp32, about to be / just stored as bf16), on layernorm.hip's lane-group
// block map (duplicated here, not shared: ln_fwd_kernel keeps its instructions). A lane's E columns are E/4
// chunks of 4 that each lie in one 32-column block; GL lanes cover NB whole blocks (E = 12: 8 lanes, 3
// blocks; E = 16: 2 lanes, 1 block), so a block's amax is log2(GL) xor-exchanges of NB per-lane partial
// maxima. One 4-byte payload store per chunk; the lane holding a block's first chunk writes its scale
// byte. qrow = q8 + r * H + c0 (4-byte aligned: E % 4 == 0), srow = sc8 + r * (H / 32). All 64 lanes call
// it together (the row loop is wave-uniform). v is left bf16-rounded.
template <int E, bool E5>
__device__ __forceinline__ void mx_row_store(float (&v)[E], int lane, uint8_t* __restrict__ qrow,
                                             uint8_t* __restrict__ srow) {
  static_assert(E == 12 || E == 16, "MX block map written for H = 768 / 1024");
  constexpr int NC = E / 4, GL = (E == 12) ? 8 : 2, NB = (E == 12) ? 3 : 1;
  constexpr float fmax = E5 ? 57344.f : 448.f;
  const int c0 = lane * E;
  const int g0 = (lane & (GL - 1)) * E;  // first column of this lane inside its lane group's NB blocks
  float bm[NB];
#pragma unroll
  for (int k = 0; k < NB; ++k) bm[k] = 0.f;
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    float cm = 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[4 * j + e] = bf16_to_f32(f32_to_bf16(v[4 * j + e]));  // as stored
      cm = fmaxf(cm, fabsf(v[4 * j + e]));
    }
    const int kb = (g0 + 4 * j) >> 5;
#pragma unroll
    for (int k = 0; k < NB; ++k) bm[k] = (kb == k) ? fmaxf(bm[k], cm) : bm[k];
  }
#pragma unroll
  for (int o = 1; o < GL; o <<= 1)
#pragma unroll
    for (int k = 0; k < NB; ++k) bm[k] = fmaxf(bm[k], __shfl_xor(bm[k], o));
#pragma unroll
  for (int j = 0; j < NC; ++j) {
    const int kb = (g0 + 4 * j) >> 5;
    float am = bm[0];
#pragma unroll
    for (int k = 1; k < NB; ++k) am = (kb == k) ? bm[k] : am;
    const int eb = mx_exp_byte(am, fmax);
    const float inv = __uint_as_float((uint32_t)(254 - eb) << 23);  // 2^(127 - eb), as mx_quant8
    uint32_t w = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w |= (uint32_t)f32_to_f8<E5>(v[4 * j + e] * inv) << (8 * e);
    *reinterpret_cast<uint32_t*>(qrow + 4 * j) = w;
    if (((c0 + 4 * j) & 31) == 0) srow[(c0 + 4 * j) >> 5] = (uint8_t)eb;
  }
}
}  // namespace

// ADD: with the branch h (r_new is written); without it r_new is r and only y / rstd are written.
// MX: also the MX e4m3 copy of y (q8, sc8)
template <int E, bool ADD, bool MX>
__global__ __launch_bounds__(256) void rms_fwd_kernel(const uint16_t* __restrict__ r_in, const uint16_t* __restrict__ h,
                                                      const uint16_t* __restrict__ gamma, uint16_t* __restrict__ r_new,
                                                      uint16_t* __restrict__ y, float* __restrict__ rstd_out,
                                                      int64_t rows, float eps, uint32_t seed,
                                                      const int64_t* __restrict__ step, uint32_t thresh, float scale,
                                                      uint8_t* __restrict__ q8, uint8_t* __restrict__ sc8) {
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
    if constexpr (MX) mx_row_store<E, false>(xv, lane, q8 + off, sc8 + r * (H / 32));
    if (lane == 0) rstd_out[r] = rstd;
  }
}

// DRN: the gradient dr_new arriving at the residual stream is added (else it counts as zero and is not
// read). DH: the pre-dropout gradient dh is written too (p > 0 with a branch; at p == 0 dh is dr itself).
// MXG: also the MX e5m2 copy (q8, sc8) of the tensor returned as dh: dh with DH, else dr
template <int E, bool DRN, bool DH, bool MXG>
__global__ __launch_bounds__(256) void rms_bwd_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ drn,
                                                      const uint16_t* __restrict__ rnew,
                                                      const float* __restrict__ rstd_in,
                                                      const uint16_t* __restrict__ gamma, uint16_t* __restrict__ dr,
                                                      uint16_t* __restrict__ dh, float* __restrict__ part, int64_t rows,
                                                      uint32_t seed, const int64_t* __restrict__ step, uint32_t thresh,
                                                      float scale, uint8_t* __restrict__ q8,
                                                      uint8_t* __restrict__ sc8) {
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
    if constexpr (MXG) mx_row_store<E, true>(dv, lane, q8 + off, sc8 + r * (H / 32));
  }
  // block partials of dgamma: [blk][H], waves summed in a fixed order
  __shared__ float red[4][H];
#pragma unroll
  for (int i = 0; i < E; ++i) red[wv][c0 + i] = pg[i];
  __syncthreads();
  for (int c = threadIdx.x; c < H; c += blockDim.x)
    part[(int64_t)blockIdx.x * H + c] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
}

bool rms_supported(int H) { return H == 768 || H == 1024 || rms_wide(H); }

// one row per wave, four waves per workgroup, <= 2048 workgroups: past 8192 rows the waves take further rows
// (the wide sizes: rmsnorm_wide.hip's own grids)
int rms_fwd_blocks(int64_t rows, int H) {
  if (rms_wide(H)) return rms_wide_fwd_blocks(rows);
  const int64_t want = (rows + 3) / 4;
  return (int)(want < 1 ? 1 : (want > 2048 ? 2048 : want));
}

// >= 8 rows per wave, <= 512 workgroups (two per CU): at most 512 dgamma partial rows for the finalize
int rms_bwd_blocks(int64_t rows, int H) {
  if (rms_wide(H)) return rms_wide_bwd_blocks(rows);
  const int64_t want = (rows + 4 * 8 - 1) / (4 * 8);
  return (int)(want < 1 ? 1 : (want > 512 ? 512 : want));
}

hipError_t launch_rms_fwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  if (rms_wide(a.H)) return launch_rms_wide_fwd(a, st);
  const int blocks = rms_fwd_blocks(a.rows, a.H);
  const bool add = a.h != nullptr;
  const uint32_t th = add ? keep_thresh(a.p) : 0u;
  const float sc = (add && a.p > 0.f) ? 1.f / (1.f - a.p) : 1.f;
  if ((a.q8 == nullptr) != (a.sc8 == nullptr)) return hipErrorInvalidValue;
  const bool mx = a.q8 != nullptr;
#define PSD_RMSF(E, ADD, MX)                                                                                        \
  hipLaunchKernelGGL((rms_fwd_kernel<E, ADD, MX>), dim3(blocks), dim3(256), 0, st, a.r, a.h, a.gamma, a.r_new, a.y, \
                     a.rstd, a.rows, a.eps, a.seed, a.step, th, sc, a.q8, a.sc8)
#define PSD_RMSF_E(E)                         \
  do {                                        \
    if (add && mx) PSD_RMSF(E, true, true);   \
    else if (add) PSD_RMSF(E, true, false);   \
    else if (mx) PSD_RMSF(E, false, true);    \
    else PSD_RMSF(E, false, false);           \
  } while (0)
  if (a.H == 768) PSD_RMSF_E(12);
  else PSD_RMSF_E(16);
#undef PSD_RMSF_E
#undef PSD_RMSF
  return hipGetLastError();
}

hipError_t launch_rms_bwd(const RmsArgs& a, hipStream_t st) {
  if (!rms_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  if (rms_wide(a.H)) return launch_rms_wide_bwd(a, st);
  const int blocks = rms_bwd_blocks(a.rows, a.H);
  const uint32_t th = keep_thresh(a.p);
  const bool drn = a.dr_new != nullptr;
  const bool dh = a.dh != nullptr;  // null at p == 0: dh is dr, written once
  const float sc = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  if ((a.dq8 == nullptr) != (a.dsc8 == nullptr)) return hipErrorInvalidValue;
  const bool mx = a.dq8 != nullptr;
#define PSD_RMSB(E, DRN, DH, MXG)                                                                                \
  hipLaunchKernelGGL((rms_bwd_kernel<E, DRN, DH, MXG>), dim3(blocks), dim3(256), 0, st, a.dy, a.dr_new, a.rn,    \
                     a.rstd_in, a.gamma, a.dr, a.dh, a.part, a.rows, a.seed, a.step, th, sc, a.dq8, a.dsc8)
#define PSD_RMSB_M(E, MXG)                        \
  do {                                            \
    if (drn && dh) PSD_RMSB(E, true, true, MXG);  \
    else if (drn) PSD_RMSB(E, true, false, MXG);  \
    else if (dh) PSD_RMSB(E, false, true, MXG);   \
    else PSD_RMSB(E, false, false, MXG);          \
  } while (0)
#define PSD_RMSB_E(E)            \
  do {                           \
    if (mx) PSD_RMSB_M(E, true); \
    else PSD_RMSB_M(E, false);   \
  } while (0)
  if (a.H == 768) PSD_RMSB_E(12);
  else PSD_RMSB_E(16);
#undef PSD_RMSB_E
#undef PSD_RMSB_M
#undef PSD_RMSB
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_ln_param_grad(a.part, blocks, a.H, 1, a.dgamma, nullptr, nullptr, st);
}

}  // namespace psd
