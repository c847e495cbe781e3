// The post-norm residual tail of layernorm.hip -- s = x + dropout(h), y = LayerNorm(s) * gamma + beta, and its
// backward -- for the wide hidden sizes H = 256 n, n = 5 .. 32 (1280 .. 8192). Same LnArgs, same outputs, same
// arithmetic contract as layernorm.hip (its header and launchers_ln.h spell them out); another row layout, because
// one wave per row with the row in fp32 registers stops fitting past H = 1024.
//
// Work split (row_wide.h, as rmsnorm_wide.hip): one 256-lane workgroup per row per round, grid-stride over rows
// (64-bit offsets). A row is H / 8 = 32 n chunks of 8 consecutive columns (16 bytes of bf16); lane t owns chunks
// j = t + 256 s, s < S = ceil(H / 2048) (template, 1 .. 4). A chunk exists when j < 32 n: a partly filled last slab
// idles whole half-waves (H = 1280: wave 2's upper half and wave 3), and a 32-column MX block, four chunks, is one
// aligned lane quad that is wholly in or out.
//
// Registers: the forward holds the current row in fp32, 8 S <= 32 values per lane. The next row's 16-byte loads
// are issued before this row's reductions and stay packed as loaded (4 VGPRs per slab per tensor) until they become
// current; gamma and beta stay packed too. The backward, whose registers go to the 16 S or 24 S partial sums, keeps
// the current dy and s packed across its barrier and unpacks them a second time after it.
//
// Forward statistics, as layernorm.hip: s = bf16(x + h keep / (1 - p)) first, mean and rstd in fp32 from that
// rounded s, the variance about the mean from the registers (two passes over registers, never E[s^2] - mean^2).
// Each of the two sums: per-lane chain, wave butterfly, the four wave sums through LDS added by every lane in one
// fixed order. The mean uses LDS slot 0 and the variance slot 1: a wave that writes slot 0 for row k + 1 has passed
// row k's second barrier, which every reader of row k's slot 0 reached after reading, and likewise for slot 1 and
// the first barrier of row k + 1. Two barriers per row. Idle lanes add 0 and take the barriers.
//
// Backward: a = mean(g), b = mean(g xh) with g = dy gamma, xh = (s - mean) rstd go through one barrier together
// (two slots alternating by round, as rmsnorm_wide.hip); dx = rstd (g - a - xh b), dh = dx keep / (1 - p) from the
// fp32 dx. A column belongs to one lane of the workgroup, so its dgamma / dbeta (/ dhsum: the dh column sums)
// partials over the rows the workgroup visits accumulate in that lane's registers and go straight to
// part[blk][2 or 3][H] -- no LDS, no cross-wave add -- and layernorm.hip's fixed-order finalize sums the block
// partials. They are functions of rows and ln_wide_bwd_blocks(rows, H) only.
//
// Grid: forward min(rows, LN_WIDE_FWD_CAP) workgroups, the narrow kernels' cap. Backward min(ceil(rows /
// LN_WIDE_BWD_ROWS), cap): at least 16 rows per workgroup, so the three fp32 partial rows are at most 3 / 8 of one
// activation tensor's bytes; the cap is LN_WIDE_BWD_CAP = 1024 up to H = 4096 and half that above, where the
// S = 3, 4 register counts (195 - 226, and past 256 at S = 4) leave two workgroups or one resident per CU.
//
// Measured (profiles/layernorm_wide.md, 16,384 rows, H = 1280 / 2048 / 4096 / 8192): 5.3 - 6.2 TB/s forward, 3.7 -
// 5.3 TB/s backward with the finalize; the MX side output takes 0.85 - 0.87 of plain + quant_mx_kernel at all four.
//
// MX side output: mx_quant8 (mx_common.h) on the aligned lane quad, one 8-byte payload store per chunk, the quad's
// first lane writes the scale byte; quantised from the bf16-rounded y the same launch stores. The file is built
// without packed fp32 instructions and without contraction (every intended FMA is an fmaf), so both variants of
// the forward run one arithmetic and y keeps its bits. No atomics; every output but the parameter gradients is a
// function of its own row; the step is read on the device; nothing is read on the host.
#include "common.h"
#include "launchers_ln.h"

#pragma clang fp contract(off)

#include "row_wide.h"

namespace psd {

namespace {
// two row sums over the workgroup through one barrier: the same bits on every lane. red: this round's [2][4]
__device__ __forceinline__ void row_sum2(float& a, float& b, float (*red)[4], int lane, int wv) {
  a = wave_sum(a);
  b = wave_sum(b);
  if (lane == 0) {
    red[0][wv] = a;
    red[1][wv] = b;
  }
  __syncthreads();
  a = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  b = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
}
}  // namespace

// MX as ln_fwd_kernel
template <int S, bool MX>
__global__ __launch_bounds__(256) void ln_wide_fwd_kernel(const uint16_t* __restrict__ x, const uint16_t* __restrict__ h,
                                                          const uint16_t* __restrict__ gamma,
                                                          const uint16_t* __restrict__ beta, uint16_t* __restrict__ y,
                                                          uint16_t* __restrict__ s_out, float* __restrict__ mean_out,
                                                          float* __restrict__ rstd_out, int64_t rows, int H, float eps,
                                                          uint32_t seed, const int64_t* __restrict__ step,
                                                          uint32_t thresh, float scale, uint8_t* __restrict__ q8,
                                                          uint8_t* __restrict__ sc8) {
  __shared__ float red[2][4];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = H >> 3;
  const float inv_h = 1.f / (float)H;
  u32x4 gp[S], bp[S], nx[S], nh[S];
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (has_chunk<S>(s, t, nch)) {
      gp[s] = ld16(gamma + 8 * (t + 256 * s));
      bp[s] = ld16(beta + 8 * (t + 256 * s));
    }
  const uint32_t key = dropout_key(seed, step);
  int64_t r = blockIdx.x;
  if (r < rows) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        nx[s] = ld16(x + r * H + 8 * (t + 256 * s));
        nh[s] = ld16(h + r * H + 8 * (t + 256 * s));
      }
  }
  for (; r < rows; r += gridDim.x) {
    float xv[S][8];
    float sum = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
        float hv[8];
        bool kp[8];
        unpack8(nx[s], xv[s]);
        unpack8(nh[s], hv);
        if (thresh != 0u) keep_flags<8>(key, off, thresh, kp);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = (thresh == 0u || kp[i]) ? hv[i] * scale : 0.f;
          xv[s][i] = bf16_to_f32(f32_to_bf16(xv[s][i] + d));  // s, rounded as stored (the LN input)
          sum += xv[s][i];
        }
        store8_bf16(s_out + off, xv[s]);
      }
    const int64_t rn = r + gridDim.x;  // the next row's loads, in flight over both reductions
    if (rn < rows) {
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (has_chunk<S>(s, t, nch)) {
          nx[s] = ld16(x + rn * H + 8 * (t + 256 * s));
          nh[s] = ld16(h + rn * H + 8 * (t + 256 * s));
        }
    }
    const float mean = row_sum(sum, red, 0, lane, wv) * inv_h;
    float sq = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          const float d = xv[s][i] - mean;
          sq = fmaf(d, d, sq);
        }
      }
    const float rstd = rsqrtf(row_sum(sq, red, 1, lane, wv) * inv_h + eps);
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
        float g[8], b[8];
        unpack8(gp[s], g);
        unpack8(bp[s], b);
#pragma unroll
        for (int i = 0; i < 8; ++i) xv[s][i] = fmaf((xv[s][i] - mean) * rstd, g[i], b[i]);
        store8_bf16(y + off, xv[s]);
        if constexpr (MX) mx_chunk_store<false>(xv[s], q8, sc8, off);
      }
    if (t == 0) {
      mean_out[r] = mean;
      rstd_out[r] = rstd;
    }
  }
}

// HS as ln_bwd_kernel: also the column sums of dh, a third partial row per block
template <int S, bool HS>
__global__ __launch_bounds__(256) void ln_wide_bwd_kernel(const uint16_t* __restrict__ dy, const uint16_t* __restrict__ sn,
                                                          const float* __restrict__ mean_in,
                                                          const float* __restrict__ rstd_in,
                                                          const uint16_t* __restrict__ gamma, uint16_t* __restrict__ dx,
                                                          uint16_t* __restrict__ dh, float* __restrict__ part,
                                                          int64_t rows, int H, uint32_t seed,
                                                          const int64_t* __restrict__ step, uint32_t thresh,
                                                          float scale) {
  __shared__ float red[2][2][4];
  constexpr int NP = HS ? 3 : 2;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int nch = H >> 3;
  const float inv_h = 1.f / (float)H;
  u32x4 gp[S], nd[S], nx[S];
  float pg[S][8], pb[S][8], ph[HS ? S : 1][8];
#pragma unroll
  for (int s = 0; s < S; ++s) {
    if (has_chunk<S>(s, t, nch)) gp[s] = ld16(gamma + 8 * (t + 256 * s));
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      pg[s][i] = pb[s][i] = 0.f;
      if constexpr (HS) ph[s][i] = 0.f;
    }
  }
  const uint32_t key = dropout_key(seed, step);
  int64_t r = blockIdx.x;
  float nmean = 0.f, nrstd = 0.f;
  if (r < rows) {
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        nd[s] = ld16(dy + r * H + 8 * (t + 256 * s));
        nx[s] = ld16(sn + r * H + 8 * (t + 256 * s));
      }
    nmean = mean_in[r];
    nrstd = rstd_in[r];
  }
  for (int slot = 0; r < rows; r += gridDim.x, slot ^= 1) {
    const float mean = nmean, rstd = nrstd;
    u32x4 cd[S], cx[S];  // this row, packed: unpacked again after the barrier (the same operations, the same bits)
    float a = 0.f, b = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        float dv[8], xh[8], g[8];
        cd[s] = nd[s];
        cx[s] = nx[s];
        unpack8(cd[s], dv);
        unpack8(cx[s], xh);
        unpack8(gp[s], g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xh[i] = (xh[i] - mean) * rstd;
          pg[s][i] = fmaf(dv[i], xh[i], pg[s][i]);
          pb[s][i] += dv[i];
          dv[i] *= g[i];  // dxhat
          a += dv[i];
          b = fmaf(dv[i], xh[i], b);
        }
      }
    const int64_t rn = r + gridDim.x;  // the next row's loads, in flight over the reduction
    if (rn < rows) {
#pragma unroll
      for (int s = 0; s < S; ++s)
        if (has_chunk<S>(s, t, nch)) {
          nd[s] = ld16(dy + rn * H + 8 * (t + 256 * s));
          nx[s] = ld16(sn + rn * H + 8 * (t + 256 * s));
        }
      nmean = mean_in[rn];
      nrstd = rstd_in[rn];
    }
    row_sum2(a, b, red[slot], lane, wv);
    a *= inv_h;
    b *= inv_h;
#pragma unroll
    for (int s = 0; s < S; ++s)
      if (has_chunk<S>(s, t, nch)) {
        const int64_t off = r * H + 8 * (t + 256 * s);
        float dv[8], xh[8], g[8];
        bool kp[8];
        unpack8(cd[s], dv);
        unpack8(cx[s], xh);
        unpack8(gp[s], g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          xh[i] = (xh[i] - mean) * rstd;
          dv[i] = rstd * (dv[i] * g[i] - a - xh[i] * b);  // d s
        }
        store8_bf16(dx + off, dv);
        if (thresh != 0u) keep_flags<8>(key, off, thresh, kp);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
          dv[i] = (thresh == 0u || kp[i]) ? dv[i] * scale : 0.f;  // from the fp32 dx
          if constexpr (HS) ph[s][i] += dv[i];
        }
        store8_bf16(dh + off, dv);
      }
  }
  // this workgroup's partial rows [blk][NP][H]: each column from the one lane that owns it
  float* prow = part + (int64_t)blockIdx.x * NP * H;
#pragma unroll
  for (int s = 0; s < S; ++s)
    if (has_chunk<S>(s, t, nch)) {
      const int c = 8 * (t + 256 * s);
      store8_f32(prow + c, pg[s]);
      store8_f32(prow + H + c, pb[s]);
      if constexpr (HS) store8_f32(prow + 2 * H + c, ph[s]);
    }
}

bool ln_wide_supported(int H) { return H >= 1280 && H <= 8192 && H % 256 == 0; }

int ln_wide_fwd_blocks(int64_t rows) {
  return (int)(rows < 1 ? 1 : (rows > LN_WIDE_FWD_CAP ? LN_WIDE_FWD_CAP : rows));
}

int ln_wide_bwd_blocks(int64_t rows, int H) {
  const int64_t want = (rows + LN_WIDE_BWD_ROWS - 1) / LN_WIDE_BWD_ROWS;
  const int cap = H <= 4096 ? LN_WIDE_BWD_CAP : LN_WIDE_BWD_CAP / 2;
  return (int)(want < 1 ? 1 : (want > cap ? cap : want));
}

hipError_t launch_ln_wide_fwd(const LnArgs& a, hipStream_t st) {
  if (!ln_wide_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  if ((a.q8 == nullptr) != (a.sc8 == nullptr)) return hipErrorInvalidValue;
  const int blocks = ln_wide_fwd_blocks(a.rows);
  const uint32_t th = keep_thresh(a.p);
  const float sc = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
#define PSD_LNWF(S, MX)                                                                                            \
  hipLaunchKernelGGL((ln_wide_fwd_kernel<S, MX>), dim3(blocks), dim3(256), 0, st, a.x, a.h, a.gamma, a.beta, a.y, \
                     a.s, a.mean, a.rstd, a.rows, a.H, a.eps, a.seed, a.step, th, sc, a.q8, a.sc8)
#define PSD_LNWF_S(S)                          \
  do {                                         \
    if (a.q8 != nullptr) PSD_LNWF(S, true);    \
    else PSD_LNWF(S, false);                   \
  } while (0)
  PSD_WIDE_S(a.H, PSD_LNWF_S);
#undef PSD_LNWF_S
#undef PSD_LNWF
  return hipGetLastError();
}

hipError_t launch_ln_wide_bwd(const LnArgs& a, hipStream_t st) {
  if (!ln_wide_supported(a.H) || a.rows < 0) return hipErrorInvalidValue;
  const int blocks = ln_wide_bwd_blocks(a.rows, a.H);
  const uint32_t th = keep_thresh(a.p);
  const float sc = a.p > 0.f ? 1.f / (1.f - a.p) : 1.f;
  const bool hs = a.dhsum != nullptr;
#define PSD_LNWB(S, HS)                                                                                            \
  hipLaunchKernelGGL((ln_wide_bwd_kernel<S, HS>), dim3(blocks), dim3(256), 0, st, a.dy, a.s, a.mean, a.rstd, a.gamma, \
                     a.dx, a.dh, a.part, a.rows, a.H, a.seed, a.step, th, sc)
#define PSD_LNWB_S(S)             \
  do {                            \
    if (hs) PSD_LNWB(S, true);    \
    else PSD_LNWB(S, false);      \
  } while (0)
  PSD_WIDE_S(a.H, PSD_LNWB_S);
#undef PSD_LNWB_S
#undef PSD_LNWB
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_ln_param_grad(a.part, blocks, a.H, hs ? 3 : 2, a.dgamma, a.dbeta, a.dhsum, st);
}

}  // namespace psd
