// Transposing MX fp8 quantiser: x [R, C] bf16 -> the MX copy of x^T, q [C, R] (e4m3 / e5m2) with one
// E8M0 byte per 32 consecutive R (scales [C, R/32]) -- bitwise quant_mx_kernel (fp8.hip) applied to
// x.t().contiguous(), in one launch and one read of x instead of a bf16 transpose copy plus a
// quantise pass. The bwd-data GEMM of an fp8 Linear takes W^T [in, out] with blocks along `out` from
// the bf16 working weight W [out, in] this way (ops/linear.py).
//
// A workgroup takes a 128-row x 64-column tile: 16-byte global loads (8 columns per lane, 4 per
// thread) written to LDS row-major as loaded. Wave w then owns row block w (rows 32w .. 32w+31) and
// lane l column l: a lane reads its column's 32 values (the 64 lanes of a wave read 32 consecutive
// dwords of one tile row per step, so the un-padded 128-byte row pitch is conflict-free for the
// column reads as well as for the 16-byte row writes), which are one whole MX block -- amax, scale and
// rounding need no cross-lane exchange -- and stores them as two 16-byte payload pieces plus the
// scale byte. No atomics; every output byte is written by exactly one lane from the values of its own
// block, so the result does not depend on the grid.
#include "common.h"
#include "launchers.h"
#include "mx_common.h"

namespace psd {

namespace {
constexpr int kTR = 128;  // tile rows: 4 MX blocks, one per wave
constexpr int kTC = 64;   // tile columns: one per lane
}  // namespace

template <bool E5>
__global__ __launch_bounds__(256) void quant_mx_t_kernel(const uint16_t* __restrict__ x, int64_t R, int64_t C,
                                                         uint8_t* __restrict__ q, uint8_t* __restrict__ sc) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTR * kTC];
  const int64_t gx = (C + kTC - 1) / kTC;  // column tiles; the grid is 1-D (row tiles x column tiles)
  const int64_t by = blockIdx.x / gx, bx = blockIdx.x - by * gx;
  const int64_t r0 = by * kTR, c0 = bx * kTC;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int v = (int)threadIdx.x + 256 * u;  // 16-byte vector of the tile: row v / 8, columns 8 (v % 8) ..
    const int tr = v >> 3, tc = (v & 7) << 3;
    if (r0 + tr < R && c0 + tc < C)  // C % 8 == 0: a vector is inside or outside as a whole
      *reinterpret_cast<u32x4*>(tile + tr * kTC + tc) = *reinterpret_cast<const u32x4*>(x + (r0 + tr) * C + c0 + tc);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t rb = r0 + 32 * wv, c = c0 + lane;
  if (rb >= R || c >= C) return;  // R % 32 == 0: a row block is inside or outside as a whole
  const float fmax = E5 ? 57344.f : 448.f;
  float t[32];
  float m = 0.f;
#pragma unroll
  for (int i = 0; i < 32; ++i) {
    t[i] = bf16_to_f32(tile[(32 * wv + i) * kTC + lane]);
    m = fmaxf(m, fabsf(t[i]));
  }
  const int eb = mx_exp_byte(m, fmax);
  const float inv = __uint_as_float((uint32_t)(254 - eb) << 23);  // 2^(127 - eb), as mx_quant8
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    w[j] = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) w[j] |= (uint32_t)f32_to_f8<E5>(t[4 * j + e] * inv) << (8 * e);
  }
  uint8_t* dst = q + c * R + rb;  // 32-byte aligned: R % 32 == 0 and rb % 32 == 0
  *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
  *reinterpret_cast<u32x4*>(dst + 16) = u32x4{w[4], w[5], w[6], w[7]};
  sc[c * (R >> 5) + (rb >> 5)] = (uint8_t)eb;
}

hipError_t launch_quant_mx_t(const void* x, int64_t R, int64_t C, int e5m2, uint8_t* q, uint8_t* scales,
                             hipStream_t st) {
  if (R <= 0 || C <= 0) return hipSuccess;
  if (R % 32 != 0 || C % 8 != 0) return hipErrorInvalidValue;
  const int64_t gx = (C + kTC - 1) / kTC, gy = (R + kTR - 1) / kTR;
  if (gx * gy > 2147483647) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(gx * gy));
  const uint16_t* xp = static_cast<const uint16_t*>(x);
  if (e5m2) hipLaunchKernelGGL(quant_mx_t_kernel<true>, grid, dim3(256), 0, st, xp, R, C, q, scales);
  else hipLaunchKernelGGL(quant_mx_t_kernel<false>, grid, dim3(256), 0, st, xp, R, C, q, scales);
  return hipGetLastError();
}

}  // namespace psd
