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

// Dual MX quantiser: one read of x [R, C] bf16 -> BOTH MX copies a fp8 Linear's backward takes of dy':
//   q_row [R, C], s_row [R * C / 32]   blocks of 32 along C: bitwise quant_mx_kernel (fp8.hip) of x
//   q_t   [C, R], s_t   [C, R / 32]    blocks of 32 along R: bitwise quant_mx_t_kernel above
// each in its own fp8 format (bwd-data takes the row copy in e5m2, the weight gradient the transposed
// copy in e4m3). The same 128 x 64 LDS tile: the transposed half is quant_mx_t_kernel's column read; the
// row half takes the tile's 128 x 2 = 256 row blocks, one per thread (thread t: tile row t / 2, columns
// 32 (t % 2) ..), as four 16-byte LDS reads. Un-swizzled, lane t's piece j sits in 16-byte slot
// (4 t + j) % 16 of the 256-byte bank row, so the 16 lanes ds_read_b128 serves per cycle would share 4
// slots (4-way conflict); lane t therefore reads its pieces in the rotated order j = (i + t / 4) % 4 --
// within each of the instruction's lane groups t / 4 takes four values distinct mod 4, so the 16 lanes
// cover all 16 slots -- and the LDS layout stays the un-padded one the 16-byte writes and the column
// reads are conflict-free on. A piece is 8 payload bytes: each goes out as one 8-byte store at its own
// place (no register shuffle to undo the rotation). No atomics; every output byte is written by exactly
// one lane from the values of its own block.
template <bool E5R, bool E5T>
__global__ __launch_bounds__(256) void quant_mx_dual_kernel(const uint16_t* __restrict__ x, int64_t R, int64_t C,
                                                            uint8_t* __restrict__ qr, uint8_t* __restrict__ sr,
                                                            uint8_t* __restrict__ qt, uint8_t* __restrict__ stc) {
  __shared__ __attribute__((aligned(16))) uint16_t tile[kTR * kTC];
  const int64_t gx = (C + kTC - 1) / kTC;
  const int64_t by = blockIdx.x / gx, bx = blockIdx.x - by * gx;
  const int64_t r0 = by * kTR, c0 = bx * kTC;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int v = (int)threadIdx.x + 256 * u;
    const int tr = v >> 3, tc = (v & 7) << 3;
    if (r0 + tr < R && c0 + tc < C)
      *reinterpret_cast<u32x4*>(tile + tr * kTC + tc) = *reinterpret_cast<const u32x4*>(x + (r0 + tr) * C + c0 + tc);
  }
  __syncthreads();
  {  // transposed half: quant_mx_t_kernel
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t rb = r0 + 32 * wv, c = c0 + lane;
    if (rb < R && c < C) {  // R % 32 == 0: a row block is inside or outside as a whole
      const float fmax = E5T ? 57344.f : 448.f;
      float t[32];
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        t[i] = bf16_to_f32(tile[(32 * wv + i) * kTC + lane]);
        m = fmaxf(m, fabsf(t[i]));
      }
      const int eb = mx_exp_byte(m, fmax);
      const float inv = __uint_as_float((uint32_t)(254 - eb) << 23);
      uint32_t w[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w[j] = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[j] |= (uint32_t)f32_to_f8<E5T>(t[4 * j + e] * inv) << (8 * e);
      }
      uint8_t* dst = qt + c * R + rb;
      *reinterpret_cast<u32x4*>(dst) = u32x4{w[0], w[1], w[2], w[3]};
      *reinterpret_cast<u32x4*>(dst + 16) = u32x4{w[4], w[5], w[6], w[7]};
      stc[c * (R >> 5) + (rb >> 5)] = (uint8_t)eb;
    }
  }
  {  // row half: quant_mx_kernel's blocks, from the same tile
    const int tr = (int)threadIdx.x >> 1, cb = ((int)threadIdx.x & 1) << 5;
    const int64_t r = r0 + tr, c = c0 + cb;
    if (r < R && c < C) {  // C % 32 == 0: a column block is inside or outside as a whole
      const float fmax = E5R ? 57344.f : 448.f;
      const int rot = ((int)threadIdx.x >> 2) & 3;
      float t[4][8];
      float m = 0.f;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = (i + rot) & 3;
        const u32x4 p = *reinterpret_cast<const u32x4*>(tile + tr * kTC + cb + 8 * j);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[i][2 * e] = __uint_as_float(p[e] << 16);
          t[i][2 * e + 1] = __uint_as_float(p[e] & 0xffff0000u);
          m = fmaxf(m, fmaxf(fabsf(t[i][2 * e]), fabsf(t[i][2 * e + 1])));
        }
      }
      const int eb = mx_exp_byte(m, fmax);
      const float inv = __uint_as_float((uint32_t)(254 - eb) << 23);
      uint8_t* dst = qr + r * C + c;  // 32-byte aligned: C % 32 == 0
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int j = (i + rot) & 3;
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          lo |= (uint32_t)f32_to_f8<E5R>(t[i][e] * inv) << (8 * e);
          hi |= (uint32_t)f32_to_f8<E5R>(t[i][e + 4] * inv) << (8 * e);
        }
        *reinterpret_cast<uint2*>(dst + 8 * j) = make_uint2(lo, hi);
      }
      sr[(r * C + c) >> 5] = (uint8_t)eb;
    }
  }
}

hipError_t launch_quant_mx_dual(const void* x, int64_t R, int64_t C, int e5m2_row, int e5m2_t, uint8_t* q_row,
                                uint8_t* s_row, uint8_t* q_t, uint8_t* s_t, hipStream_t st) {
  if (R <= 0 || C <= 0) return hipSuccess;
  if (R % 32 != 0 || C % 32 != 0) return hipErrorInvalidValue;
  const int64_t gx = (C + kTC - 1) / kTC, gy = (R + kTR - 1) / kTR;
  if (gx * gy > 2147483647) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(gx * gy));
  const uint16_t* xp = static_cast<const uint16_t*>(x);
#define PSD_QDUAL(ER, ET) \
  hipLaunchKernelGGL((quant_mx_dual_kernel<ER, ET>), grid, dim3(256), 0, st, xp, R, C, q_row, s_row, q_t, s_t)
  if (e5m2_row) {
    if (e5m2_t) PSD_QDUAL(true, true);
    else PSD_QDUAL(true, false);
  } else {
    if (e5m2_t) PSD_QDUAL(false, true);
    else PSD_QDUAL(false, false);
  }
#undef PSD_QDUAL
  return hipGetLastError();
}

}  // namespace psd
