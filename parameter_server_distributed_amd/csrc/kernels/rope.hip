// Rotary position embedding (RoPE) on the packed QKV tensor for gfx950: one in-place pass over the Q and K
// thirds of qkv [B, S, 3, H, 64] bf16, between the QKV Linear and the attention kernels.
//
// Convention: rotate-half (GPT-NeoX / Llama), pairs (i, i + 32), i = 0 .. 31, of each Q head and each K
// head. With c = cos[pos, i], s = sin[pos, i] (fp32 tables, no trigonometry here):
//     y1 = bf16(x1 * c - x2 * s),  y2 = bf16(x2 * c + x1 * s)
// one fma and one product each in fp32, one rounding to bf16 (nearest even). inverse: -s, the backward.
// Position of row (b, t): t - clamp(doc[b, t], 0, t) (t without doc): the clamp of the attention kernels,
// so no doc value can index outside the tables. A row at position 0 (the first token of every document)
// is the rotation by angle 0: it is skipped, neither read nor written, so it keeps its bits whatever it
// holds. Rows t >= clamp(lens[b], 0, S) and their doc entries are neither read nor written either, and
// the V third never is.
//
// Work item: 8 consecutive elements i0 .. i0 + 7 of a head's first half with the matching 8 of its second
// half: two 16-byte loads and stores of bf16 and two 16-byte loads each of cos and sin per lane. Four
// lanes cover a head, 8 H lanes a row's Q and K (they are contiguous: heads 0 .. 2H - 1 of the row). The
// items are numbered row-major and walked by a grid-stride loop of 256-lane workgroups (<= 2048); a lane
// keeps (b, t, item in row) and advances them by the stride's precomputed (rows, items) split, so the loop
// has no division and nothing is sized by S; row and element offsets are 64-bit.
//
// Regime: pure streaming, 2/3 of qkv read and written once. Plain loads and stores: the attention reads
// qkv next, and the tables (<= 1 MB at P = 4096) stay in L2. No LDS, no atomics, nothing summed: each
// output element is a function of its own pair and table entries, so results are bitwise independent of
// the grid and two runs are equal.
#include "common.h"
#include "launchers_rope.h"

namespace psd {

// srow / srem: the grid stride (gridDim * 256 items) as whole rows and left-over items; db / dt: srow as
// whole sequences and left-over rows
__global__ __launch_bounds__(256) void rope_kernel(RopeArgs a, uint32_t srem, int64_t db, int64_t dt) {
  const uint32_t L = 8u * (uint32_t)a.H;  // items per row
  const int64_t S = a.S, B = a.B;
  const uint32_t idx0 = blockIdx.x * 256u + threadIdx.x;  // < 2048 * 256
  const uint32_t row0 = idx0 / L;
  uint32_t rem = idx0 - row0 * L;
  int64_t b = row0 / (uint32_t)a.S;
  int64_t t = row0 - (uint32_t)b * (uint32_t)a.S;
  const float sgn = a.inverse ? -1.f : 1.f;
  const int64_t row_elems = 192 * (int64_t)a.H;
  while (b < B) {
    int64_t len = S;
    if (a.lens) {
      const int64_t l = a.lens[b];
      len = l < 0 ? 0 : (l > S ? S : l);
    }
    if (t < len) {
      const int64_t row = b * S + t;
      int64_t pos = t;
      if (a.doc) {
        int64_t d = a.doc[row];
        d = d < 0 ? 0 : (d > t ? t : d);
        pos = t - d;
      }
      if (pos != 0) {
        const uint32_t i0 = (rem & 3u) * 8u;
        uint16_t* p = a.qkv + row * row_elems + (int64_t)(rem >> 2) * 64 + i0;
        float x1[8], x2[8], c[8], s[8], y1[8], y2[8];
        load8_bf16(p, x1);
        load8_bf16(p + 32, x2);
        load8_f32(a.cos + pos * 32 + i0, c);
        load8_f32(a.sin + pos * 32 + i0, s);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float se = s[e] * sgn;
          y1[e] = fmaf(x1[e], c[e], -(x2[e] * se));
          y2[e] = fmaf(x2[e], c[e], x1[e] * se);
        }
        store8_bf16(p, y1);
        store8_bf16(p + 32, y2);
      }
    }
    rem += srem;
    int64_t carry = 0;
    if (rem >= L) {
      rem -= L;
      carry = 1;
    }
    t += dt + carry;  // < 2 S
    if (t >= S) {
      t -= S;
      ++b;
    }
    b += db;
  }
}

hipError_t launch_rope(const RopeArgs& a, hipStream_t st) {
  if (a.B < 0 || a.S < 0 || a.H <= 0 || a.blocks < 0 || a.H > (1 << 20)) return hipErrorInvalidValue;
  if (a.B == 0 || a.S == 0) return hipSuccess;
  if (!a.qkv || !a.cos || !a.sin) return hipErrorInvalidValue;
  const int64_t L = 8 * (int64_t)a.H;
  const int64_t items = (int64_t)a.B * a.S * L;
  int64_t grid = stream_grid(items, 256);
  if (a.blocks > 0 && grid > a.blocks) grid = a.blocks;
  const int64_t stride = grid * 256;
  const int64_t srow = stride / L;
  hipLaunchKernelGGL(rope_kernel, dim3((unsigned)grid), dim3(256), 0, st, a, (uint32_t)(stride % L), srow / a.S,
                     srow % a.S);
  return hipGetLastError();
}

}  // namespace psd
