// Fused LM head + softmax cross-entropy for gfx950: the loss of a decoder LM from (hidden states, head
// weight, labels) without the [tokens, vocabulary] logits ever reaching memory.
//
//   Z[M,V] = X[M,K] . W[V,K]^T (+ bias)      bf16 in, fp32 accumulate (v_mfma_f32_32x32x16_bf16)
//
// Why: GPTForLM ended in head(x) -> [B*S, 40512] bf16 logits, which ops/loss.cross_entropy kept for
// its backward, and that backward wrote a second tensor of the same size: 2 x 2.65 GB at 8 x 4096
// tokens, the largest tensors of the step, and the logits were rounded to bf16 before the softmax
// saw them. One main loop, two epilogues (template MODE):
//
// MODE 0, forward statistics. A workgroup owns 128 rows and a contiguous slice of the vocabulary and
// walks the slice in 128-column tiles. After a tile's K loop the fp32 accumulators feed a per-lane
// online (max, sum of exp) of each of the lane's 16 rows -- the lane's own 4 columns of the tile, no
// cross-lane traffic during the walk -- and the label's logit is picked out when its column lies in
// the tile (a wave-uniform test of the 32 labels against the tile's range; the rare hit writes one
// LDS word). At the end of the slice the 32 lanes that share a row are merged with DPP (quad
// permutes, row_half_mirror, row_mirror) and the half-row swap, and three floats per (slice, row)
// go out: max, sum, label logit (0 when the label is elsewhere). lmhead_xent_finalize_kernel merges
// the slices in index order: lse = max + log(sum), loss_row = log(sum) + (max - z_label), formed
// from the fp32 parts so the subtraction does not cancel. No atomics: bitwise reproducible for a
// fixed slice count, and the slice count only reassociates the merge.
// The vocabulary is sliced because the rows alone make too few workgroups (M = 4096: 32 blocks);
// the launcher picks the slice count so that blocks x slices covers the chip about twice.
//
// MODE 1, logit gradient. One 128 x 128 tile per workgroup on a plain 2-D grid; the epilogue turns
// the accumulators into dZ = (exp(z - lse[row]) - [col == label]) * *scale (0 for ignored rows),
// rounds once to bf16, stages the tile through the (dead) ring and stores whole 16-byte row chunks.
//
// Layout: 256 lanes = 4 waves stacked along the rows (32 x 128 of the tile each: 4 MFMA tiles, 64
// accumulator registers), so a row's statistics never leave its wave. K-tiles of 64: X (128 x 64) and
// W (128 x 64) are staged by buffer-descriptor LDS-DMA into the swizzled K-major image of
// mfma_common.h (kmaj_off), 4 + 4 one-KiB pieces per wave, in a ring of two stages (64 KiB): K-tile
// u + 1 lands while K-tile u is multiplied, one barrier per K-tile. The K-tiles of consecutive
// vocabulary tiles form one stream, so the ring never drains between tiles. Two stages, not three:
// 64.5 KiB lets two workgroups share a CU, and the second one's MFMAs cover the first one's epilogue
// (about 450 VALU instructions per tile against 192 MFMAs at K = 768), which a deeper ring at one
// workgroup per CU would leave exposed.
// The X block is re-fetched for every vocabulary tile instead of being held: at most 128 x 1024 x 2 B
// per block, it stays in L2, and holding it would cost 192 KiB of LDS at K = 768 or every register
// the statistics need. Blocks are ordered XCD-aware so that the blocks of one vocabulary slice (one
// W panel) run on one XCD's L2.
// Rows past M rely on the descriptor's zero fill and are never stored. W rows past V load zeros too,
// so columns past V in the last tile are forced to -inf before they reach the max / sum (MODE 0) and
// to 0 in dZ, where they are not stored either (MODE 1).
#include "mfma_common.h"
#include "cu_count.h"
#include "launchers_lmhead_xent.h"

#include <algorithm>

namespace psd {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int BM = 128, BN = 128, BK = 64;
constexpr int kTile = BM * BK * 2;               // one operand's K-tile image: 16 KiB
constexpr int kStage = 2 * kTile;                // X | W
constexpr int kLds = 2 * kStage + BM * 4;        // ring of two + the label logits of the block's rows
constexpr int kLdc = BN + 8;                     // bf16 row pitch of the dZ staging (16-B pad)
static_assert(BM * kLdc * 2 <= 2 * kStage, "the dZ tile is staged in the ring");

struct LmHeadDev {
  const uint16_t* x;
  const uint16_t* w;
  const uint16_t* bias;
  const int64_t* labels;
  int M, K, V;
  int slices;          // MODE 0
  float* part;         // MODE 0: [slices][3][M]
  const float* lse;    // MODE 1
  const float* scale;  // MODE 1
  uint16_t* dz;        // MODE 1: [M][V]
};

// (m, s) <- (m, s) merged with (m2, s2): s sums exp(z - m). An all-masked side has m = -inf, s = 0.
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mm = fmaxf(m, m2);
  const float ms = mm == -INFINITY ? 0.f : mm;  // exp(-inf - -inf) would be NaN
  s = s * __expf(m - ms) + s2 * __expf(m2 - ms);
  m = mm;
}

template <int CTRL>
__device__ __forceinline__ void merge_dpp(float& m, float& s) {
  const float m2 = dpp_q<CTRL>(m), s2 = dpp_q<CTRL>(s);
  merge(m, s, m2, s2);
}

// a label as the kernels use it: its column, or -1 for an ignored row (negative, or not a column)
__device__ __forceinline__ int label_col(const int64_t* labels, int row, int M, int V) {
  if (row >= M) return -1;
  const int64_t y = labels[row];
  return (y >= 0 && y < V) ? (int)y : -1;
}

}  // namespace

template <int MODE>
__global__ __launch_bounds__(256) void lmhead_xent_kernel(LmHeadDev a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  float* zl_s = reinterpret_cast<float*>(smem + 2 * kStage);
  const int lane = threadIdx.x & 63;
  const int wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int hl = lane >> 5, cl = lane & 31;
  const int tiles_m = (a.M + BM - 1) / BM, tiles_n = (a.V + BN - 1) / BN;
  // this workgroup's row block tm and vocabulary tiles [t0, t1)
  int tm, t0, t1, slice = 0;
  if (MODE == 0) {
    const int wg = xcd_remap(blockIdx.x, tiles_m * a.slices);
    slice = wg / tiles_m;
    tm = wg - slice * tiles_m;
    t0 = (int)((int64_t)slice * tiles_n / a.slices);
    t1 = (int)((int64_t)(slice + 1) * tiles_n / a.slices);
  } else {
    const int wg = xcd_remap(blockIdx.x, tiles_m * tiles_n);
    t0 = wg / tiles_m;
    tm = wg - t0 * tiles_m;
    t1 = t0 + 1;
  }
  const int m0 = tm * BM;
  const int nk = a.K / BK;
  // accumulator register r of a 32 x 32 MFMA tile: column cl, row rowl(r) of the wave's 32
  auto rowl = [&](int r) { return (r & 3) + 8 * (r >> 2) + 4 * hl; };

  // staging: piece (i * 4 + wid) = 8 rows x 128 B of either operand (both K-major with pitch K);
  // the lane's 16 bytes are chunk (lane & 7) ^ swizzle of its row, written to LDS slot lane & 7
  uint32_t vo[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int row = (i * 4 + wid) * 8 + (lane >> 3);
    const int c = (lane & 7) ^ ((row >> 1) & 7);
    vo[i] = (uint32_t)row * (uint32_t)a.K * 2u + c * 16;
  }
  const rsrc_t rx = make_rsrc(a.x, (uint32_t)a.M * (uint32_t)a.K * 2u);
  const rsrc_t rw = make_rsrc(a.w, (uint32_t)a.V * (uint32_t)a.K * 2u);
  auto issue = [&](int slot, int n0, int k0) {
    uint8_t* xs = smem + slot * kStage;
    uint8_t* ws = xs + kTile;
    const uint32_t sx = __builtin_amdgcn_readfirstlane(((uint32_t)m0 * (uint32_t)a.K + (uint32_t)k0) * 2u);
    const uint32_t sw = __builtin_amdgcn_readfirstlane(((uint32_t)n0 * (uint32_t)a.K + (uint32_t)k0) * 2u);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, (__attribute__((address_space(3))) void*)(xs + (i * 4 + wid) * 1024),
                                               16, vo[i] + sx, 0, 0, 0);
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rw, (__attribute__((address_space(3))) void*)(ws + (i * 4 + wid) * 1024),
                                               16, vo[i] + sw, 0, 0, 0);
    }
  };
  auto frag = [&](const uint8_t* img, int r0, int ks) {
    const u32x4 v = *reinterpret_cast<const u32x4*>(img + kmaj_off(r0 + cl, ks * 2 + hl));
    return __builtin_bit_cast(bf16x8, v);
  };

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  // MODE 0 state: the lane's running (max, sum) and label column of each of its 16 rows
  float rm[16], rs[16];
  int lab[16];
  if (MODE == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      rm[r] = -INFINITY;
      rs[r] = 0.f;
      lab[r] = label_col(a.labels, m0 + wid * 32 + rowl(r), a.M, a.V);
    }
    if (threadIdx.x < BM) zl_s[threadIdx.x] = 0.f;  // ordered before any write by the loop's first barrier
  }

  // the tile's bias, one value per MFMA tile column of the lane (0 past V)
  auto load_bias = [&](int n0, float (&b)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int n = n0 + j * 32 + cl;
      b[j] = (a.bias != nullptr && n < a.V) ? bf16_to_f32(a.bias[n]) : 0.f;
    }
  };

  const int total = (t1 - t0) * nk;  // K-tiles of the stream
  int n0 = t0 * BN, kt = 0;          // the K-tile being multiplied
  int nn0 = n0, nkt = 0;             // the K-tile being staged
  float bj[4];
  load_bias(n0, bj);
  issue(0, nn0, 0);
  for (int u = 0; u < total; ++u) {
    wait_vm<0>();     // this wave's pieces of K-tile u have landed
    __syncthreads();  // ... and everyone's; K-tile u - 1 has been read by all: its slot is free
    if (u + 1 < total) {
      if (++nkt == nk) {
        nkt = 0;
        nn0 += BN;
      }
      issue((u + 1) & 1, nn0, nkt * BK);
    }
    const uint8_t* xs = smem + (u & 1) * kStage;
    const uint8_t* ws = xs + kTile;
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      const bf16x8 af = frag(xs, wid * 32, ks);
      bf16x8 bf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = frag(ws, j * 32, ks);
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af, bf[j], acc[j], 0, 0, 0);
    }
    if (++kt < nk) continue;
    if (MODE == 1) break;  // the one tile of the logit-gradient grid: its epilogue follows the loop

    // ---- statistics epilogue of vocabulary tile [n0, n0 + 128)
    const bool ragged = n0 + BN > a.V;  // wave-uniform: only the last tile of the vocabulary
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool dead = ragged && n0 + j * 32 + cl >= a.V;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = dead ? -INFINITY : acc[j][r] + bj[j];
    }
    bool hit = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) hit |= (unsigned)(lab[r] - n0) < (unsigned)BN;
    if (__any(hit)) {  // some row of this wave has its label in the tile: one lane per such row writes
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (n0 + j * 32 + cl == lab[r]) zl_s[wid * 32 + rowl(r)] = acc[j][r];
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float mx = fmaxf(fmaxf(acc[0][r], acc[1][r]), fmaxf(acc[2][r], acc[3][r]));
      const float mn = fmaxf(rm[r], mx);
      const float ms = mn == -INFINITY ? 0.f : mn;
      float sum = rs[r] * __expf(rm[r] - ms);
#pragma unroll
      for (int j = 0; j < 4; ++j) sum += __expf(acc[j][r] - ms);
      rs[r] = sum;
      rm[r] = mn;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
    kt = 0;
    n0 += BN;
    if (u + 1 < total) load_bias(n0, bj);
  }

  if (MODE == 0) {
    __syncthreads();  // the label logits of every wave are in LDS
    // the 32 lanes of a half-wave hold the same 16 rows: merge them (all lanes end with the result)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float m = rm[r], s = rs[r];
      merge_dpp<0xB1>(m, s);   // quad_perm [1,0,3,2]
      merge_dpp<0x4E>(m, s);   // quad_perm [2,3,0,1]
      merge_dpp<0x141>(m, s);  // row_half_mirror: the other quad of the 8
      merge_dpp<0x140>(m, s);  // row_mirror: the other 8 of the 16
      const float m2 = xor16(m, lane), s2 = xor16(s, lane);
      merge(m, s, m2, s2);
      const int rl = wid * 32 + rowl(r), row = m0 + rl;
      if (cl == 0 && row < a.M) {
        float* p = a.part + (int64_t)slice * 3 * a.M + row;
        p[0] = m;
        p[a.M] = s;
        p[2 * (int64_t)a.M] = zl_s[rl];
      }
    }
    return;
  }

  // ---- logit-gradient epilogue: dZ of tile (m0, n0) -> bf16, staged through the ring, 16-byte stores
  const float scale = *a.scale;
  float l[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = m0 + wid * 32 + rowl(r);
    lab[r] = label_col(a.labels, row, a.M, a.V);
    l[r] = row < a.M ? a.lse[row] : 0.f;
  }
  __syncthreads();  // every wave has read the last K-tile: the ring is free
  uint16_t* cs = reinterpret_cast<uint16_t*>(smem);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int nl = j * 32 + cl, n = n0 + nl;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const float p = __expf((acc[j][r] + bj[j]) - l[r]);
      const float g = (lab[r] >= 0 && n < a.V) ? (p - (n == lab[r] ? 1.f : 0.f)) * scale : 0.f;
      cs[(wid * 32 + rowl(r)) * kLdc + nl] = f32_to_bf16(g);
    }
  }
  __syncthreads();
  constexpr int CPR = BN / 8;  // 16-byte chunks per tile row
  for (int c = threadIdx.x; c < BM * CPR; c += 256) {
    const int ml = c / CPR, nl = (c % CPR) * 8;
    const int m = m0 + ml, n = n0 + nl;
    if (m >= a.M || n >= a.V) continue;  // V % 8 == 0: a chunk is wholly inside or wholly outside
    *reinterpret_cast<u32x4*>(a.dz + (int64_t)m * a.V + n) = *reinterpret_cast<const u32x4*>(cs + ml * kLdc + nl);
  }
}

// lse and loss_row from the per-slice (max, sum, label logit), slices merged in index order
__global__ __launch_bounds__(256) void lmhead_xent_finalize_kernel(const float* __restrict__ part,
                                                                   const int64_t* __restrict__ labels, int M, int V,
                                                                   int slices, float* __restrict__ lse,
                                                                   float* __restrict__ loss_row) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= M) return;
  float m = part[row], s = part[(int64_t)M + row], zl = part[2 * (int64_t)M + row];
  for (int sl = 1; sl < slices; ++sl) {
    const float* p = part + (int64_t)sl * 3 * M + row;
    merge(m, s, p[0], p[M]);
    zl += p[2 * (int64_t)M];  // every slice but the label's holds 0: exact
  }
  const float lg = logf(s);
  lse[row] = m + lg;
  const int64_t y = labels[row];
  loss_row[row] = (y >= 0 && y < V) ? lg + (m - zl) : 0.f;
}

// ------------------------------------------------------------------ host side
namespace {
bool contract_ok(const LmHeadXentArgs& a) {
  auto al16 = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; };
  const int64_t lim = (int64_t)1 << 31;
  return a.x != nullptr && a.w != nullptr && a.labels != nullptr && a.M >= 1 && a.K >= BK && a.K % BK == 0 &&
         a.V >= 8 && a.V % 8 == 0 && al16(a.x) && al16(a.w) && (a.bias == nullptr || al16(a.bias)) &&
         (a.M + BM) * a.K < lim && (a.V + BN) * a.K < lim && a.M * a.V / BN < lim;
}

LmHeadDev dev_args(const LmHeadXentArgs& a) {
  LmHeadDev d{};
  d.x = a.x;
  d.w = a.w;
  d.bias = a.bias;
  d.labels = a.labels;
  d.M = (int)a.M;
  d.K = (int)a.K;
  d.V = (int)a.V;
  return d;
}

template <int MODE>
hipError_t launch_mode(const LmHeadDev& d, int nwg, hipStream_t st) {
  static bool attr_set = false;  // per instantiation: the > 64 KiB LDS limit, set once
  if (!attr_set) {
    const hipError_t e = hipFuncSetAttribute((const void*)lmhead_xent_kernel<MODE>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, kLds);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL((lmhead_xent_kernel<MODE>), dim3(nwg), dim3(256), kLds, st, d);
  return hipGetLastError();
}
}  // namespace

int lmhead_xent_slices(int64_t M, int64_t V) {
  const int64_t tiles_m = (M + BM - 1) / BM, tiles_n = (V + BN - 1) / BN;
  const int64_t s = (2 * (int64_t)cu_count() + tiles_m - 1) / tiles_m;
  return (int)std::max<int64_t>(1, std::min<int64_t>(s, tiles_n));
}

hipError_t launch_lmhead_xent_fwd(const LmHeadXentArgs& a, int slices, float* part, float* lse, float* loss_row,
                                  hipStream_t st) {
  if (!contract_ok(a) || part == nullptr || lse == nullptr || loss_row == nullptr || slices < 0)
    return hipErrorInvalidValue;
  const int tiles_m = (int)((a.M + BM - 1) / BM), tiles_n = (int)((a.V + BN - 1) / BN);
  LmHeadDev d = dev_args(a);
  d.slices = slices == 0 ? lmhead_xent_slices(a.M, a.V) : std::min(slices, tiles_n);
  d.part = part;
  if ((int64_t)tiles_m * d.slices >= ((int64_t)1 << 31)) return hipErrorInvalidValue;
  const hipError_t e = launch_mode<0>(d, tiles_m * d.slices, st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(lmhead_xent_finalize_kernel, dim3((unsigned)((a.M + 255) / 256)), dim3(256), 0, st, part, a.labels,
                     d.M, d.V, d.slices, lse, loss_row);
  return hipGetLastError();
}

hipError_t launch_lmhead_xent_dz(const LmHeadXentArgs& a, const float* lse, const float* scale, uint16_t* dz,
                                 hipStream_t st) {
  if (!contract_ok(a) || lse == nullptr || scale == nullptr || dz == nullptr ||
      (reinterpret_cast<uintptr_t>(dz) & 15) != 0)
    return hipErrorInvalidValue;
  const int64_t tiles = ((a.M + BM - 1) / BM) * ((a.V + BN - 1) / BN);
  LmHeadDev d = dev_args(a);
  d.lse = lse;
  d.scale = scale;
  d.dz = dz;
  return launch_mode<1>(d, (int)tiles, st);
}

}  // namespace psd
