// Fused multi-head self-attention for short sequences (BERT pre-training, S <= 128, head dim 64) on
// gfx950, forward and backward, reading the packed QKV projection output [B, S, 3, H, 64] in place and
// writing O as [B, S, H, 64] (the output projection's input, no transpose) and dQKV in the packed
// layout (the QKV projection's dgrad input, no stack/cat).
//
// One workgroup per (batch, head), S/32 waves; the whole head (Q, K, V, dO: S x 64 bf16 each) lives
// in LDS and every product is a v_mfma_f32_32x32x16_bf16:
//   forward   S^T = K Q^T (keys x queries: the softmax reduction runs over a lane's own registers
//             plus one lane^32 exchange), P = softmax, dropout, then O = P V with P staged through
//             LDS; the row log-sum-exp is saved for backward.
//   backward  wave w owns key block w: S^T and dP^T = V dO^T recomputed, dS = P (dP - rowsum(dO.O)),
//             dV = Pd^T dO and dK = dS^T Q from transposed LDS reads (ds_read_b64_tr_b16); then
//             wave w owns query block w: dQ = dS K.
// Dropout keeps (b, h, q, key) from the same counter hash as the fused LayerNorm (seed, device step
// counter), so the mask is regenerated in backward and a replayed hipGraph draws fresh masks.
// Padded batches pass per-sequence lengths (AttnArgs::lens): separate VARLEN instantiations skip the
// 32-row blocks past a length, mask the partial one and never read a padded row; without lengths the
// launchers pick the VARLEN = false instantiations, which are the full-length kernels unchanged.
// Longer sequences (128 < S <= 512, S % 64 == 0) do not fit this whole-head image; they run the
// streaming kernels of attention_long.hip under the same contracts (launch_attn_fwd / launch_attn_bwd
// serve S <= 128 only; the tensor glue in attn_ops.cpp picks the family by S).
//
// Replaces what the reference's stub gradient (src/worker.cpp:316-329) stands in for: the model's
// real forward/backward; the attention is BERT's (BASELINE config 4).
#include <algorithm>

#include "common.h"
#include "cu_count.h"
#include "launchers_attn.h"
#include "attn_frag.h"

namespace psd {

namespace {

// (fragment, dropout-hash and length helpers: attn_frag.h, shared with attention_long.hip)

// rows [0, S) of a [.., S, 3, H, 64] (or [.., S, H, 64]) tensor -> LDS tile [S][LDT]
__device__ __forceinline__ void stage_rows(uint8_t* lds, const uint16_t* src, int64_t row_stride, int S) {
  for (int c = threadIdx.x; c < S * 8; c += blockDim.x) {
    const int r = c >> 3, ch = c & 7;
    *reinterpret_cast<u32x4*>(lds + r * LDT * 2 + ch * 16) =
        *reinterpret_cast<const u32x4*>(src + (int64_t)r * row_stride + ch * 8);
  }
}

}  // namespace

// Persistent (as many workgroups per CU as registers and the 36 KiB K + V image allow): the next
// (batch, head) item's K, V rows and this lane's Q fragments are loaded into registers while the
// current item is computed. The probabilities never leave registers (P V takes them as its B
// operand in accumulator-row key order) and O leaves in 8-B pieces.
//
// VARLEN (a.lens given): sequence b has L = item_len valid rows, nb = ceil(L / 32) blocks. Rows >= L of
// K, V and Q are never loaded: zeros are staged in their place, so no padded (or stale) row enters a
// product. A wave whose query block lies past L stores zeros and runs no MFMA; the others walk key
// blocks j < nb only, with the scores of keys >= L at -inf (probability exactly 0). Every skip is
// wave-uniform and every wave reaches both barriers. Without lengths (VARLEN false) every such test
// is a compile-time constant and the kernel is the full-length one.
// CAUSAL (a.causal; always with VARLEN, L = S when a.lens is null): wave w owns query block w and walks
// key blocks j <= w only (all of them < nb, since a wave that computes has 32 w < L); in the diagonal
// block j == w the scores of keys > q go to -inf by the same select as keys >= L. Key 32 w is visible
// to every query of the block, so the row max is finite. Future rows of the diagonal block are staged
// and multiplied (finite inputs give exact-zero probabilities); without a.causal every such test is a
// compile-time constant.
// (The length-aware copy asks for two waves per SIMD: left alone the compiler takes 233 + 80 registers
// at NW = 4, one workgroup per CU instead of two; a minimum of 1 is the default and leaves the
// full-length copy as it was.)
// DOCS (a.doc; always with CAUSAL): query q sees keys doc[q] <= key <= q. Wave w walks key blocks
// jlo <= j <= w, jlo = doc[32 w] >> 5 (the block's first query has the smallest start), and keys < doc[q]
// of the blocks up to the one with the largest start of the wave go to -inf by the same select. A valid
// query sees itself and a padded one (doc not read: start 0) key 32 w, so the row max stays finite. The
// starts ride in the item prefetch; with a.doc null the launchers never pick this copy.
template <int NW, bool VARLEN, bool CAUSAL, bool DOCS = false>
__global__ __launch_bounds__(64 * NW) __attribute__((amdgpu_waves_per_eu(VARLEN ? 2 : 1)))
void attn_fwd_kernel(AttnArgs a) {
  static_assert(VARLEN || !CAUSAL, "the causal copy is length-aware");
  static_assert(CAUSAL || !DOCS, "the document copy is causal");
  constexpr int S = 32 * NW;
  constexpr int NT = 64 * NW;
  constexpr int CH = S * 8 / NT;  // 16-B chunks per lane per tile (= 4)
  static_assert(CH * NT == S * 8, "chunking");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* Ks = smem;
  uint8_t* Vs = Ks + S * LDT * 2;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5;
  const int HD = a.H * D;
  const int64_t qkv_rs = 3 * (int64_t)HD;
  const int nitems = a.B * a.H;
  const int q0 = 32 * w, q = q0 + (lane & 31);
  const float sl = a.scale * 1.4426950408889634f;
  const uint32_t key = attn_key(a.seed, a.step);
  const bool drop = a.thresh != 0u;

  u32x4 pk[CH], pv[CH], pq[4];
  int pdq = 0;  // DOCS: the start of query q's document (0 for a padded query)
  auto fetch = [&](int bh) {
    const int b = bh / a.H, h = bh % a.H;
    const uint16_t* base = a.qkv + (int64_t)b * S * qkv_rs + h * D;
    const int Lf = item_len<VARLEN, CAUSAL>(a, b, S);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = threadIdx.x + i * NT, r = c >> 3, ch = c & 7;
      u32x4 k4 = zero4(), v4 = zero4();
      if (!VARLEN || r < Lf) {
        k4 = *reinterpret_cast<const u32x4*>(base + HD + (int64_t)r * qkv_rs + ch * 8);
        v4 = *reinterpret_cast<const u32x4*>(base + 2 * HD + (int64_t)r * qkv_rs + ch * 8);
      }
      pk[i] = k4;
      pv[i] = v4;
    }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      u32x4 q4 = zero4();
      if (!VARLEN || q < Lf) q4 = *reinterpret_cast<const u32x4*>(base + (int64_t)q * qkv_rs + 16 * ks + 8 * hh);
      pq[ks] = q4;
    }
    if constexpr (DOCS) pdq = q < Lf ? doc_of<DOCS>(a, b, S, q) : 0;
  };
  if ((int)blockIdx.x < nitems) fetch(blockIdx.x);

  for (int bh = blockIdx.x; bh < nitems; bh += gridDim.x) {
    const int b = bh / a.H, h = bh % a.H;
    const int L = item_len<VARLEN, CAUSAL>(a, b, S);
    const int nb = (L + 31) >> 5;  // key / query blocks with a valid row
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = threadIdx.x + i * NT, r = c >> 3, ch = c & 7;
      *reinterpret_cast<u32x4*>(Ks + r * LDT * 2 + ch * 16) = pk[i];
      *reinterpret_cast<u32x4*>(Vs + r * LDT * 2 + ch * 16) = pv[i];
    }
    abf16x8 qf[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) qf[ks] = __builtin_bit_cast(abf16x8, pq[ks]);
    const int dq = pdq;
    __syncthreads();
    if (bh + (int)gridDim.x < nitems) fetch(bh + gridDim.x);  // in flight during this item

    if (!VARLEN || q0 < L) {
      const bool vq = !VARLEN || q < L;  // a padded query of the partial block: zero q, stores zeros
      // DOCS: first key block walked, and the last one with a key before some query's document
      int jlo = 0, jhi = -1;
      if constexpr (DOCS) {
        jlo = __builtin_amdgcn_readfirstlane(dq) >> 5;
        jhi = __builtin_amdgcn_readlane(dq, __builtin_amdgcn_readfirstlane(min(31, L - 1 - q0))) >> 5;
      }
      af32x16 sc[NW];  // S^T tiles: lane owns query q, keys 32j + acc_row(i)
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if ((VARLEN && j >= nb) || (CAUSAL && j > w) || (DOCS && j < jlo)) continue;
        sc[j] = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) sc[j] = mfma(rowfrag(Ks, LDT * 2, 32 * j, 16 * ks), qf[ks], sc[j]);
        if constexpr (CAUSAL) {
          if (j == w) {  // the diagonal block (the partial key block is this one or is not walked)
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (32 * j + acc_row(i, hh) > q || 32 * j + acc_row(i, hh) >= L) sc[j][i] = -INFINITY;
          }
          if constexpr (DOCS) {
            if (j <= jhi) {  // keys of an earlier document
#pragma unroll
              for (int i = 0; i < 16; ++i)
                if (32 * j + acc_row(i, hh) < dq) sc[j][i] = -INFINITY;
            }
          }
        } else if constexpr (VARLEN) {
          if (j == nb - 1) {  // the partial key block: keys >= L leave the max and the sum
#pragma unroll
            for (int i = 0; i < 16; ++i)
              if (32 * j + acc_row(i, hh) >= L) sc[j][i] = -INFINITY;
          }
        }
      }
      float m = -INFINITY;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if ((VARLEN && j >= nb) || (CAUSAL && j > w) || (DOCS && j < jlo)) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) m = fmaxf(m, sc[j][i]);
      }
      m = fmaxf(m, __shfl_xor(m, 32));
      float l = 0.f;
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if ((VARLEN && j >= nb) || (CAUSAL && j > w) || (DOCS && j < jlo)) continue;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          sc[j][i] = exp2f((sc[j][i] - m) * sl);
          l += sc[j][i];
        }
      }
      l += __shfl_xor(l, 32);
      if (hh == 0) a.lse[(int64_t)bh * S + q] = vq ? m * a.scale + logf(l) : 0.f;
      const float inv = 1.f / l;
      const uint64_t rowidx = ((uint64_t)bh * S + q) * S;
      // O^T[d][q] = sum_key V^T[d][key] P^T[key][q]: B = this lane's probabilities (query q, keys in
      // accumulator-row order), A = V^T read in that order; no P round trip through LDS
      af32x16 ot[2] = {zero16(), zero16()};
#pragma unroll
      for (int j = 0; j < NW; ++j) {
        if ((VARLEN && j >= nb) || (CAUSAL && j > w) || (DOCS && j < jlo)) continue;
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2) {
          float v[8];
          bool kp[8];
          if (drop) {  // elements e, e + 1 (e even) are keys kk, kk + 1 with kk even: one hash per pair
#pragma unroll
            for (int e = 0; e < 8; e += 2) akeep2(key, rowidx + 32 * j + acc_row(8 * ks2 + e, hh), a.thresh, kp[e], kp[e + 1]);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            v[e] = sc[j][8 * ks2 + e] * inv;
            if (drop) v[e] = kp[e] ? v[e] * a.rescale : 0.f;
          }
          const abf16x8 pb = __builtin_bit_cast(
              abf16x8, u32x4{pack_bf16x2_rne(v[0], v[1]), pack_bf16x2_rne(v[2], v[3]), pack_bf16x2_rne(v[4], v[5]),
                             pack_bf16x2_rne(v[6], v[7])});
#pragma unroll
          for (int dt = 0; dt < 2; ++dt) ot[dt] = mfma(trfrag_accrows(Vs, LDT * 2, 32 * j + 16 * ks2, 32 * dt), pb, ot[dt]);
        }
      }
      // lane: query q, d = 32 dt + acc_row(i): 4 consecutive d per 4 accumulators -> 8-B stores
      uint16_t* out = a.o + ((int64_t)b * S + q) * HD + h * D;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g)
          *reinterpret_cast<uint2*>(out + 32 * dt + 8 * g + 4 * hh) =
              vq ? make_uint2(pack_bf16x2_rne(ot[dt][4 * g], ot[dt][4 * g + 1]), pack_bf16x2_rne(ot[dt][4 * g + 2], ot[dt][4 * g + 3]))
                 : make_uint2(0u, 0u);
    } else {  // the whole query block is padding: zero O and lse, no MFMA
      if (hh == 0) a.lse[(int64_t)bh * S + q] = 0.f;
      uint16_t* out = a.o + ((int64_t)b * S + q) * HD + h * D;
#pragma unroll
      for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) *reinterpret_cast<uint2*>(out + 32 * dt + 8 * g + 4 * hh) = make_uint2(0u, 0u);
    }
    __syncthreads();  // K, V of this item read by every wave before the next item's stores
  }
}

// 2*NW waves: the LDS image (Q, K, V, dO, Pd, dS: ~144 KiB at S = 128) allows one workgroup per
// CU, so a 32-row block is split between two waves (query blocks / head-dim halves) to keep two
// waves per SIMD: at one wave per SIMD (the first version) nothing hid the LDS and MFMA latencies
// and the kernel ran at 3.5x its HBM time (profiles/bert_base_b256_r2_kernels.md).
// Persistent: one workgroup per CU walks (batch, head) items; the next item's Q, K, V, dO, O rows
// and lse are loaded into registers (2 chunks of 16 B per tile per lane) while the current item is
// computed, so the HBM time of one item hides behind the MFMA/LDS work of the previous one (a
// workgroup per item loaded, synchronised and computed strictly in turn: 189 us per BERT layer,
// ~2 TB/s, profiles/bert_base_b256_r4 profile).
//
// VARLEN (a.lens given; L, nb as in the forward): rows >= L of Q, K, V, dO, O and lse are never loaded,
// zeros are staged over the whole tile height instead, so nothing of a previous, longer item is left
// in those five tiles (and D_s, lse_s). Pd and dS are written in phase 1 for key blocks < nb and
// query blocks < nb only, with zeros at masked keys and padded queries, and phases 2 and 3 read
// exactly that region (chunks < 2 nb of blocks < nb); what the previous item left outside it is
// never read. Blocks >= nb store zero dK, dV / dQ and zero column sums. All skips are wave-uniform.
//
// CAUSAL (always with VARLEN; L = S when a.lens is null): phase 1 writes Pd and dS for key block w
// against query blocks w <= t < nb only, with zeros at keys > q inside the diagonal block t == w; the
// blocks above the diagonal are written by no item. Phase 2 (key block w) reduces over the query
// chunks 2 w <= ks < 2 nb, i.e. query blocks w .. nb - 1 of key block w, and phase 3 (query block w)
// over the key chunks ks < 2 (w + 1) <= 2 nb, i.e. key blocks 0 .. w of query block w: both inside
// what phase 1 of this item wrote.
//
// DOCS (always with CAUSAL): the clamped starts of the valid rows are staged in LDS with the item
// (doc_s, zeros past L). Key block w is visible to the query blocks w <= t < tend, tend the first t with
// doc[32 t] > 32 w + 31 (monotone starts: every later block is invisible too), and query block w sees the
// key blocks jlo = doc[32 w] >> 5 <= j <= w. Phase 1 writes exactly the blocks w <= t < tend with zeros
// at keys < doc[q]; phase 2 reduces over the query chunks 2 w <= ks < 2 tend and phase 3 over the key
// chunks 2 jlo <= ks < 2 (w + 1). For a well-formed row t < tend(j) is jlo(t) <= j, so both read only
// what phase 1 of this item wrote; no skipped block is read.
// (The document copy asks for two waves per SIMD, as the forward's length-aware copies do: left alone
// the compiler takes 222 + 64 registers at NW = 2; a minimum of 1 is the default.)
template <int NW, bool VARLEN, bool CAUSAL, bool DOCS = false>
__global__ __launch_bounds__(128 * NW) __attribute__((amdgpu_waves_per_eu(DOCS ? 2 : 1)))
void attn_bwd_kernel(AttnArgs a) {
  static_assert(VARLEN || !CAUSAL, "the causal copy is length-aware");
  static_assert(CAUSAL || !DOCS, "the document copy is causal");
  constexpr int S = 32 * NW, LDP = S + 8;
  constexpr int NT = 128 * NW;
  constexpr int CH = S * 8 / NT;  // 16-B chunks per lane per tile (= 2)
  static_assert(CH * NT == S * 8, "chunking");
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  uint8_t* Qs = smem;
  uint8_t* Ks = Qs + S * LDT * 2;
  uint8_t* Vs = Ks + S * LDT * 2;
  uint8_t* dOs = Vs + S * LDT * 2;
  uint8_t* Pd = dOs + S * LDT * 2;  // dropped, rescaled probabilities [q][key]
  uint8_t* dS = Pd + S * LDP * 2;   // dS = P (dP - D) [q][key]
  float* lse_s = reinterpret_cast<float*>(dS + S * LDP * 2);
  float* D_s = lse_s + S;
  float* cs_s = D_s + S;  // [NW][3][64] per-key/query-block column sums of dq, dk, dv (bpart)
  int* doc_s = reinterpret_cast<int*>(cs_s + NW * 3 * 64);  // DOCS: [S] document starts (bwd_lds adds them)

  const int lane = threadIdx.x & 63, hh = lane >> 5;
  const int w = threadIdx.x >> 7, sub = (threadIdx.x >> 6) & 1;  // 32-row block, half of its work
  const int HD = a.H * D;
  const int64_t qkv_rs = 3 * (int64_t)HD;
  const int nitems = a.B * a.H;
  const uint32_t key = attn_key(a.seed, a.step);
  const bool drop = a.thresh != 0u;
  const float sl = a.scale * 1.4426950408889634f;

  // register prefetch of one item: tile t (Q, K, V, dO, O) chunk i = row c >> 3, 16-B column c & 7
  u32x4 pf[5][CH];
  float plse = 0.f;  // (DOCS: threads S .. 2 S - 1 carry the document start of row tid - S in it, as int bits)
  auto fetch = [&](int bh) {
    const int b = bh / a.H, h = bh % a.H;
    const uint16_t* base = a.qkv + (int64_t)b * S * qkv_rs + h * D;
    const int64_t ob = (int64_t)b * S * HD + h * D;
    const int Lf = item_len<VARLEN, CAUSAL>(a, b, S);
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = threadIdx.x + i * NT, r = c >> 3, ch = c & 7;
      if (!VARLEN || r < Lf) {
#pragma unroll
        for (int t = 0; t < 3; ++t)
          pf[t][i] = *reinterpret_cast<const u32x4*>(base + t * HD + (int64_t)r * qkv_rs + ch * 8);
        pf[3][i] = *reinterpret_cast<const u32x4*>(a.dout + ob + (int64_t)r * HD + ch * 8);
        pf[4][i] = *reinterpret_cast<const u32x4*>(a.o + ob + (int64_t)r * HD + ch * 8);
      } else {
#pragma unroll
        for (int t = 0; t < 5; ++t) pf[t][i] = zero4();
      }
    }
    if (threadIdx.x < S) plse = (!VARLEN || (int)threadIdx.x < Lf) ? a.lse[(int64_t)bh * S + threadIdx.x] : 0.f;
    if constexpr (DOCS) {
      const int r = (int)threadIdx.x - S;
      if (r >= 0 && r < S) plse = __int_as_float(r < Lf ? doc_of<DOCS>(a, b, S, r) : 0);
    }
  };
  if ((int)blockIdx.x < nitems) fetch(blockIdx.x);

  for (int bh = blockIdx.x; bh < nitems; bh += gridDim.x) {
    const int b = bh / a.H, h = bh % a.H;
    const int L = item_len<VARLEN, CAUSAL>(a, b, S);
    const int nb = (L + 31) >> 5;  // key / query blocks with a valid row
    // the prefetched item -> LDS; D[q] = sum_d dO[q, d] O[q, d] (8 lanes per row)
#pragma unroll
    for (int i = 0; i < CH; ++i) {
      const int c = threadIdx.x + i * NT, r = c >> 3, ch = c & 7;
      uint8_t* tiles[4] = {Qs, Ks, Vs, dOs};
#pragma unroll
      for (int t = 0; t < 4; ++t) *reinterpret_cast<u32x4*>(tiles[t] + r * LDT * 2 + ch * 16) = pf[t][i];
      const uint32_t xw[4] = {pf[3][i].x, pf[3][i].y, pf[3][i].z, pf[3][i].w};
      const uint32_t yw[4] = {pf[4][i].x, pf[4][i].y, pf[4][i].z, pf[4][i].w};
      float s = 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        s = fmaf(__uint_as_float(xw[e] << 16), __uint_as_float(yw[e] << 16), s);
        s = fmaf(__uint_as_float(xw[e] & 0xffff0000u), __uint_as_float(yw[e] & 0xffff0000u), s);
      }
      s += __shfl_xor(s, 1);
      s += __shfl_xor(s, 2);
      s += __shfl_xor(s, 4);
      if (ch == 0) D_s[r] = s;
    }
    if (threadIdx.x < S) lse_s[threadIdx.x] = plse;
    if constexpr (DOCS) {
      if (threadIdx.x >= S && threadIdx.x < 2 * S) doc_s[threadIdx.x - S] = __float_as_int(plse);
    }
    __syncthreads();
    if (bh + (int)gridDim.x < nitems) fetch(bh + gridDim.x);  // in flight during this item's phases

    // phase 1: waves (w, sub) own keys k0..k0+31; recompute S^T and dP^T against the query blocks
    // t = sub, sub + 2, ...
    const int k0 = 32 * w;
    // DOCS: query blocks [w, tend) see key block w (tend <= nb)
    int tend = nb;
    if constexpr (DOCS) {
      if (w < nb) {
#pragma unroll
        for (int t = NW - 1; t >= 0; --t)
          if (t >= w && t < nb && __builtin_amdgcn_readfirstlane(doc_s[32 * t]) > k0 + 31) tend = t;
      }
    }
    if (!VARLEN || w < nb) {
      abf16x8 kf[4], vf[4];
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) {
        kf[ks] = rowfrag(Ks, LDT * 2, k0, 16 * ks);
        vf[ks] = rowfrag(Vs, LDT * 2, k0, 16 * ks);
      }
#pragma unroll
      for (int t = sub; t < NW; t += 2) {
        if ((VARLEN && t >= (DOCS ? tend : nb)) || (CAUSAL && t < w)) continue;
        af32x16 st = zero16(), dpt = zero16();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
          st = mfma(kf[ks], rowfrag(Qs, LDT * 2, 32 * t, 16 * ks), st);
          dpt = mfma(vf[ks], rowfrag(dOs, LDT * 2, 32 * t, 16 * ks), dpt);
        }
        const int q = 32 * t + (lane & 31);
        const float lse2 = lse_s[q] * 1.4426950408889634f, Dq = D_s[q];
        // DOCS: one window test for the three masks below. Query q sees keys doc[q] <= key <= q when
        // q < L (then key < L too); krel = key - doc[q] of the lane's first key, kspan = q - doc[q], or
        // -1 (no key) for a padded query, compared as unsigned
        int krel = 0, kspan = 0;
        if constexpr (DOCS) {
          const int dq = doc_s[q];
          krel = k0 + 4 * hh - dq;
          kspan = q < L ? q - dq : -1;
        }
        const uint64_t rowidx = ((uint64_t)bh * S + q) * S;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          float pv[4], dv[4];
          bool kp[4];
          if (drop) {  // keys k0 + 8g + 4hh + e: pairs (0, 1), (2, 3) share one hash
            akeep2(key, rowidx + k0 + 8 * g + 4 * hh, a.thresh, kp[0], kp[1]);
            akeep2(key, rowidx + k0 + 8 * g + 4 * hh + 2, a.thresh, kp[2], kp[3]);
          }
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int i = 4 * g + e;
            const float p = exp2f(st[i] * sl - lse2);
            float pd = p, dp = dpt[i];
            if (drop) {
              pd = kp[e] ? p * a.rescale : 0.f;
              dp = kp[e] ? dp * a.rescale : 0.f;
            }
            pv[e] = pd;
            dv[e] = p * (dp - Dq);
            if constexpr (DOCS) {  // padded query, key of an earlier document or future key: exact zeros
              if (kspan < 0 || (uint32_t)(krel + 8 * g + e) > (uint32_t)kspan) pv[e] = dv[e] = 0.f;
            } else {
              if constexpr (VARLEN) {  // masked key or padded query: exact zeros into Pd and dS
                if (q >= L || k0 + 8 * g + 4 * hh + e >= L) pv[e] = dv[e] = 0.f;
              }
              if constexpr (CAUSAL) {  // a future key of the diagonal block (t > w has every key <= q)
                if (k0 + 8 * g + 4 * hh + e > q) pv[e] = dv[e] = 0.f;
              }
            }
          }
          const int off = q * LDP * 2 + (k0 + 8 * g + 4 * hh) * 2;
          *reinterpret_cast<uint2*>(Pd + off) = make_uint2(pack_bf16x2_rne(pv[0], pv[1]), pack_bf16x2_rne(pv[2], pv[3]));
          *reinterpret_cast<uint2*>(dS + off) = make_uint2(pack_bf16x2_rne(dv[0], dv[1]), pack_bf16x2_rne(dv[2], dv[3]));
        }
      }
    }
    __syncthreads();

    // phase 2: dV[key, d] = sum_q Pd[q, key] dO[q, d];  dK = scale * sum_q dS[q, key] Q[q, d]
    // (wave (w, sub): keys of block w, head dims 32*sub..)
    uint16_t* dq_base = a.dqkv + (int64_t)b * S * qkv_rs + h * D;
    {
      const int dt = sub;
      af32x16 dv = zero16(), dk = zero16();
#pragma unroll
      for (int ks = 0; ks < S / 16; ++ks) {
        // a key block past L keeps its zeros (DOCS: tend for nb, the documents that start after the key
        // block see none of its keys either)
        if (VARLEN && (w >= nb || ks >= 2 * (DOCS ? tend : nb))) break;
        if (CAUSAL && ks < 2 * w) continue;              // queries before the key block see none of its keys
        dv = mfma(trfrag(Pd, LDP * 2, 16 * ks, k0), trfrag(dOs, LDT * 2, 16 * ks, 32 * dt), dv);
        dk = mfma(trfrag(dS, LDP * 2, 16 * ks, k0), trfrag(Qs, LDT * 2, 16 * ks, 32 * dt), dk);
      }
      const int d = 32 * dt + (lane & 31);
      float sk = 0.f, sv = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const int64_t r = (int64_t)(k0 + acc_row(i, hh)) * qkv_rs + d;
        dq_base[r + HD] = f32_to_bf16(dk[i] * a.scale);
        dq_base[r + 2 * HD] = f32_to_bf16(dv[i]);
        sk += dk[i];
        sv += dv[i];
      }
      if (a.bpart) {  // this wave's 32 keys: the two lane halves hold 16 rows each
        sk += __shfl_xor(sk, 32);
        sv += __shfl_xor(sv, 32);
        if (hh == 0) {
          cs_s[(w * 3 + 1) * 64 + d] = sk * a.scale;
          cs_s[(w * 3 + 2) * 64 + d] = sv;
        }
      }
    }
    // phase 3: waves (w, sub) own queries q0..q0+31, head dims 32*sub..: dQ = scale * dS K
    const int q0 = 32 * w;
    {
      const int dt = sub;
      af32x16 dq = zero16();
      int jlo = 0;  // DOCS: query block w sees key blocks [jlo, w]
      if constexpr (DOCS) {
        if (w < nb) jlo = __builtin_amdgcn_readfirstlane(doc_s[32 * w]) >> 5;
      }
#pragma unroll
      for (int ks = 0; ks < S / 16; ++ks) {
        if (VARLEN && (w >= nb || ks >= 2 * nb)) break;  // a query block past L keeps its zeros
        if (CAUSAL && ks >= 2 * (w + 1)) break;          // keys after the query block
        if (DOCS && ks < 2 * jlo) continue;              // keys before the first document of the query block
        dq = mfma(rowfrag(dS, LDP * 2, q0, 16 * ks), trfrag(Ks, LDT * 2, 16 * ks, 32 * dt), dq);
      }
      const int d = 32 * dt + (lane & 31);
      float sq = 0.f;
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        dq_base[(int64_t)(q0 + acc_row(i, hh)) * qkv_rs + d] = f32_to_bf16(dq[i] * a.scale);
        sq += dq[i];
      }
      if (a.bpart) {
        sq += __shfl_xor(sq, 32);
        if (hh == 0) cs_s[(w * 3 + 0) * 64 + d] = sq * a.scale;
      }
    }
    if (a.bpart) {  // the item's column sums in a fixed order over the blocks -> bpart[b][t * HD + h * 64 + d]
      __syncthreads();
      // 3 * 64 sums; at S = 32 the workgroup has 128 threads, which take a second one each (the V sums
      // were left unwritten there before: an uninitialised third of the QKV bias gradient)
      for (int c = threadIdx.x; c < 3 * 64; c += NT) {
        const int t = c >> 6, d = c & 63;
        float acc = 0.f;
#pragma unroll
        for (int ww = 0; ww < NW; ++ww) acc += cs_s[(ww * 3 + t) * 64 + d];
        a.bpart[(int64_t)b * 3 * HD + t * HD + h * D + d] = acc;
      }
    }
    __syncthreads();  // every read of this item's LDS done before the next item overwrites it
  }
}


bool attn_supported(int S, int head_dim) { return head_dim == D && S >= 32 && S <= 128 && S % 32 == 0; }

static int fwd_lds(int S) { return 2 * S * LDT * 2; }
static int bwd_lds(int S, bool docs) {  // docs: + the [S] document starts
  return 4 * S * LDT * 2 + 2 * S * (S + 8) * 2 + 2 * S * 4 + (S / 32) * 3 * 64 * 4 + (docs ? S * 4 : 0);
}

template <int NW, bool VARLEN, bool CAUSAL, bool DOCS = false>
static hipError_t launch_fwd_t(const AttnArgs& a, hipStream_t st) {
  const int lds = fwd_lds(32 * NW);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_kernel<NW, VARLEN, CAUSAL, DOCS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  // persistent: the resident workgroups per CU (registers / LDS), each walks items bh, bh + grid, ...
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(&attn_fwd_kernel<NW, VARLEN, CAUSAL, DOCS>), 64 * NW,
                                                   lds) != hipSuccess || per_cu < 1)
    per_cu = 1;
  int grid = std::min(a.B * a.H, per_cu * cu_count());
  if (a.grid_cap > 0) grid = std::min(grid, a.grid_cap);
  hipLaunchKernelGGL((attn_fwd_kernel<NW, VARLEN, CAUSAL, DOCS>), dim3(grid), dim3(64 * NW), lds, st, a);
  return hipGetLastError();
}
template <int NW, bool VARLEN, bool CAUSAL, bool DOCS = false>
static hipError_t launch_bwd_t(const AttnArgs& a, hipStream_t st) {
  const int lds = bwd_lds(32 * NW, DOCS);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_bwd_kernel<NW, VARLEN, CAUSAL, DOCS>),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e != hipSuccess) return e;
  // persistent: one workgroup per CU (the LDS image admits one), each walks items bh, bh + grid, ...
  int grid = std::min(a.B * a.H, cu_count());
  if (a.grid_cap > 0) grid = std::min(grid, a.grid_cap);
  hipLaunchKernelGGL((attn_bwd_kernel<NW, VARLEN, CAUSAL, DOCS>), dim3(grid), dim3(128 * NW), lds, st, a);
  return hipGetLastError();
}

// (VARLEN, CAUSAL, DOCS): full length, lengths, causal (with or without lengths), causal with documents;
// without a.doc the choice is the one made before the document copies existed
#define PSD_ATTN_PICK(fn, nw)                                                  \
  (a.doc      ? fn<nw, true, true, true>(a, st)                                \
   : a.causal ? fn<nw, true, true>(a, st)                                      \
   : a.lens   ? fn<nw, true, false>(a, st)                                     \
              : fn<nw, false, false>(a, st))

hipError_t launch_attn_fwd(const AttnArgs& a, hipStream_t st) {
  if (!attn_supported(a.S, D) || (a.doc && !a.causal) || a.window) return hipErrorInvalidValue;  // no window copies here
  switch (a.S / 32) {
    case 1: return PSD_ATTN_PICK(launch_fwd_t, 1);
    case 2: return PSD_ATTN_PICK(launch_fwd_t, 2);
    case 3: return PSD_ATTN_PICK(launch_fwd_t, 3);
    default: return PSD_ATTN_PICK(launch_fwd_t, 4);
  }
}
hipError_t launch_attn_bwd(const AttnArgs& a, hipStream_t st) {
  if (!attn_supported(a.S, D) || (a.doc && !a.causal) || a.window) return hipErrorInvalidValue;  // no window copies here
  switch (a.S / 32) {
    case 1: return PSD_ATTN_PICK(launch_bwd_t, 1);
    case 2: return PSD_ATTN_PICK(launch_bwd_t, 2);
    case 3: return PSD_ATTN_PICK(launch_bwd_t, 3);
    default: return PSD_ATTN_PICK(launch_bwd_t, 4);
  }
}

#undef PSD_ATTN_PICK

}  // namespace psd
