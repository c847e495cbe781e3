// Fused multi-head self-attention for sequences of 192 to 4096 tokens (128 < S <= 4096, S % 64 == 0,
// head dim 64, bf16) on gfx950: streaming (flash-style) forward and backward with the contracts of the
// whole-head kernels in attention.hip -- packed QKV [B, S, 3, H, 64] in, O [B, S, H, 64] and the
// packed dQKV out, the row log-sum-exp, per-sequence lengths, the counter-hash dropout mask, the
// QKV-bias partial sums and grid_cap.
//
// The whole head no longer fits LDS (K and V alone are 147 KB at S = 512), and nothing below is sized by
// S: LDS holds two 64-row chunks whatever the length, every row, pair and partial index is 64-bit, and
// the one S-bound structure is the 64-lane ballot over chunks in the dK/dV document walk (S <= 4096,
// attn_long_supported). Every kernel here keeps
// one operand set in registers, streams the other through LDS in 64-row chunks (register-staged,
// double-buffered, one barrier per chunk) and holds all score-sized data in accumulators. Three
// forward-shaped kernels, every product a v_mfma_f32_32x32x16_bf16:
//   forward   item (batch, head, 128-query tile), wave w owns 32 queries, Q fragments in registers.
//             Per key chunk S^T = K Q^T (a lane owns one query: the row reduction is its own registers
//             plus one lane^32 exchange), online softmax (running max m, sum l, O^T rescaled by
//             exp2((m_old - m_new) * scale * log2 e) at every chunk: no threshold, no rare branch),
//             dropout on the un-normalised probabilities, O^T += V^T P^T with P straight from the
//             accumulators; one 1/l at the end, lse = m * scale + log l.
//   dQ pass   same item and orientation: S^T and dP^T = V dO^T recomputed per chunk, p = exp2(s * sl -
//             lse * log2 e), dS^T = P (dP - D), dQ^T += K^T dS^T. D[q] = sum_d dO[q, d] O[q, d] comes
//             from the lane's own dO / O fragments and is also written to an fp32 [B, H, S] scratch.
//   dK/dV     item (batch, head, 128-key tile), wave w holds its 32 keys' K and V fragments and
//             streams Q, dO, lse and D: S = Q K^T and dP = dO V^T with the key on the lane, so the
//             accumulators are the B operands of dV^T += dO^T Pd and dK^T += Q^T dS.
// Seven products instead of five; in exchange no Pd / dS image touches LDS, nothing is summed across
// workgroups and there are no atomics: a result does not depend on the grid, two runs are bitwise equal.
//
// Lengths (VARLEN instantiations, a.lens given; L = clamp(lens[b], 0, S)): rows >= L are never loaded
// (zeros are staged in their place), chunks, 32-row blocks and whole tiles past L are skipped
// wave-uniformly (every wave reaches every barrier), keys >= L get probability exactly 0 and rows >= L
// of O, lse and dQKV are exact zeros. Without lengths L = S: the block skips and key masks are compiled
// out, and what is left (row < S) only keeps the waves of a 64-row last tile inside the tensors.
// Dropout keeps (b, h, q, key) by drop_keep over ((b*H + h)*S + q)*S + key with attn_key(seed, step) in
// all three kernels: one hash per key pair where a lane holds both keys of a pair (forward, dQ), one
// per element where the pair sits in two lanes (dK/dV) -- the same bits either way.
// Causal (CAUSAL instantiations, a.causal; always length-aware, L = S when a.lens is null): query q sees
// keys <= q and < L. Forward and dQ walk key chunks c < min(nck, 2 (qt + 1)) of query tile qt; a wave
// (32 queries from q0) computes only in chunks with 64 c <= q0, skips the 32-key block that starts
// past q0 and masks by element in the block that starts at q0 (blocks and q0 are multiples of 32, so
// a block lies before, on or after the wave's queries). dK/dV starts its query-chunk walk at chunk
// 2 kt, skips the 32-query block that ends before the wave's keys and writes exact zeros where
// query < key in the block on them. Every skip is wave-uniform and every wave reaches every barrier.
// Future rows inside the chunks walked are staged and multiplied: finite values there change nothing.
// Item map of the causal copies: a query tile qt costs about (qt + 1) of a key tile's chunks, and with
// items numbered (bh, tile) and a grid that is a multiple of the tile count every workgroup met the same
// tile index in all its items, so the workgroups with the last tile ran as long as the full kernel
// (measured: causal no faster than bidirectional at S = 256, 512). The causal copies number the items
// tile-major, heaviest first (qt descending for forward / dQ, kt ascending for dK/dV): a workgroup's
// items it, it + grid, .. then spread over the tiles. Only the item-to-workgroup map changes: every
// item is still computed whole by one workgroup, so no result depends on it.
// Documents (DOCS instantiations, a.doc; always causal): query q sees keys doc[q] <= key <= q (and < L);
// doc is clamped to [0, t] where it is read, only compared, and never read at a position >= L. Forward
// and dQ start the chunk walk of tile qt at the chunk of its first query's start; a wave computes only
// in the chunks that overlap [doc[q0], q0 + 31], skips the 32-key blocks that end before doc[q0] and
// masks keys < doc[q] by element. A wave can then compute a chunk in which some lanes see no key: while
// a lane's running max is -inf its alpha is 1 and its p is 0, by select (see the forward). dK/dV stops
// its query-chunk walk at the first chunk whose first query starts past the tile's last key (starts are
// monotone: so does every later chunk), skips the 32-query blocks whose first query starts past the
// wave's last key and writes exact zeros where key < doc[query]; the chunk's starts ride in LDS beside
// lse and D. With a.doc null the launchers pick the copies they picked before.
// Windows (WINDOW instantiations, a.window = W >= 1; always causal, with or without a.doc -- they test
// the pointer as the causal copies test a.lens): query q sees keys lb(q) <= key <= q (and < L) with
// lb(q) = max(doc[q], q - W + 1, 0) (attn_frag.h lb_of). They are the document copies with lb read
// wherever a document start is read: lb(q) <= q and lb is non-decreasing, which is all those walks and
// skips rely on. It is not a fixed point (lb(lb(q)) < lb(q)), and nothing needs one: lane 0 of a wave
// sees the key lb(q0) because lb(q0) <= q0, and any lane that sees no key of a chunk takes the selects.
// Skips, per 32-row block by the block's first query: forward / dQ never multiply a 32-key block that
// ends before lb(q0) (q0 the wave's first query), dK/dV never a 32-query block whose first query has
// lb > the wave's last key; chunks outside [lb(128 qt) >> 6, 2 qt + 1] (forward / dQ) or past the first
// query chunk with lb > 128 kt + 127 (dK/dV) are not even staged. W >= S is passed as S.
// With a.window == 0 the launchers pick the copies they picked before; the other instantiations
// contain no window code (if constexpr), and AttnArgs::window sits in former padding.
// Bias hand-over: bpart[(b * ceil(S/128) + tile)][3*H*64] gets the fp32 column sums of the item's dQ
// (dQ pass) and dK, dV (dK/dV pass), summed in a fixed order; launch_colsum_final reduces the rows.
#include <algorithm>

#include "common.h"
#include "cu_count.h"
#include "launchers_attn.h"
#include "attn_frag.h"

// No implicit fused multiply-adds below: whether `l * alpha + p` contracts depended on the surrounding
// branches, so the VARLEN copy at full lengths was not bitwise the full-length copy (lse differed in
// the last bit). Every FMA in this file is written as fmaf.
#pragma clang fp contract(off)

namespace psd {

namespace {

constexpr int KC = 64;                   // rows per streamed chunk
constexpr int TILE_B = KC * LDT * 2;     // bytes of one chunk tile [64][LDT] bf16 (9216)
constexpr int NT = 256;                  // 4 waves
constexpr int RLD = D + 1;               // fp32 row stride of the column-sum patch
constexpr int RED_B = 4 * 32 * RLD * 4;  // four waves' [32][RLD] fp32 patches (33,280 B, inside the 4 tiles)
constexpr float LOG2E = 1.4426950408889634f;

// bare v_exp_f32: exp2f() wraps it in a compare, two selects, an add and a v_ldexp per value to keep
// denormal results; a probability below 2^-126 may flush to zero here (-inf gives 0 either way)
__device__ __forceinline__ float aexp2(float x) { return __builtin_amdgcn_exp2f(x); }

// rows r0 .. r0 + 63 of a tensor with 64 contiguous bf16 per row -> two 16-B pieces per lane; rows >= L
// are not read (zeros instead)
__device__ __forceinline__ void fetch_rows(u32x4 (&r)[2], const uint16_t* src, int64_t row_stride, int r0, int L) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + i * NT, row = r0 + (c >> 3), ch = c & 7;
    u32x4 v = zero4();
    if (row < L) v = *reinterpret_cast<const u32x4*>(src + (int64_t)row * row_stride + ch * 8);
    r[i] = v;
  }
}
__device__ __forceinline__ void put_rows(uint8_t* tile, const u32x4 (&r)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int c = threadIdx.x + i * NT;
    *reinterpret_cast<u32x4*>(tile + (c >> 3) * LDT * 2 + (c & 7) * 16) = r[i];
  }
}
// this lane's B-operand fragments of row `row` (64 bf16 at p): k = 16 ks + 8 hh + e; zeros when !ok
__device__ __forceinline__ void lane_frags(abf16x8 (&f)[4], const uint16_t* p, bool ok, int hh) {
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    u32x4 v = zero4();
    if (ok) v = *reinterpret_cast<const u32x4*>(p + 16 * ks + 8 * hh);
    f[ks] = __builtin_bit_cast(abf16x8, v);
  }
}
__device__ __forceinline__ abf16x8 pack8(const float (&v)[8]) {
  return __builtin_bit_cast(abf16x8, u32x4{pack_bf16x2_rne(v[0], v[1]), pack_bf16x2_rne(v[2], v[3]),
                                           pack_bf16x2_rne(v[4], v[5]), pack_bf16x2_rne(v[6], v[7])});
}
// lane: row `row` (64 bf16 at out), d = 32 dt + acc_row(i): 4 consecutive d per 4 accumulators -> 8-B stores
__device__ __forceinline__ void store_row(uint16_t* out, const af32x16 (&t)[2], float mul, bool nz, int hh) {
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<uint2*>(out + 32 * dt + 8 * g + 4 * hh) =
          nz ? make_uint2(pack_bf16x2_rne(t[dt][4 * g] * mul, t[dt][4 * g + 1] * mul),
                          pack_bf16x2_rne(t[dt][4 * g + 2] * mul, t[dt][4 * g + 3] * mul))
             : make_uint2(0u, 0u);
}
// sum over this wave's 32 rows (lane % 32) of t[d][row], returned for d = lane: through the wave's own
// fp32 patch of LDS, rows added in a fixed order. Called by every wave of the workgroup together.
__device__ __forceinline__ float wave_colsum(float* red, const af32x16 (&t)[2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5;
  float* mine = red + w * 32 * RLD;
#pragma unroll
  for (int dt = 0; dt < 2; ++dt)
#pragma unroll
    for (int i = 0; i < 16; ++i) mine[(lane & 31) * RLD + 32 * dt + acc_row(i, hh)] = t[dt][i];
  __syncthreads();
  float s = 0.f;
#pragma unroll 8
  for (int r = 0; r < 32; ++r) s += mine[r * RLD + lane];
  __syncthreads();
  return s;
}

}  // namespace

// Forward. Persistent over items (bh, query tile); LDS: K and V chunk tiles, two buffers.
template <bool VARLEN, bool CAUSAL, bool DOCS = false, bool WINDOW = false>
__global__ __launch_bounds__(NT) void attn_long_fwd_kernel(AttnArgs a) {
  static_assert(VARLEN || !CAUSAL, "the causal copy is length-aware");
  static_assert(CAUSAL || !DOCS, "the document copy is causal");
  static_assert(DOCS || !WINDOW, "the window copy is the document copy with lb_of for the start");
  __shared__ __attribute__((aligned(16))) uint8_t smem[4 * TILE_B];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5;
  const int S = a.S, HD = a.H * D;
  const int64_t qkv_rs = 3 * (int64_t)HD;
  const int nqt = (S + 127) >> 7;
  const int nitems = a.B * a.H * nqt;
  const float sl = a.scale * LOG2E;
  const uint32_t key = attn_key(a.seed, a.step);
  const bool drop = a.thresh != 0u;

  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    int bh = it / nqt, qt = it - bh * nqt;
    if constexpr (CAUSAL) {  // tile qt costs ~(qt + 1) chunks: the heavy tiles first, see item map above
      bh = it % (a.B * a.H);
      qt = nqt - 1 - it / (a.B * a.H);
    }
    const int b = bh / a.H, h = bh - b * a.H;
    const int L = item_len<VARLEN, CAUSAL>(a, b, S);
    const int q0 = 128 * qt + 32 * w, q = q0 + (lane & 31);
    const bool live = q0 < L;  // this wave has a valid query (wave-uniform)
    const bool vq = q < L;
    int nck = 128 * qt < L ? (L + KC - 1) / KC : 0;  // key chunks with a valid key; none for a padded tile
    if (CAUSAL) nck = min(nck, 2 * (qt + 1));        // and with a key <= the tile's last query
    const uint16_t* base = a.qkv + (int64_t)b * S * qkv_rs + h * D;
    // DOCS: the tile's first chunk (the start of its first query's document; that query is valid when
    // nck > 0), the starts of the wave's first and last valid query (wave-uniform) and the lane's own
    // (a padded query: doc is not read, start 0). WINDOW: the same with the lower bound lb_of for the
    // start; all that is used of it is lb(t) <= t and that it does not decrease with t. (Loading the first chunk index one item ahead, so that
    // the first K / V fetch does not wait for it, measured 1 % slower forward + backward: not done.)
    int c0 = 0, dlo = 0, dhi = 0, dq = 0;
    if constexpr (DOCS) {
      if (nck > 0) c0 = lb_of<DOCS, WINDOW>(a, b, S, 128 * qt) >> 6;
      if (vq) dq = lb_of<DOCS, WINDOW>(a, b, S, q);
      if (live) {
        dlo = __builtin_amdgcn_readfirstlane(dq);
        dhi = __builtin_amdgcn_readlane(dq, __builtin_amdgcn_readfirstlane(min(31, L - 1 - q0)));
      }
    }

    abf16x8 qf[4];
    lane_frags(qf, base + (int64_t)q * qkv_rs, vq, hh);
    u32x4 pk[2], pv[2];
    if (nck > 0) {  // the first chunk walked, into its own buffer
      fetch_rows(pk, base + HD, qkv_rs, KC * c0, L);
      fetch_rows(pv, base + 2 * HD, qkv_rs, KC * c0, L);
      put_rows(smem + (c0 & 1) * 2 * TILE_B, pk);
      put_rows(smem + (c0 & 1) * 2 * TILE_B + TILE_B, pv);
    }
    __syncthreads();

    float m = -INFINITY, l = 0.f;  // l: this lane half's share of the row sum
    af32x16 ot[2] = {zero16(), zero16()};
    const uint64_t rowidx = ((uint64_t)bh * S + q) * S;
    for (int c = c0; c < nck; ++c) {
      const uint8_t* Ks = smem + (c & 1) * 2 * TILE_B;
      const uint8_t* Vs = Ks + TILE_B;
      const bool more = c + 1 < nck;
      if (more) {  // in flight during this chunk's products
        fetch_rows(pk, base + HD, qkv_rs, KC * (c + 1), L);
        fetch_rows(pv, base + 2 * HD, qkv_rs, KC * (c + 1), L);
      }
      // causal: a wave computes in chunks with 64 c <= q0 only and leaves m, l, ot alone in the others
      // (documents: nor in a chunk that ends before the start of its first query's document)
      if (live && (!CAUSAL || KC * c <= q0) && (!DOCS || KC * c + KC - 1 >= dlo)) {
        const int kb0 = KC * c;
        af32x16 sc[2];  // S^T tiles: lane owns query q, keys kb0 + 32 j + acc_row(i)
        float cm = -INFINITY;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (VARLEN && kb0 + 32 * j >= L) continue;
          if (CAUSAL && kb0 + 32 * j > q0) continue;  // every key of the block is past the wave's queries
          if (DOCS && kb0 + 32 * j + 31 < dlo) continue;  // or before the documents of all of them
          // end of the keys this lane's query sees: L, and q + 1 in the block on the diagonal
          const int kend = CAUSAL && kb0 + 32 * j == q0 ? min(L, q + 1) : L;
          // first key this lane's query sees: its document's start, in the blocks that hold a key before
          // the largest start of the wave; 0 (no test) elsewhere
          const int kbeg = DOCS && kb0 + 32 * j < dhi ? dq : 0;
          sc[j] = zero16();
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) sc[j] = mfma(rowfrag(Ks, LDT * 2, 32 * j, 16 * ks), qf[ks], sc[j]);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            if (VARLEN && kb0 + 32 * j + acc_row(i, hh) >= kend) sc[j][i] = -INFINITY;  // leaves the max and the sum
            if (DOCS && kb0 + 32 * j + acc_row(i, hh) < kbeg) sc[j][i] = -INFINITY;
            cm = fmaxf(cm, sc[j][i]);
          }
        }
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        // key kb0 is valid in every chunk walked, so cm is finite; m = -inf on the first chunk gives alpha 0.
        // Causal: per wave, a chunk is computed only when kb0 = 64 c <= q0 (q0 a multiple of 32, 64 c of 64),
        // and then key kb0 <= q0 <= q is visible to every query of the wave and kb0 <= q0 < L: cm stays finite
        // Documents: a wave computes a chunk in which some lanes see no key (a document that starts inside
        // the wave's queries: the earlier queries see the chunk before it, the later ones do not). Their m
        // and cm are both -inf and (m - mn), (s - m) would be NaN: by select, alpha = 1 and p = 0 while the
        // lane's running max is -inf (l and ot are still zero then). A lane with a finite max takes the
        // arithmetic above unchanged. A valid query sees itself, so no lane ends with m = -inf.
        // Windows: the same lanes, and more of them (with W < 32 most lanes of a wave see no key of the
        // first block it computes); the two selects below test every lane's own m, whatever its start is.
        const float mn = fmaxf(m, cm);
        float alpha = aexp2((m - mn) * sl);
        if constexpr (DOCS) {
          if (mn == -INFINITY) alpha = 1.f;
        }
        m = mn;
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
          for (int i = 0; i < 16; ++i) ot[dt][i] *= alpha;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (VARLEN && kb0 + 32 * j >= L) continue;
          if (CAUSAL && kb0 + 32 * j > q0) continue;
          if (DOCS && kb0 + 32 * j + 31 < dlo) continue;
#pragma unroll
          for (int ks2 = 0; ks2 < 2; ++ks2) {
            float v[8];
            bool kp[8];
            if (drop) {  // elements e, e + 1 (e even) are keys kk, kk + 1 with kk even: one hash per pair
#pragma unroll
              for (int e = 0; e < 8; e += 2)
                akeep2(key, rowidx + kb0 + 32 * j + acc_row(8 * ks2 + e, hh), a.thresh, kp[e], kp[e + 1]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              float p = aexp2((sc[j][8 * ks2 + e] - m) * sl);
              if constexpr (DOCS) {
                if (m == -INFINITY) p = 0.f;
              }
              l += p;
              v[e] = p;
              if (drop) v[e] = kp[e] ? p * a.rescale : 0.f;
            }
            const abf16x8 pb = pack8(v);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) ot[dt] = mfma(trfrag_accrows(Vs, LDT * 2, 32 * j + 16 * ks2, 32 * dt), pb, ot[dt]);
          }
        }
      }
      if (more) {
        uint8_t* nx = smem + ((c + 1) & 1) * 2 * TILE_B;
        put_rows(nx, pk);
        put_rows(nx + TILE_B, pv);
      }
      __syncthreads();  // the next chunk staged; this chunk read by every wave
    }
    if (q0 < S) {  // (a 64-query last tile leaves waves 2, 3 without rows)
      float lse = 0.f, inv = 0.f;
      if (live) {
        l += __shfl_xor(l, 32);
        inv = 1.f / l;
        lse = m * a.scale + logf(l);
      }
      if (hh == 0) a.lse[(int64_t)bh * S + q] = vq ? lse : 0.f;
      store_row(a.o + ((int64_t)b * S + q) * HD + h * D, ot, inv, vq, hh);
    }
  }
}

// Backward, dQ pass: the forward's item and orientation; also writes D = rowsum(dO . O) to dsum.
template <bool VARLEN, bool CAUSAL, bool DOCS = false, bool WINDOW = false>
__global__ __launch_bounds__(NT) void attn_long_dq_kernel(AttnArgs a, float* __restrict__ dsum) {
  static_assert(VARLEN || !CAUSAL, "the causal copy is length-aware");
  static_assert(CAUSAL || !DOCS, "the document copy is causal");
  static_assert(DOCS || !WINDOW, "the window copy is the document copy with lb_of for the start");
  __shared__ __attribute__((aligned(16))) uint8_t smem[4 * TILE_B];
  float* red = reinterpret_cast<float*>(smem);
  float* cs_s = reinterpret_cast<float*>(smem + RED_B);  // [4][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5;
  const int S = a.S, HD = a.H * D;
  const int64_t qkv_rs = 3 * (int64_t)HD;
  const int nqt = (S + 127) >> 7;
  const int nitems = a.B * a.H * nqt;
  const float sl = a.scale * LOG2E;
  const uint32_t key = attn_key(a.seed, a.step);
  const bool drop = a.thresh != 0u;

  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    int bh = it / nqt, qt = it - bh * nqt;
    if constexpr (CAUSAL) {  // tile qt costs ~(qt + 1) chunks: the heavy tiles first, see item map above
      bh = it % (a.B * a.H);
      qt = nqt - 1 - it / (a.B * a.H);
    }
    const int b = bh / a.H, h = bh - b * a.H;
    const int L = item_len<VARLEN, CAUSAL>(a, b, S);
    const int q0 = 128 * qt + 32 * w, q = q0 + (lane & 31);
    const bool live = q0 < L;
    const bool vq = q < L;
    int nck = 128 * qt < L ? (L + KC - 1) / KC : 0;
    if (CAUSAL) nck = min(nck, 2 * (qt + 1));
    const uint16_t* base = a.qkv + (int64_t)b * S * qkv_rs + h * D;
    // DOCS: the tile's first chunk (the start of its first query's document; that query is valid when
    // nck > 0), the starts of the wave's first and last valid query (wave-uniform) and the lane's own
    // (a padded query: doc is not read, start 0). WINDOW: the same with the lower bound lb_of for the
    // start; all that is used of it is lb(t) <= t and that it does not decrease with t. (Loading the first chunk index one item ahead, so that
    // the first K / V fetch does not wait for it, measured 1 % slower forward + backward: not done.)
    int c0 = 0, dlo = 0, dhi = 0, dq = 0;
    if constexpr (DOCS) {
      if (nck > 0) c0 = lb_of<DOCS, WINDOW>(a, b, S, 128 * qt) >> 6;
      if (vq) dq = lb_of<DOCS, WINDOW>(a, b, S, q);
      if (live) {
        dlo = __builtin_amdgcn_readfirstlane(dq);
        dhi = __builtin_amdgcn_readlane(dq, __builtin_amdgcn_readfirstlane(min(31, L - 1 - q0)));
      }
    }
    const int64_t orow = ((int64_t)b * S + q) * HD + h * D;

    abf16x8 qf[4], dof[4];
    lane_frags(qf, base + (int64_t)q * qkv_rs, vq, hh);
    lane_frags(dof, a.dout + orow, vq, hh);
    float Dq = 0.f, lse2 = 0.f;
    {
      abf16x8 of[4];
      lane_frags(of, a.o + orow, vq, hh);
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) Dq = fmaf((float)dof[ks][e], (float)of[ks][e], Dq);
      Dq += __shfl_xor(Dq, 32);
      if (vq) {
        lse2 = a.lse[(int64_t)bh * S + q] * LOG2E;
        if (hh == 0) dsum[(int64_t)bh * S + q] = Dq;
      }
    }
    u32x4 pk[2], pv[2];
    if (nck > 0) {  // the first chunk walked, into its own buffer
      fetch_rows(pk, base + HD, qkv_rs, KC * c0, L);
      fetch_rows(pv, base + 2 * HD, qkv_rs, KC * c0, L);
      put_rows(smem + (c0 & 1) * 2 * TILE_B, pk);
      put_rows(smem + (c0 & 1) * 2 * TILE_B + TILE_B, pv);
    }
    __syncthreads();

    af32x16 dqt[2] = {zero16(), zero16()};  // dQ^T: lane owns query q, d = 32 dt + acc_row(i)
    const uint64_t rowidx = ((uint64_t)bh * S + q) * S;
    for (int c = c0; c < nck; ++c) {
      const uint8_t* Ks = smem + (c & 1) * 2 * TILE_B;
      const uint8_t* Vs = Ks + TILE_B;
      const bool more = c + 1 < nck;
      if (more) {
        fetch_rows(pk, base + HD, qkv_rs, KC * (c + 1), L);
        fetch_rows(pv, base + 2 * HD, qkv_rs, KC * (c + 1), L);
      }
      if (live && (!CAUSAL || KC * c <= q0) && (!DOCS || KC * c + KC - 1 >= dlo)) {
        const int kb0 = KC * c;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          if (VARLEN && kb0 + 32 * j >= L) continue;
          if (CAUSAL && kb0 + 32 * j > q0) continue;  // every key of the block is past the wave's queries
          if (DOCS && kb0 + 32 * j + 31 < dlo) continue;  // or before the documents of all of them
          const int kend = CAUSAL && kb0 + 32 * j == q0 ? min(L, q + 1) : L;  // as in the forward
          const int kbeg = DOCS && kb0 + 32 * j < dhi ? dq : 0;
          af32x16 st = zero16(), dpt = zero16();
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            st = mfma(rowfrag(Ks, LDT * 2, 32 * j, 16 * ks), qf[ks], st);
            dpt = mfma(rowfrag(Vs, LDT * 2, 32 * j, 16 * ks), dof[ks], dpt);
          }
#pragma unroll
          for (int ks2 = 0; ks2 < 2; ++ks2) {
            float v[8];
            bool kp[8];
            if (drop) {
#pragma unroll
              for (int e = 0; e < 8; e += 2)
                akeep2(key, rowidx + kb0 + 32 * j + acc_row(8 * ks2 + e, hh), a.thresh, kp[e], kp[e + 1]);
            }
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int i = 8 * ks2 + e;
              const float p = aexp2(fmaf(st[i], sl, -lse2));
              float dp = dpt[i];
              if (drop) dp = kp[e] ? dp * a.rescale : 0.f;
              v[e] = p * (dp - Dq);
              if constexpr (VARLEN) {  // masked key or padded query: exact zero
                if (!vq || kb0 + 32 * j + acc_row(i, hh) >= kend) v[e] = 0.f;
              }
              if constexpr (DOCS) {  // a key of an earlier document
                if (kb0 + 32 * j + acc_row(i, hh) < kbeg) v[e] = 0.f;
              }
            }
            const abf16x8 dsb = pack8(v);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) dqt[dt] = mfma(trfrag_accrows(Ks, LDT * 2, 32 * j + 16 * ks2, 32 * dt), dsb, dqt[dt]);
          }
        }
      }
      if (more) {
        uint8_t* nx = smem + ((c + 1) & 1) * 2 * TILE_B;
        put_rows(nx, pk);
        put_rows(nx + TILE_B, pv);
      }
      __syncthreads();
    }
    if (q0 < S) store_row(a.dqkv + ((int64_t)b * S + q) * qkv_rs + h * D, dqt, a.scale, vq, hh);
    if (a.bpart) {  // column sums of this tile's dQ (waves without a valid query hold zeros), waves in order
      const float s = wave_colsum(red, dqt);
      cs_s[w * 64 + lane] = s;
      __syncthreads();
      if (threadIdx.x < 64) {
        float acc = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) acc += cs_s[ww * 64 + threadIdx.x];
        a.bpart[((int64_t)b * nqt + qt) * 3 * HD + h * D + threadIdx.x] = acc * a.scale;
      }
      __syncthreads();  // the patch is the next item's chunk buffer
    }
  }
}

// Backward, dK/dV pass: item (bh, 128-key tile), the key on the lane. LDS: Q and dO chunk tiles, two
// buffers, plus the chunk's lse and D.
template <bool VARLEN, bool CAUSAL, bool DOCS = false, bool WINDOW = false>
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(2))) void attn_long_dkv_kernel(AttnArgs a, const float* __restrict__ dsum) {
  static_assert(VARLEN || !CAUSAL, "the causal copy is length-aware");
  static_assert(CAUSAL || !DOCS, "the document copy is causal");
  static_assert(DOCS || !WINDOW, "the window copy is the document copy with lb_of for the start");
  constexpr int NR = DOCS ? 3 : 2;  // per-row values of a chunk: lse, D and (DOCS) the document start / lower bound
  __shared__ __attribute__((aligned(16))) uint8_t smem[4 * TILE_B + 2 * NR * KC * 4];
  float* row_s = reinterpret_cast<float*>(smem + 4 * TILE_B);  // [buf][lse, D(, doc)][64]
  float* red = reinterpret_cast<float*>(smem);
  float* cs_s = reinterpret_cast<float*>(smem + RED_B);  // [4][2][64]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, hh = lane >> 5;
  const int S = a.S, HD = a.H * D;
  const int64_t qkv_rs = 3 * (int64_t)HD;
  const int nkt = (S + 127) >> 7;
  const int nitems = a.B * a.H * nkt;
  const float sl = a.scale * LOG2E;
  const uint32_t key = attn_key(a.seed, a.step);
  const bool drop = a.thresh != 0u;

  for (int it = blockIdx.x; it < nitems; it += gridDim.x) {
    int bh = it / nkt, kt = it - bh * nkt;
    if constexpr (CAUSAL) {  // key tile kt is seen by the query chunks from 2 kt on: the heavy tiles first
      bh = it % (a.B * a.H);
      kt = it / (a.B * a.H);
    }
    const int b = bh / a.H, h = bh - b * a.H;
    const int L = item_len<VARLEN, CAUSAL>(a, b, S);
    const int k0 = 128 * kt + 32 * w, kg = k0 + (lane & 31);
    const bool live = k0 < L;  // this wave has a valid key (wave-uniform)
    const bool vk = kg < L;
    const int nqc = 128 * kt < L ? (L + KC - 1) / KC : 0;  // query chunks with a valid row
    const uint16_t* base = a.qkv + (int64_t)b * S * qkv_rs + h * D;
    const uint16_t* dob = a.dout + (int64_t)b * S * HD + h * D;

    abf16x8 kf[4], vf[4];
    lane_frags(kf, base + HD + (int64_t)kg * qkv_rs, vk, hh);
    lane_frags(vf, base + 2 * HD + (int64_t)kg * qkv_rs, vk, hh);
    u32x4 pq[2], pd[2];
    float pr = 0.f;
    auto fetch = [&](int c) {
      fetch_rows(pq, base, qkv_rs, KC * c, L);
      fetch_rows(pd, dob, HD, KC * c, L);
      if (threadIdx.x < 2 * KC) {
        const int r = KC * c + (threadIdx.x & (KC - 1));
        pr = r < L ? (threadIdx.x < KC ? a.lse : dsum)[(int64_t)bh * S + r] : 0.f;
      }
      if constexpr (DOCS) {  // the third wave: the chunk's document starts (as int bits; zeros past L)
        if (threadIdx.x >= 2 * KC && threadIdx.x < 3 * KC) {
          const int r = KC * c + (threadIdx.x & (KC - 1));
          pr = __int_as_float(r < L ? lb_of<DOCS, WINDOW>(a, b, S, r) : 0);
        }
      }
    };
    auto put = [&](int bf) {
      put_rows(smem + bf * 2 * TILE_B, pq);
      put_rows(smem + bf * 2 * TILE_B + TILE_B, pd);
      if (threadIdx.x < NR * KC) row_s[bf * NR * KC + threadIdx.x] = pr;
    };
    const int c0 = CAUSAL ? 2 * kt : 0;  // causal: queries before the key tile see none of it (c0 < nqc when nqc > 0)
    // DOCS: the walk stops at the first chunk whose first query's document starts past the tile's last
    // key; monotone starts make every later chunk invisible too (WINDOW: its lower bound, monotone as
    // well). Lane c tests chunk c: 64 lanes, so at most 64 chunks -- S <= 4096, which attn_long_supported
    // guarantees and the launchers check.
    int cend = nqc;
    if constexpr (DOCS) {
      const bool past = lane >= c0 && lane < nqc && lb_of<DOCS, WINDOW>(a, b, S, KC * lane) > 128 * kt + 127;  // 64 lane < L
      const uint64_t bal = __ballot(past);
      if (bal) cend = __ffsll((unsigned long long)bal) - 1;
    }
    if (nqc > 0) {
      fetch(c0);
      put(c0 & 1);
    }
    __syncthreads();

    af32x16 dvt[2] = {zero16(), zero16()}, dkt[2] = {zero16(), zero16()};  // lane owns key kg, d = 32 dt + acc_row(i)
    for (int c = c0; c < (DOCS ? cend : nqc); ++c) {
      const uint8_t* Qs = smem + (c & 1) * 2 * TILE_B;
      const uint8_t* dOs = Qs + TILE_B;
      const float* lse_s = row_s + (c & 1) * NR * KC;
      const float* D_s = lse_s + KC;
      const int* doc_s = reinterpret_cast<const int*>(D_s + KC);  // DOCS only
      const bool more = c + 1 < (DOCS ? cend : nqc);
      if (more) fetch(c + 1);
      if (live) {
        const int qb0 = KC * c;
        // (rolled, and two waves per SIMD asked for: unrolled the compiler interleaves both query blocks
        // and takes 256 + ~200 registers, one wave per SIMD)
#pragma unroll 1
        for (int j = 0; j < 2; ++j) {
          if (VARLEN && qb0 + 32 * j >= L) continue;
          if (CAUSAL && qb0 + 32 * j < k0) continue;  // every query of the block is before the wave's keys
          if constexpr (DOCS) {  // or its first query's (so every query's) document starts past them
            if (__builtin_amdgcn_readfirstlane(doc_s[32 * j]) > k0 + 31) continue;
          }
          const int qfirst = CAUSAL && qb0 + 32 * j == k0 ? kg : 0;  // first query that sees this lane's key
          af32x16 st = zero16(), dpt = zero16();  // S and dP: rows = queries qb0 + 32 j + acc_row(i), col = key kg
#pragma unroll
          for (int ks = 0; ks < 4; ++ks) {
            st = mfma(rowfrag(Qs, LDT * 2, 32 * j, 16 * ks), kf[ks], st);
            dpt = mfma(rowfrag(dOs, LDT * 2, 32 * j, 16 * ks), vf[ks], dpt);
          }
#pragma unroll
          for (int ks2 = 0; ks2 < 2; ++ks2) {
            float pv[8], dv[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
              const int i = 8 * ks2 + e;
              const int ql = 32 * j + acc_row(i, hh), qg = qb0 + ql;
              const float p = aexp2(fmaf(st[i], sl, -(lse_s[ql] * LOG2E)));
              float pdv = p, dp = dpt[i];
              if (drop) {  // the pair's other key is the neighbouring lane's: one hash per element, same bits
                const bool kp = drop_keep(key, ((uint64_t)bh * S + qg) * S + kg, a.thresh);
                pdv = kp ? p * a.rescale : 0.f;
                dp = kp ? dp * a.rescale : 0.f;
              }
              pv[e] = pdv;
              dv[e] = p * (dp - D_s[ql]);
              if constexpr (VARLEN) {  // masked key or padded query: exact zeros
                if (!vk || qg >= L || (CAUSAL && qg < qfirst)) pv[e] = dv[e] = 0.f;
              }
              if constexpr (DOCS) {  // the key is of an earlier document than the query
                if (kg < doc_s[ql]) pv[e] = dv[e] = 0.f;
              }
            }
            const abf16x8 pb = pack8(pv), dsb = pack8(dv);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
              dvt[dt] = mfma(trfrag_accrows(dOs, LDT * 2, 32 * j + 16 * ks2, 32 * dt), pb, dvt[dt]);
              dkt[dt] = mfma(trfrag_accrows(Qs, LDT * 2, 32 * j + 16 * ks2, 32 * dt), dsb, dkt[dt]);
            }
          }
        }
      }
      if (more) put((c + 1) & 1);
      __syncthreads();
    }
    if (k0 < S) {
      uint16_t* out = a.dqkv + ((int64_t)b * S + kg) * qkv_rs + h * D;
      store_row(out + HD, dkt, a.scale, vk, hh);
      store_row(out + 2 * HD, dvt, 1.f, vk, hh);
    }
    if (a.bpart) {
      const float sk = wave_colsum(red, dkt);
      const float sv = wave_colsum(red, dvt);
      cs_s[(w * 2 + 0) * 64 + lane] = sk * a.scale;
      cs_s[(w * 2 + 1) * 64 + lane] = sv;
      __syncthreads();
      if (threadIdx.x < 128) {
        const int t = threadIdx.x >> 6, d = threadIdx.x & 63;
        float acc = 0.f;
#pragma unroll
        for (int ww = 0; ww < 4; ++ww) acc += cs_s[(ww * 2 + t) * 64 + d];
        a.bpart[((int64_t)b * nkt + kt) * 3 * HD + (1 + t) * HD + h * D + d] = acc;
      }
      __syncthreads();
    }
  }
}

// S <= 4096: 64 chunks of 64 rows, one per lane of the dK/dV pass's ballot over the chunks (the only
// structure here with a size limit; every row, pair and partial index is 64-bit)
bool attn_long_supported(int S, int head_dim) { return head_dim == D && S > 128 && S <= 4096 && S % 64 == 0; }
int attn_long_bpart_rows(int B, int S) { return B * ((S + 127) / 128); }

template <typename K, typename... Extra>
static hipError_t launch_long(K kernel, const AttnArgs& a, hipStream_t st, Extra... extra) {
  if ((a.doc || a.window) && !a.causal) return hipErrorInvalidValue;
  if (a.window < 0) return hipErrorInvalidValue;
  // persistent: the resident workgroups per CU (registers / LDS), each walks items it, it + grid, ...
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), NT, 0) != hipSuccess || per_cu < 1)
    per_cu = 1;
  const int64_t nitems = (int64_t)a.B * a.H * ((a.S + 127) / 128);
  int grid = (int)std::min<int64_t>(nitems, (int64_t)per_cu * cu_count());
  if (a.grid_cap > 0) grid = std::min(grid, a.grid_cap);
  if (grid < 1) return hipSuccess;
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(NT), 0, st, a, extra...);
  return hipGetLastError();
}

// (VARLEN, CAUSAL, DOCS, WINDOW): full length, lengths, causal (with or without lengths), causal with
// documents, causal with a window (with or without documents); with a.window == 0 the choice is the one
// made before the window copies existed, without a.doc the one before the document copies
#define PSD_ATTN_LONG_PICK(k, ...)                                               \
  (a.window ? launch_long(&k<true, true, true, true>, a, st __VA_OPT__(, ) __VA_ARGS__) \
   : a.doc ? launch_long(&k<true, true, true>, a, st __VA_OPT__(, ) __VA_ARGS__)    \
   : a.causal ? launch_long(&k<true, true>, a, st __VA_OPT__(, ) __VA_ARGS__)    \
            : a.lens ? launch_long(&k<true, false>, a, st __VA_OPT__(, ) __VA_ARGS__) \
                     : launch_long(&k<false, false>, a, st __VA_OPT__(, ) __VA_ARGS__))

hipError_t launch_attn_long_fwd(const AttnArgs& a, hipStream_t st) {
  if (!attn_long_supported(a.S, D)) return hipErrorInvalidValue;
  return PSD_ATTN_LONG_PICK(attn_long_fwd_kernel);
}
hipError_t launch_attn_long_bwd(const AttnArgs& a, float* dsum, hipStream_t st) {
  if (!attn_long_supported(a.S, D) || !dsum) return hipErrorInvalidValue;
  hipError_t e = PSD_ATTN_LONG_PICK(attn_long_dq_kernel, dsum);
  if (e != hipSuccess) return e;
  return PSD_ATTN_LONG_PICK(attn_long_dkv_kernel, (const float*)dsum);
}

#undef PSD_ATTN_LONG_PICK

}  // namespace psd
