#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {
// Fused self-attention (kernels/attention.hip for S <= 128, attention_long.hip above): packed qkv [B, S, 3, H, 64] in,
// o [B, S, H, 64] out; backward writes the packed dqkv.
struct AttnArgs {
  const uint16_t* qkv;    // [B, S, 3, H, 64] bf16
  uint16_t* o;            // fwd out / bwd in: [B, S, H, 64] bf16
  float* lse;             // fwd out / bwd in: [B, H, S] fp32 (natural-log row log-sum-exp)
  const uint16_t* dout;   // bwd in: [B, S, H, 64] bf16
  uint16_t* dqkv;         // bwd out: [B, S, 3, H, 64] bf16
  float* bpart;           // bwd out or null: [B][3*H*64] fp32 column sums of dqkv over each sequence
                          // (the QKV Linear's bias gradient, summed over B by the caller)
  const int64_t* step;    // device step counter mixed into the dropout hash (may be null)
  int32_t B, S, H;
  float scale;            // softmax scale (1/sqrt(64))
  uint32_t thresh;        // dropout: drop when hash < thresh (0: no dropout)
  float rescale;          // 1 / (1 - p)
  uint32_t seed;
  int32_t window;         // 0: off; W >= 1 (causal only): query q sees keys max(doc[b, q], q - W + 1, 0) <= key <= q,
                          // W keys with itself; the WINDOW copies of the streaming kernels, with or without doc.
                          // (Sits in what was padding before the pointer below: no other field moved.)
  const int32_t* lens;   // [B] device lengths or null (every sequence full): sequence b has valid rows
                          // 0 .. clamp(lens[b], 0, S) - 1; read by the kernel only, never by the host
  int32_t grid_cap;       // 0: the launcher's own grid; > 0: at most this many (persistent) workgroups
  int32_t causal;         // != 0: query q sees keys <= q only (and < its length, with lens); the CAUSAL copies
  const int32_t* doc;     // [B, S] device document starts or null (off); causal only: query q sees keys
                          // doc[b, q] <= key <= q. Clamped to [0, t] and only compared on the device, entries
                          // at positions >= the length are never read; the DOCS copies
};
bool attn_supported(int S, int head_dim);
hipError_t launch_attn_fwd(const AttnArgs& a, hipStream_t stream);
hipError_t launch_attn_bwd(const AttnArgs& a, hipStream_t stream);

// Streaming kernels for 128 < S <= 4096, S % 64 == 0 (kernels/attention_long.hip): the same AttnArgs and
// contracts, except that bpart has attn_long_bpart_rows(B, S) rows of [3*H*64] (one per 128-row tile
// of a sequence) and backward takes an fp32 [B, H, S] scratch for D = rowsum(dO . O). Only they serve
// a.window (the whole-head launchers refuse it).
bool attn_long_supported(int S, int head_dim);
int attn_long_bpart_rows(int B, int S);
hipError_t launch_attn_long_fwd(const AttnArgs& a, hipStream_t stream);
hipError_t launch_attn_long_bwd(const AttnArgs& a, float* dsum, hipStream_t stream);
}  // namespace psd
