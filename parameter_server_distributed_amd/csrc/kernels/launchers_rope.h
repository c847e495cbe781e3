// Launch API of the rotary position embedding pass for gfx950 (kernels/rope.hip).
//
// Like everything in launchers.h: raw pointers, explicit stream, no allocation, no synchronisation,
// no memcpy, legal under stream capture.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {

// Rotates, in place, the Q and K heads of a packed qkv [B, S, 3, H, 64] bf16 (rotate-half pairs
// (i, i + 32) of each head) by the angle of the row's position, read from the fp32 tables; the V third
// is never touched.
struct RopeArgs {
  uint16_t* qkv;        // [B, S, 3, H, 64] bf16, 16-byte aligned
  const float* cos;     // [P, 32] fp32, P >= S, 16-byte aligned
  const float* sin;     // [P, 32] fp32
  const int32_t* lens;  // [B] or null: rows t >= clamp(lens[b], 0, S) are neither read nor written
  const int32_t* doc;   // [B, S] or null: position t - clamp(doc[b, t], 0, t); entries at rows past a
                        // length are never read. Without it the position is t
  int32_t B, S, H;
  int32_t inverse;      // != 0: the angle negated (the backward)
  int32_t blocks;       // 0: the launcher's own grid; > 0: at most this many workgroups
};
hipError_t launch_rope(const RopeArgs& a, hipStream_t stream);

}  // namespace psd
