// Launch API of the gated SiLU activation (SwiGLU) between the FFN's two GEMMs for gfx950
// (kernels/swiglu.hip).
//
// Like everything in launchers.h: raw pointers, explicit stream, no allocation, no synchronisation,
// no memcpy, legal under stream capture.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {

// gu [T, 2F] bf16 is the packed output of the gate/up GEMM, read in place: gate g = columns [0, F), up
// u = columns [F, 2F). Forward a = silu(g) * u [T, F]; backward dgu [T, 2F] = (dg | du) from da and gu.
struct SwigluArgs {
  const uint16_t* gu;  // [T, 2F] bf16, 16-byte aligned
  const uint16_t* da;  // bwd in [T, F] bf16
  uint16_t* a;         // fwd out [T, F] bf16
  uint16_t* dgu;       // bwd out [T, 2F] bf16
  int64_t T;
  int64_t F;           // F % 8 == 0
  int32_t blocks;      // 0: the launcher's own grid; > 0: at most this many workgroups
};
hipError_t launch_swiglu_fwd(const SwigluArgs& a, hipStream_t stream);
hipError_t launch_swiglu_bwd(const SwigluArgs& a, hipStream_t stream);

}  // namespace psd
