#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {
// The pre-norm residual step r_new = r + dropout_p(h), y = RMSNorm(r_new) * gamma over rows of H
// (kernels/rmsnorm.hip) and its backward.
struct RmsArgs {
  const uint16_t* r;       // fwd: residual stream in [rows, H] bf16
  const uint16_t* h;       // fwd: branch output or null (then r_new is r: nothing added, nothing written)
  const uint16_t* gamma;   // [H] bf16
  uint16_t* r_new;         // fwd out [rows, H] (unused without h)
  uint16_t* y;             // fwd out [rows, H]
  float* rstd;             // fwd out [rows]
  const uint16_t* dy;      // bwd in [rows, H]
  const uint16_t* dr_new;  // bwd in or null (zero): the gradient arriving at the residual stream
  const uint16_t* rn;      // bwd in: r_new as stored
  const float* rstd_in;    // bwd in [rows]
  uint16_t* dr;            // bwd out [rows, H]
  uint16_t* dh;            // bwd out [rows, H] or null (no h, or p == 0: dh is dr)
  uint16_t* dgamma;        // bwd out [H] bf16 (may be the PS gradient sink)
  float* part;             // bwd workspace [rms_bwd_blocks(rows)][H] fp32
  const int64_t* step;     // device step counter mixed into the dropout hash (may be null)
  int64_t rows;
  int32_t H;
  float eps;
  float p;                 // dropout probability (0: identity)
  uint32_t seed;           // per call site
};
bool rms_supported(int H);
int rms_fwd_blocks(int64_t rows);
int rms_bwd_blocks(int64_t rows);
hipError_t launch_rms_fwd(const RmsArgs& a, hipStream_t stream);
hipError_t launch_rms_bwd(const RmsArgs& a, hipStream_t stream);
}  // namespace psd
