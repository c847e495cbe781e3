// Launch API of the fused softmax cross-entropy (xent.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {
// per row r of bf16 logits x [rows][ldx] (V valid columns): lse[r] and loss_row[r] = lse - x[label];
// lse_lo[r] (may be null): what the fp32 sum max + log(sum exp) rounded away, lse + lse_lo being the
// log-sum-exp to about 2^-24 of log(sum exp) instead of 2^-24 of |lse|
hipError_t launch_xent_fwd(const uint16_t* x, const int64_t* labels, int64_t rows, int64_t V, int64_t ldx, float* lse,
                           float* lse_lo, float* loss_row, hipStream_t stream);
// dx [rows][V] bf16 = (softmax(x) - onehot(label)) * *scale (rows with label < 0: 0); softmax =
// exp((x - lse) - lse_lo), lse_lo null: 0
hipError_t launch_xent_bwd(const uint16_t* x, const int64_t* labels, const float* lse, const float* lse_lo,
                           const float* scale, int64_t rows, int64_t V, int64_t ldx, uint16_t* dx, hipStream_t stream);
}  // namespace psd
