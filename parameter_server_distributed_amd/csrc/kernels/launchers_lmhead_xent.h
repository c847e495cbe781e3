// Launch API of the fused LM head + softmax cross-entropy (lmhead_xent.hip).
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {
// Z = X W^T (+ bias): X [M][K] bf16, W [V][K] bf16 (both K-major, contiguous), bias [V] bf16 or null,
// labels [M] int64 (negative: the row is ignored). Contract: M >= 1, K % 64 == 0, V % 8 == 0,
// 16-byte aligned pointers, (M + 128) K and (V + 128) K below 2^31 elements: anything else returns
// hipErrorInvalidValue and launches nothing.
struct LmHeadXentArgs {
  const uint16_t* x;
  const uint16_t* w;
  const uint16_t* bias;
  const int64_t* labels;
  int64_t M, K, V;
};

// vocabulary slices of the forward grid for this problem: ceil(M / 128) * slices covers the chip about twice
int lmhead_xent_slices(int64_t M, int64_t V);

// lse[M] and loss_row[M] = log(sum) + (max - z[label]) (0 for ignored rows); no logit is stored.
// slices: 1 .. ceil(V / 128) (clamped), 0: lmhead_xent_slices; part: fp32 scratch of slices * 3 * M
hipError_t launch_lmhead_xent_fwd(const LmHeadXentArgs& a, int slices, float* part, float* lse, float* loss_row,
                                  hipStream_t stream);

// dz [M][V] bf16 = (exp(z - lse[row]) - [col == label]) * *scale (ignored rows: 0); scale: device scalar
hipError_t launch_lmhead_xent_dz(const LmHeadXentArgs& a, const float* lse, const float* scale, uint16_t* dz,
                                 hipStream_t stream);
}  // namespace psd
