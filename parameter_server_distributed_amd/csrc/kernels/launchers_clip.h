// Launch API of the global-norm gradient clipping pass for gfx950 (kernels/clip.hip).
//
// A worker of the async plane pushes its raw gradient buckets while backward runs; at the end of
// backward these two launches turn the whole flat gradient into one scalar, the clipping coefficient
// c = min(1, clip_norm / (||g||_2 + 1e-6)) of torch.nn.utils.clip_grad_norm_, which travels after the
// buckets and is multiplied in by the owner's fused apply (SourceList::scale, launchers.h).
//
// Like everything in launchers.h: raw pointers, explicit stream, no allocation, no synchronisation,
// no memcpy, legal under stream capture. Nothing needs zeroing between steps.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstdint>

namespace psd {

constexpr int64_t kClipChunk = 8192;  // elements per chunk: one workgroup of 256, 4 vectors of 8 per lane

inline int64_t clip_chunks(int64_t n) { return n <= 0 ? 0 : (n + kClipChunk - 1) / kClipChunk; }

// partials[c] = sum of g[i]^2 over chunk c (fp32), c < clip_chunks(n). g: bf16 or fp32 (DType),
// 16-byte aligned, read once. The order of every sum is fixed (lane-sequential fma, xor butterfly,
// waves 0..3), so the bits do not depend on the grid or on grid_cap.
hipError_t launch_sumsq_partials(const void* g, int32_t dtype, int64_t n, float* partials, hipStream_t stream,
                                 int grid_cap = 0);

// out[1] = n = sqrt(sum_c partials[c]) (chunks summed in a fixed order in fp64, rounded to fp32),
// out[0] = c = min(1, clip_norm / (n + 1e-6)) in fp32; a non-finite n propagates (NaN -> NaN, inf -> 0).
// `out`: the first two floats of a 256-byte device block (the "push scalars").
hipError_t launch_clip_finalize(const float* partials, int64_t n_chunks, float clip_norm, float* out,
                                hipStream_t stream);

}  // namespace psd
