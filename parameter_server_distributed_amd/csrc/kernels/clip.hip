// Global L2 norm of a flat gradient and its clipping coefficient for gfx950.
//
// The async plane cannot clip with torch.nn.utils.clip_grad_norm_: the gradient buckets leave for
// the owners' inboxes while backward still runs, and the norm of the whole gradient is known only
// after the last one has left. So the worker pushes raw buckets, runs this pass over its flat
// gradient buffer at the end of backward, and sends one scalar after them; the owner's fused apply
// multiplies each source by its scalar (optim_update.h load_sources8<.., SCALED>).
//
//   sumsq_partials   one read of the buffer (bf16 or fp32, 16-byte loads). The buffer is cut into
//                    chunks of 8192 elements; a workgroup of 256 owns a whole chunk (4 vectors of 8
//                    per lane, fmaf(g, g, acc)) and walks the chunks with a grid-stride loop
//                    (<= 2048 workgroups). Each chunk writes its own float: no atomics, nothing to
//                    zero between steps.
//   clip_finalize    one workgroup adds the chunk partials in a fixed order in fp64 -> n, c.
//
// Regime: pure HBM streaming (2 or 4 B/element, no reuse, no LDS beyond the 4-float exchange of the
// block sum). Above 128 MB (BERT-base: ~220 MB) the loads are nontemporal, the threshold of the BN
// streaming passes: the bytes are touched once and would only evict what the step still needs from
// the Infinity Cache.
//
// Every sum has a fixed order -- 32 sequential fmas per lane at most, xor butterfly, waves 0..3,
// chunks lane-strided then an LDS tree in fp64 -- so the result is bitwise independent of the grid and
// of grid_cap. An element passes through at most 32 sequential + 9 tree fp32 additions.
#include "block_sum.h"
#include "common.h"
#include "launchers.h"
#include "launchers_clip.h"

namespace psd {

namespace {

template <bool NT>
__device__ __forceinline__ void load8_f32_nt(const float* p, float v[8]) {
  f32x4 a, b;
  if constexpr (NT) {
    a = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    b = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p + 4));
  } else {
    a = *reinterpret_cast<const f32x4*>(p);
    b = *reinterpret_cast<const f32x4*>(p + 4);
  }
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

}  // namespace

template <int DT, bool NT>
__global__ __launch_bounds__(256) void sumsq_partials_kernel(const void* __restrict__ g, int64_t n,
                                                             float* __restrict__ partials, int64_t n_chunks) {
  __shared__ float red[4];
  for (int64_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const int64_t off = c * kClipChunk;
    const int64_t left = n - off;
    const int len = (int)(left < kClipChunk ? left : kClipChunk);
    const int nvec = len >> 3;
    float acc = 0.f;
    if (nvec == (int)(kClipChunk >> 3)) {
      // a whole chunk: the lane's 4 vectors are loaded together, then added in the loop's order
      float t[4][8];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t i = off + ((int64_t)(threadIdx.x + 256 * j) << 3);
        if (DT == DT_BF16) load8_bf16<NT>(static_cast<const uint16_t*>(g) + i, t[j]);
        else load8_f32_nt<NT>(static_cast<const float*>(g) + i, t[j]);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(t[j][e], t[j][e], acc);
    } else {
      for (int v = threadIdx.x; v < nvec; v += 256) {
        const int64_t i = off + ((int64_t)v << 3);
        float t[8];
        if (DT == DT_BF16) load8_bf16<NT>(static_cast<const uint16_t*>(g) + i, t);
        else load8_f32_nt<NT>(static_cast<const float*>(g) + i, t);
#pragma unroll
        for (int e = 0; e < 8; ++e) acc = fmaf(t[e], t[e], acc);
      }
    }
    // the n % 8 tail (last chunk only, which then holds at most 1023 vectors): lane 255 has at most
    // 3 vectors there, so its 24 + 7 sequential additions stay within the 32 of a full lane
    if (threadIdx.x == 255) {
      for (int64_t i = off + ((int64_t)nvec << 3); i < off + len; ++i) {
        const float x = (DT == DT_BF16) ? bf16_to_f32(static_cast<const uint16_t*>(g)[i])
                                        : static_cast<const float*>(g)[i];
        acc = fmaf(x, x, acc);
      }
    }
    block_sum1_store(acc, red, partials + c);
  }
}

// lane l adds chunks l, l + 256, ... in order (fp64), then an LDS tree over the 256 lanes
__global__ __launch_bounds__(256) void clip_finalize_kernel(const float* __restrict__ partials, int64_t n_chunks,
                                                            float clip_norm, float* __restrict__ out) {
  __shared__ double sh[256];
  double a = 0.0;
  for (int64_t c = threadIdx.x; c < n_chunks; c += 256) a += (double)partials[c];
  sh[threadIdx.x] = a;
  __syncthreads();
  for (int s = 128; s >= 1; s >>= 1) {
    if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const float nrm = (float)sqrt(sh[0]);
    const float q = clip_norm / (nrm + 1e-6f);
    out[0] = q > 1.f ? 1.f : q;  // NaN stays NaN (torch: clamp(max=1) of a NaN coefficient)
    out[1] = nrm;
  }
}

hipError_t launch_sumsq_partials(const void* g, int32_t dtype, int64_t n, float* partials, hipStream_t st,
                                 int grid_cap) {
  if (n <= 0) return hipSuccess;
  if (!g || !partials || (dtype != DT_BF16 && dtype != DT_F32)) return hipErrorInvalidValue;
  const int64_t chunks = clip_chunks(n);
  int64_t grid = chunks > 2048 ? 2048 : chunks;
  if (grid_cap > 0 && grid > grid_cap) grid = grid_cap;
  const bool nt = n * (dtype == DT_BF16 ? 2 : 4) > (128LL << 20);
#define PSD_SUMSQ(DT, NT) \
  hipLaunchKernelGGL((sumsq_partials_kernel<DT, NT>), dim3((unsigned)grid), dim3(256), 0, st, g, n, partials, chunks)
  if (dtype == DT_BF16) {
    if (nt) PSD_SUMSQ(DT_BF16, true);
    else PSD_SUMSQ(DT_BF16, false);
  } else {
    if (nt) PSD_SUMSQ(DT_F32, true);
    else PSD_SUMSQ(DT_F32, false);
  }
#undef PSD_SUMSQ
  return hipGetLastError();
}

hipError_t launch_clip_finalize(const float* partials, int64_t n_chunks, float clip_norm, float* out,
                                hipStream_t st) {
  if (!out || n_chunks < 0 || (n_chunks > 0 && !partials)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(clip_finalize_kernel, dim3(1), dim3(256), 0, st, partials, n_chunks, clip_norm, out);
  return hipGetLastError();
}

}  // namespace psd
