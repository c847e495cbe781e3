// Fixed-order block sums shared by the segmented apply (optim_lw.hip) and the gradient-norm pass
// (clip.hip): xor butterfly over the 64 lanes of each wave, then waves 0..3 in order. The order
// depends on nothing but the lane ids, so a chunk's sum is the same bits on any grid.
#pragma once
#include "common.h"

namespace psd {

// xor butterfly over the 64 lanes: every lane ends with the same sum, in an order that depends on
// nothing but the lane ids
__device__ __forceinline__ float wave_sum(float x) {
#pragma unroll
  for (int m = kWave / 2; m >= 1; m >>= 1) x += __shfl_xor(x, m, kWave);
  return x;
}

// (a, b) summed over the 256 threads of the block -> out[0], out[1]; red: 8 floats of LDS
__device__ __forceinline__ void block_sum2_store(float a, float b, float* red, float* out) {
  a = wave_sum(a);
  b = wave_sum(b);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & (kWave - 1)) == 0) {
    red[wave] = a;
    red[4 + wave] = b;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    out[0] = ((red[0] + red[1]) + red[2]) + red[3];
    out[1] = ((red[4] + red[5]) + red[6]) + red[7];
  }
  __syncthreads();  // red is reused by the block's next chunk
}

// one value summed over the 256 threads of the block -> out[0]; red: 4 floats of LDS
__device__ __forceinline__ void block_sum1_store(float a, float* red, float* out) {
  a = wave_sum(a);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & (kWave - 1)) == 0) red[wave] = a;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = ((red[0] + red[1]) + red[2]) + red[3];
  __syncthreads();  // red is reused by the block's next chunk
}

}  // namespace psd
