// Launch API of the segmented (per-tensor) parameter-server apply for gfx950: LARS, LAMB and
// per-tensor weight-decay exclusion for the flat optimizers (kernels/optim_lw.hip).
//
// The flat apply of launchers.h sees one buffer and one scalar weight decay. These kernels also see
// a layer table: the buffer is a run of segments (one per tensor, from its start to the next
// tensor's start, so the alignment padding belongs to the tensor in front of it), each with a
// weight-decay multiplier and an "adapt" flag, and cut into chunks of at most kLwChunk elements
// numbered from the segment's start. A chunk never crosses a segment; workgroups walk the chunk
// table with a grid-stride loop, so any grid (and any grid_cap) computes the same bits, and so does
// any cut of the buffer into shards whose boundaries are tensor starts.
//
// Like everything in launchers.h: raw pointers, explicit stream, no allocation, no synchronisation,
// legal under stream capture. Every table pointer is device memory owned by the caller.
#pragma once
#include "launchers.h"

namespace psd {

constexpr int64_t kLwChunk = 8192;

struct LwTable {
  const int64_t* seg_start;  // [n_seg + 1] element offset of each segment in the buffer; [n_seg] = n
  const int32_t* seg_chunk;  // [n_seg + 1] first chunk of each segment; [n_seg] = n_chunks
  const float* wd_mult;      // [n_seg] weight-decay multiplier (0: excluded)
  const int32_t* adapt;      // [n_seg] 1: trust ratio applies, 0: ratio 1
  const int32_t* chunk_seg;  // [n_chunks] segment of each chunk
  const int64_t* chunk_off;  // [n_chunks] element offset of each chunk in the buffer (8-aligned)
  float* partials;           // [2 * n_chunks] per-chunk (sum w^2, sum g^2 | sum u^2)
  float* ratio;              // [n_seg] trust ratio of the current step
  int32_t n_seg;
  int32_t n_chunks;
  float trust_coef;          // LARS eta
  int32_t _pad;
};

// Norm pass. LARS: partials[c] = (sum w^2, sum g^2) of chunk c, g = grad_scale * sum_k src_k.
// LAMB (stage 1): also m, v <- Adam moments of g (stored), partials[c] = (sum w^2, sum u^2) with
// u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) + wd_t w. The master is only read.
hipError_t launch_lw_norms(const OptimHyper& hyper, const OptimDyn* dyn, const float* master,
                           const SourceList& grads, float* state1, float* state2, const LwTable& tab,
                           hipStream_t stream, int grid_cap = 0);

// ratio[t] from the segment's chunk partials, summed in a fixed order (one wave per segment).
hipError_t launch_lw_finalize(const OptimHyper& hyper, const LwTable& tab, hipStream_t stream, int grid_cap = 0);

// Segmented apply: master / state / bf16 shadow in one pass. LARS reads the gradient sources again;
// LAMB (stage 2) recomputes u from the stored m, v and reads no gradient; SGD / momentum / Adam /
// AdamW run the flat kernel's update with weight_decay * wd_mult[t] (no norm pass, ratio unused).
hipError_t launch_lw_apply(const OptimHyper& hyper, const OptimDyn* dyn, float* master, const SourceList& grads,
                           float* state1, float* state2, uint16_t* shadow_bf16, const LwTable& tab,
                           hipStream_t stream, int grid_cap = 0);

}  // namespace psd
