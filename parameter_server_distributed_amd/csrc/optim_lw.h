// How the shared host code (ops.cpp, and through it async_ps.cpp and ps_core.cpp) reaches the
// layer-table kernels without a link-time reference to them: optim_lw.cpp registers the three
// launchers here from a static initializer. A build without optim_lw.cpp (the host-only sanitizer
// programs under csrc/tests) still links; there a layer table is legal on CPU tensors only.
#pragma once
#include "kernels/launchers_optim_lw.h"

namespace psd {

struct LwGpu {
  hipError_t (*norms)(const OptimHyper&, const OptimDyn*, const float*, const SourceList&, float*, float*,
                      const LwTable&, hipStream_t, int);
  hipError_t (*finalize)(const OptimHyper&, const LwTable&, hipStream_t, int);
  hipError_t (*apply)(const OptimHyper&, const OptimDyn*, float*, const SourceList&, float*, float*, uint16_t*,
                      const LwTable&, hipStream_t, int);
};

// null until optim_lw.cpp's initializer ran (ops.cpp owns the slot)
const LwGpu*& lw_gpu();

}  // namespace psd
