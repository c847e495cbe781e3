// Compute units of the device that is current at the first call (256 if the query fails), cached
// for the process: the persistent kernels size their grids by it.
#pragma once
#include <hip/hip_runtime_api.h>

namespace psd {

inline int cu_count() {
  static const int n = [] {
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess ||
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
      return 256;
    return cus;
  }();
  return n;
}

}  // namespace psd
