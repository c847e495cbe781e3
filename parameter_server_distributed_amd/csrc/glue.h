// Host-side helpers shared by the tensor glue (csrc/*_ops.cpp).
#pragma once
#include <ATen/ATen.h>
#include <c10/hip/HIPStream.h>

#include <cstdint>

namespace psd {

// the current stream of t's device
inline hipStream_t stream_of(const at::Tensor& t) { return c10::hip::getCurrentHIPStream(t.device().index()).stream(); }

// an optional tensor argument that was passed and is not the undefined tensor
inline bool given(const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); }

template <typename T>
T* opt_ptr(const c10::optional<at::Tensor>& t) {
  return given(t) ? reinterpret_cast<T*>(t->data_ptr()) : nullptr;
}

inline bool aligned16(const at::Tensor& t) { return (reinterpret_cast<uintptr_t>(t.data_ptr()) & 15) == 0; }

// laid out like an NHWC activation: channels_last when 4-D, contiguous otherwise (its 2-D [pixels, C] view)
inline bool nhwc_laid(const at::Tensor& t) {
  return t.dim() == 4 ? t.is_contiguous(at::MemoryFormat::ChannelsLast) : t.is_contiguous();
}

// log2 of a power of two (the callers decline other channel counts first)
inline int log2_exact(int64_t c) {
  int l = 0;
  while (((int64_t)1 << l) < c) ++l;
  return l;
}

// a launcher's error as the op's failure: "<op>: <hipGetErrorString>"
inline void check_hip(hipError_t e, const char* op) { TORCH_CHECK(e == hipSuccess, op, ": ", hipGetErrorString(e)); }

}  // namespace psd
