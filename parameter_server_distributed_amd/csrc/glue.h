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

// a bf16 tensor's elements as the launchers take them
inline const uint16_t* bf16(const at::Tensor& t) { return reinterpret_cast<const uint16_t*>(t.data_ptr()); }
inline uint16_t* bf16_mut(const at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// t's elements, or null for the undefined tensor
template <typename T>
T* ptr_or_null(const at::Tensor& t) {
  return t.defined() ? reinterpret_cast<T*>(t.data_ptr()) : nullptr;
}

// a per-channel vector: n contiguous elements of dtype st on like's device; an optional one may be absent
inline void check_vec(const char* op, const at::Tensor& t, int64_t n, at::ScalarType st, const at::Tensor& like,
                      const char* name) {
  TORCH_CHECK(t.defined() && t.numel() == n && t.scalar_type() == st && t.is_contiguous() && t.device() == like.device(),
              op, ": ", name, " must be a contiguous ", st, " [", n, "] on the input's device");
}
inline void check_vec(const char* op, const c10::optional<at::Tensor>& t, int64_t n, at::ScalarType st,
                      const at::Tensor& like, const char* name) {
  if (given(t)) check_vec(op, *t, n, st, like, name);
}

// the statistics block of a BN forward launch (bn_ops.cpp): checks the parameter vectors, allocates
// the saved statistics and (training) the scale/shift on like's device, and fills gamma .. counter,
// M, C, training, momentum and eps of a. Eval mode takes the scale/shift from ss_eval.
struct BnFwdArgs;
struct BnFwdStats {
  at::Tensor mean, invstd, ss;
};
BnFwdStats bn_fwd_stats(BnFwdArgs& a, const at::Tensor& like, int64_t M, int64_t C,
                        const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                        const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                        const c10::optional<at::Tensor>& counter, double momentum, double eps, bool training = true,
                        const c10::optional<at::Tensor>& ss_eval = c10::nullopt);

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
