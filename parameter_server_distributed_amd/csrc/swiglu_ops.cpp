// Tensor glue for the gated SiLU activation (kernels/swiglu.hip) on the packed gate/up tensor. Every check
// runs before any allocation or launch and names the argument it rejects.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <climits>

#include "glue.h"
#include "kernels/launchers_swiglu.h"
#include "ops.h"

namespace psd {

namespace {
void check_act(const char* op, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", name, " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK(aligned16(t), op, ": ", name, " must be 16-byte aligned");
}
// gu [..., 2F] -> F; T = the leading dimensions' product
int64_t check_gu(const char* op, const at::Tensor& gu, int64_t blocks) {
  check_act(op, gu, "gu");
  TORCH_CHECK(gu.dim() >= 1 && gu.size(-1) % 2 == 0, op, ": gu must be [..., 2F] (gate | up), got ", gu.sizes());
  const int64_t F = gu.size(-1) / 2;
  TORCH_CHECK(F % 8 == 0 && F <= INT32_MAX, op, ": gu's F = ", F, " must be a multiple of 8");
  TORCH_CHECK(blocks >= 0 && blocks <= INT32_MAX, op, ": blocks must be >= 0 (0: the op chooses), got ", blocks);
  return F;
}
}  // namespace

// a [..., F] = bf16(silu(gu[..., :F]) * gu[..., F:]). blocks > 0 bounds the grid (tests); the bits do not depend on it.
at::Tensor swiglu_fwd(const at::Tensor& gu, int64_t blocks) {
  const char* op = "psd swiglu_fwd";
  const int64_t F = check_gu(op, gu, blocks);
  const c10::DeviceGuard g(gu.device());
  auto shape = gu.sizes().vec();
  shape.back() = F;
  at::Tensor out = at::empty(shape, gu.options());
  SwigluArgs a{};
  a.gu = bf16(gu);
  a.a = bf16_mut(out);
  a.F = F;
  a.T = F > 0 ? out.numel() / F : 0;
  a.blocks = (int32_t)blocks;
  check_hip(launch_swiglu_fwd(a, stream_of(gu)), op);
  return out;
}

// dgu [..., 2F] = (dg | du), recomputed from gu: dg = da u sig (1 + g (1 - sig)), du = da g sig.
at::Tensor swiglu_bwd(const at::Tensor& da, const at::Tensor& gu, int64_t blocks) {
  const char* op = "psd swiglu_bwd";
  const int64_t F = check_gu(op, gu, blocks);
  check_act(op, da, "da");
  TORCH_CHECK(da.device() == gu.device(), op, ": da must be on gu's device");
  auto shape = gu.sizes().vec();
  shape.back() = F;
  TORCH_CHECK(da.sizes() == at::IntArrayRef(shape), op, ": da must be ", at::IntArrayRef(shape), " for gu ", gu.sizes(),
              ", got ", da.sizes());
  const c10::DeviceGuard g(gu.device());
  at::Tensor dgu = at::empty_like(gu);
  SwigluArgs a{};
  a.gu = bf16(gu);
  a.da = bf16(da);
  a.dgu = bf16_mut(dgu);
  a.F = F;
  a.T = F > 0 ? da.numel() / F : 0;
  a.blocks = (int32_t)blocks;
  check_hip(launch_swiglu_bwd(a, stream_of(gu)), op);
  return dgu;
}

}  // namespace psd
