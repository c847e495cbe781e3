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
// the MX side output of `like` (a or dgu): payload `q` (fp8 dtype `qt`, like's shape) and E8M0 scales `sc` (uint8,
// one per 32 columns), both or neither; rows of whole 32-column blocks (F % 32 == 0). True when given
bool check_mx(const char* op, const c10::optional<at::Tensor>& q, const c10::optional<at::Tensor>& sc,
              at::IntArrayRef shape, const at::Tensor& gu, int64_t F, at::ScalarType qt, const char* like_name) {
  TORCH_CHECK(given(q) == given(sc), op, ": q8_out and sc8_out come together");
  if (!given(q)) return false;
  TORCH_CHECK(F % 32 == 0, op, ": q8_out needs gu's F = ", F, " to be a multiple of 32 (whole MX blocks per row)");
  int64_t n = 1;
  for (const int64_t d : shape) n *= d;
  TORCH_CHECK(q->is_cuda() && q->device() == gu.device(), op, ": q8_out must be on gu's device");
  TORCH_CHECK(q->scalar_type() == qt, op, ": q8_out must be ", qt, ", got ", q->scalar_type());
  TORCH_CHECK(q->is_contiguous(), op, ": q8_out must be contiguous");
  TORCH_CHECK(q->sizes() == shape, op, ": q8_out must have ", like_name, "'s shape ", shape, ", got ", q->sizes());
  TORCH_CHECK((reinterpret_cast<uintptr_t>(q->data_ptr()) & 7) == 0, op, ": q8_out must be 8-byte aligned");
  TORCH_CHECK(sc->is_cuda() && sc->device() == gu.device(), op, ": sc8_out must be on gu's device");
  TORCH_CHECK(sc->scalar_type() == at::kByte, op, ": sc8_out must be uint8, got ", sc->scalar_type());
  TORCH_CHECK(sc->is_contiguous(), op, ": sc8_out must be contiguous");
  TORCH_CHECK(sc->numel() == n / 32, op, ": sc8_out must hold ", n / 32, " bytes (one per 32 columns of ", like_name,
              "), got ", sc->sizes());
  return true;
}
}  // namespace

// a [..., F] = bf16(silu(gu[..., :F]) * gu[..., F:]). blocks > 0 bounds the grid (tests); the bits do not depend on it.
// q8_out / sc8_out: also the MX e4m3 copy of a (bitwise quant_mx_ of a), float8_e4m3fn like a and uint8 [T, F/32].
at::Tensor swiglu_fwd(const at::Tensor& gu, int64_t blocks, c10::optional<at::Tensor> q8_out,
                      c10::optional<at::Tensor> sc8_out) {
  const char* op = "psd swiglu_fwd";
  const int64_t F = check_gu(op, gu, blocks);
  auto shape = gu.sizes().vec();
  shape.back() = F;
  const bool mx = check_mx(op, q8_out, sc8_out, shape, gu, F, at::kFloat8_e4m3fn, "a");
  const c10::DeviceGuard g(gu.device());
  at::Tensor out = at::empty(shape, gu.options());
  SwigluArgs a{};
  a.gu = bf16(gu);
  a.a = bf16_mut(out);
  a.q8 = mx ? reinterpret_cast<uint8_t*>(q8_out->data_ptr()) : nullptr;
  a.sc8 = mx ? sc8_out->data_ptr<uint8_t>() : nullptr;
  a.F = F;
  a.T = F > 0 ? out.numel() / F : 0;
  a.blocks = (int32_t)blocks;
  check_hip(launch_swiglu_fwd(a, stream_of(gu)), op);
  return out;
}

// dgu [..., 2F] = (dg | du), recomputed from gu: dg = da u sig (1 + g (1 - sig)), du = da g sig.
// q8_out / sc8_out: also the MX e5m2 copy of dgu (bitwise quant_mx_ of it, e5m2), float8_e5m2 like gu and uint8
// [T, 2F/32].
at::Tensor swiglu_bwd(const at::Tensor& da, const at::Tensor& gu, int64_t blocks, c10::optional<at::Tensor> q8_out,
                      c10::optional<at::Tensor> sc8_out) {
  const char* op = "psd swiglu_bwd";
  const int64_t F = check_gu(op, gu, blocks);
  check_act(op, da, "da");
  TORCH_CHECK(da.device() == gu.device(), op, ": da must be on gu's device");
  auto shape = gu.sizes().vec();
  shape.back() = F;
  TORCH_CHECK(da.sizes() == at::IntArrayRef(shape), op, ": da must be ", at::IntArrayRef(shape), " for gu ", gu.sizes(),
              ", got ", da.sizes());
  const bool mx = check_mx(op, q8_out, sc8_out, gu.sizes(), gu, F, at::kFloat8_e5m2, "gu");
  const c10::DeviceGuard g(gu.device());
  at::Tensor dgu = at::empty_like(gu);
  SwigluArgs a{};
  a.gu = bf16(gu);
  a.da = bf16(da);
  a.dgu = bf16_mut(dgu);
  a.q8 = mx ? reinterpret_cast<uint8_t*>(q8_out->data_ptr()) : nullptr;
  a.sc8 = mx ? sc8_out->data_ptr<uint8_t>() : nullptr;
  a.F = F;
  a.T = F > 0 ? da.numel() / F : 0;
  a.blocks = (int32_t)blocks;
  check_hip(launch_swiglu_bwd(a, stream_of(gu)), op);
  return dgu;
}

}  // namespace psd
