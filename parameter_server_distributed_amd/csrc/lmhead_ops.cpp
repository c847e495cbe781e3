// Tensor glue for the fused LM head + softmax cross-entropy (kernels/lmhead_xent.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <algorithm>

#include "glue.h"
#include "kernels/launchers_lmhead_xent.h"
#include "ops.h"

namespace psd {

namespace {
// the operands every entry point shares; the launcher checks the shape contract (K % 64, V % 8, sizes)
LmHeadXentArgs lmhead_args(const char* op, const at::Tensor& x, const at::Tensor& w,
                           const c10::optional<at::Tensor>& bias, const at::Tensor& labels) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kBFloat16 && x.is_contiguous(), op,
              ": x must be a contiguous 2-D bf16 device tensor");
  TORCH_CHECK(w.device() == x.device() && w.dim() == 2 && w.scalar_type() == at::kBFloat16 && w.is_contiguous() &&
                  w.size(1) == x.size(1),
              op, ": w must be a contiguous bf16 [V, K] on x's device");
  check_vec(op, bias, w.size(0), at::kBFloat16, x, "bias");
  check_vec(op, labels, x.size(0), at::kLong, x, "labels");
  return LmHeadXentArgs{bf16(x), bf16(w), opt_ptr<const uint16_t>(bias), labels.data_ptr<int64_t>(),
                        x.size(0), x.size(1), w.size(0)};
}
}  // namespace

int64_t lmhead_xent_slices_(int64_t M, int64_t V) { return lmhead_xent_slices(M, V); }

// {loss_row [M] fp32, lse [M] fp32} of softmax cross-entropy over Z = x w^T (+ bias); Z is never stored.
// slices: vocabulary slices of the grid (0: chosen from the CU count; tests force it)
std::vector<at::Tensor> lmhead_xent_fwd(const at::Tensor& x, const at::Tensor& w, c10::optional<at::Tensor> bias,
                                        const at::Tensor& labels, int64_t slices) {
  const LmHeadXentArgs a = lmhead_args("psd lmhead_xent_fwd", x, w, bias, labels);
  TORCH_CHECK(slices >= 0 && slices <= (1 << 20), "psd lmhead_xent_fwd: slices");
  const c10::DeviceGuard g(x.device());
  const int64_t tiles_n = (a.V + 127) / 128;
  const int64_t s = slices == 0 ? lmhead_xent_slices(a.M, a.V) : std::min(slices, tiles_n);
  auto f32 = x.options().dtype(at::kFloat);
  at::Tensor part = at::empty({s * 3 * a.M}, f32), lse = at::empty({a.M}, f32), loss_row = at::empty({a.M}, f32);
  check_hip(launch_lmhead_xent_fwd(a, (int)s, part.data_ptr<float>(), lse.data_ptr<float>(),
                                   loss_row.data_ptr<float>(), stream_of(x)),
            "psd lmhead_xent_fwd");
  return {loss_row, lse};
}

// dz_out [rows, V] bf16 = (softmax(x w^T + bias) - onehot(labels)) * scale from the saved lse; scale: fp32
// device scalar. x, labels and lse are the same row chunk.
void lmhead_xent_dz_(const at::Tensor& x, const at::Tensor& w, c10::optional<at::Tensor> bias,
                     const at::Tensor& labels, const at::Tensor& lse, const at::Tensor& scale, at::Tensor dz_out) {
  const LmHeadXentArgs a = lmhead_args("psd lmhead_xent_dz_", x, w, bias, labels);
  check_vec("psd lmhead_xent_dz_", lse, a.M, at::kFloat, x, "lse");
  TORCH_CHECK(scale.device() == x.device() && scale.scalar_type() == at::kFloat && scale.numel() >= 1,
              "psd lmhead_xent_dz_: scale must be an fp32 device scalar");
  TORCH_CHECK(dz_out.device() == x.device() && dz_out.scalar_type() == at::kBFloat16 && dz_out.is_contiguous() &&
                  dz_out.dim() == 2 && dz_out.size(0) == a.M && dz_out.size(1) == a.V,
              "psd lmhead_xent_dz_: dz_out must be a contiguous bf16 [rows, V]");
  const c10::DeviceGuard g(x.device());
  check_hip(launch_lmhead_xent_dz(a, lse.data_ptr<float>(), scale.data_ptr<float>(), bf16_mut(dz_out), stream_of(x)),
            "psd lmhead_xent_dz_");
}

}  // namespace psd
