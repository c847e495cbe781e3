// Tensor glue for the fused softmax cross-entropy (kernels/xent.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include "glue.h"
#include "kernels/launchers_xent.h"

namespace psd {

namespace {
void check_logits(const at::Tensor& x, const at::Tensor& labels) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.scalar_type() == at::kBFloat16 && x.stride(1) == 1 &&
                  x.stride(0) % 8 == 0 && aligned16(x),
              "psd xent: logits must be a 2-D bf16 device tensor with 16-B aligned rows");
  TORCH_CHECK(labels.is_cuda() && labels.dim() == 1 && labels.scalar_type() == at::kLong && labels.is_contiguous() &&
                  labels.size(0) == x.size(0),
              "psd xent: labels must be int64 [rows] on the device");
}
}  // namespace

// returns {loss_row [rows] fp32, lse [rows] fp32, lse_lo [rows] fp32: lse's rounding error, for xent_bwd}
std::vector<at::Tensor> xent_fwd(const at::Tensor& x, const at::Tensor& labels) {
  check_logits(x, labels);
  const c10::DeviceGuard g(x.device());
  const int64_t rows = x.size(0), V = x.size(1);
  auto f32 = x.options().dtype(at::kFloat);
  at::Tensor lse = at::empty({rows}, f32), lse_lo = at::empty({rows}, f32), loss_row = at::empty({rows}, f32);
  hipError_t e = launch_xent_fwd(reinterpret_cast<const uint16_t*>(x.data_ptr()), labels.data_ptr<int64_t>(), rows, V,
                                 x.stride(0), lse.data_ptr<float>(), lse_lo.data_ptr<float>(),
                                 loss_row.data_ptr<float>(), stream_of(x));
  check_hip(e, "psd xent fwd");
  return {loss_row, lse, lse_lo};
}

// dx [rows, V] bf16 = (softmax(x) - onehot) * scale; scale: fp32 device scalar; lse_lo: xent_fwd's third output
// (without it the softmax is exp(x - lse) on the rounded lse alone)
at::Tensor xent_bwd(const at::Tensor& x, const at::Tensor& labels, const at::Tensor& lse, const at::Tensor& scale,
                    c10::optional<at::Tensor> lse_lo) {
  check_logits(x, labels);
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.numel() == x.size(0) && lse.is_contiguous(),
              "psd xent bwd: lse fp32 [rows]");
  TORCH_CHECK(scale.is_cuda() && scale.scalar_type() == at::kFloat && scale.numel() >= 1, "psd xent bwd: scale");
  TORCH_CHECK(!given(lse_lo) || (lse_lo->is_cuda() && lse_lo->scalar_type() == at::kFloat &&
                                 lse_lo->numel() == x.size(0) && lse_lo->is_contiguous()),
              "psd xent bwd: lse_lo fp32 [rows]");
  // the gradient is written contiguous [rows, V] in 16-byte vectors: its rows are aligned only for V % 8 == 0
  // (the logits' own row stride may be any multiple of 8)
  TORCH_CHECK(x.size(1) % 8 == 0, "psd xent bwd: the class count must be a multiple of 8 (got ", x.size(1), ")");
  const c10::DeviceGuard g(x.device());
  const int64_t rows = x.size(0), V = x.size(1);
  at::Tensor dx = at::empty({rows, V}, x.options());
  hipError_t e = launch_xent_bwd(reinterpret_cast<const uint16_t*>(x.data_ptr()), labels.data_ptr<int64_t>(),
                                 lse.data_ptr<float>(), given(lse_lo) ? lse_lo->data_ptr<float>() : nullptr,
                                 scale.data_ptr<float>(), rows, V, x.stride(0),
                                 reinterpret_cast<uint16_t*>(dx.data_ptr()), stream_of(x));
  check_hip(e, "psd xent bwd");
  return dx;
}

}  // namespace psd
