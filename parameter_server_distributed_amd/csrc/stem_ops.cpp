// Tensor glue for the ResNet stem: the 7x7/s2 convolution and its weight gradient (kernels/stem.hip)
// in front of the fused BN + ReLU + max-pool (kernels/bn.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "glue.h"
#include "kernels/launchers_bn.h"
#include "kernels/launchers_stem.h"
#include "ops.h"

namespace psd {

// ResNet stem forward: conv 7x7/s2/p3 (3 -> 64, kernels/stem.hip, BN statistics reduced in its
// epilogue) -> BN finalize -> fused BN + ReLU + max-pool. Returns {y_pool, argmax, mean, invstd, ss,
// conv_out}; conv_out (the BN input) is kept for the backward.
std::vector<at::Tensor> stem_fwd(const at::Tensor& x_in, const at::Tensor& w, const at::Tensor& gamma,
                                 const at::Tensor& beta, const at::Tensor& running_mean, const at::Tensor& running_var,
                                 double momentum, double eps, c10::optional<at::Tensor> counter) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kBFloat16 && x_in.dim() == 4 && x_in.size(1) == 3,
              "psd stem: bf16 [N, 3, H, W] input");
  TORCH_CHECK(w.scalar_type() == at::kBFloat16 && w.sizes() == at::IntArrayRef({64, 3, 7, 7}) &&
                  w.device() == x_in.device(),
              "psd stem: weight [64,3,7,7]");
  const c10::DeviceGuard g(x_in.device());
  at::Tensor x = x_in.contiguous(at::MemoryFormat::ChannelsLast);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3), Ho = H / 2, Wo = W / 2;
  TORCH_CHECK(stem_conv_supported((int)H, (int)W, (int)Ho, (int)Wo) && bn_pool_supported((int)Ho, (int)Wo, 64),
              "psd stem: unsupported input ", x.sizes());
  BnFwdArgs a{};
  const BnFwdStats s = bn_fwd_stats(a, x, N * Ho * Wo, 64, gamma, beta, running_mean, running_var, counter, momentum, eps);
  // [co][ci][kh][kw] -> [co][kh*24 + kw*3 + ci], zero for kw*3+ci >= 21 and the 8th kh block
  at::Tensor wk = at::constant_pad_nd(w.permute({0, 2, 3, 1}).reshape({64, 7, 21}), {0, 3, 0, 1}).reshape({64, 192})
                      .contiguous();
  const auto cl = x.options().memory_format(at::MemoryFormat::ChannelsLast);
  at::Tensor conv = at::empty({N, 64, Ho, Wo}, cl);
  const int nblk = stem_conv_blocks((int)N, (int)Ho);
  at::Tensor part = at::empty({(int64_t)nblk * 128}, x.options().dtype(at::kFloat));
  hipStream_t st = stream_of(x);
  hipError_t e = launch_stem_conv(bf16(x), bf16(wk), bf16_mut(conv), running_mean.data_ptr<float>(),
                                  part.data_ptr<float>(), (int)N, (int)H, (int)W, (int)Ho, (int)Wo, st);
  check_hip(e, "psd stem conv");
  at::Tensor y = at::empty({N, 64, Ho / 2, Wo / 2}, cl);
  at::Tensor arg = at::empty({N, 64, Ho / 2, Wo / 2}, cl.dtype(at::kByte));
  a.x = bf16(conv);
  a.y = bf16_mut(y);
  a.part = part.data_ptr<float>();
  a.part_ready = nblk;
  a.pool_arg = arg.data_ptr<uint8_t>();
  a.N = (int32_t)N;
  a.H = (int32_t)Ho;
  a.W = (int32_t)Wo;
  a.relu = 1;
  e = launch_bn_fwd(a, st);
  check_hip(e, "psd stem bn_pool");
  return {y, arg, s.mean, s.invstd, s.ss, conv};
}

// Weight gradient of the stem conv (kernels/stem.hip): x [N, 3, H, W], dy [N, 64, H/2, W/2] (both
// channels_last bf16) -> dW [64, 3, 7, 7] bf16 channels_last.
at::Tensor stem_wgrad(const at::Tensor& x_in, const at::Tensor& dy_in) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kBFloat16 && x_in.dim() == 4 && x_in.size(1) == 3,
              "psd stem wgrad: bf16 [N, 3, H, W] input");
  const c10::DeviceGuard g(x_in.device());
  at::Tensor x = x_in.contiguous(at::MemoryFormat::ChannelsLast);
  const int64_t N = x.size(0), H = x.size(2), W = x.size(3), Ho = H / 2, Wo = W / 2;
  TORCH_CHECK(dy_in.scalar_type() == at::kBFloat16 && dy_in.sizes() == at::IntArrayRef({N, 64, Ho, Wo}) &&
                  dy_in.device() == x.device(),
              "psd stem wgrad: dy shape");
  at::Tensor dy = dy_in.contiguous(at::MemoryFormat::ChannelsLast);
  TORCH_CHECK(stem_wgrad_supported((int)H, (int)W, (int)Ho, (int)Wo), "psd stem wgrad: unsupported input ", x.sizes());
  const int nblk = stem_wgrad_blocks((int)N, (int)Ho, (int)Wo);
  at::Tensor part = at::empty({(int64_t)nblk * 192 * 64}, x.options().dtype(at::kFloat));
  at::Tensor dw = at::empty({64, 3, 7, 7}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  hipError_t e = launch_stem_wgrad(bf16(x), bf16(dy), part.data_ptr<float>(), bf16_mut(dw), (int)N, (int)H, (int)W,
                                   (int)Ho, (int)Wo, stream_of(x));
  check_hip(e, "psd stem wgrad");
  return dw;
}

}  // namespace psd
