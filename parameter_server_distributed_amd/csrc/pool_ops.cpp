// Tensor glue for the NHWC pooling kernels (kernels/pool.hip): 3x3/s2/p1 max-pool, global average
// pool and the 2x2 subsample.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "glue.h"
#include "kernels/launchers_pool.h"
#include "ops.h"

namespace psd {

std::vector<at::Tensor> maxpool3s2_fwd(const at::Tensor& x_in) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kBFloat16 && x_in.dim() == 4, "psd maxpool: bf16 NCHW-shaped");
  const c10::DeviceGuard g(x_in.device());
  at::Tensor x = x_in.contiguous(at::MemoryFormat::ChannelsLast);
  const int N = x.size(0), C = x.size(1), H = x.size(2), W = x.size(3);
  const int Ho = (H + 2 - 3) / 2 + 1, Wo = (W + 2 - 3) / 2 + 1;
  at::Tensor y = at::empty({N, C, Ho, Wo}, x.options().memory_format(at::MemoryFormat::ChannelsLast));
  at::Tensor arg = at::empty({N, C, Ho, Wo}, x.options().dtype(at::kByte).memory_format(at::MemoryFormat::ChannelsLast));
  hipError_t e = launch_maxpool_fwd(bf16(x), bf16_mut(y), arg.data_ptr<uint8_t>(), N, H, W, C, Ho, Wo, stream_of(x));
  check_hip(e, "psd maxpool fwd");
  return {y, arg};
}

at::Tensor maxpool3s2_bwd(const at::Tensor& dy_in, const at::Tensor& arg, int64_t H, int64_t W,
                          const c10::optional<at::Tensor>& dy2_in) {
  TORCH_CHECK(dy_in.is_cuda() && dy_in.scalar_type() == at::kBFloat16 && dy_in.dim() == 4,
              "psd maxpool bwd: bf16 NCHW-shaped dy on the device");
  const c10::DeviceGuard g(dy_in.device());
  at::Tensor dy = dy_in.contiguous(at::MemoryFormat::ChannelsLast);
  const int N = dy.size(0), C = dy.size(1), Ho = dy.size(2), Wo = dy.size(3);
  TORCH_CHECK(arg.is_contiguous(at::MemoryFormat::ChannelsLast) && arg.sizes() == dy.sizes() &&
                  arg.scalar_type() == at::kByte && arg.device() == dy.device(),
              "psd maxpool bwd: argmax shape");
  at::Tensor dy2;
  if (given(dy2_in)) {
    TORCH_CHECK(dy2_in->sizes() == dy.sizes() && dy2_in->scalar_type() == at::kBFloat16 && dy2_in->device() == dy.device(),
                "psd maxpool bwd: dy2 shape/dtype");
    dy2 = dy2_in->contiguous(at::MemoryFormat::ChannelsLast);
  }
  at::Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  hipError_t e = launch_maxpool_bwd(bf16(dy), ptr_or_null<const uint16_t>(dy2), arg.data_ptr<uint8_t>(), bf16_mut(dx), N,
                                    (int)H, (int)W, C, Ho, Wo, stream_of(dy));
  check_hip(e, "psd maxpool bwd");
  return dx;
}

at::Tensor gap_fwd(const at::Tensor& x_in) {
  TORCH_CHECK(x_in.is_cuda() && x_in.scalar_type() == at::kBFloat16 && x_in.dim() == 4 && x_in.size(1) % 8 == 0,
              "psd gap: bf16 NCHW-shaped, C % 8 == 0");
  const c10::DeviceGuard g(x_in.device());
  at::Tensor x = x_in.contiguous(at::MemoryFormat::ChannelsLast);
  const int N = x.size(0), C = x.size(1), HW = x.size(2) * x.size(3);
  at::Tensor y = at::empty({N, C}, x.options());
  hipError_t e = launch_gap_fwd(bf16(x), bf16_mut(y), N, HW, C, stream_of(x));
  check_hip(e, "psd gap fwd");
  return y;
}

at::Tensor gap_bwd(const at::Tensor& dy_in, int64_t H, int64_t W) {
  TORCH_CHECK(dy_in.is_cuda() && dy_in.scalar_type() == at::kBFloat16 && dy_in.dim() == 2 && dy_in.size(1) % 8 == 0,
              "psd gap bwd: bf16 [N, C], C % 8 == 0");
  const c10::DeviceGuard g(dy_in.device());
  at::Tensor dy = dy_in.contiguous();
  const int N = dy.size(0), C = dy.size(1);
  at::Tensor dx = at::empty({N, C, H, W}, dy.options().memory_format(at::MemoryFormat::ChannelsLast));
  hipError_t e = launch_gap_bwd(bf16(dy), bf16_mut(dx), N, (int)(H * W), C, stream_of(dy));
  check_hip(e, "psd gap bwd");
  return dx;
}

at::Tensor subsample2(const at::Tensor& x) {
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == at::kBFloat16 && x.dim() == 4 &&
                  x.is_contiguous(at::MemoryFormat::ChannelsLast) && x.size(1) % 8 == 0 && x.size(2) % 2 == 0 &&
                  x.size(3) % 2 == 0,
              "psd subsample2: channels_last bf16 [N, C, H, W], C % 8 == 0, H and W even");
  const c10::DeviceGuard g(x.device());
  at::Tensor y = at::empty({x.size(0), x.size(1), x.size(2) / 2, x.size(3) / 2},
                           x.options().memory_format(at::MemoryFormat::ChannelsLast));
  hipError_t e = launch_subsample2(bf16(x), bf16_mut(y), (int)x.size(0), (int)x.size(2), (int)x.size(3), (int)x.size(1),
                                   stream_of(x));
  check_hip(e, "psd subsample2");
  return y;
}

}  // namespace psd
