// Tensor glue for the rotary position embedding pass (kernels/rope.hip): rope_ rotates the Q and K heads of
// a packed qkv in place.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <climits>

#include "glue.h"
#include "kernels/launchers_rope.h"
#include "ops.h"

namespace psd {

namespace {
void check_table(const at::Tensor& t, const at::Tensor& qkv, const char* name) {
  TORCH_CHECK(t.is_cuda() && t.device() == qkv.device() && t.scalar_type() == at::kFloat && t.is_contiguous() &&
                  t.dim() == 2 && t.size(1) == 32 && aligned16(t),
              "psd rope: ", name, " must be a contiguous fp32 [P, 32] tensor on qkv's device");
  TORCH_CHECK(t.size(0) >= qkv.size(1), "psd rope: ", name, " has ", t.size(0), " rows, fewer than S = ", qkv.size(1));
}
}  // namespace

// qkv: bf16 contiguous [B, S, 3*heads*64] (Q heads, K heads, V heads), rotated in place and returned.
// cos / sin: fp32 [P, 32], P >= S. lens (optional, int32 [B]): rows past a length are not touched.
// doc_start (optional, int32 [B, S], with or without lens): positions restart at each document.
// inverse: the angle negated (the backward). blocks > 0 bounds the grid (tests); the bits do not depend on it.
at::Tensor rope_(at::Tensor qkv, int64_t heads, const at::Tensor& cos, const at::Tensor& sin,
                 c10::optional<at::Tensor> lens, c10::optional<at::Tensor> doc_start, bool inverse, int64_t blocks) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.is_contiguous() && aligned16(qkv),
              "psd rope: qkv must be a contiguous bf16 device tensor");
  TORCH_CHECK(heads > 0 && heads <= (1 << 20), "psd rope: heads must be positive, got ", heads);
  TORCH_CHECK(qkv.dim() == 3 && qkv.size(2) == 3 * heads * 64,
              "psd rope: qkv must be [B, S, 3*heads*64] (head dim 64), got last dim ", qkv.dim() == 3 ? qkv.size(2) : -1,
              " with heads = ", heads);
  TORCH_CHECK(qkv.size(0) <= INT32_MAX && qkv.size(1) <= INT32_MAX, "psd rope: qkv has too many rows");
  check_table(cos, qkv, "cos");
  check_table(sin, qkv, "sin");
  TORCH_CHECK(blocks >= 0 && blocks <= INT32_MAX, "psd rope: blocks must be >= 0 (0: the op chooses), got ", blocks);
  RopeArgs a{};
  if (given(lens)) {  // clamped and read on the device only
    TORCH_CHECK(lens->scalar_type() == at::kInt && lens->is_contiguous() && lens->dim() == 1 &&
                    lens->numel() == qkv.size(0) && lens->device() == qkv.device(),
                "psd rope: lens must be a contiguous int32 [B] tensor on qkv's device");
    a.lens = lens->data_ptr<int32_t>();
  }
  if (given(doc_start)) {  // clamped and subtracted on the device only, never read by the host
    TORCH_CHECK(doc_start->scalar_type() == at::kInt && doc_start->is_contiguous() && doc_start->dim() == 2 &&
                    doc_start->size(0) == qkv.size(0) && doc_start->size(1) == qkv.size(1) &&
                    doc_start->device() == qkv.device(),
                "psd rope: doc_start must be a contiguous int32 [B, S] tensor on qkv's device");
    a.doc = doc_start->data_ptr<int32_t>();
  }
  const c10::DeviceGuard g(qkv.device());
  a.qkv = bf16_mut(qkv);
  a.cos = cos.data_ptr<float>();
  a.sin = sin.data_ptr<float>();
  a.B = (int32_t)qkv.size(0);
  a.S = (int32_t)qkv.size(1);
  a.H = (int32_t)heads;
  a.inverse = inverse ? 1 : 0;
  a.blocks = (int32_t)blocks;
  check_hip(launch_rope(a, stream_of(qkv)), "psd rope");
  return qkv;
}

}  // namespace psd
