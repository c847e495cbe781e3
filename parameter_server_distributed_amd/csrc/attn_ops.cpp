// Tensor glue for the fused self-attention kernels: kernels/attention.hip (S <= 128, the whole head in
// LDS) and kernels/attention_long.hip (128 < S <= 4096, streaming); attn_fwd / attn_bwd dispatch on S.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "glue.h"
#include "kernels/launchers_attn.h"
#include "kernels/launchers_gemm.h"

namespace psd {

namespace {
// packed documents are served by the causal kernels only (checked first: an argument error, whatever the tensors)
void check_docs(const c10::optional<at::Tensor>& doc_start, bool causal) {
  TORCH_CHECK(!given(doc_start) || causal,
              "psd attn: doc_start needs causal=True (the kernels do not serve bidirectional packing)");
}
// a sliding window (window = W >= 1 keys, the query's own included) is causal; 0 is off (also checked first)
void check_window(int64_t window, bool causal) {
  TORCH_CHECK(window >= 0, "psd attn: window must be >= 0 (0: off), got ", window);
  TORCH_CHECK(window == 0 || causal, "psd attn: window needs causal=True (the kernels serve no symmetric window)");
}
void check_attn(const at::Tensor& t, const char* what) {
  TORCH_CHECK(t.is_cuda() && t.scalar_type() == at::kBFloat16 && t.is_contiguous(), "psd attn: ", what,
              " must be a contiguous bf16 device tensor");
}
AttnArgs make_args(const at::Tensor& qkv, int64_t heads, double p, int64_t seed, const c10::optional<at::Tensor>& step,
                   const c10::optional<at::Tensor>& lens, int64_t grid_cap, bool causal,
                   const c10::optional<at::Tensor>& doc_start, int64_t window) {
  TORCH_CHECK(qkv.dim() == 3 && heads > 0 && qkv.size(2) % (3 * heads) == 0, "psd attn: qkv must be [B, S, 3*H*Dh]");
  const int64_t dh = qkv.size(2) / (3 * heads);
  TORCH_CHECK(attn_supported((int)qkv.size(1), (int)dh) || attn_long_supported((int)qkv.size(1), (int)dh),
              "psd attn: needs head dim 64 and S in {32, 64, 96, 128} (whole-head kernels) or a multiple of 64 in "
              "192 .. 4096 (streaming kernels)");
  TORCH_CHECK(window == 0 || attn_long_supported((int)qkv.size(1), (int)dh),
              "psd attn: window is served by the streaming kernels only (S a multiple of 64 in 192 .. 4096), got S = ",
              qkv.size(1));
  TORCH_CHECK(p >= 0.0 && p < 1.0, "psd attn: dropout p must be in [0, 1)");
  AttnArgs a{};
  a.qkv = reinterpret_cast<const uint16_t*>(qkv.data_ptr());
  a.B = (int32_t)qkv.size(0);
  a.S = (int32_t)qkv.size(1);
  a.H = (int32_t)heads;
  a.scale = (float)(1.0 / std::sqrt((double)dh));
  a.thresh = p > 0.0 ? (uint32_t)std::min(4294967295.0, std::floor(p * 4294967296.0)) : 0u;
  a.rescale = (float)(1.0 / (1.0 - p));
  a.seed = (uint32_t)seed;
  a.step = given(step) ? step->data_ptr<int64_t>() : nullptr;
  if (given(lens)) {  // per-sequence lengths, clamped and read on the device only
    TORCH_CHECK(lens->scalar_type() == at::kInt && lens->is_contiguous() && lens->numel() == qkv.size(0) &&
                    lens->device() == qkv.device(),
                "psd attn: lens must be a contiguous int32 [B] tensor on qkv's device");
    a.lens = lens->data_ptr<int32_t>();
  }
  TORCH_CHECK(grid_cap >= 0 && grid_cap <= INT32_MAX, "psd attn: grid_cap must be >= 0");
  a.grid_cap = (int32_t)grid_cap;
  a.causal = causal ? 1 : 0;  // query q sees keys <= q (and < its length): the CAUSAL kernel copies
  if (given(doc_start)) {  // packed documents: clamped and compared on the device only, never read by the host
    TORCH_CHECK(doc_start->scalar_type() == at::kInt && doc_start->is_contiguous() && doc_start->dim() == 2 &&
                    doc_start->size(0) == qkv.size(0) && doc_start->size(1) == qkv.size(1) &&
                    doc_start->device() == qkv.device(),
                "psd attn: doc_start must be a contiguous int32 [B, S] tensor on qkv's device");
    a.doc = doc_start->data_ptr<int32_t>();
  }
  // window > 0 always takes the WINDOW copies; W >= S is the plain causal / document mask, so S stands for more
  a.window = (int32_t)std::min<int64_t>(window, qkv.size(1));
  return a;
}
}  // namespace

std::vector<at::Tensor> attn_fwd(const at::Tensor& qkv, int64_t heads, double p, int64_t seed,
                                 c10::optional<at::Tensor> step, c10::optional<at::Tensor> lens, int64_t grid_cap,
                                 bool causal, c10::optional<at::Tensor> doc_start, int64_t window) {
  check_docs(doc_start, causal);
  check_window(window, causal);
  check_attn(qkv, "qkv");
  const c10::DeviceGuard g(qkv.device());
  AttnArgs a = make_args(qkv, heads, p, seed, step, lens, grid_cap, causal, doc_start, window);
  at::Tensor o = at::empty({qkv.size(0), qkv.size(1), qkv.size(2) / 3}, qkv.options());
  at::Tensor lse = at::empty({qkv.size(0), heads, qkv.size(1)}, qkv.options().dtype(at::kFloat));
  a.o = reinterpret_cast<uint16_t*>(o.data_ptr());
  a.lse = lse.data_ptr<float>();
  hipError_t e = attn_long_supported(a.S, (int)(qkv.size(2) / (3 * heads))) ? launch_attn_long_fwd(a, stream_of(qkv))
                                                                            : launch_attn_fwd(a, stream_of(qkv));
  check_hip(e, "psd attn fwd");
  return {o, lse};
}

// bias_out (optional, [3*H*Dh] bf16/fp32): also the QKV Linear's bias gradient = the column sums of
// dqkv, from per-sequence (streaming kernels: per 128-row tile) partials the kernel writes + one
// deterministic column reduce (with lens the padded rows of dqkv are written as zeros, so the same
// sums hold).
// lens (optional, int32 [B]): valid rows per sequence; grid_cap > 0 bounds the persistent grid (tests);
// causal: the mask the forward used (keys <= q); doc_start (optional, int32 [B, S], causal only): the
// document starts the forward used (keys doc_start[b, q] <= key <= q); window: the forward's window.
at::Tensor attn_bwd(const at::Tensor& dout_in, const at::Tensor& qkv, const at::Tensor& o, const at::Tensor& lse,
                    int64_t heads, double p, int64_t seed, c10::optional<at::Tensor> step,
                    c10::optional<at::Tensor> bias_out, c10::optional<at::Tensor> lens, int64_t grid_cap,
                    bool causal, c10::optional<at::Tensor> doc_start, int64_t window) {
  check_docs(doc_start, causal);
  check_window(window, causal);
  at::Tensor dout = dout_in.contiguous();
  check_attn(dout, "dout");
  check_attn(qkv, "qkv");
  check_attn(o, "o");
  const c10::DeviceGuard g(qkv.device());
  AttnArgs a = make_args(qkv, heads, p, seed, step, lens, grid_cap, causal, doc_start, window);
  TORCH_CHECK(o.sizes() == dout.sizes() && o.size(0) == qkv.size(0) && o.size(1) == qkv.size(1) &&
                  o.size(2) * 3 == qkv.size(2),
              "psd attn bwd: o / dout must be [B, S, H*Dh]");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.is_contiguous() &&
                  lse.numel() == (int64_t)a.B * a.H * a.S,
              "psd attn bwd: lse must be fp32 [B, H, S]");
  at::Tensor dqkv = at::empty_like(qkv);
  a.o = reinterpret_cast<uint16_t*>(o.data_ptr());
  a.lse = lse.data_ptr<float>();
  a.dout = reinterpret_cast<const uint16_t*>(dout.data_ptr());
  a.dqkv = reinterpret_cast<uint16_t*>(dqkv.data_ptr());
  const bool bias = given(bias_out);
  const bool is_long = attn_long_supported(a.S, (int)(qkv.size(2) / (3 * heads)));
  const int prows = is_long ? attn_long_bpart_rows(a.B, a.S) : a.B;  // partial rows: one per work item of a sequence
  at::Tensor bpart;
  if (bias) {
    TORCH_CHECK(bias_out->is_cuda() && bias_out->is_contiguous() && bias_out->numel() == qkv.size(2) &&
                    (bias_out->scalar_type() == at::kBFloat16 || bias_out->scalar_type() == at::kFloat),
                "psd attn bwd: bias_out must be a contiguous [3*H*Dh] bf16/fp32 tensor");
    bpart = at::empty({(int64_t)prows, qkv.size(2)}, qkv.options().dtype(at::kFloat));
    a.bpart = bpart.data_ptr<float>();
  }
  hipError_t e;
  if (is_long) {  // D = rowsum(dO . O): written by the dQ pass, read by the dK/dV pass
    at::Tensor dsum = at::empty({(int64_t)a.B, heads, (int64_t)a.S}, qkv.options().dtype(at::kFloat));
    e = launch_attn_long_bwd(a, dsum.data_ptr<float>(), stream_of(qkv));
  } else {
    e = launch_attn_bwd(a, stream_of(qkv));
  }
  check_hip(e, "psd attn bwd");
  if (bias) {
    e = launch_colsum_final(a.bpart, prows, (int)qkv.size(2), bias_out->data_ptr(),
                            bias_out->scalar_type() == at::kBFloat16, 0, stream_of(qkv));
    check_hip(e, "psd attn bwd bias");
  }
  return dqkv;
}

}  // namespace psd
