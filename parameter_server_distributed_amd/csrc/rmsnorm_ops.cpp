// Tensor glue for the fused residual add + dropout + RMSNorm kernels (kernels/rmsnorm.hip). Every check
// runs before any allocation or launch and names the argument it rejects.
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "glue.h"
#include "kernels/launchers_rmsnorm.h"
#include "ops.h"

namespace psd {

namespace {
void check_act(const char* op, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.defined() && t.is_cuda(), op, ": ", name, " must be a device tensor");
  TORCH_CHECK(t.scalar_type() == at::kBFloat16, op, ": ", name, " must be bf16, got ", t.scalar_type());
  TORCH_CHECK(t.is_contiguous(), op, ": ", name, " must be contiguous");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 7) == 0, op, ": ", name, " must be 8-byte aligned");
}
void check_like(const char* op, const at::Tensor& t, const at::Tensor& like, const char* name, const char* like_name) {
  check_act(op, t, name);
  TORCH_CHECK(t.device() == like.device(), op, ": ", name, " must be on ", like_name, "'s device");
  TORCH_CHECK(t.sizes() == like.sizes(), op, ": ", name, " must have ", like_name, "'s shape ", like.sizes(), ", got ",
              t.sizes());
}
void check_gamma(const char* op, const at::Tensor& gamma, const at::Tensor& like, int64_t H, const char* name) {
  check_act(op, gamma, name);
  TORCH_CHECK(gamma.device() == like.device(), op, ": ", name, " must be on the input's device");
  TORCH_CHECK(gamma.dim() == 1 && gamma.numel() == H, op, ": ", name, " must be [", H, "], got ", gamma.sizes());
}
const int64_t* check_step(const char* op, const c10::optional<at::Tensor>& step, const at::Tensor& like) {
  if (!given(step)) return nullptr;
  TORCH_CHECK(step->scalar_type() == at::kLong, op, ": step must be an int64 tensor, got ", step->scalar_type());
  TORCH_CHECK(step->is_cuda() && step->device() == like.device() && step->numel() >= 1, op,
              ": step must hold one element on the input's device");
  return step->data_ptr<int64_t>();
}
int64_t check_hidden(const char* op, const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.dim() >= 1, op, ": ", name, " must have at least one dimension");
  const int64_t H = t.size(-1);
  TORCH_CHECK(rms_supported((int)H), op, ": ", name, " must have a last dimension (H) of 768 or 1024, got ", H);
  return H;
}
void check_p(const char* op, double p) { TORCH_CHECK(p >= 0.0 && p < 1.0, op, ": p must be in [0, 1), got ", p); }
}  // namespace

// r_new = bf16(r + dropout_p(h)), rstd = rsqrt(mean(r_new^2) + eps) [rows] fp32, y = bf16(r_new * rstd * gamma).
// Without h, r_new is r itself (the same tensor is returned, nothing is written) and p / seed / step are ignored.
std::vector<at::Tensor> rms_fwd(const at::Tensor& r, c10::optional<at::Tensor> h, const at::Tensor& gamma, double eps,
                                double p, int64_t seed, c10::optional<at::Tensor> step) {
  const char* op = "psd rms_fwd";
  check_act(op, r, "r");
  const int64_t H = check_hidden(op, r, "r");
  const bool add = given(h);
  if (add) check_like(op, *h, r, "h", "r");
  check_gamma(op, gamma, r, H, "gamma");
  const int64_t* stp = nullptr;
  if (add) {
    check_p(op, p);
    stp = check_step(op, step, r);
  }
  const c10::DeviceGuard g(r.device());
  const int64_t rows = r.numel() / H;
  at::Tensor r_new = add ? at::empty_like(r) : r;
  at::Tensor y = at::empty_like(r);
  at::Tensor rstd = at::empty({rows}, r.options().dtype(at::kFloat));
  RmsArgs a{};
  a.r = bf16(r);
  a.h = add ? bf16(*h) : nullptr;
  a.gamma = bf16(gamma);
  a.r_new = add ? bf16_mut(r_new) : nullptr;
  a.y = bf16_mut(y);
  a.rstd = rstd.data_ptr<float>();
  a.step = stp;
  a.rows = rows;
  a.H = (int32_t)H;
  a.eps = (float)eps;
  a.p = add ? (float)p : 0.f;
  a.seed = (uint32_t)seed;
  check_hip(launch_rms_fwd(a, stream_of(r)), op);
  return {r_new, y, rstd};
}

// dr = bf16(dr_new + rstd * (g - xh * mean(g * xh))) with xh = r_new * rstd, g = dy * gamma; dh = bf16 of the
// fp32 dr * keep / (1 - p) (p == 0: the tensor dr itself; had_h false: none); dgamma = column sums of dy * xh
// into dgamma_out when given.
std::vector<at::Tensor> rms_bwd(const at::Tensor& dy, c10::optional<at::Tensor> dr_new, const at::Tensor& r_new,
                                const at::Tensor& rstd, const at::Tensor& gamma, double p, int64_t seed,
                                c10::optional<at::Tensor> step, bool had_h, c10::optional<at::Tensor> dgamma_out) {
  const char* op = "psd rms_bwd";
  check_act(op, r_new, "r_new");
  const int64_t H = check_hidden(op, r_new, "r_new");
  check_like(op, dy, r_new, "dy", "r_new");
  const bool drn = given(dr_new);
  if (drn) check_like(op, *dr_new, r_new, "dr_new", "r_new");
  const int64_t rows = r_new.numel() / H;
  TORCH_CHECK(rstd.defined() && rstd.is_cuda() && rstd.device() == r_new.device() && rstd.scalar_type() == at::kFloat &&
                  rstd.is_contiguous() && rstd.numel() == rows,
              op, ": rstd must be a contiguous fp32 [", rows, "] tensor on r_new's device");
  check_gamma(op, gamma, r_new, H, "gamma");
  check_p(op, p);
  const int64_t* stp = check_step(op, step, r_new);
  if (given(dgamma_out)) check_gamma(op, *dgamma_out, r_new, H, "dgamma_out");
  const c10::DeviceGuard g(r_new.device());
  at::Tensor dr = at::empty_like(r_new);
  at::Tensor dh;
  if (had_h) dh = p > 0.0 ? at::empty_like(r_new) : dr;
  at::Tensor dgamma = given(dgamma_out) ? *dgamma_out : at::empty({H}, r_new.options());
  at::Tensor part = at::empty({(int64_t)rms_bwd_blocks(rows) * H}, r_new.options().dtype(at::kFloat));
  RmsArgs a{};
  a.dy = bf16(dy);
  a.dr_new = drn ? bf16(*dr_new) : nullptr;
  a.rn = bf16(r_new);
  a.rstd_in = rstd.data_ptr<float>();
  a.gamma = bf16(gamma);
  a.dr = bf16_mut(dr);
  a.dh = (had_h && p > 0.0) ? bf16_mut(dh) : nullptr;
  a.dgamma = bf16_mut(dgamma);
  a.part = part.data_ptr<float>();
  a.step = stp;
  a.rows = rows;
  a.H = (int32_t)H;
  a.p = had_h ? (float)p : 0.f;
  a.seed = (uint32_t)seed;
  check_hip(launch_rms_bwd(a, stream_of(r_new)), op);
  return {dr, dh, dgamma};
}

}  // namespace psd
