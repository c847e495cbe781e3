// Tensor glue for the fused NHWC BatchNorm kernels (kernels/bn.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "glue.h"
#include "kernels/launchers_bn.h"
#include "ops.h"

namespace psd {

namespace {

at::Tensor nhwc(const at::Tensor& t) {
  if (t.dim() == 4) return t.contiguous(at::MemoryFormat::ChannelsLast);
  return t.contiguous();
}

int64_t channels(const at::Tensor& t) { return t.dim() == 4 ? t.size(1) : t.size(-1); }

// The BN input as the kernels read it (NHWC; a 2-D [pixels, C] stays as it is) with its channel and
// pixel counts. Every entry starts here: a host tensor is refused before anything touches the device.
struct BnIn {
  at::Tensor x;
  int64_t C, M;
};
BnIn bn_input(const at::Tensor& x_in, const char* op) {
  TORCH_CHECK(x_in.is_cuda(), op, ": x must be a device tensor");
  TORCH_CHECK(x_in.scalar_type() == at::kBFloat16 && x_in.dim() >= 1, op, ": x must be bf16 [N, C, H, W] or [pixels, C]");
  const int64_t C = channels(x_in);
  TORCH_CHECK(C > 0 && C % 8 == 0, op, ": channels must be a multiple of 8, got ", C);
  return {nhwc(x_in), C, x_in.numel() / C};
}

at::TensorOptions f32_like(const BnIn& in) { return in.x.options().dtype(at::kFloat); }

// an activation-shaped argument (dy, dy2, g, xd, the residual, y): bf16 with x's sizes on x's device,
// returned NHWC; an optional one that is absent gives the undefined tensor
at::Tensor like_x(const at::Tensor& t, const BnIn& in, const char* op, const char* name) {
  TORCH_CHECK(t.defined() && t.sizes() == in.x.sizes() && t.scalar_type() == at::kBFloat16 &&
                  t.device() == in.x.device(),
              op, ": ", name, " must be bf16 with x's shape on x's device");
  return nhwc(t);
}
at::Tensor like_x(const c10::optional<at::Tensor>& t, const BnIn& in, const char* op, const char* name) {
  return given(t) ? like_x(*t, in, op, name) : at::Tensor();
}

// gamma (optional: absent means no affine) and the saved statistics of one BN
void check_stats(const char* op, const BnIn& in, const c10::optional<at::Tensor>& gamma, const at::Tensor& mean,
                 const at::Tensor& invstd) {
  check_vec(op, gamma, in.C, at::kBFloat16, in.x, "gamma");
  check_vec(op, mean, in.C, at::kFloat, in.x, "save_mean");
  check_vec(op, invstd, in.C, at::kFloat, in.x, "save_invstd");
}

// the forward ReLU bit-mask: 1 bit per element of x
void check_mbits(const char* op, const at::Tensor& m, const BnIn& in) {
  TORCH_CHECK(m.defined() && m.scalar_type() == at::kByte && m.is_contiguous() && m.numel() == in.M * in.C / 8 &&
                  m.device() == in.x.device(),
              op, ": mbits must be uint8 [M*C/8] on x's device");
}

// producer-reduced partials: at least `rows` rows of [2, C] fp32
void check_part(const char* op, const at::Tensor& p, int64_t rows, int64_t C, const at::Tensor& like, const char* name) {
  TORCH_CHECK(rows > 0 && p.defined() && p.scalar_type() == at::kFloat && p.is_contiguous() &&
                  p.numel() >= rows * 2 * C && p.device() == like.device(),
              op, ": ", name, " must be fp32 [rows, 2, C] on the input's device");
}

// a parameter-gradient buffer: the caller's sink view (bf16 contiguous [C]) or a fresh one
at::Tensor grad_buf(const char* op, const c10::optional<at::Tensor>& o, const BnIn& in, const char* name) {
  if (!given(o)) return at::empty({in.C}, in.x.options());
  check_vec(op, o, in.C, at::kBFloat16, in.x, name);
  return *o;
}

// the kernels' own reduction partials
at::Tensor reduce_ws(const BnIn& in) {
  return at::empty({(int64_t)bn_reduce_blocks(in.M, (int)in.C), 2, in.C}, f32_like(in));
}

// the slab workspace that folds more than kFoldRows producer partial rows; undefined when not needed
at::Tensor fold_ws(int64_t rows, int64_t C, const at::TensorOptions& f32) {
  return rows > kFoldRows ? at::empty({(int64_t)kFoldRows * 2 * C}, f32) : at::Tensor();
}

// what every BnBwdArgs launch shares: the gradients (dy absent: the pool fusion), the input, the
// parameters and the saved statistics. The entries add what differs.
BnBwdArgs bwd_args(const BnIn& in, const at::Tensor& dy, const at::Tensor& dy2, const c10::optional<at::Tensor>& gamma,
                   const at::Tensor& save_mean, const at::Tensor& save_invstd) {
  BnBwdArgs a{};
  a.dy = ptr_or_null<const uint16_t>(dy);
  a.dy2 = ptr_or_null<const uint16_t>(dy2);
  a.x = bf16(in.x);
  a.gamma = opt_ptr<const uint16_t>(gamma);
  a.save_mean = save_mean.data_ptr<float>();
  a.save_invstd = ptr_or_null<const float>(save_invstd);
  a.M = in.M;
  a.C = (int32_t)in.C;
  return a;
}

// a launch_bn_bwd_pre from producer partials, without dx and its MX copy
BnPreArgs pre_args(const BnIn& in, const at::Tensor& g, const c10::optional<at::Tensor>& gamma,
                   const at::Tensor& save_mean, const at::Tensor& save_invstd, const at::Tensor& part, int64_t rows,
                   const at::Tensor& fold, const at::Tensor& dgamma, const at::Tensor& dbeta, const at::Tensor& coef) {
  BnPreArgs a{};
  a.g = bf16(g);
  a.x = bf16(in.x);
  a.gamma = opt_ptr<const uint16_t>(gamma);
  a.mean = save_mean.data_ptr<float>();
  a.invstd = save_invstd.data_ptr<float>();
  a.part = part.data_ptr<float>();
  a.rows = (int)rows;
  a.fold_ws = ptr_or_null<float>(fold);
  a.dgamma = ptr_or_null<uint16_t>(dgamma);
  a.dbeta = ptr_or_null<uint16_t>(dbeta);
  a.coef = coef.data_ptr<float>();
  a.M = in.M;
  a.C = (int)in.C;
  return a;
}

// optional MX e5m2 side output of a BN backward elementwise pass (dq like x, E8M0 scales [numel/32])
void set_dq(c10::optional<at::Tensor>& dq, c10::optional<at::Tensor>& dqmx, const at::Tensor& x, uint8_t*& q,
            uint8_t*& sc) {
  q = sc = nullptr;
  if (!given(dq)) return;
  const at::Tensor& t = *dq;
  const bool laid = nhwc_laid(t);
  TORCH_CHECK(t.scalar_type() == at::kFloat8_e5m2 && t.sizes() == x.sizes() && laid && t.device() == x.device() &&
                  given(dqmx) && dqmx->scalar_type() == at::kByte && dqmx->is_contiguous() &&
                  dqmx->numel() * 32 == x.numel() && dqmx->device() == x.device() && channels(x) % 32 == 0,
              "psd bn bwd: dq must be e5m2 laid out like x with uint8 [numel / 32] scales (channels % 32 == 0)");
  q = reinterpret_cast<uint8_t*>(t.data_ptr());
  sc = dqmx->data_ptr<uint8_t>();
}

}  // namespace

BnFwdStats bn_fwd_stats(BnFwdArgs& a, const at::Tensor& like, int64_t M, int64_t C,
                        const c10::optional<at::Tensor>& gamma, const c10::optional<at::Tensor>& beta,
                        const c10::optional<at::Tensor>& running_mean, const c10::optional<at::Tensor>& running_var,
                        const c10::optional<at::Tensor>& counter, double momentum, double eps, bool training,
                        const c10::optional<at::Tensor>& ss_eval) {
  check_vec("psd bn", gamma, C, at::kBFloat16, like, "gamma");
  check_vec("psd bn", beta, C, at::kBFloat16, like, "beta");
  check_vec("psd bn", running_mean, C, at::kFloat, like, "running_mean");
  check_vec("psd bn", running_var, C, at::kFloat, like, "running_var");
  check_vec("psd bn", counter, 1, at::kLong, like, "counter");
  const auto f32 = like.options().dtype(at::kFloat);
  BnFwdStats s{at::empty({C}, f32), at::empty({C}, f32), at::Tensor()};
  if (training) {
    s.ss = at::empty({2 * C}, f32);
  } else {
    TORCH_CHECK(given(ss_eval), "psd bn: eval mode needs ss_eval [2C]");
    s.ss = ss_eval->contiguous();
    check_vec("psd bn", s.ss, 2 * C, at::kFloat, like, "ss_eval");
  }
  a.gamma = opt_ptr<const uint16_t>(gamma);
  a.beta = opt_ptr<const uint16_t>(beta);
  a.running_mean = training ? opt_ptr<float>(running_mean) : nullptr;
  a.running_var = training ? opt_ptr<float>(running_var) : nullptr;
  a.save_mean = s.mean.data_ptr<float>();
  a.save_invstd = s.invstd.data_ptr<float>();
  a.ss = s.ss.data_ptr<float>();
  a.counter = training ? opt_ptr<int64_t>(counter) : nullptr;
  a.M = M;
  a.C = (int32_t)C;
  a.training = training;
  a.momentum = (float)momentum;
  a.eps = (float)eps;
  return s;
}

std::vector<at::Tensor> bn_fwd(const at::Tensor& x_in, c10::optional<at::Tensor> gamma, c10::optional<at::Tensor> beta,
                               c10::optional<at::Tensor> running_mean, c10::optional<at::Tensor> running_var,
                               c10::optional<at::Tensor> residual, bool relu, bool training, double momentum, double eps,
                               c10::optional<at::Tensor> counter, c10::optional<at::Tensor> ss_eval, bool mask_out,
                               c10::optional<at::Tensor> residual_ss, bool stats_only,
                               c10::optional<at::Tensor> q8_out, c10::optional<at::Tensor> part_in,
                               int64_t part_rows, c10::optional<at::Tensor> q8_mx) {
  const char* op = "psd bn";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  const int64_t C = in.C, M = in.M;
  const at::Tensor res = like_x(residual, in, op, "residual");
  TORCH_CHECK(!stats_only || training, "psd bn: stats_only needs training mode");
  const bool rss = given(residual_ss);
  if (rss) {
    TORCH_CHECK(res.defined() && relu, "psd bn: residual_ss [2C] fp32 needs a residual and ReLU");
    check_vec(op, residual_ss, 2 * C, at::kFloat, x, "residual_ss");
  }
  at::Tensor y = stats_only ? at::empty({0}, x.options()) : at::empty_like(x);
  at::Tensor mbits;
  if (relu && mask_out && !stats_only) mbits = at::empty({M * C / 8}, x.options().dtype(at::kByte));
  at::Tensor part, fold;
  const bool have_part = training && given(part_in);
  if (have_part) {  // statistics partials from the producing convolution's epilogue (kernels/convn.hip)
    check_part(op, *part_in, part_rows, C, x, "part_in");
    part = *part_in;
    fold = fold_ws(part_rows, C, f32_like(in));
  } else if (training) {
    part = reduce_ws(in);
  }
  BnFwdArgs a{};
  const BnFwdStats s =
      bn_fwd_stats(a, x, M, C, gamma, beta, running_mean, running_var, counter, momentum, eps, training, ss_eval);
  a.x = bf16(x);
  a.res = ptr_or_null<const uint16_t>(res);
  a.y = bf16_mut(y);
  a.mbits = ptr_or_null<uint8_t>(mbits);
  a.part = ptr_or_null<float>(part);
  if (have_part) {
    a.part_ready = (int32_t)part_rows;
    a.fold_ws = ptr_or_null<float>(fold);
  }
  a.relu = relu;
  a.res_ss = rss ? residual_ss->data_ptr<float>() : nullptr;
  a.stats_only = stats_only;
  if (given(q8_out)) {
    const at::Tensor& q = *q8_out;
    const bool laid = nhwc_laid(q);
    TORCH_CHECK(!stats_only && relu && q.scalar_type() == at::kFloat8_e4m3fn && q.sizes() == x.sizes() && laid &&
                    q.device() == x.device() && (reinterpret_cast<uintptr_t>(q.data_ptr()) & 7) == 0,
                "psd bn: q8_out must be an e4m3fn tensor laid out like x (ReLU BNs)");
    a.q8 = reinterpret_cast<uint8_t*>(q.data_ptr());
    // MX: E8M0 per 32 channels
    TORCH_CHECK(given(q8_mx) && q8_mx->scalar_type() == at::kByte && q8_mx->is_contiguous() &&
                    q8_mx->numel() * 32 == x.numel() && C % 32 == 0 && q8_mx->device() == x.device(),
                "psd bn: q8_out needs q8_mx uint8 [numel / 32] (channels % 32 == 0)");
    a.q8mx = q8_mx->data_ptr<uint8_t>();
  }
  hipError_t e = launch_bn_fwd(a, stream_of(x));
  check_hip(e, "psd bn fwd");
  return {y, s.mean, s.invstd, s.ss, mbits};
}

at::Tensor bn_reduce_(const at::Tensor& x_in, const at::Tensor& shift) {
  const char* op = "psd bn_reduce";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  check_vec(op, shift, in.C, at::kFloat, in.x, "shift");
  at::Tensor part = reduce_ws(in);
  const hipError_t e =
      launch_bn_reduce(bf16(in.x), in.M, (int)in.C, shift.data_ptr<float>(), part.data_ptr<float>(), stream_of(in.x));
  check_hip(e, op);
  return part;
}

// Training-mode BN statistics from producer partials only (no activation is read): returns
// {mean, invstd, ss [2C]} and updates the running statistics, as bn_fwd with stats_only.
std::vector<at::Tensor> bn_finalize(const at::Tensor& part, int64_t rows, int64_t M, const at::Tensor& gamma,
                                    const at::Tensor& beta, at::Tensor running_mean, at::Tensor running_var,
                                    double momentum, double eps, c10::optional<at::Tensor> counter) {
  const char* op = "psd bn_finalize";
  TORCH_CHECK(part.is_cuda(), op, ": part must be a device tensor");  // (no activation: part stands in for x)
  const c10::DeviceGuard dg(part.device());
  const int64_t C = running_mean.numel();
  TORCH_CHECK(C > 0 && C % 8 == 0 && M > 0, op, ": channels must be a multiple of 8 and M positive");
  check_part(op, part, rows, C, part, "part");
  BnFwdArgs a{};
  const BnFwdStats s = bn_fwd_stats(a, part, M, C, gamma, beta, running_mean, running_var, counter, momentum, eps);
  const at::Tensor fold = fold_ws(rows, C, part.options());
  a.part = part.data_ptr<float>();
  a.part_ready = (int32_t)rows;
  a.fold_ws = ptr_or_null<float>(fold);
  a.stats_only = true;
  const hipError_t e = launch_bn_fwd(a, stream_of(part));
  check_hip(e, op);
  return {s.mean, s.invstd, s.ss};
}

std::vector<at::Tensor> bn_bwd(const at::Tensor& dy_in, const at::Tensor& x_in, c10::optional<at::Tensor> y_in,
                               c10::optional<at::Tensor> gamma, const at::Tensor& save_mean,
                               const at::Tensor& save_invstd, bool relu, bool need_dr,
                               c10::optional<at::Tensor> dgamma_out, c10::optional<at::Tensor> dbeta_out,
                               c10::optional<at::Tensor> dy2_in, c10::optional<at::Tensor> ss_in,
                               c10::optional<at::Tensor> mbits_in, c10::optional<at::Tensor> dq,
                               c10::optional<at::Tensor> dqmx) {
  const char* op = "psd bn bwd";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor dy = like_x(dy_in, in, op, "dy"), dy2 = like_x(dy2_in, in, op, "dy2");
  check_stats(op, in, gamma, save_mean, save_invstd);
  at::Tensor y, ss, mbits;
  if (relu) {
    // ReLU mask source: the forward bit-mask, the forward output y, or (no residual) x with the
    // forward scale/shift
    if (given(mbits_in)) {
      mbits = *mbits_in;
      TORCH_CHECK(need_dr, "psd bn bwd: the bit-mask path is for residual BNs");
      check_mbits(op, mbits, in);
    } else if (given(y_in)) {
      y = like_x(y_in, in, op, "y");
    } else {
      TORCH_CHECK(given(ss_in), "psd bn bwd: relu needs the forward output or scale/shift");
      TORCH_CHECK(!need_dr, "psd bn bwd: a residual ReLU mask needs the forward output");
      ss = ss_in->contiguous();
      check_vec(op, ss, 2 * in.C, at::kFloat, x, "ss");
    }
  }
  at::Tensor dx = at::empty_like(x);
  at::Tensor dr = need_dr ? at::empty_like(x) : at::Tensor();
  at::Tensor dgamma, dbeta;
  if (given(gamma)) {
    dgamma = grad_buf(op, dgamma_out, in, "dgamma buffer");
    dbeta = grad_buf(op, dbeta_out, in, "dbeta buffer");
  }
  at::Tensor coef = at::empty({3 * in.C}, f32_like(in));
  at::Tensor part = reduce_ws(in);
  BnBwdArgs a = bwd_args(in, dy, dy2, gamma, save_mean, save_invstd);
  a.y = ptr_or_null<const uint16_t>(y);
  a.ss = ptr_or_null<const float>(ss);
  a.mbits = ptr_or_null<const uint8_t>(mbits);
  a.dx = bf16_mut(dx);
  a.dr = ptr_or_null<uint16_t>(dr);
  a.dgamma = ptr_or_null<uint16_t>(dgamma);
  a.dbeta = ptr_or_null<uint16_t>(dbeta);
  a.coef = coef.data_ptr<float>();
  a.part = part.data_ptr<float>();
  a.relu = relu;
  set_dq(dq, dqmx, x, a.dq, a.dqmx);
  hipError_t e = launch_bn_bwd(a, stream_of(x));
  check_hip(e, op);
  return {dx, dr, dgamma, dbeta};
}

// The BN backward's reduction pass alone, as the BN would run it after a bwd-data convolution that
// does not fuse it: ReLU mask from x and ss (mbits absent), or the residual BN's bit-mask with the
// residual-branch gradient dy2 folded in and dr written. Autotune timing twin (ops/conv.py).
// Returns the partials.
at::Tensor bn_bwd_reduce_(const at::Tensor& dy_in, const at::Tensor& x_in, const at::Tensor& save_mean,
                          c10::optional<at::Tensor> ss_in, c10::optional<at::Tensor> dy2_in,
                          c10::optional<at::Tensor> mbits_in) {
  const char* op = "psd bn_bwd_reduce";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor dy = like_x(dy_in, in, op, "dy"), dy2 = like_x(dy2_in, in, op, "dy2");
  check_vec(op, save_mean, in.C, at::kFloat, x, "save_mean");
  at::Tensor ss, mbits, dr;
  if (given(mbits_in)) {
    mbits = *mbits_in;
    check_mbits(op, mbits, in);
    dr = at::empty_like(x);
  } else {
    TORCH_CHECK(given(ss_in), "psd bn_bwd_reduce: ss [2C]");
    ss = ss_in->contiguous();
    check_vec(op, ss, 2 * in.C, at::kFloat, x, "ss");
  }
  at::Tensor part = reduce_ws(in);
  BnBwdArgs a = bwd_args(in, dy, dy2, c10::nullopt, save_mean, at::Tensor());
  a.ss = ptr_or_null<const float>(ss);
  a.mbits = ptr_or_null<const uint8_t>(mbits);
  a.dr = ptr_or_null<uint16_t>(dr);
  a.part = part.data_ptr<float>();
  a.relu = 1;
  a.reduce_only = 1;
  const hipError_t e = launch_bn_bwd(a, stream_of(x));
  check_hip(e, op);
  return part;
}

// BN backward whose reduction the producing convolution's bwd-data epilogue already ran
// (kernels/convn.hip bwd modes): g = the masked gradient (for a residual BN also the residual-branch
// gradient), part = [rows, 2, C] partials. Returns {dx, dgamma, dbeta}.
std::vector<at::Tensor> bn_bwd_pre(const at::Tensor& g_in, const at::Tensor& x_in, c10::optional<at::Tensor> gamma,
                                   const at::Tensor& save_mean, const at::Tensor& save_invstd, const at::Tensor& part,
                                   int64_t rows, c10::optional<at::Tensor> dgamma_out,
                                   c10::optional<at::Tensor> dbeta_out, c10::optional<at::Tensor> dq,
                                   c10::optional<at::Tensor> dqmx) {
  const char* op = "psd bn_bwd_pre";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard dg(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor g = like_x(g_in, in, op, "g");
  check_stats(op, in, gamma, save_mean, save_invstd);
  check_part(op, part, rows, in.C, x, "part");
  at::Tensor dx = at::empty_like(x);
  at::Tensor dgamma, dbeta;
  if (given(gamma)) {
    dgamma = grad_buf(op, dgamma_out, in, "dgamma buffer");
    dbeta = grad_buf(op, dbeta_out, in, "dbeta buffer");
  }
  at::Tensor coef = at::empty({3 * in.C}, f32_like(in));
  const at::Tensor fold = fold_ws(rows, in.C, f32_like(in));
  BnPreArgs a = pre_args(in, g, gamma, save_mean, save_invstd, part, rows, fold, dgamma, dbeta, coef);
  a.dx = bf16_mut(dx);
  set_dq(dq, dqmx, x, a.dq, a.dqmx);
  const hipError_t e = launch_bn_bwd_pre(a, stream_of(x));
  check_hip(e, op);
  return {dx, dgamma, dbeta};
}

// relu(bn3(x) + bnd(xd)) backward (ops/bn.py _BNAddBNReluFn): bn3 through its forward bit-mask, and
// the downsample BN fed by the residual gradient dr, in one reduce and one elementwise pass.
// Returns {dx, dxd, dgamma, dbeta, dgamma_d, dbeta_d}.
std::vector<at::Tensor> bn_bwd_dual(const at::Tensor& dy_in, const at::Tensor& x_in, const at::Tensor& gamma,
                                    const at::Tensor& save_mean, const at::Tensor& save_invstd, const at::Tensor& mbits,
                                    c10::optional<at::Tensor> dy2_in, const at::Tensor& xd_in, const at::Tensor& gamma_d,
                                    const at::Tensor& mean_d, const at::Tensor& invstd_d,
                                    c10::optional<at::Tensor> dgamma_out, c10::optional<at::Tensor> dbeta_out,
                                    c10::optional<at::Tensor> dgamma_d_out, c10::optional<at::Tensor> dbeta_d_out,
                                    bool fold) {
  const char* op = "psd bn bwd_dual";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor dy = like_x(dy_in, in, op, "dy"), dy2 = like_x(dy2_in, in, op, "dy2"), xd = like_x(xd_in, in, op, "xd");
  TORCH_CHECK(gamma.defined() && gamma_d.defined(), op, ": gamma and gamma_d are required");
  check_stats(op, in, gamma, save_mean, save_invstd);
  check_stats(op, in, gamma_d, mean_d, invstd_d);
  check_mbits(op, mbits, in);
  at::Tensor dgamma = grad_buf(op, dgamma_out, in, "grad buffer"), dbeta = grad_buf(op, dbeta_out, in, "grad buffer");
  at::Tensor dgamma_d = grad_buf(op, dgamma_d_out, in, "grad buffer"),
             dbeta_d = grad_buf(op, dbeta_d_out, in, "grad buffer");
  const auto f32 = f32_like(in);
  // fold: no dx (the consumer convolution folds it); its coefficients and dr (= g) are returned
  at::Tensor dx = fold ? at::Tensor() : at::empty_like(x), dxd = at::empty_like(x), dr = at::empty_like(x);
  at::Tensor coef = at::empty({3 * in.C}, f32), coef_d = at::empty({3 * in.C}, f32);
  at::Tensor part = reduce_ws(in), part_d = reduce_ws(in);
  BnBwdArgs a = bwd_args(in, dy, dy2, gamma, save_mean, save_invstd);
  a.mbits = mbits.data_ptr<uint8_t>();
  a.dx = ptr_or_null<uint16_t>(dx);
  a.dr = bf16_mut(dr);
  a.dgamma = bf16_mut(dgamma);
  a.dbeta = bf16_mut(dbeta);
  a.coef = coef.data_ptr<float>();
  a.part = part.data_ptr<float>();
  a.relu = 1;
  a.xd = bf16(xd);
  a.gamma_d = bf16(gamma_d);
  a.mean_d = mean_d.data_ptr<float>();
  a.invstd_d = invstd_d.data_ptr<float>();
  a.dxd = bf16_mut(dxd);
  a.dgamma_d = bf16_mut(dgamma_d);
  a.dbeta_d = bf16_mut(dbeta_d);
  a.coef_d = coef_d.data_ptr<float>();
  a.part_d = part_d.data_ptr<float>();
  hipError_t e = launch_bn_bwd(a, stream_of(x));
  check_hip(e, op);
  if (fold) return {dx, dxd, dgamma, dbeta, dgamma_d, dbeta_d, coef, dr};
  return {dx, dxd, dgamma, dbeta, dgamma_d, dbeta_d};
}

// BN backward without the elementwise pass (the BN-backward fold: the consumer convolution's dgrad /
// wgrad take g and these coefficients, kernels/bnfold.hip): returns {g, coef [3C] = (A, B, C) of
// dx = A g + B x + C, dgamma, dbeta}. With `part` the producer-reduced partials of an already masked
// g = dy (kernels/convn.hip bwd mode 2); else one reduction pass over dy (+ dy2) under the forward
// bit-mask that also writes g (the residual-branch gradient).
std::vector<at::Tensor> bn_bwd_coef(const at::Tensor& dy_in, const at::Tensor& x_in, const at::Tensor& gamma,
                                    const at::Tensor& save_mean, const at::Tensor& save_invstd,
                                    c10::optional<at::Tensor> mbits_in, c10::optional<at::Tensor> dy2_in,
                                    c10::optional<at::Tensor> part, int64_t rows, c10::optional<at::Tensor> dgamma_out,
                                    c10::optional<at::Tensor> dbeta_out) {
  const char* op = "psd bn_bwd_coef";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard dg(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor dy = like_x(dy_in, in, op, "dy");
  TORCH_CHECK(gamma.defined(), op, ": gamma is required");
  check_stats(op, in, gamma, save_mean, save_invstd);
  if (given(part)) check_part(op, *part, rows, in.C, x, "part");
  else {
    TORCH_CHECK(given(mbits_in), "psd bn_bwd_coef: without partials the forward bit-mask (uint8 [M*C/8]) is required");
    check_mbits(op, *mbits_in, in);
  }
  at::Tensor dgamma = grad_buf(op, dgamma_out, in, "grad buffer"), dbeta = grad_buf(op, dbeta_out, in, "grad buffer");
  at::Tensor coef = at::empty({3 * in.C}, f32_like(in));
  if (given(part)) {
    const at::Tensor fold = fold_ws(rows, in.C, f32_like(in));
    const BnPreArgs a = pre_args(in, dy, gamma, save_mean, save_invstd, *part, rows, fold, dgamma, dbeta, coef);
    const hipError_t e = launch_bn_bwd_pre(a, stream_of(x));
    check_hip(e, op);
    return {dy, coef, dgamma, dbeta};
  }
  const at::Tensor dy2 = like_x(dy2_in, in, op, "dy2");
  at::Tensor g = at::empty_like(x);
  at::Tensor pt = reduce_ws(in);
  BnBwdArgs a = bwd_args(in, dy, dy2, gamma, save_mean, save_invstd);
  a.mbits = mbits_in->data_ptr<uint8_t>();
  a.dr = bf16_mut(g);
  a.dgamma = bf16_mut(dgamma);
  a.dbeta = bf16_mut(dbeta);
  a.coef = coef.data_ptr<float>();
  a.part = pt.data_ptr<float>();
  a.relu = 1;
  a.coef_only = 1;
  const hipError_t e = launch_bn_bwd(a, stream_of(x));
  check_hip(e, op);
  return {g, coef, dgamma, dbeta};
}

// dx = A g + B x + C from finalized coefficients: the elementwise pass that bn_bwd_coef leaves out
at::Tensor bn_elemt_coef(const at::Tensor& g_in, const at::Tensor& x_in, const at::Tensor& coef) {
  const char* op = "psd bn_elemt_coef";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard dg(in.x.device());
  const at::Tensor g = like_x(g_in, in, op, "g");
  check_vec(op, coef, 3 * in.C, at::kFloat, in.x, "coef");
  at::Tensor dx = at::empty_like(in.x);
  const hipError_t e = launch_bn_elemt_coef(bf16(g), bf16(in.x), coef.data_ptr<float>(), bf16_mut(dx), in.M, (int)in.C,
                                            stream_of(in.x));
  check_hip(e, op);
  return dx;  // empty_like keeps the channels_last layout
}

// Dual tail backward from convn bwd-mode-3 partials: {dx (undefined with fold), dxd, dgamma, dbeta,
// dgamma_d, dbeta_d, coef} (kernels/bn.hip launch_bn_bwd_dual_pre)
std::vector<at::Tensor> bn_bwd_dual_pre(const at::Tensor& g_in, const at::Tensor& x_in, const at::Tensor& gamma,
                                        const at::Tensor& save_mean, const at::Tensor& save_invstd,
                                        const at::Tensor& part, const at::Tensor& part_d, int64_t rows,
                                        const at::Tensor& xd_in, const at::Tensor& gamma_d, const at::Tensor& mean_d,
                                        const at::Tensor& invstd_d, c10::optional<at::Tensor> dgamma_out,
                                        c10::optional<at::Tensor> dbeta_out, c10::optional<at::Tensor> dgamma_d_out,
                                        c10::optional<at::Tensor> dbeta_d_out, bool fold, bool fold_d, bool derive_d) {
  const char* op = "psd bn_bwd_dual_pre";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard dg(in.x.device());
  const at::Tensor& x = in.x;
  const at::Tensor g = like_x(g_in, in, op, "g"), xd = like_x(xd_in, in, op, "xd");
  TORCH_CHECK(gamma.defined() && gamma_d.defined(), op, ": gamma and gamma_d are required");
  check_stats(op, in, gamma, save_mean, save_invstd);
  check_stats(op, in, gamma_d, mean_d, invstd_d);
  check_part(op, part, rows, in.C, x, "part");
  check_part(op, part_d, derive_d ? 1 : rows, in.C, x, "part_d (derive_d: [2, C])");
  // fold / fold_d: the BN input gradient of bn3 / of the downsample BN is folded into its
  // convolution's backward (ops/conv.py _fold_backward): not written here
  TORCH_CHECK(!fold_d || fold, "psd bn_bwd_dual_pre: fold_d needs fold");
  at::Tensor dgamma = grad_buf(op, dgamma_out, in, "grad buffer"), dbeta = grad_buf(op, dbeta_out, in, "grad buffer");
  at::Tensor dgamma_d = grad_buf(op, dgamma_d_out, in, "grad buffer"),
             dbeta_d = grad_buf(op, dbeta_d_out, in, "grad buffer");
  const auto f32 = f32_like(in);
  at::Tensor coef = at::empty({3 * in.C}, f32), coef_d = at::empty({3 * in.C}, f32);
  const at::Tensor fw = fold_ws(rows, in.C, f32), fwd = derive_d ? at::Tensor() : fold_ws(rows, in.C, f32);
  at::Tensor dx = fold ? at::Tensor() : at::empty_like(x), dxd = fold_d ? at::Tensor() : at::empty_like(x);
  BnDualPreArgs a{};
  a.g = bf16(g);
  a.x = bf16(x);
  a.xd = bf16(xd);
  a.gamma = bf16(gamma);
  a.gamma_d = bf16(gamma_d);
  a.mean = save_mean.data_ptr<float>();
  a.invstd = save_invstd.data_ptr<float>();
  a.mean_d = mean_d.data_ptr<float>();
  a.invstd_d = invstd_d.data_ptr<float>();
  a.part = part.data_ptr<float>();
  a.part_d = part_d.data_ptr<float>();
  a.rows = (int)rows;
  a.fold_ws = ptr_or_null<float>(fw);
  a.fold_ws_d = ptr_or_null<float>(fwd);
  a.derive_d = derive_d ? 1 : 0;
  a.dgamma = bf16_mut(dgamma);
  a.dbeta = bf16_mut(dbeta);
  a.dgamma_d = bf16_mut(dgamma_d);
  a.dbeta_d = bf16_mut(dbeta_d);
  a.coef = coef.data_ptr<float>();
  a.coef_d = coef_d.data_ptr<float>();
  a.dx = ptr_or_null<uint16_t>(dx);
  a.dxd = ptr_or_null<uint16_t>(dxd);
  a.M = in.M;
  a.C = (int)in.C;
  const hipError_t e = launch_bn_bwd_dual_pre(a, stream_of(x));
  check_hip(e, op);
  return {dx, dxd, dgamma, dbeta, dgamma_d, dbeta_d, coef, coef_d};
}

// Stem BN + ReLU + 3x3/s2 max-pool (training forward): returns {y_pool, argmax, mean, invstd, ss}.
std::vector<at::Tensor> bn_pool_fwd(const at::Tensor& x_in, const at::Tensor& gamma, const at::Tensor& beta,
                                    const at::Tensor& running_mean, const at::Tensor& running_var, double momentum,
                                    double eps, c10::optional<at::Tensor> counter) {
  const char* op = "psd bn_pool";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  TORCH_CHECK(x.dim() == 4, "psd bn_pool: bf16 NCHW-shaped x");
  const int64_t N = x.size(0), C = in.C, H = x.size(2), W = x.size(3);
  TORCH_CHECK(bn_pool_supported((int)H, (int)W, (int)C), "psd bn_pool: unsupported shape ", x.sizes());
  BnFwdArgs a{};
  const BnFwdStats s = bn_fwd_stats(a, x, in.M, C, gamma, beta, running_mean, running_var, counter, momentum, eps);
  const auto cl = x.options().memory_format(at::MemoryFormat::ChannelsLast);
  at::Tensor y = at::empty({N, C, H / 2, W / 2}, cl);
  at::Tensor arg = at::empty({N, C, H / 2, W / 2}, cl.dtype(at::kByte));
  at::Tensor part = reduce_ws(in);
  a.x = bf16(x);
  a.y = bf16_mut(y);
  a.part = part.data_ptr<float>();
  a.pool_arg = arg.data_ptr<uint8_t>();
  a.N = (int32_t)N;
  a.H = (int32_t)H;
  a.W = (int32_t)W;
  a.relu = 1;
  hipError_t e = launch_bn_fwd(a, stream_of(x));
  check_hip(e, "psd bn_pool fwd");
  return {y, arg, s.mean, s.invstd, s.ss};
}

// Backward of bn_pool_fwd: gpool (+ gpool2, a second consumer's gradient of the pooled output)
// -> {dx, dgamma, dbeta}; the pool gradient is recomputed inside the BN passes.
std::vector<at::Tensor> bn_pool_bwd(const at::Tensor& gpool_in, c10::optional<at::Tensor> gpool2_in, const at::Tensor& arg,
                                    const at::Tensor& x_in, const at::Tensor& gamma, const at::Tensor& save_mean,
                                    const at::Tensor& save_invstd, const at::Tensor& ss,
                                    c10::optional<at::Tensor> dgamma_out, c10::optional<at::Tensor> dbeta_out) {
  const char* op = "psd bn_pool bwd";
  const BnIn in = bn_input(x_in, op);
  const c10::DeviceGuard g(in.x.device());
  const at::Tensor& x = in.x;
  TORCH_CHECK(x.dim() == 4, op, ": bf16 NCHW-shaped x");
  const int64_t N = x.size(0), C = in.C, H = x.size(2), W = x.size(3);
  TORCH_CHECK(bn_pool_supported((int)H, (int)W, (int)C), "psd bn_pool bwd: unsupported shape ", x.sizes());
  TORCH_CHECK(gamma.defined(), op, ": gamma is required");
  check_stats(op, in, gamma, save_mean, save_invstd);
  check_vec(op, ss, 2 * C, at::kFloat, x, "ss");
  const std::vector<int64_t> ps{N, C, H / 2, W / 2};
  auto pooled = [&](const at::Tensor& t, at::ScalarType st) {
    return t.sizes() == ps && t.scalar_type() == st && t.device() == x.device();
  };
  TORCH_CHECK(pooled(gpool_in, at::kBFloat16), "psd bn_pool bwd: gpool shape/dtype");
  TORCH_CHECK(pooled(arg, at::kByte) && arg.is_contiguous(at::MemoryFormat::ChannelsLast),
              "psd bn_pool bwd: argmax shape");
  at::Tensor gp = nhwc(gpool_in), gp2;
  if (given(gpool2_in)) {
    TORCH_CHECK(pooled(*gpool2_in, at::kBFloat16), "psd bn_pool bwd: gpool2 shape/dtype");
    gp2 = nhwc(*gpool2_in);
  }
  at::Tensor dx = at::empty_like(x);
  at::Tensor dgamma = grad_buf(op, dgamma_out, in, "dgamma"), dbeta = grad_buf(op, dbeta_out, in, "dbeta");
  at::Tensor coef = at::empty({3 * C}, f32_like(in));
  at::Tensor part = at::empty({(int64_t)bn_pool_reduce_blocks((int)N, (int)H, (int)W, (int)C) * 2 * C}, f32_like(in));
  BnBwdArgs a = bwd_args(in, at::Tensor(), at::Tensor(), gamma, save_mean, save_invstd);
  a.gpool = bf16(gp);
  a.gpool2 = ptr_or_null<const uint16_t>(gp2);
  a.pool_arg = arg.data_ptr<uint8_t>();
  a.ss = ss.data_ptr<float>();
  a.dx = bf16_mut(dx);
  a.dgamma = bf16_mut(dgamma);
  a.dbeta = bf16_mut(dbeta);
  a.coef = coef.data_ptr<float>();
  a.part = part.data_ptr<float>();
  a.N = (int32_t)N;
  a.H = (int32_t)H;
  a.W = (int32_t)W;
  a.relu = 1;
  hipError_t e = launch_bn_bwd(a, stream_of(x));
  check_hip(e, op);
  return {dx, dgamma, dbeta};
}

}  // namespace psd
