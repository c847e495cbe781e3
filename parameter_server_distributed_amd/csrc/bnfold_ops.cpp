// Tensor glue for the BN-backward fold of a 1x1 conv -> BN pair (kernels/bnfold.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <vector>

#include "glue.h"
#include "kernels/launchers_bn.h"
#include "ops.h"

namespace psd {

namespace {
at::Tensor fold_w2d(const at::Tensor& w) {
  TORCH_CHECK(w.is_cuda() && w.scalar_type() == at::kBFloat16 && (w.dim() == 2 || (w.dim() == 4 && w.size(2) == 1 &&
                                                                                   w.size(3) == 1)),
              "psd bnfold: w must be the bf16 [Cout, Cin(, 1, 1)] weight of a 1x1 convolution");
  return w.reshape({w.size(0), w.size(1)}).contiguous();
}
}  // namespace

// The folded dgrad operands: w2 [Cin, Cout + Cin] bf16 = [(A o W)^T | W^T (B o W)] and the bias
// bvec [Cin] fp32 = C^T W, so dgrad = [g | x] . w2^T + bvec (kernels/convn.hip with x2 = x).
std::vector<at::Tensor> bnfold_dgrad_weights(const at::Tensor& w_in, const at::Tensor& coef) {
  const c10::DeviceGuard dg(w_in.device());
  const at::Tensor w = fold_w2d(w_in);
  const int64_t Cout = w.size(0), Cin = w.size(1);
  TORCH_CHECK(coef.scalar_type() == at::kFloat && coef.is_contiguous() && coef.numel() == 3 * Cout &&
                  coef.device() == w.device(),
              "psd bnfold: coef must be fp32 [3 * Cout]");
  at::Tensor w2 = at::empty({Cin, Cout + Cin}, w.options());
  at::Tensor bw = at::empty({Cout, Cin}, w.options());
  at::Tensor bvec = at::empty({Cin}, w.options().dtype(at::kFloat));
  hipError_t e = launch_bnfold_prep(bf16(w), coef.data_ptr<float>(), (int)Cout, (int)Cin, bf16_mut(w2), (int)(Cout + Cin),
                                    bf16_mut(bw), bvec.data_ptr<float>(), stream_of(w));
  check_hip(e, "psd bnfold prep");
  // M = (B o W)^T W (Cin x Cin, symmetric) into the right block of w2 (the MFMA GEMM, TN layout)
  gemm_(bw, w, false, false, w2.narrow(1, Cout, Cin), c10::nullopt, 0, c10::nullopt, c10::nullopt, c10::nullopt);
  return {w2, bvec};
}

// dW = A o P[:Cout] + B o (W P[Cout:Cout+Cin]) + C P[Cout+Cin] (P = kernels/convw.hip fold output)
// into out (bf16 [Cout, Cin] view, += with accumulate)
void bnfold_combine(const at::Tensor& P, const at::Tensor& w_in, const at::Tensor& coef, at::Tensor out,
                    bool accumulate) {
  const c10::DeviceGuard dg(w_in.device());
  const at::Tensor w = fold_w2d(w_in);
  const int64_t Cout = w.size(0), Cin = w.size(1);
  TORCH_CHECK(P.scalar_type() == at::kFloat && P.is_contiguous() && P.dim() == 2 && P.size(1) == Cin &&
                  P.size(0) > Cout + Cin && P.device() == w.device(),
              "psd bnfold combine: P must be the fp32 convw fold result [rows, Cin]");
  TORCH_CHECK(coef.scalar_type() == at::kFloat && coef.is_contiguous() && coef.numel() == 3 * Cout,
              "psd bnfold combine: coef must be fp32 [3 * Cout]");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.is_contiguous() && out.numel() == Cout * Cin &&
                  out.device() == w.device(),
              "psd bnfold combine: out must be a contiguous bf16 [Cout, Cin]");
  hipError_t e = launch_bnfold_combine(P.data_ptr<float>(), bf16(w), coef.data_ptr<float>(), (int)Cout, (int)Cin,
                                       bf16_mut(out), accumulate ? 1 : 0, stream_of(w));
  check_hip(e, "psd bnfold combine");
}

// row [2, Cout] (a view into a partials buffer) = (0, sum_i W[c][i] P[c][i]): the sum g y of a BN
// whose input y = x W^T was never stored (ops/tail.py)
void bnfold_rowdot(const at::Tensor& P, const at::Tensor& w_in, at::Tensor row) {
  const c10::DeviceGuard dg(w_in.device());
  const at::Tensor w = fold_w2d(w_in);
  const int64_t Cout = w.size(0), Cin = w.size(1);
  TORCH_CHECK(P.scalar_type() == at::kFloat && P.is_contiguous() && P.dim() == 2 && P.size(1) == Cin &&
                  P.size(0) >= Cout && P.device() == w.device(),
              "psd bnfold rowdot: P must be the fp32 convw fold result [rows, Cin]");
  TORCH_CHECK(row.scalar_type() == at::kFloat && row.is_contiguous() && row.numel() == 2 * Cout &&
                  row.device() == w.device(),
              "psd bnfold rowdot: row must be a contiguous fp32 [2, Cout]");
  hipError_t e = launch_bnfold_rowdot(P.data_ptr<float>(), bf16(w), (int)Cout, (int)Cin, row.data_ptr<float>(),
                                      stream_of(w));
  check_hip(e, "psd bnfold rowdot");
}

// row [2, Cout] = the shifted batch statistics of y = x W^T from P = convw(x, x) in fold mode (the
// Gram matrix and column sums of x), without forming y (ops/tail.py)
void bnfold_gram_stats(const at::Tensor& P, const at::Tensor& w_in, const at::Tensor& shift, int64_t M, at::Tensor row) {
  const c10::DeviceGuard dg(w_in.device());
  const at::Tensor w = fold_w2d(w_in);
  const int64_t Cout = w.size(0), Cin = w.size(1);
  TORCH_CHECK(P.scalar_type() == at::kFloat && P.is_contiguous() && P.dim() == 2 && P.size(1) == Cin &&
                  P.size(0) > Cin && P.device() == w.device() && (Cin == 64 || Cin == 128 || Cin == 256) &&
                  Cout % 4 == 0,
              "psd bnfold gram stats: P must be the fp32 convw_gram_ result [rows > Cin, Cin], Cin 64/128/256, "
              "Cout % 4 == 0");
  TORCH_CHECK(shift.scalar_type() == at::kFloat && shift.numel() == Cout && shift.is_contiguous(),
              "psd bnfold gram stats: shift must be fp32 [Cout]");
  TORCH_CHECK(row.scalar_type() == at::kFloat && row.is_contiguous() && row.numel() == 2 * Cout,
              "psd bnfold gram stats: row must be a contiguous fp32 [2, Cout]");
  hipError_t e = launch_bnfold_gram_stats(P.data_ptr<float>(), bf16(w), shift.data_ptr<float>(), (int)Cout, (int)Cin, M,
                                          row.data_ptr<float>(), stream_of(w));
  check_hip(e, "psd bnfold gram stats");
}

// The dual tail's apply operands from both convolutions' weights and both BNs' scale/shift
// (kernels/bnfold.hip bnfold_dual_weights_kernel): {wcat [Cout, C3 + Cd] bf16, ss [2 Cout] fp32}
std::vector<at::Tensor> bnfold_dual_weights(const at::Tensor& w3_in, const at::Tensor& wd_in, const at::Tensor& ss3,
                                            const at::Tensor& ssd) {
  const c10::DeviceGuard dg(w3_in.device());
  const at::Tensor w3 = fold_w2d(w3_in), wd = fold_w2d(wd_in);
  const int64_t Cout = w3.size(0), C3 = w3.size(1), Cd = wd.size(1);
  TORCH_CHECK(wd.size(0) == Cout && w3.scalar_type() == at::kBFloat16 && wd.scalar_type() == at::kBFloat16,
              "psd bnfold dual weights: bf16 weights with one Cout");
  for (const at::Tensor* t : {&ss3, &ssd})
    TORCH_CHECK(t->scalar_type() == at::kFloat && t->is_contiguous() && t->numel() == 2 * Cout && t->device() == w3.device(),
                "psd bnfold dual weights: ss must be fp32 [2 Cout]");
  at::Tensor wcat = at::empty({Cout, C3 + Cd}, w3.options());
  at::Tensor ss = at::empty({2 * Cout}, ss3.options());
  hipError_t e = launch_bnfold_dual_weights(bf16(w3), bf16(wd), ss3.data_ptr<float>(), ssd.data_ptr<float>(), (int)Cout,
                                            (int)C3, (int)Cd, bf16_mut(wcat), ss.data_ptr<float>(), stream_of(w3));
  check_hip(e, "psd bnfold dual weights");
  return {wcat, ss};
}

}  // namespace psd
