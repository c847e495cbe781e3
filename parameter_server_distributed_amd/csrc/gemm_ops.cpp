// Tensor glue for the MFMA GEMM (kernels/gemm.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <algorithm>

#include "glue.h"
#include "kernels/launchers_gemm.h"
#include "ops.h"

namespace psd {

namespace {
void chk2d(const at::Tensor& t, const char* n) {
  TORCH_CHECK(t.is_cuda() && t.dim() == 2 && t.scalar_type() == at::kBFloat16 && t.stride(1) == 1 &&
                  t.stride(0) % 8 == 0 && aligned16(t),
              "psd gemm: ", n, " must be a 2-D bf16 device tensor, unit inner stride, 16-B aligned rows");
}

// extents of A op B. A: a_kmajor ? [M,K] : [K,M]; B: b_kmajor ? [N,K] : [K,N] (Kb: B's K)
struct Mnk {
  int64_t M, N, K, Kb;
};
Mnk mnk_of(const at::Tensor& A, const at::Tensor& B, bool a_kmajor, bool b_kmajor) {
  return {a_kmajor ? A.size(0) : A.size(1), b_kmajor ? B.size(0) : B.size(1), a_kmajor ? A.size(1) : A.size(0),
          b_kmajor ? B.size(1) : B.size(0)};
}

// what every launch shares: the operands, extents, leading dimensions and majors; out (null: the
// split-K slabs stand in for C) with its row stride ldc. The entry points add what differs.
GemmArgs gemm_args(const at::Tensor& A, const at::Tensor& B, bool a_kmajor, bool b_kmajor, const Mnk& d,
                   const at::Tensor* out, int64_t ldc) {
  GemmArgs a{};
  a.A = A.data_ptr();
  a.B = B.data_ptr();
  a.C = out ? out->data_ptr() : nullptr;
  a.M = (int)d.M;
  a.N = (int)d.N;
  a.K = (int)d.K;
  a.lda = (int)A.stride(0);
  a.ldb = (int)B.stride(0);
  a.ldc = (int)ldc;
  a.a_kmajor = a_kmajor;
  a.b_kmajor = b_kmajor;
  a.c_f32 = out && out->scalar_type() == at::kFloat;
  return a;
}

// the output and bias of gemm_ / gemm_fp8_: out [M, N] bf16 or fp32 with unit inner stride, bias bf16 [N]
void check_out_bias(const char* op, const at::Tensor& out, const Mnk& d, const c10::optional<at::Tensor>& bias) {
  TORCH_CHECK(out.dim() == 2 && out.size(0) == d.M && out.size(1) == d.N && out.stride(1) == 1, op, ": out shape");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat, op, ": out dtype");
  if (opt_ptr<void>(bias))  // (an empty tensor has no data: no bias)
    TORCH_CHECK(bias->numel() == d.N && bias->scalar_type() == at::kBFloat16, op, ": bias [N] bf16");
}
}  // namespace

int64_t gemm_stats_rows_(int64_t M) { return (M + 127) / 128 * 2; }

// the consumer BN's statistics partials in the 8-phase epilogue: part fp32 >= gemm_stats_rows(M) x 2 x N,
// shift fp32 [N] (the BN's running mean)
void set_stats(GemmArgs& a, const c10::optional<at::Tensor>& part, const c10::optional<at::Tensor>& shift,
               const at::Tensor& out, int* rows) {
  if (!given(part)) return;
  const int64_t M = out.size(0), N = out.size(1);
  TORCH_CHECK(part->scalar_type() == at::kFloat && part->is_contiguous() && part->device() == out.device() &&
                  part->numel() >= gemm_stats_rows_(M) * 2 * N,
              "psd gemm: part must be fp32 contiguous with >= gemm_stats_rows(M) x 2 x N elements");
  TORCH_CHECK(given(shift) && shift->scalar_type() == at::kFloat && shift->is_contiguous() && shift->numel() == N &&
                  shift->device() == out.device(),
              "psd gemm: statistics need shift fp32 [N]");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16, "psd gemm: statistics need a bf16 output");
  a.part = part->data_ptr<float>();
  a.shift = shift->data_ptr<float>();
  a.rows_out = rows;
}

// out[M,N] = A op B (+bias)(act). A: a_kmajor ? [M,K] : [K,M]; B: b_kmajor ? [N,K] : [K,N]. With
// part/shift also the consumer BN's statistics partials: returns the partial rows written, 0 when the
// shape cannot carry them (nothing launched); 1 without statistics.
int64_t gemm_(const at::Tensor& A, const at::Tensor& B, bool a_kmajor, bool b_kmajor, at::Tensor out,
              c10::optional<at::Tensor> bias, int64_t act, c10::optional<at::Tensor> aux,
              c10::optional<at::Tensor> part, c10::optional<at::Tensor> shift) {
  chk2d(A, "A");
  chk2d(B, "B");
  const Mnk d = mnk_of(A, B, a_kmajor, b_kmajor);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(K == d.Kb, "psd gemm: K mismatch ", K, " vs ", d.Kb);
  check_out_bias("psd gemm", out, d, bias);
  TORCH_CHECK(K % 8 == 0 || !(a_kmajor && b_kmajor), "psd gemm: K must be a multiple of 8 for K-major operands");
  TORCH_CHECK(a_kmajor || M % 8 == 0, "psd gemm: M must be a multiple of 8 for an M-major A");
  TORCH_CHECK(b_kmajor || N % 8 == 0, "psd gemm: N must be a multiple of 8 for an N-major B");
  TORCH_CHECK(!(a_kmajor ^ b_kmajor) || K % 8 == 0, "psd gemm: K must be a multiple of 8");
  const c10::DeviceGuard g(A.device());
  GemmArgs a = gemm_args(A, B, a_kmajor, b_kmajor, d, &out, out.stride(0));
  a.bias = opt_ptr<void>(bias);
  a.aux = opt_ptr<void>(aux);
  a.act = (int)act;
  int rows = 0;
  set_stats(a, part, shift, out, &rows);
  hipError_t e = launch_gemm(a, stream_of(A));
  if (a.part && e == hipErrorNotSupported) return 0;
  check_hip(e, "psd gemm");
  return a.part ? rows : 1;
}

bool gemm_ct_(const at::Tensor& A, const at::Tensor& B, at::Tensor out, c10::optional<at::Tensor> bias, int64_t act,
              c10::optional<at::Tensor> aux) {
  chk2d(A, "A");
  chk2d(B, "B");
  const Mnk d = mnk_of(A, B, true, true);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(d.Kb == K, "psd gemm_ct: K mismatch ", K, " vs ", d.Kb);
  TORCH_CHECK(out.dim() == 2 && out.size(0) == N && out.size(1) == M && out.stride(1) == 1 &&
                  (out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat),
              "psd gemm_ct: out must be [N, M] bf16 / fp32 with unit inner stride");
  TORCH_CHECK(act >= 0 && act <= 2, "psd gemm_ct: act 0-2");
  if (given(aux))
    TORCH_CHECK(aux->sizes() == out.sizes() && aux->strides() == out.strides() && aux->scalar_type() == at::kBFloat16,
                "psd gemm_ct: aux like out (bf16)");
  if (given(bias))
    TORCH_CHECK(bias->numel() == M && bias->scalar_type() == at::kBFloat16, "psd gemm_ct: bias [M] bf16");
  const c10::DeviceGuard g(A.device());
  GemmArgs a = gemm_args(A, B, true, true, d, &out, out.stride(0));
  a.bias = opt_ptr<void>(bias);
  a.aux = opt_ptr<void>(aux);
  a.act = (int)act;
  hipError_t e = launch_gemm_ct(a, stream_of(A));
  if (e == hipErrorNotSupported) return false;
  check_hip(e, "psd gemm_ct");
  return true;
}

// GELU-backward GEMM: out[M,N] = bf16(bf16(A op B) * gelu'(pre)) with the bias gradient
// db[N] (+)= colsum(out) from the epilogue's per-tile partials (kernels/gemm.hip ACT 3): the
// gradient of a GELU Linear's output computed by the next Linear's bwd-data GEMM goes straight to
// the pre-activation gradient. False (nothing launched) when the shape is not on the 8-phase kernel.
bool gemm_gelu_bwd_(const at::Tensor& A, const at::Tensor& B, bool a_kmajor, bool b_kmajor, const at::Tensor& pre,
                    at::Tensor out, at::Tensor db, bool accumulate) {
  chk2d(A, "A");
  chk2d(B, "B");
  chk2d(pre, "pre");
  const Mnk d = mnk_of(A, B, a_kmajor, b_kmajor);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(K == d.Kb, "psd gemm_gelu_bwd: K mismatch ", K, " vs ", d.Kb);
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 && out.is_contiguous() && out.dim() == 2 && out.size(0) == M &&
                  out.size(1) == N && pre.is_contiguous() && pre.sizes() == out.sizes(),
              "psd gemm_gelu_bwd: out and pre must be contiguous bf16 [M, N]");
  TORCH_CHECK(db.numel() == N && db.is_contiguous() &&
                  (db.scalar_type() == at::kBFloat16 || db.scalar_type() == at::kFloat),
              "psd gemm_gelu_bwd: db must be [N] bf16/fp32");
  if (N % 8 != 0 || K % 8 != 0 || (!a_kmajor && M % 8 != 0)) return false;
  const c10::DeviceGuard g(A.device());
  at::Tensor part = at::empty({gemm_stats_rows_(M) * N}, A.options().dtype(at::kFloat));
  GemmArgs a = gemm_args(A, B, a_kmajor, b_kmajor, d, &out, N);
  a.aux = const_cast<void*>(pre.data_ptr());
  a.act = 3;
  a.part = part.data_ptr<float>();
  int rows = 0;
  a.rows_out = &rows;
  hipError_t e = launch_gemm(a, stream_of(A));
  if (e == hipErrorNotSupported) return false;
  check_hip(e, "psd gemm_gelu_bwd");
  TORCH_CHECK(rows > 0 && rows <= gemm_stats_rows_(M), "psd gemm_gelu_bwd: partial rows ", rows);
  e = launch_colsum_final(part.data_ptr<float>(), rows, (int)N, db.data_ptr(), db.scalar_type() == at::kBFloat16,
                          accumulate, stream_of(A));
  check_hip(e, "psd gemm_gelu_bwd colsum");
  return true;
}

// out[M,N] (+)= scale * (A op B) via split-K fp32 slabs (weight gradients: K = tokens).
void gemm_splitk_(const at::Tensor& A, const at::Tensor& B, bool a_kmajor, bool b_kmajor, at::Tensor out,
                  bool accumulate, double scale, int64_t splits) {
  chk2d(A, "A");
  chk2d(B, "B");
  const Mnk d = mnk_of(A, B, a_kmajor, b_kmajor);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(K == d.Kb, "psd gemm_splitk: K mismatch");
  TORCH_CHECK(out.is_contiguous() && out.numel() == M * N, "psd gemm_splitk: out must be contiguous [M,N]");
  TORCH_CHECK(a_kmajor || M % 8 == 0, "psd gemm_splitk: M % 8");
  TORCH_CHECK(b_kmajor || N % 8 == 0, "psd gemm_splitk: N % 8");
  const c10::DeviceGuard g(A.device());
  const int s = splits > 0 ? (int)splits : gemm_splits((int)M, (int)N, (int)K);
  if (s == 1 && !accumulate && scale == 1.0) {
    // one split (enough output tiles to fill the chip, e.g. the BERT MLM head's weight gradient:
    // 120 x 3 256-tiles): the single-split GEMM writes the output itself -- no fp32 slab
    // (94 MB written and read back there) and no reduce launch
    check_hip(launch_gemm(gemm_args(A, B, a_kmajor, b_kmajor, d, &out, N), stream_of(A)),
              "psd gemm_splitk (single split)");
    return;
  }
  at::Tensor slab = at::empty({(int64_t)s * M * N}, A.options().dtype(at::kFloat));
  hipError_t e = launch_gemm_splitk(gemm_args(A, B, a_kmajor, b_kmajor, d, nullptr, N), slab.data_ptr<float>(), s,
                                    out.data_ptr(), out.scalar_type() == at::kBFloat16, accumulate, (float)scale,
                                    stream_of(A));
  check_hip(e, "psd gemm_splitk");
}

// out[M,N] = (A_q . B_q^T) * a_scale * b_scale (+bias)(act): A [M,K], B [N,K] OCP e4m3fn, K % 128 == 0
int64_t gemm_fp8_(const at::Tensor& A, const at::Tensor& B, const at::Tensor& a_scale, const at::Tensor& b_scale,
                  at::Tensor out, c10::optional<at::Tensor> bias, int64_t act, c10::optional<at::Tensor> aux,
                  c10::optional<at::Tensor> part, c10::optional<at::Tensor> shift) {
  for (const at::Tensor* t : {&A, &B})
    TORCH_CHECK(t->is_cuda() && t->dim() == 2 && t->stride(1) == 1 && t->stride(0) % 16 == 0 && aligned16(*t),
                "psd gemm_fp8: operands must be 2-D fp8 device tensors, unit inner stride, 16-B aligned rows");
  TORCH_CHECK((A.scalar_type() == at::kFloat8_e4m3fn || A.scalar_type() == at::kFloat8_e5m2) &&
                  B.scalar_type() == at::kFloat8_e4m3fn,
              "psd gemm_fp8: A e4m3fn or e5m2, B e4m3fn");
  const Mnk d = mnk_of(A, B, true, true);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(d.Kb == K, "psd gemm_fp8: K mismatch");
  TORCH_CHECK(K % 128 == 0, "psd gemm_fp8: K must be a multiple of 128");
  // per-tensor (fp32 device scalars) or MX (uint8 E8M0 per 32 contiguous K: A [M, K/32], B [N, K/32])
  const bool mx = a_scale.scalar_type() == at::kByte;
  if (mx) {
    TORCH_CHECK(b_scale.scalar_type() == at::kByte && a_scale.is_cuda() && b_scale.is_cuda() &&
                    a_scale.is_contiguous() && b_scale.is_contiguous() && a_scale.numel() == M * (K / 32) &&
                    b_scale.numel() == N * (K / 32) && A.stride(0) == K && B.stride(0) == K,
                "psd gemm_fp8: MX scales must be uint8 [M, K/32] / [N, K/32] (contiguous operands)");
  } else {
    TORCH_CHECK(a_scale.scalar_type() == at::kFloat && b_scale.scalar_type() == at::kFloat && a_scale.numel() >= 1 &&
                    b_scale.numel() >= 1 && a_scale.is_cuda() && b_scale.is_cuda(),
                "psd gemm_fp8: scales must be fp32 device scalars (or MX uint8 block scales)");
  }
  check_out_bias("psd gemm_fp8", out, d, bias);
  const c10::DeviceGuard g(A.device());
  GemmArgs a = gemm_args(A, B, true, true, d, &out, out.stride(0));
  a.bias = opt_ptr<void>(bias);
  a.aux = opt_ptr<void>(aux);
  a.act = (int)act;
  if (mx) {
    a.a_mx = a_scale.data_ptr<uint8_t>();
    a.b_mx = b_scale.data_ptr<uint8_t>();
  } else {
    a.a_scale = a_scale.data_ptr<float>();
    a.b_scale = b_scale.data_ptr<float>();
  }
  a.f8a = A.scalar_type() == at::kFloat8_e5m2 ? 1 : 0;
  int rows = 0;
  set_stats(a, part, shift, out, &rows);
  hipError_t e = launch_gemm_fp8(a, stream_of(A));
  if (a.part && e == hipErrorNotSupported) return 0;
  check_hip(e, "psd gemm_fp8");
  return a.part ? rows : 1;
}

// out[M,N] (+)= scale * dq(A) dq(B)^T via split-K fp32 slabs on the block-scaled fp8 MFMA (the fp8 weight
// gradient of a Linear: A = q_t(dy') [out, tokens], B = q_t(x) [in, tokens], K = tokens): A [M,K], B [N,K]
// e4m3fn with MX scales uint8 [M, K/32] / [N, K/32]; splits 0: gemm_fp8_splits
void gemm_fp8_splitk_(const at::Tensor& A, const at::Tensor& B, const at::Tensor& a_scale, const at::Tensor& b_scale,
                      at::Tensor out, bool accumulate, double scale, int64_t splits) {
  for (const at::Tensor* t : {&A, &B})
    TORCH_CHECK(t->is_cuda() && t->dim() == 2 && t->stride(1) == 1 && t->stride(0) % 16 == 0 && aligned16(*t),
                "psd gemm_fp8_splitk: operands must be 2-D fp8 device tensors, unit inner stride, 16-B aligned rows");
  TORCH_CHECK(A.scalar_type() == at::kFloat8_e4m3fn && B.scalar_type() == at::kFloat8_e4m3fn,
              "psd gemm_fp8_splitk: A and B e4m3fn");
  const Mnk d = mnk_of(A, B, true, true);
  const int64_t M = d.M, N = d.N, K = d.K;
  TORCH_CHECK(d.Kb == K, "psd gemm_fp8_splitk: K mismatch");
  TORCH_CHECK(K >= 128 && K % 128 == 0, "psd gemm_fp8_splitk: K must be a multiple of 128");
  TORCH_CHECK(N % 8 == 0, "psd gemm_fp8_splitk: N must be a multiple of 8");
  TORCH_CHECK(a_scale.scalar_type() == at::kByte && b_scale.scalar_type() == at::kByte && a_scale.is_cuda() &&
                  b_scale.is_cuda() && a_scale.is_contiguous() && b_scale.is_contiguous() &&
                  a_scale.numel() == M * (K / 32) && b_scale.numel() == N * (K / 32) && A.stride(0) == K &&
                  B.stride(0) == K && a_scale.device() == A.device() && b_scale.device() == A.device() &&
                  B.device() == A.device(),
              "psd gemm_fp8_splitk: MX scales must be uint8 [M, K/32] / [N, K/32] (contiguous operands)");
  TORCH_CHECK(out.is_cuda() && out.device() == A.device() && out.dim() == 2 && out.size(0) == M && out.size(1) == N &&
                  out.is_contiguous(),
              "psd gemm_fp8_splitk: out must be contiguous [M, N]");
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat, "psd gemm_fp8_splitk: out dtype");
  TORCH_CHECK(splits >= 0 && splits <= 4096, "psd gemm_fp8_splitk: splits");
  const c10::DeviceGuard g(A.device());
  const int s = splits > 0 ? (int)splits : gemm_fp8_splits((int)M, (int)N, (int)K);
  GemmArgs a = gemm_args(A, B, true, true, d, &out, N);
  a.a_mx = a_scale.data_ptr<uint8_t>();
  a.b_mx = b_scale.data_ptr<uint8_t>();
  if (s == 1 && !accumulate && scale == 1.0) {  // one split: the single-split MX GEMM writes out itself, no slab
    check_hip(launch_gemm_fp8(a, stream_of(A)), "psd gemm_fp8_splitk (single split)");
    return;
  }
  at::Tensor slab = at::empty({(int64_t)s * M * N}, A.options().dtype(at::kFloat));
  hipError_t e = launch_gemm_fp8_splitk(a, slab.data_ptr<float>(), s, out.data_ptr(), out.scalar_type() == at::kBFloat16,
                                        accumulate, (float)scale, stream_of(A));
  check_hip(e, "psd gemm_fp8_splitk");
}

// out[N] (+)= column sums of x[M,N] (bias gradient)
void colsum_(const at::Tensor& x, at::Tensor out, bool accumulate) {
  chk2d(x, "x");
  const int64_t M = x.size(0), N = x.size(1);
  TORCH_CHECK(N % 8 == 0 && x.is_contiguous(), "psd colsum: N % 8 and contiguous");
  TORCH_CHECK(out.numel() == N && out.is_contiguous(), "psd colsum: out [N]");
  const c10::DeviceGuard g(x.device());
  TORCH_CHECK(out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat, "psd colsum: out dtype");
  at::Tensor part = at::empty({(int64_t)kColsumPartRows * N}, x.options().dtype(at::kFloat));
  hipError_t e = launch_colsum(reinterpret_cast<const uint16_t*>(x.data_ptr()), M, (int)N, part.data_ptr<float>(),
                               out.data_ptr(), out.scalar_type() == at::kBFloat16, accumulate, stream_of(x));
  check_hip(e, "psd colsum");
}

// GELU(tanh) backward fused with the bias gradient: dx = bf16(dy * gelu'(pre)) and out[N] (+)= colsum(dx)
void gelu_bwd_colsum_(const at::Tensor& dy, const at::Tensor& pre, at::Tensor dx, at::Tensor out, bool accumulate) {
  chk2d(dy, "dy");
  chk2d(pre, "pre");
  chk2d(dx, "dx");
  const int64_t M = dy.size(0), N = dy.size(1);
  TORCH_CHECK(N % 8 == 0 && dy.is_contiguous() && pre.is_contiguous() && dx.is_contiguous() && pre.sizes() == dy.sizes() &&
                  dx.sizes() == dy.sizes(),
              "psd gelu_bwd_colsum: contiguous [M, N] tensors, N % 8");
  TORCH_CHECK(out.numel() == N && out.is_contiguous() &&
                  (out.scalar_type() == at::kBFloat16 || out.scalar_type() == at::kFloat),
              "psd gelu_bwd_colsum: out [N] bf16/fp32");
  const c10::DeviceGuard g(dy.device());
  at::Tensor part = at::empty({(int64_t)kColsumPartRows * N}, dy.options().dtype(at::kFloat));
  hipError_t e = launch_colsum(reinterpret_cast<const uint16_t*>(dy.data_ptr()), M, (int)N, part.data_ptr<float>(),
                               out.data_ptr(), out.scalar_type() == at::kBFloat16, accumulate, stream_of(dy),
                               reinterpret_cast<const uint16_t*>(pre.data_ptr()),
                               reinterpret_cast<uint16_t*>(dx.data_ptr()));
  check_hip(e, "psd gelu_bwd_colsum");
}

}  // namespace psd
