// Tensor glue for the implicit-GEMM convolutions: the 8-phase GEMM's gathered forward and weight
// gradient (kernels/gemm.hip), the narrow-output kernel (kernels/convn.hip) and the narrow weight
// gradient (kernels/convw.hip).
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>

#include <algorithm>

#include "glue.h"
#include "kernels/launchers_convn.h"
#include "kernels/launchers_convw.h"
#include "kernels/launchers_gemm.h"
#include "ops.h"

namespace psd {

namespace {

// A convolution's geometry, derived once from its channels_last input [Nb, C, H, W] and (R, S, stride,
// pad): M output pixels, the input's bytes, logC (the kernels take power-of-two channel counts; every
// entry point declines the others, each with its own minimum and size limits).
struct ConvGeo {
  int64_t Nb, C, H, W, R, S, stride, pad, Ho, Wo, M, bytes;
  int logC;
  bool pow2_c() const { return (C & (C - 1)) == 0; }
};

ConvGeo conv_geo(const at::Tensor& x, int64_t R, int64_t S, int64_t stride, int64_t pad) {
  ConvGeo g{};
  g.Nb = x.size(0), g.C = x.size(1), g.H = x.size(2), g.W = x.size(3);
  g.R = R, g.S = S, g.stride = stride, g.pad = pad;
  g.Ho = (g.H + 2 * pad - R) / stride + 1;
  g.Wo = (g.W + 2 * pad - S) / stride + 1;
  g.M = g.Nb * g.Ho * g.Wo;
  g.bytes = x.numel() * (int64_t)x.element_size();
  g.logC = log2_exact(g.C);
  return g;
}

bool is_nhwc_dev(const at::Tensor& t, at::ScalarType dt) {
  return t.is_cuda() && t.dim() == 4 && t.scalar_type() == dt && t.is_contiguous(at::MemoryFormat::ChannelsLast);
}

// dy [Nb, Cout, Ho, Wo] is the output gradient of the convolution g
bool dy_matches(const at::Tensor& dy, const ConvGeo& g) {
  return dy.size(0) == g.Nb && dy.size(2) == g.Ho && dy.size(3) == g.Wo;
}

// the gathered-A fields of an 8-phase launch
void set_geo(GemmArgs& a, const ConvGeo& g) {
  a.cv_H = (int)g.H;
  a.cv_W = (int)g.W;
  a.cv_logC = g.logC;
  a.cv_Ho = (int)g.Ho;
  a.cv_Wo = (int)g.Wo;
  a.cv_S = (int)g.S;
  a.cv_stride = (int)g.stride;
  a.cv_pad = (int)g.pad;
  a.cv_abytes = (uint32_t)g.bytes;
}

// a narrow-kernel launch of g with N output channels over K (R*S*C, plus the x2 operand's channels)
void set_geo(ConvnArgs& a, const ConvGeo& g, int64_t wbytes, int64_t N, int64_t K, int64_t ldc, int64_t variant) {
  a.K1 = (int)(g.R * g.S * g.C);
  a.xbytes = (uint32_t)g.bytes;
  a.wbytes = (uint32_t)wbytes;
  a.M = (int)g.M;
  a.N = (int)N;
  a.K = (int)K;
  a.H = (int)g.H;
  a.W = (int)g.W;
  a.logC = g.logC;
  a.Ho = (int)g.Ho;
  a.Wo = (int)g.Wo;
  a.R = (int)g.R;
  a.S = (int)g.S;
  a.stride = (int)g.stride;
  a.pad = (int)g.pad;
  a.ldc = (int)ldc;
  a.variant = (int)variant;
}

void set_geo(ConvwArgs& a, const ConvGeo& g) {
  a.xbytes = (uint32_t)g.bytes;
  a.M = (int)g.M;
  a.H = (int)g.H;
  a.W = (int)g.W;
  a.logC = g.logC;
  a.Ho = (int)g.Ho;
  a.Wo = (int)g.Wo;
  a.S = (int)g.S;
  a.stride = (int)g.stride;
  a.pad = (int)g.pad;
}

// partial rows to allocate for a narrow-kernel launch with statistics (whichever tiling the variant takes)
int64_t part_rows_bound(int64_t M, int64_t N, int64_t variant, int64_t Ho, int64_t Wo, int64_t R) {
  return std::max(convn_stats_rows((int)M), convn_part_rows_geo((int)M, (int)N, (int)std::max<int64_t>(variant, 0),
                                                                (int)Ho, (int)Wo, (int)R));
}

}  // namespace

// Implicit-GEMM NHWC convolution forward on the persistent 8-phase MFMA kernel (no bias/activation):
// x [Nb, C, H, W] channels_last, w2 [Cout, R*S*C] ((r, s, ci) order, i.e. an OHWI weight viewed
// 2-D), out [Nb*Ho*Wo, Cout] bf16 (an NHWC output's 2-D view). bf16 operands, or OCP e4m3 ones with
// per-tensor dequant scales (xs, ws: fp32 device scalars). Returns false (nothing launched) when the
// shape is outside the kernel's contract -- the caller falls back.
static int64_t conv_fwd_impl(const at::Tensor& x, const at::Tensor& w2, at::Tensor out, int64_t R, int64_t S,
                             int64_t stride, int64_t pad, const at::Tensor* xs, const at::Tensor* ws,
                             const c10::optional<at::Tensor>& part, const c10::optional<at::Tensor>& shift) {
  const bool f8 = xs != nullptr;
  const auto dt = f8 ? at::kFloat8_e4m3fn : at::kBFloat16;
  const bool x_e5 = f8 && x.scalar_type() == at::kFloat8_e5m2;  // bwd-data: e5m2 dY
  const int esz = f8 ? 1 : 2;
  TORCH_CHECK(is_nhwc_dev(x, x_e5 ? at::kFloat8_e5m2 : dt), "psd conv_fwd: x must be a channels_last ",
              f8 ? "e4m3fn / e5m2" : "bf16", " device tensor");
  TORCH_CHECK(w2.is_cuda() && w2.dim() == 2 && w2.scalar_type() == dt && w2.stride(1) == 1 &&
                  (w2.stride(0) * esz) % 16 == 0 && aligned16(w2),
              "psd conv_fwd: w2 must be a 2-D device tensor like x, unit inner stride, 16-B aligned rows");
  TORCH_CHECK(out.dim() == 2 && out.stride(1) == 1 && out.scalar_type() == at::kBFloat16, "psd conv_fwd: out");
  const bool mx = f8 && xs->scalar_type() == at::kByte;  // MX: E8M0 per 32 channels of x, per 32 K of w2
  if (mx) {
    TORCH_CHECK(ws->scalar_type() == at::kByte && xs->is_cuda() && ws->is_cuda() && xs->is_contiguous() &&
                    ws->is_contiguous() && xs->numel() == x.numel() / 32 && ws->numel() == w2.numel() / 32 &&
                    w2.stride(0) == w2.size(1),
                "psd conv_fwd_fp8: MX scales must be uint8 [pixels, C/32] / [Cout, K/32] (contiguous w2)");
  } else if (f8) {
    TORCH_CHECK(xs->scalar_type() == at::kFloat && ws->scalar_type() == at::kFloat && xs->is_cuda() && ws->is_cuda() &&
                    xs->numel() >= 1 && ws->numel() >= 1,
                "psd conv_fwd_fp8: scales must be fp32 device scalars (or MX uint8 block scales)");
  }
  const ConvGeo g = conv_geo(x, R, S, stride, pad);
  const int64_t M = g.M, Cout = w2.size(0), K = R * S * g.C;
  TORCH_CHECK(w2.size(1) == K, "psd conv_fwd: w2 must be [Cout, R*S*C]");
  TORCH_CHECK(out.size(0) == M && out.size(1) == Cout, "psd conv_fwd: out must be [Nb*Ho*Wo, Cout]");
  if (!g.pow2_c() || g.C < (f8 ? 128 : 64) || g.bytes >= ((int64_t)1 << 32) || M >= ((int64_t)1 << 31)) return 0;
  const c10::DeviceGuard dg(x.device());
  GemmArgs a{};
  a.A = x.data_ptr();
  a.B = w2.data_ptr();
  a.C = out.data_ptr();
  a.M = (int)M;
  a.N = (int)Cout;
  a.K = (int)K;
  a.lda = (int)K;
  a.ldb = (int)w2.stride(0);
  a.ldc = (int)out.stride(0);
  a.a_kmajor = a.b_kmajor = 1;
  set_geo(a, g);
  if (mx) {
    a.a_mx = xs->data_ptr<uint8_t>();
    a.b_mx = ws->data_ptr<uint8_t>();
  } else if (f8) {
    a.a_scale = xs->data_ptr<float>();
    a.b_scale = ws->data_ptr<float>();
  }
  a.f8a = x_e5 ? 1 : 0;
  int rows = 0;
  set_stats(a, part, shift, out, &rows);
  hipError_t e = f8 ? launch_conv_fwd_fp8(a, stream_of(x)) : launch_conv_fwd(a, stream_of(x));
  if (e == hipErrorNotSupported) return 0;
  check_hip(e, "psd conv_fwd");
  return a.part ? rows : 1;
}

int64_t conv_fwd_(const at::Tensor& x, const at::Tensor& w2, at::Tensor out, int64_t R, int64_t S, int64_t stride,
                  int64_t pad, c10::optional<at::Tensor> part, c10::optional<at::Tensor> shift) {
  return conv_fwd_impl(x, w2, out, R, S, stride, pad, nullptr, nullptr, part, shift);
}

int64_t conv_fwd_fp8_(const at::Tensor& x, const at::Tensor& w2, const at::Tensor& x_scale, const at::Tensor& w_scale,
                      at::Tensor out, int64_t R, int64_t S, int64_t stride, int64_t pad, c10::optional<at::Tensor> part,
                      c10::optional<at::Tensor> shift) {
  return conv_fwd_impl(x, w2, out, R, S, stride, pad, &x_scale, &w_scale, part, shift);
}

// Implicit-GEMM convolution weight gradient: out [Cout, R*S*C] (an OHWI weight viewed 2-D, bf16) =
// dY^T . im2col(x), dY [Nb, Cout, Ho, Wo] and x [Nb, C, H, W] channels_last bf16; split-K over the
// output pixels (splits <= 0: about one round of workgroups). False (nothing launched) outside the
// kernel's contract.
bool conv_wgrad_(const at::Tensor& dy, const at::Tensor& x, at::Tensor out, int64_t R, int64_t S, int64_t stride,
                 int64_t pad, int64_t splits) {
  TORCH_CHECK(is_nhwc_dev(dy, at::kBFloat16) && is_nhwc_dev(x, at::kBFloat16),
              "psd conv_wgrad: dy and x must be channels_last bf16 device tensors");
  const ConvGeo g = conv_geo(x, R, S, stride, pad);
  const int64_t Cout = dy.size(1);
  TORCH_CHECK(dy_matches(dy, g), "psd conv_wgrad: dy shape does not match the convolution");
  const int64_t N = R * S * g.C, K = g.M;
  TORCH_CHECK(out.dim() == 2 && out.size(0) == Cout && out.size(1) == N && out.is_contiguous() &&
                  out.scalar_type() == at::kBFloat16,
              "psd conv_wgrad: out must be a contiguous bf16 [Cout, R*S*C]");
  if (!g.pow2_c() || g.C < 8 || g.bytes >= ((int64_t)1 << 32) || K >= ((int64_t)1 << 31) || K < 128) return false;
  const c10::DeviceGuard dg(x.device());
  const int64_t tiles = ((Cout + 255) / 256) * ((N + 255) / 256);
  int64_t s = splits > 0 ? splits : std::max<int64_t>(1, 256 / tiles);
  s = std::min<int64_t>(s, std::max<int64_t>(1, K / 128));  // >= 2 K-tiles per split
  at::Tensor slab = at::empty({s * Cout * N}, x.options().dtype(at::kFloat));
  GemmArgs a{};
  a.A = dy.data_ptr();
  a.B = x.data_ptr();
  a.M = (int)Cout;
  a.N = (int)N;
  a.K = (int)K;
  a.lda = (int)Cout;
  a.ldb = (int)N;
  a.ldc = (int)N;
  a.a_kmajor = a.b_kmajor = 0;
  set_geo(a, g);
  hipError_t e = launch_conv_wgrad(a, slab.data_ptr<float>(), (int)s, out.data_ptr(), stream_of(x));
  if (e == hipErrorNotSupported) return false;
  check_hip(e, "psd conv_wgrad");
  return true;
}

int64_t convn_stats_rows_(int64_t M) { return convn_stats_rows((int)M); }
// partial rows a launch of this variant writes (allocate at least this many: HALO variants tile by rows)
int64_t convn_part_rows_(int64_t M, int64_t N, int64_t v, int64_t Ho, int64_t Wo, int64_t R) {
  return convn_part_rows_geo((int)M, (int)N, (int)v, (int)Ho, (int)Wo, (int)R);
}
bool convn_variant_ok_(int64_t N, int64_t v, int64_t R, int64_t S, int64_t stride, int64_t pad, int64_t Wo,
                       bool has_x2) {
  return convn_variant_ok((int)N, (int)v, (int)R, (int)S, (int)stride, (int)pad, (int)Wo, has_x2);
}
int64_t convn_variants_(int64_t N) { return convn_variants((int)N); }
int64_t convn_variant_kind_(int64_t N, int64_t v) { return convn_variant_kind((int)N, (int)v); }

namespace {
// K-concatenated second operand + epilogue bias of a convn launch (the BN-backward fold); returns the
// extra K (C2) or -1 when x2 is unusable. x2: channels_last bf16 [Nb, C2, H, W] like the input.
int64_t convn_x2(ConvnArgs& a, const at::Tensor& x, c10::optional<at::Tensor> x2, c10::optional<at::Tensor> bias,
                 int64_t N) {
  if (given(bias)) {
    TORCH_CHECK(bias->scalar_type() == at::kFloat && bias->numel() == N && bias->is_contiguous() &&
                    bias->device() == x.device(),
                "psd convn: bias must be fp32 [N] on the input's device");
    a.bias = bias->data_ptr<float>();
  }
  if (!given(x2)) return 0;
  TORCH_CHECK(is_nhwc_dev(*x2, at::kBFloat16) && x2->device() == x.device() && x2->size(0) == x.size(0) &&
                  x2->size(2) == x.size(2) && x2->size(3) == x.size(3),
              "psd convn: x2 must be a channels_last bf16 tensor with the input's N, H, W");
  const int64_t C2 = x2->size(1), bytes = x2->numel() * 2;
  if (C2 < 64 || (C2 & (C2 - 1)) != 0 || bytes > 0xFFFFFF00ll) return -1;
  a.x2 = x2->data_ptr();
  a.x2bytes = (uint32_t)bytes;
  a.logC2 = log2_exact(C2);
  return C2;
}
}  // namespace

int64_t convn_(const at::Tensor& x, const at::Tensor& w2, at::Tensor out, int64_t R, int64_t S, int64_t stride,
               int64_t pad, c10::optional<at::Tensor> part, c10::optional<at::Tensor> shift, int64_t variant,
               c10::optional<at::Tensor> x2, c10::optional<at::Tensor> bias, bool no_store,
               c10::optional<at::Tensor> apply_ss, c10::optional<at::Tensor> apply_res,
               c10::optional<at::Tensor> apply_mask, bool epi_prefetch) {
  TORCH_CHECK(is_nhwc_dev(x, at::kBFloat16), "psd convn: x must be a channels_last bf16 device tensor");
  TORCH_CHECK(w2.is_cuda() && w2.dim() == 2 && w2.scalar_type() == at::kBFloat16 && w2.is_contiguous(),
              "psd convn: w2 must be a contiguous bf16 [Cout, R*S*C] device tensor");
  TORCH_CHECK(no_store || (out.is_cuda() && out.dim() == 2 && out.stride(1) == 1 &&
                           out.scalar_type() == at::kBFloat16 && aligned16(out)),
              "psd convn: out must be a bf16 [M, Cout] device tensor, 16-B aligned");
  const bool apply = given(apply_ss);
  const ConvGeo g = conv_geo(x, R, S, stride, pad);
  const int64_t M = g.M, Cout = w2.size(0), Ho = g.Ho, Wo = g.Wo;
  ConvnArgs a{};
  const int64_t C2 = convn_x2(a, x, x2, bias, Cout);
  if (C2 < 0) return 0;
  const int64_t K = R * S * g.C + C2;
  TORCH_CHECK(w2.size(1) == K, "psd convn: w2 must be [Cout, R*S*C (+ C2)]");
  TORCH_CHECK(no_store || (out.size(0) == M && out.size(1) == Cout), "psd convn: out must be [Nb*Ho*Wo, Cout]");
  const bool stats = given(part);
  TORCH_CHECK(!no_store || (stats && !apply), "psd convn: no_store is a statistics-only pass");
  if (apply) {
    TORCH_CHECK(!stats && apply_ss->scalar_type() == at::kFloat && apply_ss->numel() == 2 * Cout &&
                    apply_ss->is_contiguous() && apply_ss->device() == x.device(),
                "psd convn: apply_ss must be fp32 [2 Cout] (no statistics in an apply pass)");
    TORCH_CHECK(!given(apply_res) ||
                    (apply_res->scalar_type() == at::kBFloat16 && apply_res->numel() == M * Cout &&
                     apply_res->device() == x.device() && nhwc_laid(*apply_res)),
                "psd convn: apply_res must be a bf16 [M, Cout] (or channels_last) residual, or None");
    TORCH_CHECK(given(apply_mask) && apply_mask->scalar_type() == at::kByte && apply_mask->numel() == M * Cout / 8 &&
                    apply_mask->is_contiguous(),
                "psd convn: apply_mask must be uint8 [M * Cout / 8]");
    TORCH_CHECK(out.stride(0) == Cout, "psd convn: the apply pass writes a dense [M, Cout] output");
  }
  if (stats) {
    TORCH_CHECK(given(shift) && shift->numel() == Cout && shift->scalar_type() == at::kFloat &&
                    shift->is_contiguous() && shift->device() == x.device(),
                "psd convn: statistics need an fp32 [Cout] shift on x's device");
    TORCH_CHECK(part->scalar_type() == at::kFloat && part->is_contiguous() && part->device() == x.device() &&
                    part->numel() >= part_rows_bound(M, Cout, variant, Ho, Wo, R) * 2 * Cout,
                "psd convn: part must be fp32 [convn_part_rows(...), 2, Cout]");
  }
  const int64_t wbytes = w2.numel() * 2;
  if (!g.pow2_c() || g.C < 64 || g.bytes > 0xFFFFFF00ll || wbytes >= ((int64_t)1 << 32) ||
      M >= ((int64_t)1 << 31) - 256 || convn_tile_n((int)Cout) == 0 || (!no_store && out.stride(0) % 8 != 0) ||
      Ho <= 0 || Wo <= 0 || variant >= convn_variants((int)Cout))
    return 0;
  const c10::DeviceGuard dg(x.device());
  a.x = x.data_ptr();
  a.w = w2.data_ptr();
  a.y = no_store ? nullptr : out.data_ptr();
  a.part = stats ? part->data_ptr<float>() : nullptr;
  a.shift = stats ? shift->data_ptr<float>() : nullptr;
  if (apply) {
    a.bwd = 8;
    a.bss = apply_ss->data_ptr<float>();
    a.ares = opt_ptr<const uint16_t>(apply_res);
    a.amask = apply_mask->data_ptr<uint8_t>();
  }
  a.epi_prefetch = epi_prefetch ? 1 : 0;
  set_geo(a, g, wbytes, Cout, K, no_store ? Cout : out.stride(0), variant);
  const hipError_t e = launch_convn(a, stream_of(x));
  if (e == hipErrorNotSupported) return 0;
  check_hip(e, "psd convn");
  return stats ? convn_part_rows_geo((int)M, (int)Cout, (int)std::max<int64_t>(variant, 0), (int)Ho, (int)Wo, (int)R)
               : 1;
}

// Stride-2 3x3 (pad 1) bwd-data as four phase launches of the gathered narrow kernel: output parity
// class (ph, pw) of dX[2i + ph][2j + pw] gathers dY rows {i, i + 1}^ph x columns {j, j + 1}^pw, i.e. a
// stride-1 / pad-0 convolution of dY with a (1 + ph) x (1 + pw) tap subset of the weights
// (wph[k], k = ph << 1 | pw, bf16 [Ci, (1 + ph)(1 + pw) Co], ordered (dr, ds, co): ops/conv.py
// _dgrad_s2_phases), written at its own pixels of the full-size dX (convn.hip ophase). 9 taps in
// all -- the forward's MACs, no zero-insertion, no zero-fill of dX (every pixel is in one class).
// Optional mode-1 epilogue (the producing BN + ReLU's backward reduction, bx = its input at dX's
// resolution): the four launches' partial rows are written one after another into part. Returns the
// partial rows written (1 without part), 0 when the kernel declines (nothing launched).
int64_t convn_dgrad_s2_(const at::Tensor& dy, const std::vector<at::Tensor>& wph, at::Tensor out, int64_t variant,
                        c10::optional<at::Tensor> part, c10::optional<at::Tensor> bx, c10::optional<at::Tensor> bmean,
                        c10::optional<at::Tensor> bss) {
  TORCH_CHECK(is_nhwc_dev(dy, at::kBFloat16), "psd convn_dgrad_s2: dy must be a channels_last bf16 device tensor");
  TORCH_CHECK(wph.size() == 4, "psd convn_dgrad_s2: four phase weights");
  // every phase runs over dY's own Ho x Wo grid (stride 1, pad 0, output = input extent) with its R x S
  ConvGeo g = conv_geo(dy, 1, 1, 1, 0);
  const int64_t Co = g.C, Ho = g.Ho, Wo = g.Wo, M = g.M;
  const int64_t Ci = wph[0].size(0);
  for (int k = 0; k < 4; ++k) {
    const int64_t taps = (1 + (k >> 1)) * (1 + (k & 1));
    TORCH_CHECK(wph[k].is_cuda() && wph[k].dim() == 2 && wph[k].scalar_type() == at::kBFloat16 &&
                    wph[k].is_contiguous() && wph[k].size(0) == Ci && wph[k].size(1) == taps * Co &&
                    wph[k].device() == dy.device(),
                "psd convn_dgrad_s2: wph[k] must be a contiguous bf16 [Ci, taps * Co] tensor");
  }
  TORCH_CHECK(out.dim() == 2 && out.is_contiguous() && out.scalar_type() == at::kBFloat16 && out.size(0) == 4 * M &&
                  out.size(1) == Ci && out.device() == dy.device(),
              "psd convn_dgrad_s2: out must be a contiguous bf16 [Nb * 2Ho * 2Wo, Ci] tensor");
  const bool fused = given(part);
  if (fused) {
    TORCH_CHECK(given(bx) && bx->scalar_type() == at::kBFloat16 && bx->numel() == 4 * M * Ci &&
                    bx->device() == dy.device() && nhwc_laid(*bx),
                "psd convn_dgrad_s2: bx must be the BN input, bf16 like dX");
    TORCH_CHECK(given(bmean) && bmean->scalar_type() == at::kFloat && bmean->numel() == Ci && bmean->is_contiguous() &&
                    given(bss) && bss->scalar_type() == at::kFloat && bss->numel() == 2 * Ci && bss->is_contiguous(),
                "psd convn_dgrad_s2: mode 1 needs the BN's fp32 mean [Ci] and scale/shift [2 Ci]");
    TORCH_CHECK(part->scalar_type() == at::kFloat && part->is_contiguous() && part->device() == dy.device() &&
                    part->numel() >= 4 * part_rows_bound(M, Ci, variant, Ho, Wo, 2) * 2 * Ci,
                "psd convn_dgrad_s2: part must be fp32 [4 * convn_dgrad_s2_rows(...), 2, Ci]");
  }
  if (!g.pow2_c() || Co < 64 || g.bytes > 0xFFFFFF00ll || convn_tile_n((int)Ci) == 0 || Ci % 8 != 0 || variant < 0 ||
      variant >= convn_variants((int)Ci) || convn_variant_kind((int)Ci, (int)variant) != 0 || M >= (1 << 24))
    return 0;
  const c10::DeviceGuard dg(dy.device());
  const hipStream_t st = stream_of(dy);
  int64_t rows = 0;
  for (int k = 0; k < 4; ++k) {
    g.R = 1 + (k >> 1), g.S = 1 + (k & 1);
    ConvnArgs a{};
    a.x = dy.data_ptr();
    a.w = wph[k].data_ptr();
    a.y = out.data_ptr();
    set_geo(a, g, wph[k].numel() * 2, Ci, g.R * g.S * Co, Ci, variant);
    a.ophase = 1 + k;
    if (fused) {
      a.bwd = 1;
      a.part = part->data_ptr<float>() + rows * 2 * Ci;
      a.bx = reinterpret_cast<const uint16_t*>(bx->data_ptr());
      a.bmean = bmean->data_ptr<float>();
      a.bss = bss->data_ptr<float>();
    }
    const hipError_t e = launch_convn(a, st);
    if (e == hipErrorNotSupported) {
      TORCH_CHECK(k == 0, "psd convn_dgrad_s2: phase ", k, " declined after phase 0 ran");
      return 0;
    }
    check_hip(e, "psd convn_dgrad_s2");
    if (fused) rows += convn_part_rows_geo((int)M, (int)Ci, (int)variant, (int)Ho, (int)Wo, (int)g.R);
  }
  return fused ? rows : 1;
}

// partial rows to allocate for convn_dgrad_s2_ (all four phases) with this variant
int64_t convn_dgrad_s2_rows(int64_t Nb, int64_t Ho, int64_t Wo, int64_t Ci, int64_t variant) {
  return 4 * part_rows_bound((int)(Nb * Ho * Wo), Ci, variant, Ho, Wo, 2);
}

// bwd-data on the narrow kernel with the producing BN's backward reduction in the epilogue
// (kernels/convn.hip bwd modes): out = g = mask (conv(dy, w2) [+ dr]); part gets the partials.
// Returns the partial rows written, 0 when the kernel declines (nothing launched).
int64_t convn_bwd_(const at::Tensor& dy, const at::Tensor& w2, at::Tensor out, int64_t R, int64_t S, int64_t stride,
                   int64_t pad, at::Tensor part, int64_t variant, int64_t mode, c10::optional<at::Tensor> bx,
                   const at::Tensor& bmean, c10::optional<at::Tensor> bss, c10::optional<at::Tensor> bdr,
                   c10::optional<at::Tensor> bmbits, c10::optional<at::Tensor> x2, c10::optional<at::Tensor> bias,
                   c10::optional<at::Tensor> bxd, c10::optional<at::Tensor> bmean_d, c10::optional<at::Tensor> part_d,
                   bool epi_prefetch) {
  TORCH_CHECK(is_nhwc_dev(dy, at::kBFloat16), "psd convn_bwd: dy must be a channels_last bf16 device tensor");
  TORCH_CHECK(w2.is_cuda() && w2.dim() == 2 && w2.scalar_type() == at::kBFloat16 && w2.is_contiguous(),
              "psd convn_bwd: w2 must be a contiguous bf16 [N, R*S*C] tensor");
  TORCH_CHECK(out.dim() == 2 && out.is_contiguous() && out.scalar_type() == at::kBFloat16, "psd convn_bwd: out");
  TORCH_CHECK(mode == 1 || mode == 2 || mode == 3 || mode == 5,
              "psd convn_bwd: mode 1 (mask from x, ss), 2 (bit-mask + dr), 3 (2 + the dual tail's second BN) or 5 "
              "(2 with dr on the stride-2 quarter grid)");
  const ConvGeo g = conv_geo(dy, R, S, stride, pad);
  const int64_t Nb = g.Nb, Ho = g.Ho, Wo = g.Wo, M = g.M, N = w2.size(0);
  ConvnArgs a{};
  const int64_t C2 = convn_x2(a, dy, x2, bias, N);
  if (C2 < 0) return 0;
  const int64_t K = R * S * g.C + C2;
  TORCH_CHECK(w2.size(1) == K && out.size(0) == M && out.size(1) == N, "psd convn_bwd: shapes");
  auto like_out = [&](const at::Tensor& t, const char* what) {
    TORCH_CHECK(t.scalar_type() == at::kBFloat16 && t.numel() == M * N && t.device() == dy.device() && nhwc_laid(t),
                "psd convn_bwd: ", what, " must be a contiguous bf16 [M, N] (or channels_last) tensor");
  };
  const bool has_bx = given(bx);
  TORCH_CHECK(has_bx || mode == 2 || mode == 5, "psd convn_bwd: only modes 2 and 5 run without the BN input bx");
  if (has_bx) like_out(*bx, "bx");
  TORCH_CHECK(bmean.scalar_type() == at::kFloat && bmean.numel() == N && bmean.is_contiguous(), "psd convn_bwd: bmean");
  TORCH_CHECK(part.scalar_type() == at::kFloat && part.is_contiguous() &&
                  part.numel() >= part_rows_bound(M, N, variant, Ho, Wo, R) * 2 * N,
              "psd convn_bwd: part must be fp32 [convn_part_rows(...), 2, N]");
  if (mode == 1) {
    TORCH_CHECK(given(bss) && bss->numel() == 2 * N && bss->scalar_type() == at::kFloat && bss->is_contiguous(),
                "psd convn_bwd: mode 1 needs ss fp32 [2N]");
  } else {
    if (mode == 3) {
      TORCH_CHECK(given(bxd) && given(bmean_d) && given(part_d), "psd convn_bwd: mode 3 needs bxd, bmean_d and part_d");
      like_out(*bxd, "bxd");
      TORCH_CHECK(bmean_d->scalar_type() == at::kFloat && bmean_d->numel() == N && bmean_d->is_contiguous(),
                  "psd convn_bwd: bmean_d");
      TORCH_CHECK(part_d->scalar_type() == at::kFloat && part_d->is_contiguous() && part_d->numel() >= part.numel(),
                  "psd convn_bwd: part_d like part");
    }
    TORCH_CHECK(given(bdr), "psd convn_bwd: mode 2 needs dr");
    if (mode == 5) {
      TORCH_CHECK(bdr->scalar_type() == at::kBFloat16 && bdr->dim() == 4 && bdr->size(0) == Nb && bdr->size(1) == N &&
                      bdr->size(2) * 2 == Ho && bdr->size(3) * 2 == Wo &&
                      bdr->is_contiguous(at::MemoryFormat::ChannelsLast) && bdr->device() == dy.device(),
                  "psd convn_bwd: mode 5 dr must be channels_last bf16 [Nb, N, Ho/2, Wo/2]");
    } else {
      like_out(*bdr, "dr");
    }
    TORCH_CHECK(given(bmbits) && bmbits->scalar_type() == at::kByte && bmbits->numel() == M * N / 8 &&
                    bmbits->is_contiguous(),
                "psd convn_bwd: mode 2 needs the uint8 [M*N/8] bit-mask");
  }
  const int64_t wbytes = w2.numel() * 2;
  if (!g.pow2_c() || g.C < 64 || g.bytes > 0xFFFFFF00ll || wbytes >= ((int64_t)1 << 32) ||
      M >= ((int64_t)1 << 31) - 256 || convn_tile_n((int)N) == 0 || variant >= convn_variants((int)N) || N % 8 != 0)
    return 0;
  const c10::DeviceGuard dg(dy.device());
  a.x = dy.data_ptr();
  a.w = w2.data_ptr();
  a.y = out.data_ptr();
  a.part = part.data_ptr<float>();
  set_geo(a, g, wbytes, N, K, N, variant);
  a.epi_prefetch = epi_prefetch ? 1 : 0;
  a.bwd = (int)mode;
  a.bx = opt_ptr<const uint16_t>(bx);
  a.bmean = bmean.data_ptr<float>();
  a.bss = mode == 1 ? bss->data_ptr<float>() : nullptr;
  a.bdr = mode >= 2 ? reinterpret_cast<const uint16_t*>(bdr->data_ptr()) : nullptr;
  a.bmbits = mode >= 2 ? bmbits->data_ptr<uint8_t>() : nullptr;
  if (mode == 3) {
    a.bxd = reinterpret_cast<const uint16_t*>(bxd->data_ptr());
    a.bmean_d = bmean_d->data_ptr<float>();
    a.part_d = part_d->data_ptr<float>();
  }
  const hipError_t e = launch_convn(a, stream_of(dy));
  if (e == hipErrorNotSupported) return 0;
  check_hip(e, "psd convn_bwd");
  return convn_part_rows_geo((int)M, (int)N, (int)std::max<int64_t>(variant, 0), (int)Ho, (int)Wo, (int)R);
}

// Narrow implicit-GEMM weight gradient (kernels/convw.hip): out[Cout][R*S*C] (bf16, the OHWI weight
// layout) = dY^T . im2col(x), or out += that with accumulate. Returns false when the kernel declines
// the shape (nothing launched).
int64_t convw_variants_(int64_t Cout, int64_t KK) { return convw_variants((int)Cout, (int)KK); }

// rows of a fold launch's fp32 result: [g^T x (Cout) | x^T x (Cin) | column sums of x (+ padding)]
// 0 when the fold launch is not supported for this shape
int64_t convw_fold_rows(int64_t Cout, int64_t Cin) {
  const int64_t rows = (Cout + Cin + 16 + 127) / 128 * 128;
  return convw_fold_ok((int)Cout, (int)Cin, (int)rows) ? rows : 0;
}

namespace {
// plan, workspace and launch of a filled ConvwArgs; false when the kernel declines (nothing launched)
bool run_convw(ConvwArgs& a, const at::Tensor& x, const char* op) {
  const ConvwPlan p = convw_plan(a);
  if (p.splits <= 0) return false;
  at::Tensor slab = at::empty({p.slab_floats}, x.options().dtype(at::kFloat));
  a.slab = slab.data_ptr<float>();
  const hipError_t e = launch_convw(a, stream_of(x));
  if (e == hipErrorNotSupported) return false;
  check_hip(e, op);
  return true;
}
}  // namespace

bool convw_(const at::Tensor& dy, const at::Tensor& x, at::Tensor out, int64_t R, int64_t S, int64_t stride,
            int64_t pad, int64_t variant, bool accumulate, bool fold) {
  TORCH_CHECK(is_nhwc_dev(dy, at::kBFloat16) && is_nhwc_dev(x, at::kBFloat16) && dy.device() == x.device(),
              "psd convw: dy and x must be channels_last bf16 tensors on one device");
  const ConvGeo g = conv_geo(x, R, S, stride, pad);
  const int64_t Cout = dy.size(1);
  TORCH_CHECK(dy_matches(dy, g), "psd convw: dy shape does not match the convolution");
  const int64_t KK = R * S * g.C, M = g.M;
  const int64_t rows = fold ? convw_fold_rows(Cout, KK) : Cout;
  TORCH_CHECK(out.is_cuda() && out.device() == x.device() && out.dim() == 2 && out.size(0) == rows &&
                  out.size(1) == KK && out.is_contiguous() &&
                  out.scalar_type() == (fold ? at::kFloat : at::kBFloat16) && aligned16(out),
              "psd convw: out must be a contiguous [Cout, R*S*C] bf16 tensor (fold: fp32 [convw_fold_rows, C]) "
              "on x's device");
  if (fold && (R != 1 || S != 1 || stride != 1 || pad != 0 || accumulate)) return false;
  const int64_t dybytes = dy.numel() * 2;
  if (!g.pow2_c() || g.C < 64 || g.bytes > 0xFFFFFF00ll || dybytes > 0xFFFFFF00ll || M >= ((int64_t)1 << 31) ||
      (!fold && variant >= convw_variants((int)Cout, (int)KK)) || g.H >= 32768 || g.W >= 32768)
    return false;
  const c10::DeviceGuard dg(x.device());
  ConvwArgs a{};
  a.dy = dy.data_ptr();
  a.x = x.data_ptr();
  a.out = out.data_ptr();
  a.dybytes = (uint32_t)dybytes;
  set_geo(a, g);
  a.Cout = (int)Cout;
  a.KK = (int)KK;
  a.variant = (int)variant;
  a.accumulate = accumulate ? 1 : 0;
  a.fold = fold ? 1 : 0;
  a.Arows = (int)rows;
  return run_convw(a, x, "psd convw");
}

int64_t convw_gram_rows_(int64_t C) { return convw_gram_rows((int)C); }

// out = fp32 [convw_gram_rows(C), C]: rows [0, C) the Gram matrix x^T x of the [M, C] pixel rows of
// x, row C their column sums -- one read of x (the BN statistics of y = x W^T without forming y:
// ops/tail.py). False when the shape is unsupported.
bool convw_gram_(const at::Tensor& x, at::Tensor out, int64_t variant) {
  TORCH_CHECK(is_nhwc_dev(x, at::kBFloat16), "psd convw_gram: x must be a channels_last bf16 tensor");
  const ConvGeo g = conv_geo(x, 1, 1, 1, 0);  // the pixel rows of x: a 1x1 over its own grid
  const int64_t C = g.C, M = g.M;
  const int64_t rows = convw_gram_rows((int)C);
  TORCH_CHECK(out.is_cuda() && out.device() == x.device() && out.dim() == 2 && out.size(0) == rows &&
                  out.size(1) == C && out.is_contiguous() && out.scalar_type() == at::kFloat && aligned16(out),
              "psd convw_gram: out must be a contiguous fp32 [convw_gram_rows(C), C] tensor on x's device");
  if (rows == 0 || g.bytes > 0xFFFFFF00ll || M >= ((int64_t)1 << 31) || M == 0) return false;
  const c10::DeviceGuard dg(x.device());
  ConvwArgs a{};
  a.dy = x.data_ptr();
  a.x = x.data_ptr();
  a.out = out.data_ptr();
  a.dybytes = (uint32_t)g.bytes;
  set_geo(a, g);
  a.Cout = 0;
  a.KK = (int)C;
  a.fold = 2;
  a.variant = (int)variant;  // 1: the two-stage ring at two workgroups per CU
  a.Arows = (int)rows;
  return run_convw(a, x, "psd convw_gram");
}

}  // namespace psd
