// Tensor-level entry points for the gfx950 kernels, with bit-compatible CPU implementations for the
// host-memory PS mode (reference parity: the reference PS keeps fp32 params in host memory,
// include/parameter_server.h:9-14) and for CPU-only CI.
//
// Device tensors dispatch to the HIP launchers on the caller's current HIP stream; nothing here
// allocates device memory on the apply path, so the calls are legal under hipGraph capture.
#include "ops.h"

#include <ATen/Parallel.h>
#include <c10/core/DeviceGuard.h>

#include <cmath>
#include <cstring>
#include <limits>
#include <tuple>

#include "glue.h"
#include "kernels/launchers.h"
#include "kernels/launchers_clip.h"
#include "kernels/launchers_optim_lw.h"
#include "kernels/launchers_xfer.h"
#include "optim_lw.h"

namespace psd {

namespace {

inline void hip_check(hipError_t e, const char* what) {
  TORCH_CHECK(e == hipSuccess, "psd: ", what, " failed: ", hipGetErrorString(e));
}

inline int32_t dt_of(const at::Tensor& t) {
  switch (t.scalar_type()) {
    case at::kFloat: return DT_F32;
    case at::kBFloat16: return DT_BF16;
    case at::kFloat8_e4m3fn: return DT_F8E4M3;
    default: TORCH_CHECK(false, "psd: unsupported dtype ", t.scalar_type());
  }
}

inline void check_aligned(const at::Tensor& t, const char* name) {
  TORCH_CHECK((reinterpret_cast<uintptr_t>(t.data_ptr()) & 15u) == 0, "psd: ", name,
              " must be 16-byte aligned (flat buffers are carved at 8-element granularity)");
}

inline float bf16f(uint16_t h) {
  uint32_t u = ((uint32_t)h) << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
inline uint16_t f2bf(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40u);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}

// OCP e4m3fn byte -> fp32 (kernels/mx_common.h e4m3_to_f32)
inline float e4m3f(uint8_t b) {
  const uint32_t sg = b >> 7, e = (b >> 3) & 0xF, m = b & 7;
  if (e == 0xF && m == 7) return std::numeric_limits<float>::quiet_NaN();
  const float v = e == 0 ? std::ldexp((float)m, -9) : std::ldexp(1.f + (float)m / 8.f, (int)e - 7);
  return sg ? -v : v;
}
// element i of an MX source: q * 2^(scale byte - 127) in fp32 (ops dequantize_mx_ref)
inline float mx_elem(const uint8_t* q, const uint8_t* sc, int64_t i) {
  return e4m3f(q[i]) * std::ldexp(1.f, (int)sc[i >> 5] - 127);
}

// Scalar optimizer step: identical operation order to the device kernel (optim.hip).
inline void cpu_update(const OptimHyper& h, float lr, float bc1, float bc2s, bool first, float& p, float g,
                       float& s1, float& s2) {
  if (h.maximize) g = -g;
  switch (h.kind) {
    case OPT_SGD:
      if (h.weight_decay != 0.f) g = std::fma(h.weight_decay, p, g);
      p = std::fma(-lr, g, p);
      break;
    case OPT_MOMENTUM: {
      if (h.weight_decay != 0.f) g = std::fma(h.weight_decay, p, g);
      float buf = first ? g : std::fma(h.momentum, s1, (1.f - h.dampening) * g);
      s1 = buf;
      float d = h.nesterov ? std::fma(h.momentum, buf, g) : buf;
      p = std::fma(-lr, d, p);
      break;
    }
    default: {
      if (h.kind == OPT_ADAMW) p = p * (1.f - lr * h.weight_decay);
      else if (h.weight_decay != 0.f) g = std::fma(h.weight_decay, p, g);
      float m = std::fma(h.beta1, s1, (1.f - h.beta1) * g);
      float v = std::fma(h.beta2, s2, (1.f - h.beta2) * g * g);
      s1 = m;
      s2 = v;
      float denom = std::sqrt(v) / bc2s + h.eps;
      p = p - (lr / bc1) * (m / denom);
    }
  }
}

OptimDyn* dyn_ptr(const at::Tensor& dyn) {
  TORCH_CHECK(dyn.scalar_type() == at::kInt && dyn.numel() == 8 && dyn.is_contiguous(),
              "psd: dyn must be a contiguous int32[8] tensor (OptimDyn)");
  return reinterpret_cast<OptimDyn*>(dyn.data_ptr());
}

inline bool is_mx_payload(const at::Tensor& t) {
  return t.scalar_type() == at::kFloat8_e4m3fn || t.scalar_type() == at::kByte;
}

SourceList make_sources(const std::vector<at::Tensor>& srcs, int64_t n, const at::Device& dev,
                        const ScaleList& scales = {}, const MxScaleList& mx_scales = {}) {
  TORCH_CHECK(!srcs.empty() && (int)srcs.size() <= kMaxSources, "psd: 1..16 gradient sources required");
  SourceList s{};
  s.count = (int32_t)srcs.size();
  const bool mx = !mx_scales.empty();
  if (mx) {
    // MX sources: e4m3 payload + one E8M0 byte per 32 elements, for every source
    TORCH_CHECK(mx_scales.size() == srcs.size(), "psd: MX scale bytes must be given for every gradient source or for "
                "none (", mx_scales.size(), " of ", srcs.size(), " set)");
    TORCH_CHECK(n % 32 == 0, "psd: MX gradient sources come in whole 32-element blocks, got ", n, " elements");
    s.dtype = DT_MX8;
  } else {
    TORCH_CHECK(!is_mx_payload(srcs[0]), "psd: float8_e4m3fn / uint8 gradient sources are MX payloads: pass their "
                "scale bytes (mx_scales)");
    s.dtype = dt_of(srcs[0]);
  }
  for (size_t k = 0; k < srcs.size(); ++k) {
    TORCH_CHECK(srcs[k].device() == dev, "psd: gradient source on wrong device");
    if (mx) {
      TORCH_CHECK(is_mx_payload(srcs[k]), "psd: MX gradient sources must be float8_e4m3fn or uint8");
      const at::Tensor& b = mx_scales[k];
      TORCH_CHECK(b.scalar_type() == at::kByte && b.is_contiguous() && b.numel() == n / 32 && b.device() == dev,
                  "psd: an MX source's scales must be uint8 [numel / 32] on the master's device");
      s.mx_scale[k] = b.data_ptr<uint8_t>();
    } else {
      TORCH_CHECK(dt_of(srcs[k]) == s.dtype, "psd: gradient sources must share a dtype");
    }
    TORCH_CHECK(srcs[k].is_contiguous() && srcs[k].numel() == n, "psd: gradient source shape mismatch");
    s.ptr[k] = srcs[k].data_ptr();
  }
  // per-source scales: none, or one fp32 device scalar for every source
  size_t set = 0;
  for (auto& t : scales) set += given(t);
  if (set == 0) return s;
  TORCH_CHECK(scales.size() == srcs.size() && set == srcs.size(),
              "psd: per-source scales must be given for every gradient source or for none (", set, " of ",
              srcs.size(), " set)");
  for (size_t k = 0; k < srcs.size(); ++k) {
    const at::Tensor& t = *scales[k];
    TORCH_CHECK(t.scalar_type() == at::kFloat && t.numel() >= 1 && t.is_contiguous() && t.device() == dev,
                "psd: a source scale must be an fp32 tensor (element 0 is the scale) on the master's device");
    s.scale[k] = t.data_ptr<float>();
  }
  return s;
}

// Validated raw view of one apply call's tensors (shared by the flat and the layer-table entry points).
struct ApplyArgs {
  OptimHyper h{};
  int64_t n = 0;
  float* s1 = nullptr;
  float* s2 = nullptr;
  uint16_t* sh = nullptr;
  SourceList src{};
};

ApplyArgs apply_args(const at::Tensor& master, const std::vector<at::Tensor>& grads,
                     const c10::optional<at::Tensor>& state1, const c10::optional<at::Tensor>& state2,
                     const c10::optional<at::Tensor>& shadow, const at::Tensor& dyn, int64_t kind, double momentum,
                     double dampening, bool nesterov, double weight_decay, double beta1, double beta2, double eps,
                     bool maximize, const ScaleList& scales, const MxScaleList& mx_scales) {
  TORCH_CHECK(master.scalar_type() == at::kFloat && master.is_contiguous(), "psd: master must be contiguous fp32");
  ApplyArgs a;
  const int64_t n = a.n = master.numel();
  OptimHyper& h = a.h;
  h.kind = (int32_t)kind;
  h.nesterov = nesterov;
  h.maximize = maximize;
  h.momentum = (float)momentum;
  h.dampening = (float)dampening;
  h.weight_decay = (float)weight_decay;
  h.beta1 = (float)beta1;
  h.beta2 = (float)beta2;
  h.eps = (float)eps;
  const bool need1 = kind != OPT_SGD, need2 = kind == OPT_ADAM || kind == OPT_ADAMW || kind == OPT_LAMB;
  if (need1) {
    TORCH_CHECK(state1.has_value() && state1->numel() == n && state1->scalar_type() == at::kFloat &&
                    state1->is_contiguous() && state1->device() == master.device(),
                "psd: optimizer needs fp32 state1 like master");
    a.s1 = state1->data_ptr<float>();
  }
  if (need2) {
    TORCH_CHECK(state2.has_value() && state2->numel() == n && state2->scalar_type() == at::kFloat &&
                    state2->is_contiguous() && state2->device() == master.device(),
                "psd: optimizer needs fp32 state2 like master");
    a.s2 = state2->data_ptr<float>();
  }
  if (given(shadow)) {
    TORCH_CHECK(shadow->scalar_type() == at::kBFloat16 && shadow->numel() == n && shadow->is_contiguous() &&
                    shadow->device() == master.device(),
                "psd: shadow must be contiguous bf16 like master");
    a.sh = reinterpret_cast<uint16_t*>(shadow->data_ptr());
  }
  a.src = make_sources(grads, n, master.device(), scales, mx_scales);
  TORCH_CHECK(dyn.device() == master.device(), "psd: dyn must live with master");
  if (master.is_cuda()) {
    check_aligned(master, "master");
    if (a.s1) check_aligned(*state1, "state1");
    if (a.s2) check_aligned(*state2, "state2");
    if (a.sh) check_aligned(*shadow, "shadow");
    for (auto& t : grads) check_aligned(t, "grad");
  }
  return a;
}

// grad_scale * sum_k src_k[i], or with scales grad_scale * sum_k scale_k * src_k[i] (one fma per
// source, in source order: optim_update.h load_sources8)
inline float cpu_source(const SourceList& src, int64_t i, float gs) {
  float g = 0.f;
  const bool scaled = src.scale[0] != nullptr;
  for (int k = 0; k < src.count; ++k) {
    const float x = src.dtype == DT_MX8    ? mx_elem(static_cast<const uint8_t*>(src.ptr[k]), src.mx_scale[k], i)
                    : src.dtype == DT_BF16 ? bf16f(static_cast<const uint16_t*>(src.ptr[k])[i])
                                           : static_cast<const float*>(src.ptr[k])[i];
    if (scaled) g = std::fma(*src.scale[k], x, g);
    else g += x;
  }
  return g * gs;
}

// LAMB update direction (kernels/optim_lw.hip lamb_u)
inline float cpu_lamb_u(float m, float v, float w, float bc1, float bc2s, float eps, float wd) {
  const float q = (m / bc1) / (std::sqrt(v) / bc2s + eps);
  return std::fma(wd, w, q);
}

}  // namespace

void fused_apply_(at::Tensor master, const std::vector<at::Tensor>& grads, c10::optional<at::Tensor> state1,
                  c10::optional<at::Tensor> state2, c10::optional<at::Tensor> shadow, at::Tensor dyn, int64_t kind,
                  double momentum, double dampening, bool nesterov, double weight_decay, double beta1, double beta2,
                  double eps, bool maximize, int64_t grid_cap, const ScaleList& scales, const MxScaleList& mx_scales) {
  TORCH_CHECK(kind >= OPT_SGD && kind <= OPT_ADAMW,
              "psd: fused_apply_ takes sgd / momentum / adam / adamw; lars and lamb need a layer table "
              "(fused_apply_lw_)");
  const ApplyArgs a = apply_args(master, grads, state1, state2, shadow, dyn, kind, momentum, dampening, nesterov,
                                 weight_decay, beta1, beta2, eps, maximize, scales, mx_scales);
  const OptimHyper& h = a.h;
  const int64_t n = a.n;
  float *s1 = a.s1, *s2 = a.s2;
  uint16_t* sh = a.sh;
  const SourceList& src = a.src;

  if (master.is_cuda()) {
    const c10::DeviceGuard g(master.device());
    hip_check(launch_fused_apply(h, dyn_ptr(dyn), master.data_ptr<float>(), src, s1, s2, sh, n, stream_of(master),
                                 (int)grid_cap),
              "fused_apply");
    return;
  }
  const OptimDyn d = *dyn_ptr(dyn);
  const float lr = d.lr, gs = d.grad_scale, bc1 = d.bc1, bc2s = std::sqrt(d.bc2);
  const bool first = d.step <= 1;
  float* p = master.data_ptr<float>();
  at::parallel_for(0, n, 1 << 14, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; ++i) {
      float g = cpu_source(src, i, gs);
      float a = s1 ? s1[i] : 0.f, c = s2 ? s2[i] : 0.f;
      cpu_update(h, lr, bc1, bc2s, first, p[i], g, a, c);
      if (s1) s1[i] = a;
      if (s2) s2[i] = c;
      if (sh) sh[i] = f2bf(p[i]);
    }
  });
}

const LwGpu*& lw_gpu() {
  static const LwGpu* table = nullptr;
  return table;
}

std::vector<at::Tensor> lw_table_build(const std::vector<int64_t>& offsets, const std::vector<int64_t>& numels,
                                       const std::vector<int64_t>& ndims, int64_t n, bool exclude_1d, int64_t align,
                                       const at::Device& device) {
  const size_t T = offsets.size();
  TORCH_CHECK(T >= 1 && numels.size() == T && ndims.size() == T, "psd: layer table needs one (offset, numel, ndim) per tensor");
  TORCH_CHECK(align >= 8 && align % 8 == 0, "psd: layer table alignment must be a multiple of 8 elements");
  TORCH_CHECK(offsets[0] == 0, "psd: the first tensor of a layer table starts its range (offset 0)");
  TORCH_CHECK(n % 8 == 0, "psd: a layer table's range must be a multiple of 8 elements, got ", n);
  std::vector<int64_t> seg(T + 1), coff;
  std::vector<int32_t> segc(T + 1), adapt(T), cseg;
  std::vector<float> wdm(T);
  for (size_t t = 0; t < T; ++t) {
    const int64_t end = t + 1 < T ? offsets[t + 1] : n;
    TORCH_CHECK(offsets[t] % align == 0, "psd: layer table: tensor ", t, " starts at ", offsets[t],
                ", not on a ", align, "-element boundary");
    TORCH_CHECK(numels[t] >= 0 && offsets[t] + std::max<int64_t>(numels[t], 1) <= end, "psd: layer table: tensor ", t,
                " overlaps the next one or the end of the range");
    seg[t] = offsets[t];
    segc[t] = (int32_t)cseg.size();
    const bool excl = exclude_1d && ndims[t] <= 1;
    wdm[t] = excl ? 0.f : 1.f;
    adapt[t] = excl ? 0 : 1;
    for (int64_t o = offsets[t]; o < end; o += kLwChunk) {
      TORCH_CHECK(cseg.size() < (size_t)INT32_MAX, "psd: layer table: too many chunks");
      cseg.push_back((int32_t)t);
      coff.push_back(o);
    }
  }
  seg[T] = n;
  segc[T] = (int32_t)cseg.size();
  const int64_t C = (int64_t)cseg.size();
  auto dev_of = [&](const void* p, int64_t count, at::ScalarType st) {
    at::Tensor h = at::empty({count}, at::TensorOptions().dtype(st));
    std::memcpy(h.data_ptr(), p, (size_t)count * h.element_size());
    return h.to(device);
  };
  at::Tensor meta = at::empty({3}, at::kLong);
  meta.data_ptr<int64_t>()[0] = n;
  meta.data_ptr<int64_t>()[1] = (int64_t)T;
  meta.data_ptr<int64_t>()[2] = C;
  return {meta,
          dev_of(seg.data(), (int64_t)T + 1, at::kLong),
          dev_of(segc.data(), (int64_t)T + 1, at::kInt),
          dev_of(wdm.data(), (int64_t)T, at::kFloat),
          dev_of(adapt.data(), (int64_t)T, at::kInt),
          dev_of(cseg.data(), C, at::kInt),
          dev_of(coff.data(), C, at::kLong),
          at::zeros({2 * C}, at::TensorOptions().dtype(at::kFloat).device(device)),
          at::ones({(int64_t)T}, at::TensorOptions().dtype(at::kFloat).device(device))};
}

void fused_apply_lw_(at::Tensor master, const std::vector<at::Tensor>& grads, c10::optional<at::Tensor> state1,
                     c10::optional<at::Tensor> state2, c10::optional<at::Tensor> shadow, at::Tensor dyn, int64_t kind,
                     double momentum, double dampening, bool nesterov, double weight_decay, double beta1, double beta2,
                     double eps, bool maximize, double trust_coef, const std::vector<at::Tensor>& layers,
                     int64_t grid_cap, const ScaleList& scales, const MxScaleList& mx_scales) {
  TORCH_CHECK(kind >= OPT_SGD && kind <= OPT_LAMB, "psd: unknown optimizer kind ", kind);
  const ApplyArgs a = apply_args(master, grads, state1, state2, shadow, dyn, kind, momentum, dampening, nesterov,
                                 weight_decay, beta1, beta2, eps, maximize, scales, mx_scales);
  // ---- the layer table (lw_table_build): shapes, dtypes, device, and the range it was built for
  TORCH_CHECK(layers.size() == 9, "psd: layer table must be the 9 tensors of lw_table_build");
  const at::Tensor& meta = layers[0];
  TORCH_CHECK(meta.device().is_cpu() && meta.scalar_type() == at::kLong && meta.numel() == 3, "psd: layer table meta");
  const int64_t T = meta.data_ptr<int64_t>()[1], C = meta.data_ptr<int64_t>()[2];
  TORCH_CHECK(meta.data_ptr<int64_t>()[0] == a.n, "psd: layer table was built for ", meta.data_ptr<int64_t>()[0],
              " elements, master has ", a.n);
  const at::ScalarType want_dt[9] = {at::kLong, at::kLong, at::kInt, at::kFloat, at::kInt,
                                     at::kInt,  at::kLong, at::kFloat, at::kFloat};
  const int64_t want_n[9] = {3, T + 1, T + 1, T, T, C, C, 2 * C, T};
  for (int i = 1; i < 9; ++i)
    TORCH_CHECK(layers[i].scalar_type() == want_dt[i] && layers[i].numel() == want_n[i] && layers[i].is_contiguous() &&
                    layers[i].device() == master.device(),
                "psd: layer table tensor ", i, " has the wrong dtype, size or device");
  TORCH_CHECK(T >= 1 && C >= 1 && T <= INT32_MAX && C <= INT32_MAX, "psd: empty layer table");
  LwTable t{};
  t.seg_start = layers[1].data_ptr<int64_t>();
  t.seg_chunk = layers[2].data_ptr<int32_t>();
  t.wd_mult = layers[3].data_ptr<float>();
  t.adapt = layers[4].data_ptr<int32_t>();
  t.chunk_seg = layers[5].data_ptr<int32_t>();
  t.chunk_off = layers[6].data_ptr<int64_t>();
  t.partials = layers[7].data_ptr<float>();
  t.ratio = layers[8].data_ptr<float>();
  t.n_seg = (int32_t)T;
  t.n_chunks = (int32_t)C;
  t.trust_coef = (float)trust_coef;
  const OptimHyper& h = a.h;
  const bool layerwise = kind == OPT_LARS || kind == OPT_LAMB;
  float* p = master.data_ptr<float>();

  if (master.is_cuda()) {
    const LwGpu* gpu = lw_gpu();
    TORCH_CHECK(gpu != nullptr, "psd: the gfx950 layer-table kernels are not linked into this build; only CPU tensors "
                                "can take a layer table here");
    const c10::DeviceGuard g(master.device());
    hipStream_t st = stream_of(master);
    if (layerwise) {
      hip_check(gpu->norms(h, dyn_ptr(dyn), p, a.src, a.s1, a.s2, t, st, (int)grid_cap), "lw_norms");
      hip_check(gpu->finalize(h, t, st, (int)grid_cap), "lw_finalize");
    }
    hip_check(gpu->apply(h, dyn_ptr(dyn), p, a.src, a.s1, a.s2, a.sh, t, st, (int)grid_cap), "lw_apply");
    return;
  }

  // ---- host path: the same three passes. Sums go per chunk, then per segment over the chunks in
  // order, so the result does not depend on the thread count or on where the buffer was cut.
  const OptimDyn d = *dyn_ptr(dyn);
  const float lr = d.lr, gs = d.grad_scale, bc1 = d.bc1, bc2s = std::sqrt(d.bc2);
  const bool first = d.step <= 1;
  const SourceList& src = a.src;
  float *s1 = a.s1, *s2 = a.s2;
  uint16_t* sh = a.sh;
  auto chunk_end = [&](int64_t c) {
    const int64_t left = t.seg_start[t.chunk_seg[c] + 1] - t.chunk_off[c];
    return t.chunk_off[c] + std::min<int64_t>(left, kLwChunk);
  };
  if (layerwise) {
    at::parallel_for(0, C, 4, [&](int64_t cb, int64_t ce) {
      for (int64_t c = cb; c < ce; ++c) {
        const float wd = h.weight_decay * t.wd_mult[t.chunk_seg[c]];
        double aw = 0.0, ab = 0.0;
        for (int64_t i = t.chunk_off[c], e = chunk_end(c); i < e; ++i) {
          float g = cpu_source(src, i, gs);
          float b = g;
          if (kind == OPT_LAMB) {
            if (h.maximize) g = -g;
            s1[i] = std::fma(h.beta1, s1[i], (1.f - h.beta1) * g);
            s2[i] = std::fma(h.beta2, s2[i], (1.f - h.beta2) * g * g);
            b = cpu_lamb_u(s1[i], s2[i], p[i], bc1, bc2s, h.eps, wd);
          }
          aw += (double)p[i] * p[i];
          ab += (double)b * b;
        }
        t.partials[2 * c] = (float)aw;
        t.partials[2 * c + 1] = (float)ab;
      }
    });
    for (int64_t s = 0; s < T; ++s) {
      double aw = 0.0, ab = 0.0;
      for (int64_t c = t.seg_chunk[s]; c < t.seg_chunk[s + 1]; ++c) {
        aw += t.partials[2 * c];
        ab += t.partials[2 * c + 1];
      }
      const float wn = (float)std::sqrt(aw), bn = (float)std::sqrt(ab);
      float r = 1.f;
      if (t.adapt[s] && wn > 0.f && bn > 0.f) {
        if (kind == OPT_LAMB) r = wn / bn;
        else r = t.trust_coef * wn / (bn + h.weight_decay * t.wd_mult[s] * wn + h.eps);
      }
      t.ratio[s] = r;
    }
  }
  at::parallel_for(0, C, 4, [&](int64_t cb, int64_t ce) {
    for (int64_t c = cb; c < ce; ++c) {
      const int32_t s = t.chunk_seg[c];
      const float wd = h.weight_decay * t.wd_mult[s];
      const float r = layerwise ? t.ratio[s] : 1.f;
      OptimHyper hs = h;
      hs.weight_decay = kind == OPT_LARS ? 0.f : wd;
      if (kind == OPT_LARS) {
        hs.kind = OPT_MOMENTUM;
        hs.maximize = 0;
      }
      for (int64_t i = t.chunk_off[c], e = chunk_end(c); i < e; ++i) {
        if (kind == OPT_LAMB) {
          const float u = cpu_lamb_u(s1[i], s2[i], p[i], bc1, bc2s, h.eps, wd);
          p[i] = std::fma(-(lr * r), u, p[i]);
        } else {
          float g = cpu_source(src, i, gs);
          if (kind == OPT_LARS) {
            if (h.maximize) g = -g;
            if (wd != 0.f) g = std::fma(wd, p[i], g);
            g *= r;
          }
          float m = s1 ? s1[i] : 0.f, v = s2 ? s2[i] : 0.f;
          cpu_update(hs, lr, bc1, bc2s, first, p[i], g, m, v);
          if (s1) s1[i] = m;
          if (s2) s2[i] = v;
        }
        if (sh) sh[i] = f2bf(p[i]);
      }
    }
  });
}

void optim_advance_(at::Tensor dyn, double beta1, double beta2) {
  OptimDyn* d = dyn_ptr(dyn);
  if (dyn.is_cuda()) {
    const c10::DeviceGuard g(dyn.device());
    hip_check(launch_optim_advance(d, (float)beta1, (float)beta2, stream_of(dyn)), "optim_advance");
    return;
  }
  d->step += 1;
  d->bc1 = 1.f - std::pow((float)beta1, (float)d->step);
  d->bc2 = 1.f - std::pow((float)beta2, (float)d->step);
}

void multi_reduce_(at::Tensor out, const std::vector<at::Tensor>& srcs, double scale, const ScaleList& scales,
                   const MxScaleList& mx_scales) {
  TORCH_CHECK(out.is_contiguous(), "psd: out must be contiguous");
  const int64_t n = out.numel();
  SourceList s = make_sources(srcs, n, out.device(), scales, mx_scales);
  const int32_t od = dt_of(out);
  TORCH_CHECK(od == DT_F32 || od == DT_BF16, "psd: reduce output must be fp32/bf16");
  if (out.is_cuda()) {
    const c10::DeviceGuard g(out.device());
    check_aligned(out, "out");
    for (auto& t : srcs) check_aligned(t, "src");
    hip_check(launch_multi_reduce(s, out.data_ptr(), od, (float)scale, n, stream_of(out)), "multi_reduce");
    return;
  }
  at::parallel_for(0, n, 1 << 14, [&](int64_t b, int64_t e) {
    for (int64_t i = b; i < e; ++i) {
      const float acc = cpu_source(s, i, (float)scale);
      if (od == DT_BF16) static_cast<uint16_t*>(out.data_ptr())[i] = f2bf(acc);
      else static_cast<float*>(out.data_ptr())[i] = acc;
    }
  });
}

// Global L2 norm of `flat` and its clipping coefficient (kernels/clip.hip): out[0] = c, out[1] = n.
// The host path adds in the device kernels' order -- 256 lanes of sequential fmas per chunk, xor
// butterfly, waves 0..3, then the chunk partials lane-strided and an fp64 tree -- so CPU and GPU
// give the same bits for the same stored values.
void grad_clip_coef_(const at::Tensor& flat, double clip_norm, at::Tensor out, at::Tensor partials, int64_t grid_cap) {
  TORCH_CHECK(flat.is_contiguous() && (flat.scalar_type() == at::kFloat || flat.scalar_type() == at::kBFloat16),
              "psd: grad_clip_coef_ takes a contiguous fp32 or bf16 gradient buffer");
  TORCH_CHECK(std::isfinite(clip_norm) && clip_norm >= 0.0, "psd: clip_norm must be finite and >= 0, got ", clip_norm);
  const int64_t n = flat.numel(), C = clip_chunks(n);
  TORCH_CHECK(out.scalar_type() == at::kFloat && out.numel() >= 2 && out.is_contiguous() && out.device() == flat.device(),
              "psd: grad_clip_coef_ out must be an fp32 block of >= 2 elements on the gradient's device");
  TORCH_CHECK(partials.scalar_type() == at::kFloat && partials.numel() >= C && partials.is_contiguous() &&
                  partials.device() == flat.device(),
              "psd: grad_clip_coef_ partials must be fp32 [>= ", C, "] (one per 8192 elements) on the gradient's device");
  const int32_t dt = dt_of(flat);
  if (flat.is_cuda()) {
    const c10::DeviceGuard g(flat.device());
    check_aligned(flat, "flat gradient");
    hipStream_t st = stream_of(flat);
    hip_check(launch_sumsq_partials(flat.data_ptr(), dt, n, partials.data_ptr<float>(), st, (int)grid_cap), "sumsq_partials");
    hip_check(launch_clip_finalize(partials.data_ptr<float>(), C, (float)clip_norm, out.data_ptr<float>(), st),
              "clip_finalize");
    return;
  }
  float* part = partials.data_ptr<float>();
  const void* gp = flat.data_ptr();
  auto at_i = [&](int64_t i) {
    return dt == DT_BF16 ? bf16f(static_cast<const uint16_t*>(gp)[i]) : static_cast<const float*>(gp)[i];
  };
  at::parallel_for(0, C, 4, [&](int64_t cb, int64_t ce) {
    for (int64_t c = cb; c < ce; ++c) {
      const int64_t off = c * kClipChunk;
      const int len = (int)std::min<int64_t>(n - off, kClipChunk), nvec = len >> 3;
      float lane[256];
      for (int l = 0; l < 256; ++l) {
        float acc = 0.f;
        for (int v = l; v < nvec; v += 256)
          for (int e = 0; e < 8; ++e) {
            const float x = at_i(off + ((int64_t)v << 3) + e);
            acc = std::fma(x, x, acc);
          }
        lane[l] = acc;
      }
      for (int64_t i = off + ((int64_t)nvec << 3); i < off + len; ++i) {  // the n % 8 tail: lane 255
        const float x = at_i(i);
        lane[255] = std::fma(x, x, lane[255]);
      }
      float w[4];
      for (int wv = 0; wv < 4; ++wv) {  // xor butterfly of one wave: every lane ends with the same sum
        float* x = lane + 64 * wv;
        for (int m = 32; m >= 1; m >>= 1) {
          float y[64];
          for (int l = 0; l < 64; ++l) y[l] = x[l] + x[l ^ m];
          std::memcpy(x, y, sizeof(y));
        }
        w[wv] = x[0];
      }
      part[c] = ((w[0] + w[1]) + w[2]) + w[3];
    }
  });
  double sh[256];
  for (int l = 0; l < 256; ++l) {
    double a = 0.0;
    for (int64_t c = l; c < C; c += 256) a += (double)part[c];
    sh[l] = a;
  }
  for (int s = 128; s >= 1; s >>= 1)
    for (int l = 0; l < s; ++l) sh[l] += sh[l + s];
  const float nrm = (float)std::sqrt(sh[0]);
  const float q = (float)clip_norm / (nrm + 1e-6f);
  out.data_ptr<float>()[0] = q > 1.f ? 1.f : q;
  out.data_ptr<float>()[1] = nrm;
}

void xfer_(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts, int64_t blocks_per_seg,
           bool nt_store) {
  TORCH_CHECK(srcs.size() == dsts.size() && !srcs.empty() && (int)srcs.size() <= kMaxXferSeg, "psd: xfer_ segments");
  XferList L{};
  for (size_t i = 0; i < srcs.size(); ++i) {
    const at::Tensor &a = srcs[i], &b = dsts[i];
    TORCH_CHECK(a.is_cuda() && b.is_cuda() && a.is_contiguous() && b.is_contiguous() && a.nbytes() == b.nbytes(),
                "psd: xfer_ takes contiguous device tensors of equal byte size");
    check_aligned(a, "xfer_ src");
    check_aligned(b, "xfer_ dst");
    L.seg[L.count++] = XferSeg{a.data_ptr(), b.data_ptr(), (int64_t)a.nbytes()};
  }
  L.blocks_per_seg = (int32_t)blocks_per_seg;
  L.nt_store = nt_store ? 1 : 0;
  const c10::DeviceGuard g(srcs[0].device());
  hip_check(launch_xfer(L, stream_of(srcs[0])), "launch_xfer");
}

void push_quant_mx_(const at::Tensor& x, at::Tensor q, at::Tensor scales, int64_t blocks_per_seg,
                    c10::optional<at::Tensor> residual) {
  const int64_t n = x.numel();
  TORCH_CHECK(x.is_contiguous() && (x.scalar_type() == at::kFloat || x.scalar_type() == at::kBFloat16) && n % 32 == 0,
              "psd: push_quant_mx_ takes a contiguous fp32 or bf16 tensor of a multiple of 32 elements");
  TORCH_CHECK(is_mx_payload(q) && q.is_contiguous() && q.numel() == n && q.device() == x.device(),
              "psd: push_quant_mx_ q must be float8_e4m3fn or uint8 like x");
  TORCH_CHECK(scales.scalar_type() == at::kByte && scales.is_contiguous() && scales.numel() == n / 32 &&
                  scales.device() == x.device(),
              "psd: push_quant_mx_ scales must be uint8 [numel / 32] on x's device");
  TORCH_CHECK(blocks_per_seg >= 0 && blocks_per_seg <= 1024, "psd: push_quant_mx_ blocks_per_seg in [0, 1024]");
  const bool ef = residual.has_value() && residual->defined();
  if (ef)
    TORCH_CHECK(residual->scalar_type() == at::kFloat && residual->is_contiguous() && residual->numel() == n &&
                    residual->device() == x.device(),
                "psd: push_quant_mx_ residual must be contiguous fp32 [numel] on x's device");
  if (n == 0) return;
  if (x.is_cuda()) {
    check_aligned(x, "push_quant_mx_ x");
    check_aligned(q, "push_quant_mx_ q");
    if (ef) check_aligned(*residual, "push_quant_mx_ residual");
    XferQList L{};
    L.seg[L.count++] = XferQSeg{x.data_ptr(), static_cast<uint8_t*>(q.data_ptr()), scales.data_ptr<uint8_t>(), n,
                                ef ? residual->data_ptr<float>() : nullptr};
    L.blocks_per_seg = blocks_per_seg > 0 ? (int32_t)blocks_per_seg : xfer_blocks(n, 48);
    L.src_dtype = dt_of(x);
    const c10::DeviceGuard g(x.device());
    hip_check(launch_xfer_quant(L, stream_of(x)), "launch_xfer_quant");
    return;
  }
  // host: the operations of ops.quantize_mx_ref (the smallest 2^e with amax 2^-e <= 448, byte 127 for
  // an all-zero or non-finite block, round to nearest even), then the non-finite rule; with a residual
  // the operations of ops.push_quant_mx_ef_ref (v = fp32(x) + r before, r = v - dq(q) after, 0 where
  // v is not finite)
  at::Tensor xf = x.to(at::kFloat).view({-1, 32});
  if (ef) xf = xf + residual->view({-1, 32});
  const at::Tensor amax = xf.abs().amax(1);
  at::Tensor m, p;
  std::tie(m, p) = at::frexp(amax / 448.f);
  at::Tensor e = at::where(m == 0.5f, p - 1, p).clamp(-127, 127);
  e = at::where((amax > 0) & at::isfinite(amax), e, at::zeros_like(e));
  const at::Tensor v = (xf * at::exp2(-e.to(at::kFloat)).unsqueeze(1)).clamp(-448.f, 448.f);
  at::Tensor qb = v.to(at::kFloat8_e4m3fn).view(at::kByte);
  qb = at::where(at::isfinite(xf), qb, at::full({}, 0x7F, qb.options()));
  q.view(at::kByte).view({-1, 32}).copy_(qb);
  scales.copy_((e + 127).to(at::kByte));
  if (ef) {
    const at::Tensor dq = qb.view(at::kFloat8_e4m3fn).to(at::kFloat) * at::exp2(e.to(at::kFloat)).unsqueeze(1);
    residual->view({-1, 32}).copy_(at::where(at::isfinite(xf), xf - dq, at::zeros_like(xf)));
  }
}

void pack_cast_(const std::vector<at::Tensor>& srcs, const std::vector<at::Tensor>& dsts) {
  TORCH_CHECK(srcs.size() == dsts.size(), "psd: pack_cast needs matching src/dst lists");
  if (srcs.empty()) return;
  const int32_t sd = dt_of(srcs[0]), dd = dt_of(dsts[0]);
  const auto dev = srcs[0].device();
  for (size_t i = 0; i < srcs.size(); ++i) {
    TORCH_CHECK(dt_of(srcs[i]) == sd && dt_of(dsts[i]) == dd, "psd: pack_cast dtypes must be uniform");
    TORCH_CHECK(srcs[i].numel() == dsts[i].numel(), "psd: pack_cast numel mismatch at ", i);
    TORCH_CHECK(srcs[i].is_contiguous() && dsts[i].is_contiguous(), "psd: pack_cast needs contiguous tensors");
    TORCH_CHECK(srcs[i].device() == dev && dsts[i].device() == dev, "psd: pack_cast device mismatch");
  }
  if (dev.is_cuda()) {
    constexpr int64_t kChunk = 8192;
    std::vector<PackSeg> segs(srcs.size());
    std::vector<int32_t> cseg;
    std::vector<int64_t> coff;
    for (size_t i = 0; i < srcs.size(); ++i) {
      segs[i] = PackSeg{srcs[i].data_ptr(), dsts[i].data_ptr(), srcs[i].numel()};
      for (int64_t o = 0; o < srcs[i].numel(); o += kChunk) {
        cseg.push_back((int32_t)i);
        coff.push_back(o);
      }
    }
    if (cseg.empty()) return;
    // one host staging tensor -> one H2D copy for the whole table
    const int64_t seg_bytes = (int64_t)(segs.size() * sizeof(PackSeg));
    const int64_t off_bytes = (int64_t)(coff.size() * sizeof(int64_t));
    const int64_t cs_bytes = (int64_t)(cseg.size() * sizeof(int32_t));
    const int64_t total = seg_bytes + off_bytes + cs_bytes;
    auto host = at::empty({total}, at::TensorOptions().dtype(at::kByte).pinned_memory(true));
    uint8_t* hp = host.data_ptr<uint8_t>();
    std::memcpy(hp, segs.data(), seg_bytes);
    std::memcpy(hp + seg_bytes, coff.data(), off_bytes);
    std::memcpy(hp + seg_bytes + off_bytes, cseg.data(), cs_bytes);
    const c10::DeviceGuard g(dev);
    auto table = at::empty({total}, at::TensorOptions().dtype(at::kByte).device(dev));
    table.copy_(host, /*non_blocking=*/true);
    uint8_t* tp = table.data_ptr<uint8_t>();
    hip_check(launch_pack_cast(reinterpret_cast<const PackSeg*>(tp), reinterpret_cast<const int32_t*>(tp + seg_bytes + off_bytes),
                               reinterpret_cast<const int64_t*>(tp + seg_bytes), (int64_t)cseg.size(), sd, dd,
                               stream_of(srcs[0])),
              "pack_cast");
    return;
  }
  for (size_t t = 0; t < srcs.size(); ++t) {
    const int64_t n = srcs[t].numel();
    const void* sp = srcs[t].data_ptr();
    void* dp = dsts[t].data_ptr();
    at::parallel_for(0, n, 1 << 15, [&](int64_t b, int64_t e) {
      for (int64_t i = b; i < e; ++i) {
        float x = sd == DT_BF16 ? bf16f(static_cast<const uint16_t*>(sp)[i]) : static_cast<const float*>(sp)[i];
        if (dd == DT_BF16) static_cast<uint16_t*>(dp)[i] = f2bf(x);
        else static_cast<float*>(dp)[i] = x;
      }
    });
  }
}

void amax_(const at::Tensor& x, at::Tensor amax_out) {
  TORCH_CHECK(amax_out.scalar_type() == at::kFloat && amax_out.numel() >= 1, "psd: amax_out must be fp32[>=1]");
  TORCH_CHECK(x.is_contiguous(), "psd: amax input must be contiguous");
  if (x.is_cuda()) {
    const c10::DeviceGuard g(x.device());
    if (x.numel() >= 8) check_aligned(x, "x");  // 16-byte vector loads
    hip_check(launch_amax(x.data_ptr(), dt_of(x), x.numel(), amax_out.data_ptr<float>(), stream_of(x)), "amax");
    return;
  }
  float m = amax_out.data_ptr<float>()[0];
  auto xf = x.to(at::kFloat);
  const float* p = xf.data_ptr<float>();
  for (int64_t i = 0; i < xf.numel(); ++i) m = std::max(m, std::fabs(p[i]));
  amax_out.data_ptr<float>()[0] = m;
}

void quant_fp8_(const at::Tensor& x, const at::Tensor& amax, double fp8_max, at::Tensor out, at::Tensor scale_inv) {
  const bool e5 = out.scalar_type() == at::kFloat8_e5m2;
  TORCH_CHECK((out.scalar_type() == at::kFloat8_e4m3fn || e5) && out.numel() == x.numel() && out.is_contiguous(),
              "psd: quant_fp8 out must be float8_e4m3fn or float8_e5m2 like x");
  TORCH_CHECK(x.is_contiguous(), "psd: quant_fp8 input must be contiguous");
  if (x.is_cuda()) {
    const c10::DeviceGuard g(x.device());
    if (x.numel() >= 8) {
      check_aligned(x, "x");
      TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7u) == 0, "psd: fp8 out must be 8-byte aligned");
    }
    hip_check(launch_quant_fp8(x.data_ptr(), dt_of(x), x.numel(), amax.data_ptr<float>(), (float)fp8_max,
                               reinterpret_cast<uint8_t*>(out.data_ptr()), scale_inv.data_ptr<float>(), stream_of(x),
                               e5 ? 1 : 0),
              "quant_fp8");
    return;
  }
  const float a = std::max(amax.data_ptr<float>()[0], 1e-12f);
  const float scale = (float)fp8_max / a;
  scale_inv.data_ptr<float>()[0] = a / (float)fp8_max;
  out.copy_((x.to(at::kFloat) * scale).clamp(-fp8_max, fp8_max).to(out.scalar_type()));
}

// out = fp8(x * fp8_max / amax(x)), scale_inv = amax / fp8_max: amax found on the device in the same
// call (out e4m3fn or e5m2; fp8_max follows the format)
void quant_fp8_jit_(const at::Tensor& x, at::Tensor out, at::Tensor scale_inv) {
  const bool e5 = out.scalar_type() == at::kFloat8_e5m2;
  TORCH_CHECK((out.scalar_type() == at::kFloat8_e4m3fn || e5) && out.numel() == x.numel() && out.is_contiguous(),
              "psd: quant_fp8_jit out must be float8_e4m3fn or float8_e5m2 like x");
  TORCH_CHECK(x.is_contiguous() && x.is_cuda(), "psd: quant_fp8_jit input must be a contiguous device tensor");
  TORCH_CHECK(scale_inv.scalar_type() == at::kFloat && scale_inv.numel() >= 1, "psd: scale_inv fp32[>=1]");
  const c10::DeviceGuard g(x.device());
  if (x.numel() >= 8) {
    check_aligned(x, "x");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7u) == 0, "psd: fp8 out must be 8-byte aligned");
  }
  at::Tensor part = at::empty({1024}, x.options().dtype(at::kFloat));
  hip_check(launch_quant_fp8_jit(x.data_ptr(), dt_of(x), x.numel(), part.data_ptr<float>(), e5 ? 57344.f : 448.f,
                                 reinterpret_cast<uint8_t*>(out.data_ptr()), scale_inv.data_ptr<float>(), stream_of(x),
                                 e5 ? 1 : 0),
            "quant_fp8_jit");
}

// delayed scaling: out = fp8(x * fp8_max / (hist[0] * margin)); this call's amax -> hist[0] afterwards
void quant_fp8_delayed_(const at::Tensor& x, at::Tensor out, at::Tensor scale_inv, at::Tensor hist, double margin) {
  const bool e5 = out.scalar_type() == at::kFloat8_e5m2;
  TORCH_CHECK((out.scalar_type() == at::kFloat8_e4m3fn || e5) && out.numel() == x.numel() && out.is_contiguous(),
              "psd: quant_fp8_delayed out must be float8_e4m3fn or float8_e5m2 like x");
  TORCH_CHECK(x.is_contiguous() && x.is_cuda(), "psd: quant_fp8_delayed input must be a contiguous device tensor");
  TORCH_CHECK(scale_inv.scalar_type() == at::kFloat && scale_inv.numel() >= 1 && hist.scalar_type() == at::kFloat &&
                  hist.numel() >= 2 && hist.is_cuda() && hist.is_contiguous(),
              "psd: scale_inv fp32[>=1], hist fp32[2] device tensors");
  const c10::DeviceGuard g(x.device());
  if (x.numel() >= 8) {
    check_aligned(x, "x");
    TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7u) == 0, "psd: fp8 out must be 8-byte aligned");
  }
  hip_check(launch_quant_fp8_delayed(x.data_ptr(), dt_of(x), x.numel(), hist.data_ptr<float>(), e5 ? 57344.f : 448.f,
                                     (float)margin, reinterpret_cast<uint8_t*>(out.data_ptr()),
                                     scale_inv.data_ptr<float>(), stream_of(x), e5 ? 1 : 0),
            "quant_fp8_delayed");
}

void dequant_fp8_(const at::Tensor& x, const at::Tensor& scale_inv, at::Tensor out) {
  TORCH_CHECK(x.scalar_type() == at::kFloat8_e4m3fn && out.numel() == x.numel(), "psd: dequant_fp8 shape/dtype");
  if (x.is_cuda()) {
    const c10::DeviceGuard g(x.device());
    hip_check(launch_dequant_fp8(reinterpret_cast<const uint8_t*>(x.data_ptr()), x.numel(), scale_inv.data_ptr<float>(),
                                 out.data_ptr(), dt_of(out), stream_of(x)),
              "dequant_fp8");
    return;
  }
  out.copy_(x.to(at::kFloat) * scale_inv.data_ptr<float>()[0]);
}

// MX fp8: out = fp8(x / 2^(s - 127)) with one E8M0 byte s per 32 consecutive elements (scales)
void quant_mx_(const at::Tensor& x, at::Tensor out, at::Tensor scales) {
  const bool e5 = out.scalar_type() == at::kFloat8_e5m2;
  TORCH_CHECK((out.scalar_type() == at::kFloat8_e4m3fn || e5) && out.numel() == x.numel() && out.is_contiguous(),
              "psd: quant_mx out must be float8_e4m3fn or float8_e5m2 like x");
  TORCH_CHECK(x.is_contiguous() && x.is_cuda() && x.numel() % 32 == 0,
              "psd: quant_mx input must be a contiguous device tensor of a multiple of 32 elements");
  TORCH_CHECK(scales.scalar_type() == at::kByte && scales.is_contiguous() && scales.numel() == x.numel() / 32,
              "psd: quant_mx scales must be uint8 [numel / 32]");
  const c10::DeviceGuard g(x.device());
  if (x.numel() == 0) return;
  check_aligned(x, "x");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 7u) == 0, "psd: fp8 out must be 8-byte aligned");
  hip_check(launch_quant_mx(x.data_ptr(), dt_of(x), x.numel(), e5 ? 1 : 0, reinterpret_cast<uint8_t*>(out.data_ptr()),
                            scales.data_ptr<uint8_t>(), stream_of(x)),
            "quant_mx");
}

// MX fp8 of x^T in one pass: x [R, C] bf16 -> out [C, R], scales [C, R/32] (blocks along R)
void quant_mx_t_(const at::Tensor& x, at::Tensor out, at::Tensor scales) {
  const bool e5 = out.scalar_type() == at::kFloat8_e5m2;
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() && x.scalar_type() == at::kBFloat16 &&
                  x.size(0) % 32 == 0 && x.size(1) % 8 == 0,
              "psd: quant_mx_t input must be a contiguous bf16 [R, C] device tensor with R % 32 == 0 and C % 8 == 0");
  const int64_t R = x.size(0), C = x.size(1);
  TORCH_CHECK((out.scalar_type() == at::kFloat8_e4m3fn || e5) && out.dim() == 2 && out.size(0) == C &&
                  out.size(1) == R && out.is_contiguous() && out.device() == x.device(),
              "psd: quant_mx_t out must be a contiguous float8_e4m3fn or float8_e5m2 [C, R] tensor on x's device");
  TORCH_CHECK(scales.scalar_type() == at::kByte && scales.is_contiguous() && scales.numel() == x.numel() / 32 &&
                  scales.device() == x.device(),
              "psd: quant_mx_t scales must be uint8 [C, R / 32] on x's device");
  const c10::DeviceGuard g(x.device());
  if (x.numel() == 0) return;
  check_aligned(x, "x");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(out.data_ptr()) & 15u) == 0, "psd: fp8 out must be 16-byte aligned");
  hip_check(launch_quant_mx_t(x.data_ptr(), R, C, e5 ? 1 : 0, reinterpret_cast<uint8_t*>(out.data_ptr()),
                              scales.data_ptr<uint8_t>(), stream_of(x)),
            "quant_mx_t");
}

// both MX copies of x [R, C] bf16 from one read: q_row [R, C] / s_row [R * C / 32] (blocks along C, bitwise
// quant_mx_) and q_t [C, R] / s_t [C, R / 32] (blocks along R, bitwise quant_mx_t_); each output's format
// (e4m3fn / e5m2) is its tensor's dtype
void quant_mx_dual_(const at::Tensor& x, at::Tensor q_row, at::Tensor s_row, at::Tensor q_t, at::Tensor s_t) {
  TORCH_CHECK(x.is_cuda() && x.dim() == 2 && x.is_contiguous() && x.scalar_type() == at::kBFloat16 &&
                  x.size(0) % 32 == 0 && x.size(1) % 32 == 0,
              "psd: quant_mx_dual input must be a contiguous bf16 [R, C] device tensor with R % 32 == 0 and C % 32 == 0");
  const int64_t R = x.size(0), C = x.size(1);
  auto f8 = [](const at::Tensor& t) {
    return t.scalar_type() == at::kFloat8_e4m3fn || t.scalar_type() == at::kFloat8_e5m2;
  };
  TORCH_CHECK(f8(q_row) && q_row.dim() == 2 && q_row.size(0) == R && q_row.size(1) == C && q_row.is_contiguous() &&
                  q_row.device() == x.device(),
              "psd: quant_mx_dual q_row must be a contiguous float8_e4m3fn or float8_e5m2 [R, C] tensor on x's device");
  TORCH_CHECK(f8(q_t) && q_t.dim() == 2 && q_t.size(0) == C && q_t.size(1) == R && q_t.is_contiguous() &&
                  q_t.device() == x.device(),
              "psd: quant_mx_dual q_t must be a contiguous float8_e4m3fn or float8_e5m2 [C, R] tensor on x's device");
  for (const at::Tensor* s : {&s_row, &s_t})
    TORCH_CHECK(s->scalar_type() == at::kByte && s->is_contiguous() && s->numel() == x.numel() / 32 &&
                    s->device() == x.device(),
                "psd: quant_mx_dual scales must be uint8 [R * C / 32] and [C, R / 32] on x's device");
  const c10::DeviceGuard g(x.device());
  if (x.numel() == 0) return;
  check_aligned(x, "x");
  TORCH_CHECK((reinterpret_cast<uintptr_t>(q_row.data_ptr()) & 15u) == 0 &&
                  (reinterpret_cast<uintptr_t>(q_t.data_ptr()) & 15u) == 0,
              "psd: fp8 out must be 16-byte aligned");
  hip_check(launch_quant_mx_dual(x.data_ptr(), R, C, q_row.scalar_type() == at::kFloat8_e5m2 ? 1 : 0,
                                 q_t.scalar_type() == at::kFloat8_e5m2 ? 1 : 0,
                                 reinterpret_cast<uint8_t*>(q_row.data_ptr()), s_row.data_ptr<uint8_t>(),
                                 reinterpret_cast<uint8_t*>(q_t.data_ptr()), s_t.data_ptr<uint8_t>(), stream_of(x)),
            "quant_mx_dual");
}

void dequant_mx_(const at::Tensor& q, const at::Tensor& scales, at::Tensor out) {
  TORCH_CHECK(q.scalar_type() == at::kFloat8_e4m3fn && q.is_contiguous() && q.is_cuda() && out.numel() == q.numel() &&
                  out.is_contiguous() && q.numel() % 32 == 0,
              "psd: dequant_mx q must be a contiguous e4m3fn device tensor (numel % 32 == 0), out like q");
  TORCH_CHECK(scales.scalar_type() == at::kByte && scales.is_contiguous() && scales.numel() == q.numel() / 32,
              "psd: dequant_mx scales must be uint8 [numel / 32]");
  const c10::DeviceGuard g(q.device());
  if (q.numel() == 0) return;
  TORCH_CHECK((reinterpret_cast<uintptr_t>(q.data_ptr()) & 7u) == 0, "psd: fp8 q must be 8-byte aligned");
  check_aligned(out, "out");
  hip_check(launch_dequant_mx(reinterpret_cast<const uint8_t*>(q.data_ptr()), scales.data_ptr<uint8_t>(), q.numel(),
                              out.data_ptr(), dt_of(out), stream_of(q)),
            "dequant_mx");
}

}  // namespace psd
