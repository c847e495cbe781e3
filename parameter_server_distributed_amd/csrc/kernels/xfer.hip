// Peer-memory scatter / gather of the asynchronous PS data plane (csrc/async_ps.cpp).
//
// A push of one gradient bucket touches every shard whose range it overlaps, and a pull touches
// every shard: one contiguous slice per owner GPU. Issued as a sequence of hipMemcpyAsync calls on
// one stream those slices cross the node one after another, so a worker drives ONE of its 7 xGMI
// links at a time (csrc/async_ps.cpp push / pull). Here every slice of a push or a pull
// is a segment of one launch, with its own group of workgroups: all owners' links carry data at
// once, on the stream the copies already used (no extra HIP stream: the process's 4 hardware queues
// are taken by compute, the engine's apply, push and pull).
//
// Layout: workgroup b serves segment b % count (so consecutive workgroups -- dispatched together --
// spread over the peers) and is the (b / count)-th of blocks_per_seg on it, grid-striding over the
// segment in 16-byte vectors, U vectors in flight per lane (loads first, then stores). Stores into a
// peer's uncached inbox / loads from its uncached publish buffer are non-temporal. Vector memory
// instructions only.
//
// The MX pull (xfer_mx_kernel) also dequantises: 16 e4m3 bytes per lane (half a 32-element block),
// the block's E8M0 byte, written to the worker's q / scale copies (the fp8 convolutions read them)
// and, dequantised, to its bf16 working weights -- the separate dequant_mx pass over the pulled
// copy is gone.
//
// The quantising push (xfer_quant_kernel) is the same scatter with the MX quantisation of the
// gradient fused in: 1 + 1/32 bytes per element cross to the owner's inbox instead of 2 (bf16). With
// error feedback the worker's fp32 residual is added before and rewritten after, in the same pass.
#include "common.h"
#include "launchers.h"
#include "launchers_xfer.h"
#include "mx_common.h"

namespace psd {

namespace {

template <bool NT>
__device__ __forceinline__ u32x4 ld16(const u32x4* p) {
  if constexpr (NT) return __builtin_nontemporal_load(p);
  else return *p;
}
template <bool NT>
__device__ __forceinline__ void st16(u32x4* p, u32x4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, p);
  else *p = v;
}

}  // namespace

template <int U, bool NTL, bool NTS>
__global__ __launch_bounds__(256) void xfer_kernel(XferList L) {
  const int s = (int)(blockIdx.x % (unsigned)L.count);
  const int j = (int)(blockIdx.x / (unsigned)L.count);
  const XferSeg g = L.seg[s];
  const int64_t n16 = g.bytes >> 4;
  const u32x4* __restrict__ src = static_cast<const u32x4*>(g.src);
  u32x4* __restrict__ dst = static_cast<u32x4*>(g.dst);
  const int64_t stride = (int64_t)L.blocks_per_seg * 256 * U;
  for (int64_t base = (int64_t)j * 256 * U + threadIdx.x; base < n16; base += stride) {
    u32x4 v[U];
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * 256 < n16) v[u] = ld16<NTL>(src + base + u * 256);
#pragma unroll
    for (int u = 0; u < U; ++u)
      if (base + u * 256 < n16) st16<NTS>(dst + base + u * 256, v[u]);
  }
  const int tail = (int)(g.bytes & 15);
  if (j == 0 && (int)threadIdx.x < tail) {
    const int64_t o = n16 * 16 + threadIdx.x;
    static_cast<uint8_t*>(g.dst)[o] = static_cast<const uint8_t*>(g.src)[o];
  }
  if constexpr (NTS) {
    // Stores into a peer's memory (push): a system-scope release per wave before the kernel ends,
    // so the commit event recorded behind this launch (async_ps.cpp defer -> post) can never be
    // observed by the owner ahead of the bytes, whatever scope the runtime gives the end-of-kernel
    // release (hipMemcpyAsync gave this ordering before). The counted wait is inline
    // asm so the compiler cannot drop it after the release (MI355X_MICROARCH.md, compiler hazard).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
}

template <int U>
__global__ __launch_bounds__(256) void xfer_mx_kernel(XferMxList L) {
  const int s = (int)(blockIdx.x % (unsigned)L.count);
  const int j = (int)(blockIdx.x / (unsigned)L.count);
  const XferMxSeg g = L.seg[s];
  const int64_t n16 = g.n >> 4;  // 16-element items (two per 32-element block)
  const int64_t stride = (int64_t)L.blocks_per_seg * 256 * U;
  for (int64_t base = (int64_t)j * 256 * U + threadIdx.x; base < n16; base += stride) {
    u32x4 q[U];
    uint8_t sc[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * 256;
      if (i < n16) {
        q[u] = ld16<true>(reinterpret_cast<const u32x4*>(g.q_src) + i);
        sc[u] = __builtin_nontemporal_load(g.sc_src + (i >> 1));
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = base + u * 256;
      if (i >= n16) continue;
      *(reinterpret_cast<u32x4*>(g.q_dst) + i) = q[u];
      if ((i & 1) == 0) g.sc_dst[i >> 1] = sc[u];
      const float scale = __uint_as_float((uint32_t)sc[u] << 23);  // 2^(eb - 127), as dequant_mx
      const uint32_t w[4] = {q[u].x, q[u].y, q[u].z, q[u].w};
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        float t[8];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          t[e] = e4m3_to_f32((uint8_t)(w[2 * h] >> (8 * e))) * scale;
          t[e + 4] = e4m3_to_f32((uint8_t)(w[2 * h + 1] >> (8 * e))) * scale;
        }
        store8_bf16(g.bf16_dst + i * 16 + h * 8, t);
      }
    }
  }
}

namespace {

// 16 consecutive elements (half a 32-element block) of a bf16 / fp32 source: 16-byte vector loads
template <int SRC_DT>
__device__ __forceinline__ void load16_src(const void* __restrict__ src, int64_t i, float (&t)[16]) {
  if constexpr (SRC_DT == DT_BF16) {
    load8_bf16(static_cast<const uint16_t*>(src) + i * 16, t);
    load8_bf16(static_cast<const uint16_t*>(src) + i * 16 + 8, t + 8);
  } else {
    load8_f32(static_cast<const float*>(src) + i * 16, t);
    load8_f32(static_cast<const float*>(src) + i * 16 + 8, t + 8);
  }
}

// |x| as its bit pattern: for finite values the unsigned order of these is the order of |x|, and
// anything above kMaxFiniteBits is an inf or a NaN -- one integer max finds a lane's amax AND whether
// it holds a non-finite element (fmaxf would drop a NaN)
constexpr uint32_t kMaxFiniteBits = 0x7f7fffffu;
__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }

// 4 e4m3 bytes of (a, b, c, d) * inv, a in the low byte: the clamp and the two packed hardware
// conversions f32_to_e4m3 does one value at a time (round to nearest even, saturating at 448)
__device__ __forceinline__ uint32_t q8x4(float a, float b, float c, float d, float inv) {
  a = __builtin_amdgcn_fmed3f(a * inv, 448.f, -448.f);
  b = __builtin_amdgcn_fmed3f(b * inv, 448.f, -448.f);
  c = __builtin_amdgcn_fmed3f(c * inv, 448.f, -448.f);
  d = __builtin_amdgcn_fmed3f(d * inv, 448.f, -448.f);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
  return (uint32_t)w;
}

}  // namespace

// Quantising push: the gradient slices of one bucket for every owner it overlaps, bf16 / fp32 in,
// MX e4m3 out (payload + one E8M0 byte per 32 elements), mapping as xfer_kernel. A lane takes 16
// consecutive elements -- two (bf16) or four (fp32) 16-byte loads, ONE 16-byte non-temporal payload
// store -- so a block is a lane pair: the pair agrees on amax with one quad-permute DPP, and the scale
// bytes of 4 consecutive blocks are collected on every 8th lane (two lane exchanges), which stores
// them as one dword (2-byte or byte stores only where the destination is not 4-byte aligned or the
// segment ends inside the group). Scale and rounding: mx_exp_byte and the conversion of f32_to_e4m3
// (four values per pair of packed instructions), as quant_mx_kernel.
// The loop bounds are workgroup-uniform (a lane past the end idles through the exchanges), so the
// bytes written do not depend on blocks_per_seg. Vector memory instructions only.
// BLOCK: lanes per workgroup. A workgroup is the unit of the push's CU budget (blocks_per_seg), and a
// small grid of 256-lane workgroups leaves one wave per SIMD, where the conversion arithmetic and the
// memory latency of a pass add up instead of overlapping (the plain copy has no arithmetic to hide):
// below kQuantWideBelow workgroups the launch takes 1024 lanes (four waves per SIMD; ResNet-50-size
// gradient at 48 workgroups 93 -> 55 us, profiles/push_fp8.md). A grid that fills the GPU anyway keeps
// 256 lanes with four items in flight per lane (1024-lane workgroups measured 2.6x slower there).
constexpr int kQuantWideBelow = 128;
// EF (error feedback, XferQSeg::resid): the lane adds its 16 fp32 residuals to the gradient before
// anything else looks at it -- four more 16-byte loads, issued with the gradient loads -- quantises the
// sum v as above, then dequantises its own 16 bytes (packed hardware conversion, times the block's
// power of two: exact), and writes v - dq back over the residual with four 16-byte stores. The
// compiler may contract that multiply and subtract into one fma; the product is exact, so the bits
// are the same either way. The residual of a NaN / +-inf element is 0: the NaN has been delivered
// and must not come back with every later push. The residual accesses are plain, not non-temporal:
// non-temporal residual LOADS cost 1.5x - 1.8x the whole kernel's time (ResNet-50-size bf16 gradient,
// 48 workgroups: 259 us against 164 us), non-temporal stores changed nothing. One item in flight per
// lane at 1024 lanes; at 256 lanes one (bf16) or two (fp32) -- 71 / 107 VGPRs; four items (179 VGPRs,
// two waves per SIMD) and 1024-lane workgroups on a full grid were slower (profiles/push_fp8_ef.md).
template <int SRC_DT, int U, int BLOCK, bool EF = false>
__global__ __launch_bounds__(BLOCK) void xfer_quant_kernel(XferQList L) {
  const int s = (int)(blockIdx.x % (unsigned)L.count);
  const int j = (int)(blockIdx.x / (unsigned)L.count);
  const XferQSeg g = L.seg[s];
  const int64_t n16 = g.n >> 4;  // 16-element items, two per block
  const int64_t stride = (int64_t)L.blocks_per_seg * BLOCK * U;
  for (int64_t b0 = (int64_t)j * BLOCK * U; b0 < n16; b0 += stride) {
    float t[U][16];
    [[maybe_unused]] u32x4 r[EF ? U : 1][4];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = b0 + u * BLOCK + threadIdx.x;
      if (i < n16) {
        load16_src<SRC_DT>(g.src, i, t[u]);
        if constexpr (EF) {
#pragma unroll
          for (int k = 0; k < 4; ++k) r[u][k] = ld16<false>(reinterpret_cast<const u32x4*>(g.resid) + i * 4 + k);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t i = b0 + u * BLOCK + threadIdx.x;
      const bool act = i < n16;  // n16 is even: the two lanes of a block are active together
      if constexpr (EF) {
        if (act) {
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            t[u][4 * k] += __uint_as_float(r[u][k].x);
            t[u][4 * k + 1] += __uint_as_float(r[u][k].y);
            t[u][4 * k + 2] += __uint_as_float(r[u][k].z);
            t[u][4 * k + 3] += __uint_as_float(r[u][k].w);
          }
        }
      }
      uint32_t mb = 0;  // this lane's amax, as bits
      if (act) {
#pragma unroll
        for (int e = 0; e < 16; ++e) mb = max(mb, abs_bits(t[u][e]));
      }
      const bool finite = mb <= kMaxFiniteBits;
      // a NaN or an inf anywhere in the block: unit scale for the block (mx_exp_byte)
      float m = __uint_as_float(finite ? mb : 0x7f800000u);
      m = fmaxf(m, mx_dpp<0xB1>(m));  // quad_perm [1,0,3,2]: the block's two lanes agree
      const int eb = mx_exp_byte(m, 448.f);
      if (act) {
        const float inv = __uint_as_float((uint32_t)(254 - eb) << 23);  // 2^(127 - eb)
        uint32_t w[4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
          w[k] = q8x4(t[u][4 * k], t[u][4 * k + 1], t[u][4 * k + 2], t[u][4 * k + 3], inv);
        if (!finite) {
          // a NaN or +-inf element travels as the e4m3 NaN byte 0x7F (e4m3fn has no inf, and the
          // saturating conversion would turn an inf into 448): a diverged gradient must stay visible
#pragma unroll
          for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e)
              if (abs_bits(t[u][4 * k + e]) > kMaxFiniteBits) w[k] = (w[k] & ~(0xFFu << (8 * e))) | (0x7Fu << (8 * e));
        }
        st16<true>(reinterpret_cast<u32x4*>(g.q_dst) + i, u32x4{w[0], w[1], w[2], w[3]});
        if constexpr (EF) {
          const float sc = __uint_as_float(eb ? (uint32_t)eb << 23 : 0x00400000u);  // 2^(eb - 127)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], false);
            const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[k], true);
            const float d[4] = {lo[0], lo[1], hi[0], hi[1]};
            float nr[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float v = t[u][4 * k + e];
              nr[e] = v - d[e] * sc;
              if (!finite && abs_bits(v) > kMaxFiniteBits) nr[e] = 0.f;
            }
            st16<false>(reinterpret_cast<u32x4*>(g.resid) + i * 4 + k,
                        u32x4{__float_as_uint(nr[0]), __float_as_uint(nr[1]), __float_as_uint(nr[2]),
                              __float_as_uint(nr[3])});
          }
        }
      }
      // scale bytes: lane 4p gets blocks (2p, 2p + 1) of the wave, then lane 8r blocks 4r .. 4r + 3
      uint32_t sw = (uint32_t)eb | ((uint32_t)__shfl_xor(eb, 2) << 8);
      sw |= (uint32_t)__shfl_down((int)sw, 4) << 16;
      if (act && (threadIdx.x & 7) == 0) {
        const int64_t blk = i >> 1, left = (n16 - i) >> 1;
        const int nb = left < 4 ? (int)left : 4;
        uint8_t* p = g.sc_dst + blk;
        const uintptr_t a = reinterpret_cast<uintptr_t>(p);
        if (nb == 4 && (a & 3) == 0) {
          __builtin_nontemporal_store(sw, reinterpret_cast<uint32_t*>(p));
        } else if ((a & 1) == 0 && (nb & 1) == 0) {
          for (int h = 0; h < nb; h += 2)
            __builtin_nontemporal_store((uint16_t)(sw >> (8 * h)), reinterpret_cast<uint16_t*>(p + h));
        } else {
          for (int h = 0; h < nb; ++h) __builtin_nontemporal_store((uint8_t)(sw >> (8 * h)), p + h);
        }
      }
    }
  }
  // as xfer_kernel<.., NTS = true>: system-scope release per wave and a counted wait the compiler
  // cannot drop, so the commit event behind this launch is never observed ahead of the bytes
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "");
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

hipError_t launch_xfer_quant(const XferQList& L, hipStream_t st) {
  if (L.count <= 0) return hipSuccess;
  if (L.count > kMaxXferSeg || L.blocks_per_seg < 1) return hipErrorInvalidValue;
  for (int i = 0; i < L.count; ++i) {
    const XferQSeg& g = L.seg[i];
    if (g.n < 0 || g.n % 32 != 0 || !g.sc_dst ||
        ((reinterpret_cast<uintptr_t>(g.src) | reinterpret_cast<uintptr_t>(g.q_dst) |
          reinterpret_cast<uintptr_t>(g.resid)) & 15) ||
        (g.resid != nullptr) != (L.seg[0].resid != nullptr))  // all segments carry a residual or none
      return hipErrorInvalidValue;
  }
  const dim3 grid((unsigned)(L.count * L.blocks_per_seg));
  const bool wide = L.count * L.blocks_per_seg < kQuantWideBelow;
  if (L.src_dtype != DT_BF16 && L.src_dtype != DT_F32) return hipErrorInvalidValue;
#define PSD_XQ(DT, U, B, ...) \
  hipLaunchKernelGGL((xfer_quant_kernel<DT, U, B, ##__VA_ARGS__>), grid, dim3(B), 0, st, L)
  if (L.seg[0].resid) {
    if (L.src_dtype == DT_BF16) {
      if (wide) PSD_XQ(DT_BF16, 1, 1024, true);
      else PSD_XQ(DT_BF16, 1, 256, true);
    } else {
      if (wide) PSD_XQ(DT_F32, 1, 1024, true);
      else PSD_XQ(DT_F32, 2, 256, true);
    }
  } else if (L.src_dtype == DT_BF16) {
    if (wide) PSD_XQ(DT_BF16, 2, 1024);
    else PSD_XQ(DT_BF16, 4, 256);
  } else {
    if (wide) PSD_XQ(DT_F32, 2, 1024);
    else PSD_XQ(DT_F32, 2, 256);
  }
#undef PSD_XQ
  return hipGetLastError();
}

hipError_t launch_xfer(const XferList& L, hipStream_t st) {
  if (L.count <= 0) return hipSuccess;
  if (L.count > kMaxXferSeg || L.blocks_per_seg < 1) return hipErrorInvalidValue;
  for (int i = 0; i < L.count; ++i)
    if ((reinterpret_cast<uintptr_t>(L.seg[i].src) | reinterpret_cast<uintptr_t>(L.seg[i].dst)) & 15)
      return hipErrorInvalidValue;
  const dim3 grid((unsigned)(L.count * L.blocks_per_seg));
  if (L.nt_load && L.nt_store) hipLaunchKernelGGL((xfer_kernel<4, true, true>), grid, dim3(256), 0, st, L);
  else if (L.nt_load) hipLaunchKernelGGL((xfer_kernel<4, true, false>), grid, dim3(256), 0, st, L);
  else if (L.nt_store) hipLaunchKernelGGL((xfer_kernel<4, false, true>), grid, dim3(256), 0, st, L);
  else hipLaunchKernelGGL((xfer_kernel<4, false, false>), grid, dim3(256), 0, st, L);
  return hipGetLastError();
}

hipError_t launch_xfer_mx(const XferMxList& L, hipStream_t st) {
  if (L.count <= 0) return hipSuccess;
  if (L.count > kMaxXferMxSeg || L.blocks_per_seg < 1) return hipErrorInvalidValue;
  for (int i = 0; i < L.count; ++i) {
    const XferMxSeg& g = L.seg[i];
    if (g.n % 32 != 0 ||
        ((reinterpret_cast<uintptr_t>(g.q_src) | reinterpret_cast<uintptr_t>(g.q_dst) |
          reinterpret_cast<uintptr_t>(g.bf16_dst)) & 15))
      return hipErrorInvalidValue;
  }
  hipLaunchKernelGGL((xfer_mx_kernel<2>), dim3((unsigned)(L.count * L.blocks_per_seg)), dim3(256), 0, st, L);
  return hipGetLastError();
}

}  // namespace psd
