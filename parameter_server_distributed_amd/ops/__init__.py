"""Python entry points for the hand-written gfx950 kernels.

Every function routes device tensors to the HIP kernels in ``csrc/kernels`` (on the caller's
current HIP stream) and host tensors to the bit-compatible C++ loops in ``csrc/ops.cpp``. There
is no silent eager-PyTorch fallback: if ``_C`` is missing these raise.
"""
from __future__ import annotations

import torch

from .. import native
from .optim import (LayerTable, OptimConfig, OptimDyn, advance_, apply_no_advance_, fused_apply_,  # noqa: F401
                    grad_clip_coef_, multi_reduce_, push_quant_mx_)

FP8_E4M3_MAX = 448.0
FP8_E5M2_MAX = 57344.0


def multi_reduce_(out: torch.Tensor, srcs, scale: float = 1.0) -> torch.Tensor:
    """``out = scale * sum(srcs)`` (fp32/bf16, up to 16 sources)."""
    native().multi_reduce_(out, list(srcs), float(scale))
    return out


def pack_cast_(srcs, dsts) -> None:
    """Copy+cast many tensors in one launch (fp32<->bf16)."""
    native().pack_cast_(list(srcs), list(dsts))


def quantize_fp8(x: torch.Tensor, amax: torch.Tensor | None = None, e5m2: bool = False):
    """Per-tensor OCP fp8 quantisation (e4m3fn, or e5m2 for gradients); returns ``(q, scale_inv)``
    with ``x ~= q * scale_inv``."""
    C = native()
    x = x.contiguous()
    q = torch.empty(x.shape, dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn, device=x.device)
    sinv = torch.empty(1, dtype=torch.float32, device=x.device)
    if amax is None and x.is_cuda:  # amax + quantise in two launches, no atomics / zero-fill
        C.quant_fp8_jit_(x, q, sinv)
        return q, sinv
    if amax is None:
        amax = torch.zeros(1, dtype=torch.float32, device=x.device)
        C.amax_(x, amax)
    C.quant_fp8_(x, amax, FP8_E5M2_MAX if e5m2 else FP8_E4M3_MAX, q, sinv)
    return q, sinv


def dequantize_fp8(q: torch.Tensor, scale_inv: torch.Tensor, dtype=torch.bfloat16) -> torch.Tensor:
    out = torch.empty(q.shape, dtype=dtype, device=q.device)
    native().dequant_fp8_(q.contiguous(), scale_inv, out)
    return out


def quantize_mx(x: torch.Tensor, e5m2: bool = False):
    """MX (OCP microscaling) fp8: ``(q, scales)`` with one E8M0 byte per 32 consecutive elements of
    the contiguous ``x`` (numel % 32 == 0), ``x ~= q * 2^(scale - 127)`` blockwise -- the operand
    format of the block-scaled MFMA (``gemm_fp8_`` / ``conv_fwd_fp8_`` with uint8 scales). Device
    tensors run kernels/fp8.hip quant_mx_kernel; host tensors the reference below (same rounding)."""
    x = x.contiguous()
    if not x.is_cuda:
        return quantize_mx_ref(x, e5m2)
    q = torch.empty(x.shape, dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn, device=x.device)
    s = torch.empty(x.numel() // 32, dtype=torch.uint8, device=x.device)
    native().quant_mx_(x, q, s)
    return q, s


def quantize_mx_t(x: torch.Tensor, e5m2: bool = False):
    """MX fp8 of ``x^T`` from the contiguous bf16 ``x [R, C]`` (R % 32 == 0, C % 8 == 0) in one launch and
    one read of ``x``: ``(q [C, R], scales [C, R/32])`` with blocks of 32 along R -- bitwise
    ``quantize_mx(x.t().contiguous(), e5m2)`` without the bf16 transpose copy (kernels/fp8_t.hip). The
    bwd-data GEMM of an fp8 Linear takes ``W^T [in, out]`` from the working weight ``W [out, in]`` this
    way. Host tensors take the reference on the transposed copy."""
    if x.dim() != 2 or x.shape[0] % 32 or x.shape[1] % 8:
        raise ValueError(f"quantize_mx_t: x must be [R, C] with R % 32 == 0 and C % 8 == 0, got {tuple(x.shape)}")
    if not x.is_cuda:
        q, s = quantize_mx_ref(x.t().contiguous(), e5m2)
        return q, s.view(x.shape[1], x.shape[0] // 32)
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_mx_t: device tensors must be bf16, got {x.dtype}")
    x = x.contiguous()
    R, C = x.shape
    q = torch.empty(C, R, dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn, device=x.device)
    s = torch.empty(C, R // 32, dtype=torch.uint8, device=x.device)
    native().quant_mx_t_(x, q, s)
    return q, s


def quantize_mx_dual(x: torch.Tensor, e5m2_row: bool = False, e5m2_t: bool = False):
    """Both MX fp8 copies of the contiguous bf16 ``x [R, C]`` (R % 32 == 0, C % 32 == 0) from one launch and
    one read of ``x``: ``(q_row [R, C], s_row [R * C / 32], q_t [C, R], s_t [C, R/32])`` -- the first pair
    bitwise ``quantize_mx(x, e5m2_row)`` (blocks along C), the second bitwise ``quantize_mx_t(x, e5m2_t)``
    (blocks along R) (kernels/fp8_t.hip quant_mx_dual_kernel). An fp8 Linear's backward takes dy' this way:
    the e5m2 row copy for the bwd-data GEMM, the e4m3 transposed copy for the weight gradient. Host tensors
    take the reference twice."""
    if x.dim() != 2 or x.shape[0] % 32 or x.shape[1] % 32:
        raise ValueError(f"quantize_mx_dual: x must be [R, C] with R % 32 == 0 and C % 32 == 0, got {tuple(x.shape)}")
    R, C = x.shape
    if not x.is_cuda:
        qr, sr = quantize_mx_ref(x.contiguous(), e5m2_row)
        qt, st = quantize_mx_ref(x.t().contiguous(), e5m2_t)
        return qr, sr, qt, st.view(C, R // 32)
    if x.dtype != torch.bfloat16:
        raise ValueError(f"quantize_mx_dual: device tensors must be bf16, got {x.dtype}")
    x = x.contiguous()
    f8 = lambda e5: torch.float8_e5m2 if e5 else torch.float8_e4m3fn  # noqa: E731
    qr = torch.empty(R, C, dtype=f8(e5m2_row), device=x.device)
    sr = torch.empty(R * C // 32, dtype=torch.uint8, device=x.device)
    qt = torch.empty(C, R, dtype=f8(e5m2_t), device=x.device)
    st = torch.empty(C, R // 32, dtype=torch.uint8, device=x.device)
    native().quant_mx_dual_(x, qr, sr, qt, st)
    return qr, sr, qt, st


def quantize_mx_ref(x: torch.Tensor, e5m2: bool = False):
    """PyTorch reference of quant_mx_kernel: per 32-block the smallest power of two 2^e with
    amax * 2^-e <= fp8 max (E8M0 byte e + 127; 127 for an all-zero block), round-to-nearest-even."""
    fmax = FP8_E5M2_MAX if e5m2 else FP8_E4M3_MAX
    xf = x.float().reshape(-1, 32)
    amax = xf.abs().amax(1)
    m, p = torch.frexp(amax / fmax)
    e = torch.where(m == 0.5, p - 1, p).clamp(-127, 127)
    e = torch.where((amax > 0) & torch.isfinite(amax), e, torch.zeros_like(e))
    q = (xf * torch.exp2(-e.float()).unsqueeze(1)).clamp(-fmax, fmax)
    q = q.to(torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn).reshape(x.shape)
    return q, (e + 127).to(torch.uint8)


def push_quant_mx_ef_ref(g: torch.Tensor, r: torch.Tensor):
    """PyTorch reference of the fp8 gradient push with error feedback (``push_quant_mx_`` with a
    residual): ``v = fp32(g) + r``; ``(q, scales)`` = MX e4m3 of ``v`` as ``quantize_mx_ref``, except
    that a NaN or +-inf element of ``v`` becomes the e4m3 NaN byte 0x7F (its block takes the unit
    scale 127 and its finite elements saturate at +-448); ``r_new = v - dq(q, scales)`` in fp32, 0
    where ``v`` is not finite. Returns ``(q, scales, r_new)``; ``r`` is left as it was."""
    v = g.float().reshape(-1) + r.reshape(-1)
    q, s = quantize_mx_ref(v)
    fin = torch.isfinite(v)
    q = torch.where(fin, q.view(torch.uint8), torch.full_like(q.view(torch.uint8), 0x7F)).view(torch.float8_e4m3fn)
    r_new = torch.where(fin, v - dequantize_mx_ref(q, s), torch.zeros_like(v))
    return q.reshape(g.shape), s, r_new.reshape(r.shape)


def dequantize_mx_ref(q: torch.Tensor, scales: torch.Tensor) -> torch.Tensor:
    """fp32 ``q * 2^(scale - 127)`` blockwise (reference / host path of dequant_mx_)."""
    v = q.float().reshape(-1, 32) * torch.exp2(scales.float() - 127.0).unsqueeze(1)
    return v.reshape(q.shape)
