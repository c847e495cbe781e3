"""Gated SiLU activation (SwiGLU) on the packed gate/up tensor (``csrc/kernels/swiglu.hip``).

``gu [..., 2F]`` is the output of one Linear whose weight is a Llama checkpoint's ``gate_proj`` and
``up_proj`` concatenated along the output dimension: the gate ``g`` is columns ``[0, F)``, the up half ``u``
columns ``[F, 2F)``. ``a = silu(g) * u`` with ``silu(g) = g * sigmoid(g)``, fp32 math, one rounding. The
backward recomputes the sigmoid from ``gu``, which is all it saves:
``dg = da * u * sig * (1 + g * (1 - sig))``, ``du = da * g * sig``.

A contiguous, 16-byte-aligned bf16 device tensor with ``F % 8 == 0`` takes the kernels when feature
``swiglu`` is on (the default); everything else takes ``swiglu_ref`` through ordinary autograd.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import native
from ..utils.config import feature as _feat


def swiglu_ref(gu):
    """The torch composite, on any device and dtype: fp32 math (fp64 for an fp64 ``gu``), one rounding.
    The CPU path of ``SwiGLU`` and the yardstick of the tests."""
    if gu.shape[-1] % 2:
        raise ValueError(f"swiglu_ref: gu must be [..., 2F] (gate | up), got {tuple(gu.shape)}")
    f = gu.shape[-1] // 2
    mt = torch.float64 if gu.dtype == torch.float64 else torch.float32
    g, u = gu[..., :f].to(mt), gu[..., f:].to(mt)
    return (F.silu(g) * u).to(gu.dtype)


def _kernel_ok(gu) -> bool:
    return (gu.is_cuda and gu.dtype == torch.bfloat16 and gu.dim() >= 1 and gu.shape[-1] % 16 == 0
            and gu.is_contiguous() and gu.data_ptr() % 16 == 0)


class _SwigluFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, gu):
        ctx.save_for_backward(gu)
        return native().swiglu_fwd(gu, 0)

    @staticmethod
    def backward(ctx, da):
        (gu,) = ctx.saved_tensors
        return native().swiglu_bwd(da.contiguous(), gu, 0)


def swiglu(gu):
    """``silu(gu[..., :F]) * gu[..., F:]``: the kernels where they apply, else ``swiglu_ref``."""
    if _feat("swiglu") and _kernel_ok(gu):
        return _SwigluFn.apply(gu)
    return swiglu_ref(gu)


class SwiGLU(nn.Module):
    """``forward(gu [..., 2F]) -> [..., F]``, the gated SiLU between the FFN's gate/up and down Linears."""

    def forward(self, gu):
        return swiglu(gu)
