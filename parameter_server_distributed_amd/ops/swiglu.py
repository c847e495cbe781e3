"""Gated SiLU activation (SwiGLU) on the packed gate/up tensor (``csrc/kernels/swiglu.hip``).

``gu [..., 2F]`` is the output of one Linear whose weight is a Llama checkpoint's ``gate_proj`` and
``up_proj`` concatenated along the output dimension: the gate ``g`` is columns ``[0, F)``, the up half ``u``
columns ``[F, 2F)``. ``a = silu(g) * u`` with ``silu(g) = g * sigmoid(g)``, fp32 math, one rounding. The
backward recomputes the sigmoid from ``gu``, which is all it saves:
``dg = da * u * sig * (1 + g * (1 - sig))``, ``du = da * g * sig``.

MX hand-overs of the fp8 Llama block (feature ``fp8_llama_handover``, ``ops/linear.py`` ``fp8="mx"``; the
``SwiGLU`` module, ``F % 32 == 0``): the forward also writes the MX e4m3 copy of ``a`` for the Linear declared
with ``psd_mx_output_to`` (the down Linear's forward operand) and the backward the MX e5m2 copy of ``dgu`` for
the Linear declared with ``psd_mx_grad_to`` (the gate/up Linear's bwd-data operand): side outputs of the same
launches, bitwise ``quantize_mx`` of the bf16 tensors they store.

A contiguous, 16-byte-aligned bf16 device tensor with ``F % 8 == 0`` takes the kernels when feature
``swiglu`` is on (the default); everything else takes ``swiglu_ref`` through ordinary autograd.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import native
from ..utils.config import feature as _feat
from .handover import leave_dq8, leave_q8, mx_grad_gate, mx_grad_token, mx_pair


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
    def forward(ctx, gu, mod):
        ctx.save_for_backward(gu)
        ctx.mod, ctx.gtok = mod, None
        f = gu.shape[-1] // 2
        q8 = sc8 = None
        if mod is not None and f % 32 == 0 and _feat("fp8_llama_handover"):
            # MX hand-over (psd_mx_output_to): also the MX e4m3 copy of a for the fp8 Linear that reads it
            cons = mod._psd_mx_to
            if cons is not None and cons.psd_mx_input_ok(f):
                q8, sc8 = mx_pair((*gu.shape[:-1], f), gu.device)
            # backward hand-over (psd_mx_grad_to): the forward token of the fp8 Linear that produced exactly this gu
            ctx.gtok = mx_grad_token(mod._psd_mxg_to, gu)
        a = native().swiglu_fwd(gu, 0, q8, sc8)
        if q8 is not None:
            leave_q8(cons, a, q8, sc8)
        return a

    @staticmethod
    def backward(ctx, da):
        (gu,) = ctx.saved_tensors
        # the e5m2 copy of dgu for the bwd-data GEMM of the gate/up Linear (it ran MX)
        dq8, dsc8 = mx_pair(gu.shape, gu.device, e5m2=True) if mx_grad_gate(ctx.gtok) else (None, None)
        dgu = native().swiglu_bwd(da.contiguous(), gu, 0, dq8, dsc8)
        if dq8 is not None:
            leave_dq8(ctx.mod._psd_mxg_to, ctx.gtok, dgu, dq8, dsc8)
        return dgu, None


def swiglu(gu, mod=None):
    """``silu(gu[..., :F]) * gu[..., F:]``: the kernels where they apply, else ``swiglu_ref``. ``mod``: the
    ``SwiGLU`` module whose declared MX hand-overs the kernels serve."""
    if _feat("swiglu") and _kernel_ok(gu):
        return _SwigluFn.apply(gu, mod)
    return swiglu_ref(gu)


class SwiGLU(nn.Module):
    """``forward(gu [..., 2F]) -> [..., F]``, the gated SiLU between the FFN's gate/up and down Linears."""

    def __init__(self):
        super().__init__()
        self._psd_mx_to = None  # psd_mx_output_to: the fp8 MfmaLinear that reads the output a
        self._psd_mxg_to = None  # psd_mx_grad_to: the fp8 MfmaLinear that produced gu

    def psd_mx_output_to(self, lin) -> None:
        """Declare that ``lin`` (an ``MfmaLinear``) reads this activation's output: when it runs the MX fp8 recipe
        and ``F % 32 == 0``, the forward kernel also writes its MX e4m3 input operand and leaves it on ``lin`` as an
        ``ops.handover.Q8Pending`` (feature ``fp8_llama_handover``). (Kept out of the module tree.)"""
        object.__setattr__(self, "_psd_mx_to", lin)

    def psd_mx_grad_to(self, lin) -> None:
        """Declare that ``lin`` (an ``MfmaLinear``) produces ``gu``, so that ``lin``'s output gradient is this
        activation's ``dgu``: when that forward of ``lin`` ran the MX fp8 recipe and ``fp8_dgrad`` is on, the backward
        kernel also writes the MX e5m2 copy of ``dgu`` and leaves it on ``lin`` (``ops.handover.leave_dq8``, with
        ``lin``'s forward token) for its bwd-data GEMM."""
        object.__setattr__(self, "_psd_mxg_to", lin)

    def forward(self, gu):
        return swiglu(gu, self)
