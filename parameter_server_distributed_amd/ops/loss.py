"""Softmax cross-entropy on bf16 logits through the fused gfx950 kernels of ``csrc/kernels/xent.hip``.

Forward reads the logits once (per-row log-sum-exp kept for backward, with its fp32 rounding error); backward writes the bf16
gradient ``(softmax - onehot) * dloss / count`` in one pass -- no fp32 copy of the logits, no
log-prob tensor (the MLM decoder's logits are 4864 x 30528 per BERT-base b256 step). Mean over the
rows whose label is not negative (``ignore_index=-100`` semantics). Host tensors, other dtypes or
column counts that are not a multiple of 8 use ``F.cross_entropy`` on fp32 logits -- the reference
the tests compare against.

``linear_cross_entropy(x, weight, bias, labels)`` is the same loss of the logits ``x weight^T + bias``
without those logits in memory (``csrc/kernels/lmhead_xent.hip``): the forward takes each row's softmax
statistics from the head GEMM's fp32 accumulators (so the logits are never rounded to bf16 either) and
keeps ``[rows]`` floats; the backward recomputes the logits chunk by chunk, ``chunk_rows`` rows at a time
(default 4096), into one reused ``[chunk_rows, classes]`` bf16 gradient buffer that feeds the existing
bwd-data, split-K weight-gradient and column-sum kernels. The weight and bias gradients accumulate in
fp32 across chunks. The price is a fourth GEMM pass over the head (3 without it): see
``profiles/lmhead_xent.md`` for the measured step times. Feature ``head_xent`` off, host tensors, other
dtypes and shapes outside the kernel's contract (``in_features % 64``, ``classes % 8``) run the composite
``cross_entropy(F.linear(x, weight, bias), labels)``.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

from .. import native
from ..utils.config import feature as _feat


class _XentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, labels):
        loss_row, lse, lse_lo = native().xent_fwd(logits, labels)
        count = (labels >= 0).sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(logits, labels, lse, lse_lo, count)
        return loss_row.sum() / count

    @staticmethod
    def backward(ctx, g):
        logits, labels, lse, lse_lo, count = ctx.saved_tensors
        scale = (g.float() / count).reshape(1)
        return native().xent_bwd(logits, labels, lse, scale, lse_lo), None


def cross_entropy(logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
    """Mean softmax cross-entropy of ``logits [rows, classes]`` against int64 ``labels [rows]``."""
    if (logits.is_cuda and logits.dtype == torch.bfloat16 and logits.dim() == 2 and logits.shape[1] % 8 == 0
            and logits.stride(1) == 1 and logits.stride(0) % 8 == 0 and logits.data_ptr() % 16 == 0
            and labels.dtype == torch.int64 and labels.dim() == 1):
        return _XentFn.apply(logits, labels.contiguous())
    return F.cross_entropy(logits.float(), labels)


DEFAULT_CHUNK_ROWS = 4096


class _LinearXentFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, labels, chunk_rows, mod, slices):
        loss_row, lse = native().lmhead_xent_fwd(x, weight, bias, labels, slices)
        count = (labels >= 0).sum().clamp_min(1).to(torch.float32)
        ctx.save_for_backward(x, weight, bias, labels, lse, count)
        ctx.chunk_rows, ctx.mod = chunk_rows, mod
        return loss_row.sum() / count

    @staticmethod
    def backward(ctx, g):
        from .linear import _dgrad_route

        C = native()
        x, w, bias, labels, lse, count = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[0], ctx.needs_input_grad[1], bias is not None and ctx.needs_input_grad[2]
        scale = (g.float() / count).reshape(1)
        (M, K), V = x.shape, w.shape[0]
        rows = min(ctx.chunk_rows, M)
        chunks = (M + rows - 1) // rows
        dz = torch.empty(rows, V, dtype=x.dtype, device=x.device)  # the one logit-gradient buffer
        dx = torch.empty_like(x) if need_x else None
        sink = getattr(ctx.mod, "_psd_grad_sink", None)

        def dest(p, on):
            """(destination, accumulator) of p's gradient: the grad sink's view or None (a fresh bf16 tensor,
            made at the end), and what the chunks accumulate into -- the destination itself when there is one
            chunk or it is fp32, else an fp32 scratch."""
            if not on:
                return None, None
            out = sink(p) if sink is not None else None
            if chunks == 1 and out is None:
                out = torch.empty(p.shape, dtype=p.dtype, device=p.device)
            if out is not None and (chunks == 1 or out.dtype == torch.float32):
                return out, out
            return out, torch.empty(p.shape, dtype=torch.float32, device=p.device)

        def finish(out, acc):
            if out is None:
                return None if acc is None else acc.to(w.dtype)
            if out is not acc:
                out.copy_(acc)
            return out

        dw, dw_acc = dest(w, need_w)
        db, db_acc = dest(bias, need_b)
        for i in range(chunks):
            r0, r1 = i * rows, min(M, (i + 1) * rows)
            dzc, xc = dz[:r1 - r0], x[r0:r1]
            C.lmhead_xent_dz_(xc, w, bias, labels[r0:r1], lse[r0:r1], scale, dzc)
            if need_x:
                _dgrad_route(("dgrad", r1 - r0, K, V), dzc, w, dx[r0:r1])()
            if need_w and i == 0:
                C.gemm_splitk_(dzc, xc, False, False, dw_acc, False, 1.0, 0)
            elif need_w:
                # an accumulating call reduces through an fp32 slab of splits x [V, K]: blocked along the
                # vocabulary where that would outgrow half the logit-gradient buffer (small chunks only)
                s = C.gemm_splits(V, K, r1 - r0)
                vb = V
                if s * V * K * 4 > dz.numel():
                    vb = max(256, dz.numel() // (s * K * 4) // 256 * 256)
                for v0 in range(0, V, vb):
                    C.gemm_splitk_(dzc[:, v0:v0 + vb], xc, False, False, dw_acc[v0:v0 + vb], True, 1.0, s)
            if need_b:
                C.colsum_(dzc, db_acc, i > 0)
        del dz, dzc
        return dx, finish(dw, dw_acc), finish(db, db_acc), None, None, None, None


def _head_ok(x, weight, bias, labels) -> bool:
    """The contract of kernels/lmhead_xent.hip (its launcher refuses anything else)."""
    return (x.is_cuda and weight.is_cuda and labels.is_cuda and x.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16 and (bias is None or (bias.is_cuda and bias.dtype == torch.bfloat16))
            and labels.dtype == torch.int64 and labels.dim() == 1 and x.dim() == 2 and weight.dim() == 2
            and x.shape[0] >= 1 and labels.shape[0] == x.shape[0] and x.shape[1] == weight.shape[1]
            and x.shape[1] % 64 == 0 and weight.shape[0] % 8 == 0 and weight.is_contiguous()
            and (bias is None or bias.is_contiguous())
            and (x.shape[0] + 128) * x.shape[1] < 2 ** 31 and (weight.shape[0] + 128) * x.shape[1] < 2 ** 31
            and weight.data_ptr() % 16 == 0 and (bias is None or bias.data_ptr() % 16 == 0))


def linear_cross_entropy(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor | None, labels: torch.Tensor,
                         chunk_rows: int | None = None, mod=None, slices: int = 0) -> torch.Tensor:
    """Mean softmax cross-entropy of the logits ``x weight^T + bias`` against int64 ``labels [rows]`` (rows
    with a negative label are ignored: the meaning of ``cross_entropy``), without the logits in memory.

    ``x [rows, in]``, ``weight [classes, in]`` (as ``MfmaLinear`` stores it), ``bias [classes]`` or None.
    ``chunk_rows`` (default 4096): rows of logit gradient the backward holds at a time -- its peak extra
    memory is ``chunk_rows * classes * 2`` bytes plus, with more than one chunk, fp32 scratch of the weight
    and bias gradients. ``mod``: the module owning ``weight`` / ``bias``; its PS grad sink (``_psd_grad_sink``)
    receives the gradients as ``MfmaLinear``'s backward would write them. ``slices``: vocabulary slices of the
    forward grid, 0 = chosen from the device's CU count (the tests force it). Falls back to
    ``cross_entropy(F.linear(x, weight, bias), labels)`` when feature ``head_xent`` is off, on the host, for
    other dtypes and for shapes outside the kernel's contract (module docstring)."""
    rows = DEFAULT_CHUNK_ROWS if chunk_rows is None else int(chunk_rows)
    if rows < 1:
        raise ValueError(f"linear_cross_entropy: chunk_rows must be >= 1, got {chunk_rows}")
    if _feat("head_xent") and _head_ok(x, weight, bias, labels):
        x = x.contiguous()
        if x.data_ptr() % 16 == 0:
            return _LinearXentFn.apply(x, weight, bias, labels.contiguous(), rows, mod, int(slices))
    return cross_entropy(F.linear(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype)), labels)
