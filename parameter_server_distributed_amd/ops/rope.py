"""Rotary position embeddings (RoPE) on the packed QKV tensor (``csrc/kernels/rope.hip``).

``RotaryQK`` sits between the QKV Linear and ``FusedSelfAttention``: it rotates the Q and K heads of
``qkv [B, S, 3*H*64]`` (the ordering ``FusedSelfAttention._sdpa`` spells out, ``view(B, S, 3, H, 64)``) by
the angle of each row's position and leaves V alone. Convention: rotate-half (GPT-NeoX / Llama), pairs
``(i, i + 32)``, ``i = 0 .. 31``, of every head; ``theta_i = base ** (-2 i / 64)``; with ``c = cos(pos theta_i)``
and ``s = sin(pos theta_i)`` from fp32 tables, ``y1 = x1 c - x2 s`` and ``y2 = x2 c + x1 s`` in fp32, rounded
once to the tensor's dtype. The inverse (``-s``) is the backward: the rotation is orthogonal, so no
activation is saved.

The position of row ``(b, t)`` is ``t - clamp(doc_start[b, t], 0, t)`` (``t`` without a ``doc_start``): it
restarts at every document, with the clamp of the attention kernels, so no ``doc_start`` value can index
outside the tables. With ``lens``, rows ``t >= clamp(lens[b], 0, S)`` -- and the ``doc_start`` entries
there -- are neither read nor written. A row at position 0 is the rotation by angle 0: kernel and
composite both pass it through untouched, so the first token of every document keeps its bits.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from ..utils.config import feature as _feat
from .. import native

HEAD_DIM = 64


def rope_tables(max_pos: int, base: float = 10000.0, device=None):
    """``(cos, sin)``, fp32 ``[max_pos, 32]``: the angles ``pos * base ** (-2 i / 64)`` and their cos / sin are
    computed in fp64 on the host and rounded once to fp32."""
    if int(max_pos) < 1:
        raise ValueError(f"rope_tables: max_pos must be >= 1, got {max_pos}")
    if not float(base) > 0.0:
        raise ValueError(f"rope_tables: base must be > 0, got {base}")
    i = torch.arange(HEAD_DIM // 2, dtype=torch.float64)
    theta = torch.tensor(float(base), dtype=torch.float64) ** (-2.0 * i / HEAD_DIM)
    ang = torch.arange(int(max_pos), dtype=torch.float64)[:, None] * theta[None, :]
    cos, sin = ang.cos().to(torch.float32), ang.sin().to(torch.float32)
    if device is not None:
        cos, sin = cos.to(device), sin.to(device)
    return cos, sin


def _positions(B: int, S: int, device, doc_start):
    t = torch.arange(S, device=device)[None, :].expand(B, S)
    if doc_start is None:
        return t
    return t - torch.minimum(doc_start.long().clamp(min=0), t)


def rope_ref(qkv, heads: int, cos, sin, lens=None, doc_start=None, inverse: bool = False):
    """The torch composite with the semantics of the native ``rope_``, on any device and dtype, out of
    place: fp32 maths on the given tables (fp64 for an fp64 ``qkv``), one rounding to ``qkv``'s dtype,
    and a copy in which rows past a length, rows at position 0 and the V third are passed through. The
    CPU path of ``RotaryQK`` and the yardstick of the tests."""
    if qkv.dim() != 3 or qkv.shape[2] != 3 * heads * HEAD_DIM:
        raise ValueError(f"rope_ref: qkv must be [B, S, 3*heads*64], got {tuple(qkv.shape)} with heads = {heads}")
    B, S, E = qkv.shape
    if cos.shape != sin.shape or cos.dim() != 2 or cos.shape[1] != HEAD_DIM // 2 or cos.shape[0] < S:
        raise ValueError(f"rope_ref: cos / sin must be [P, 32] with P >= S = {S}, got {tuple(cos.shape)}, "
                         f"{tuple(sin.shape)}")
    mt = torch.float64 if qkv.dtype == torch.float64 else torch.float32
    pos = _positions(B, S, qkv.device, doc_start)  # in [0, t]: inside the tables whatever doc_start holds
    keep = pos != 0
    if lens is not None:
        keep = keep & (torch.arange(S, device=qkv.device)[None, :] < lens.clamp(0, S)[:, None])
    c = cos.to(mt)[pos][:, :, None, :]  # [B, S, 1, 32]
    s = sin.to(mt)[pos][:, :, None, :]
    if inverse:
        s = -s
    qk = qkv[:, :, :2 * E // 3].reshape(B, S, 2 * heads, HEAD_DIM)
    x1, x2 = qk[..., :HEAD_DIM // 2].to(mt), qk[..., HEAD_DIM // 2:].to(mt)
    rot = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1).to(qkv.dtype)
    # a select, not a blend: what a passed-through row holds (NaN included) never enters the result
    rot = torch.where(keep[:, :, None, None], rot, qk).reshape(B, S, 2 * E // 3)
    return torch.cat([rot, qkv[:, :, 2 * E // 3:]], dim=-1)


def _kernel_ok(t, heads: int) -> bool:
    return (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 3 and t.shape[2] == 3 * heads * HEAD_DIM
            and t.is_contiguous() and t.data_ptr() % 16 == 0)


class _RopeFn(torch.autograd.Function):
    """The native op through autograd: the forward rotates ``qkv`` in place (``mark_dirty``), the backward
    is the inverse rotation of the incoming gradient."""

    @staticmethod
    def forward(ctx, qkv, mod, lens, doc_start):
        ctx.mark_dirty(qkv)
        native().rope_(qkv, mod.heads, mod.cos, mod.sin, lens, doc_start, False, 0)
        ctx.mod, ctx.lens, ctx.doc = mod, lens, doc_start
        return qkv

    @staticmethod
    def backward(ctx, g):
        mod = ctx.mod
        if g.requires_grad or not _kernel_ok(g, mod.heads):
            # a gradient that is part of a graph (create_graph), expanded or otherwise not the kernel's layout
            return rope_ref(g, mod.heads, mod.cos, mod.sin, ctx.lens, ctx.doc, True), None, None, None
        if not mod.grad_in_place:
            g = g.clone()
        return native().rope_(g, mod.heads, mod.cos, mod.sin, ctx.lens, ctx.doc, True, 0), None, None, None


class RotaryQK(nn.Module):
    """Rotary position embedding of the Q and K heads of a packed ``qkv [B, S, 3*heads*64]``;
    ``forward(qkv, lens=None, doc_start=None)`` with the ``lens`` / ``doc_start`` the attention gets.

    The fp32 tables ``[max_pos, 32]`` are non-persistent buffers: they are no part of ``state_dict`` (a
    checkpoint loads into a model built for another context length) and no parameter. ``S > max_pos`` is
    a ``ValueError``.

    A contiguous bf16 device tensor with head dim 64 takes the kernel when feature ``rope`` is on (the
    default; ``PSD_FEATURES=rope=0`` takes the composite): the forward rotates ``qkv`` **in place** and
    returns the same tensor object, the backward rotates the incoming gradient by the inverse angle.
    Everything else takes ``rope_ref`` through ordinary autograd, out of place.

    The bias hand-over: the tensor returned carries no ``_psd_src`` tag. The attention backward would
    otherwise hand the QKV Linear the column sums of the ``dQKV`` it wrote (ops/attention.py), which the
    Linear accepts by the gradient's data pointer (ops/linear.py) -- and the in-place inverse rotation keeps
    that pointer while changing the values. Without the tag the attention makes no hand-over and the
    Linear sums its own bias gradient from the rotated gradient, as it does after SDPA.

    The gradient is rotated in place too when it is a contiguous bf16 device tensor outside any graph:
    the consumer's backward must then own the gradient it returns. ``FusedSelfAttention`` does on both of
    its paths (the kernels allocate ``dQKV``; SDPA's gradient is stacked into a fresh tensor). A consumer
    that passes its own incoming gradient through unchanged (``qkv + other``, a bare ``view``) shares that
    tensor with its other inputs, and a tensor hook on the returned tensor may keep it: for those set
    ``grad_in_place = False`` and the gradient is rotated into a copy. A gradient that requires grad
    (``create_graph=True``), is expanded or non-contiguous or of another dtype is always rotated out of
    place by the composite."""

    _psd_fp32_buffers = True  # models.prepare() keeps the tables fp32

    def __init__(self, heads: int, max_pos: int, base: float = 10000.0):
        super().__init__()
        if int(heads) < 1:
            raise ValueError(f"RotaryQK: heads must be >= 1, got {heads}")
        self.heads = int(heads)
        self.max_pos = int(max_pos)
        self.base = float(base)
        self.grad_in_place = True
        cos, sin = rope_tables(max_pos, base)
        self.register_buffer("cos", cos, persistent=False)
        self.register_buffer("sin", sin, persistent=False)

    def _apply(self, fn, *args, **kwargs):
        super()._apply(fn, *args, **kwargs)
        if self.cos.dtype != torch.float32:  # a dtype cast of the model: the tables stay fp32, rebuilt, not rounded twice
            self.cos, self.sin = rope_tables(self.max_pos, self.base, self.cos.device)
        return self

    def extra_repr(self) -> str:
        return f"heads={self.heads}, max_pos={self.max_pos}, base={self.base}"

    def forward(self, qkv, lens=None, doc_start=None):
        if qkv.dim() != 3 or qkv.shape[2] != 3 * self.heads * HEAD_DIM:
            raise ValueError(f"RotaryQK: qkv must be [B, S, 3*{self.heads}*64], got {tuple(qkv.shape)}")
        if qkv.shape[1] > self.max_pos:
            raise ValueError(f"RotaryQK: S = {qkv.shape[1]} exceeds max_pos = {self.max_pos}")
        if _kernel_ok(qkv, self.heads) and _feat("rope"):
            if qkv.is_leaf and qkv.requires_grad:  # autograd allows no in-place update of such a leaf
                qkv = qkv.clone()
            out = _RopeFn.apply(qkv, self, lens, doc_start)
            if hasattr(out, "_psd_src"):  # mark_dirty returns the same Python object, tag included
                del out._psd_src
            return out
        return rope_ref(qkv, self.heads, self.cos, self.sin, lens, doc_start)
