"""The Llama-style decoder block: a pre-norm residual stream, RMSNorm, a gated SiLU FFN (SwiGLU) and
bias-free Linears, on the fused gfx950 kernels of ``ops/rmsnorm.py`` and ``ops/swiglu.py`` around the
causal attention and GEMM kernels the GPT block uses.

The block carries the residual stream ``r`` and the last branch output ``h`` separately: each norm site
adds the pending branch into the stream and normalises the sum in one pass (``FusedAddRMSNorm``), so the
stream is never read by an add of its own::

    r, y = norm1(r, h)                      # r += dropout(h);  y = RMSNorm(r)
    a    = proj(attn(rot(qkv(y))))
    r, y = norm2(r, a)
    h    = down(act(gate_up(y)))            # gate_up: [hidden -> 2 ffn], gate | up packed

and returns ``(r, h)``; the owner closes the stack with one more norm, ``norm_f(r, h)``. The first block
gets ``h=None``.
"""
from __future__ import annotations

import torch.nn as nn

from ..ops.attention import FusedSelfAttention
from ..ops.linear import MfmaLinear
from ..ops.rmsnorm import FusedAddRMSNorm
from ..ops.swiglu import SwiGLU


def default_ffn(hidden: int) -> int:
    """``8/3 * hidden`` rounded up to a multiple of 256: the parameter count of a ``4 * hidden`` two-matrix
    FFN in three matrices (2048 at hidden 768)."""
    return -(-(8 * int(hidden)) // (3 * 256)) * 256


class LlamaLayer(nn.Module):
    def __init__(self, hidden=768, heads=12, ffn=2048, dropout=0.1, index=0, window=None, rope=None, eps=1e-6):
        super().__init__()
        # rope: (max_pos, base) -- rotary position embedding of Q and K between the QKV Linear and the
        # attention (ops/rope.py); None: no such module
        self.rot = None
        if rope is not None:
            from ..ops.rope import RotaryQK

            self.rot = RotaryQK(heads, int(rope[0]), float(rope[1]))
        self.heads = heads
        # seeds as BertLayer's: attention 1000 + index, the two norm sites 2 * index + 1 and 2 * index + 2
        self.norm1 = FusedAddRMSNorm(hidden, eps=eps, p=dropout, seed=2 * index + 1)
        self.qkv = MfmaLinear(hidden, 3 * hidden, bias=False)
        self.attn = FusedSelfAttention(heads, p=dropout, seed=1000 + index, causal=True, window=window)
        self.proj = MfmaLinear(hidden, hidden, bias=False)
        self.norm2 = FusedAddRMSNorm(hidden, eps=eps, p=dropout, seed=2 * index + 2)
        # gate_proj and up_proj as one Linear: its output is the packed [.., 2 ffn] the activation reads in place
        self.gate_up = MfmaLinear(hidden, 2 * ffn, bias=False)
        self.act = SwiGLU()
        self.down = MfmaLinear(ffn, hidden, bias=False)
        self.p = dropout

    def forward(self, r, h=None, lens=None, doc_start=None):
        # doc_start: packed documents (ops/attention.py), passed on to the rotation and the attention
        r, y = self.norm1(r, h)
        qkv = self.qkv(y)
        if self.rot is not None:  # rotated in place on the GPU
            qkv = self.rot(qkv, lens, doc_start)
        a = self.proj(self.attn(qkv, lens, doc_start))
        r, y = self.norm2(r, a)
        return r, self.down(self.act(self.gate_up(y)))
