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

``fp8="mx"``: the four Linears run the MX fp8 recipe of ``ops/linear.py`` (forward and bwd-data on the block-scaled
MFMA; the attention stays bf16), and the fused kernels around them write their MX operands as side outputs of the
passes they already make (feature ``fp8_llama_handover``), instead of one ``quantize_mx`` pass each::

    forward   norm1 -> qkv,  norm2 -> gate_up,  act -> down        (e4m3 inputs)
    backward  act -> gate_up,  norm2 -> proj,  the next norm1 / norm_f -> down   (e5m2 output gradients)

The last one crosses blocks and is wired by the owner (``models/gpt.py``). ``proj``'s input (the attention output)
and ``qkv``'s output gradient (the attention's ``dqkv``) come from kernels that do not write MX copies: those two
operands stay ``quantize_mx`` passes.
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
    def __init__(self, hidden=768, heads=12, ffn=2048, dropout=0.1, index=0, window=None, rope=None, eps=1e-6,
                 fp8=False, kv_heads=None):
        super().__init__()
        if not (fp8 is False or (isinstance(fp8, str) and fp8 == "mx")):
            raise ValueError(f"LlamaLayer: fp8 must be False or 'mx', got {fp8!r}")
        # kv_heads: grouped-query attention (ops/attention.py) -- the QKV Linear writes heads query heads and
        # kv_heads key and value heads of 64 per row; None: as many as heads, the block without the argument
        if kv_heads is not None and (int(kv_heads) < 1 or heads % int(kv_heads) != 0):
            raise ValueError(f"LlamaLayer: kv_heads must divide heads = {heads}, got {kv_heads}")
        # rope: (max_pos, base) -- rotary position embedding of Q and K between the QKV Linear and the
        # attention (ops/rope.py); None: no such module
        self.rot = None
        if rope is not None:
            from ..ops.rope import RotaryQK

            self.rot = RotaryQK(heads, int(rope[0]), float(rope[1]), kv_heads=kv_heads)
        self.heads = heads
        qkv_out = 3 * hidden
        if kv_heads is not None:
            if hidden != heads * 64:
                raise ValueError(f"LlamaLayer: kv_heads needs head dim 64 (hidden = heads * 64), got hidden = {hidden}, "
                                 f"heads = {heads}")
            qkv_out = (heads + 2 * int(kv_heads)) * 64
        # seeds as BertLayer's: attention 1000 + index, the two norm sites 2 * index + 1 and 2 * index + 2
        self.norm1 = FusedAddRMSNorm(hidden, eps=eps, p=dropout, seed=2 * index + 1)
        self.qkv = MfmaLinear(hidden, qkv_out, bias=False, fp8=fp8)
        self.attn = FusedSelfAttention(heads, p=dropout, seed=1000 + index, causal=True, window=window,
                                       kv_heads=kv_heads)
        self.proj = MfmaLinear(hidden, hidden, bias=False, fp8=fp8)
        self.norm2 = FusedAddRMSNorm(hidden, eps=eps, p=dropout, seed=2 * index + 2)
        # gate_proj and up_proj as one Linear: its output is the packed [.., 2 ffn] the activation reads in place
        self.gate_up = MfmaLinear(hidden, 2 * ffn, bias=False, fp8=fp8)
        self.act = SwiGLU()
        self.down = MfmaLinear(ffn, hidden, bias=False, fp8=fp8)
        self.p = dropout
        if fp8:  # the MX operands the fused kernels write for the Linears next to them (module docstring)
            self.norm1.psd_mx_output_to(self.qkv)
            self.norm2.psd_mx_output_to(self.gate_up)
            self.act.psd_mx_output_to(self.down)
            self.act.psd_mx_grad_to(self.gate_up)
            self.norm2.psd_mx_grad_to(self.proj)

    def forward(self, r, h=None, lens=None, doc_start=None):
        # doc_start: packed documents (ops/attention.py), passed on to the rotation and the attention
        r, y = self.norm1(r, h)
        qkv = self.qkv(y)
        if self.rot is not None:  # rotated in place on the GPU
            qkv = self.rot(qkv, lens, doc_start)
        a = self.proj(self.attn(qkv, lens, doc_start))
        r, y = self.norm2(r, a)
        return r, self.down(self.act(self.gate_up(y)))
