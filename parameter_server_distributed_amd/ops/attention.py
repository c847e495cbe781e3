"""Multi-head self-attention on the fused gfx950 kernels of ``csrc/kernels/attention.hip`` (S <= 128)
and ``csrc/kernels/attention_long.hip`` (S in 192 .. 512, a multiple of 64).

Input is the packed QKV projection output ``[B, S, 3*H*64]`` exactly as the QKV Linear writes it;
output is ``[B, S, H*64]`` exactly as the output projection reads it. Backward returns the packed
``dQKV``. Compared with ``F.scaled_dot_product_attention`` on q/k/v views this removes the
transpose copy of the output, the stack/cat of dq/dk/dv and the layout copy in backward. Up to
S = 128 the whole head runs out of LDS in one kernel per direction; from S = 192 to 512 (steps of 64)
streaming kernels keep Q (backward: also K, V) fragments in registers and walk the other operand in
64-row chunks with an online softmax -- same layouts, ``lse``, ``lens``, dropout hash and QKV-bias
hand-over (feature ``attn_long``; off: those lengths take SDPA as well).

Attention dropout uses the counter hash shared with the fused LayerNorm (per-site seed + the
model's device step counter, see ``ops/layernorm.bump_step``): masks are regenerated in backward
and a replayed hipGraph draws fresh ones each step.

Variable-length batches pass ``lens`` (int32 ``[B]`` on qkv's device): sequence ``b`` has valid
tokens ``0 .. lens[b]-1`` (clamped to ``[0, S]`` on the device, never read back by the host). Keys
past the length get probability exactly 0, output and gradient rows past it are exact zeros, and
padded rows of qkv / dO are never read.

``causal=True`` adds the decoder mask: query ``q`` attends to keys ``k <= q`` (and ``k < lens[b]`` with
``lens``). Both kernel families have causal instantiations that walk only the 32-row blocks on or below
the diagonal; the dropout hash index is unchanged, so the kept set is the same mask restricted to
``k <= q``. Rows ``<= j`` of the output do not depend on rows ``> j`` of a finite qkv; future rows inside
a diagonal block are loaded, so -- unlike padding -- NaN or inf there is not covered.

CPU tensors, other dtypes, head dims != 64 or S not in {32, 64, 96, 128, 192, 256, 320, 384, 448, 512}
use SDPA -- the reference the tests compare against -- with the same length and causal semantics.
"""
from __future__ import annotations


import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.config import feature as _feat
from .. import native


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, mod, p, lens=None):
        # qkv straight from an MfmaLinear with a bias (ops/linear.py tags its output): backward also
        # sums dqkv's columns -- that Linear's bias gradient -- and hands it over
        src = getattr(qkv, "_psd_src", None) if _feat("attn_bias") else None
        ctx.src = src if (src is not None and src[0].bias is not None and src[0].act in (None, "none")
                          and src[0]._psd_tok == src[1]) else None
        qkv = qkv.contiguous()
        o, lse = native().attn_fwd(qkv, mod.heads, p, mod.seed, mod.step, lens, 0, mod.causal)
        ctx.mod, ctx.p, ctx.lens = mod, p, lens
        ctx.save_for_backward(qkv, o, lse)
        return o

    @staticmethod
    def backward(ctx, do):
        qkv, o, lse = ctx.saved_tensors
        mod = ctx.mod
        db = None
        if ctx.src is not None:
            lin = ctx.src[0]
            sink = getattr(lin, "_psd_grad_sink", None)
            db = sink(lin.bias) if sink is not None else None
            if db is None:
                db = torch.empty_like(lin.bias)
        dqkv = native().attn_bwd(do, qkv, o, lse, mod.heads, ctx.p, mod.seed, mod.step, db, ctx.lens, 0, mod.causal)
        if db is not None:
            ctx.src[0]._psd_bias_hand = (ctx.src[1], dqkv.data_ptr(), db)
        return dqkv, None, None, None


class FusedSelfAttention(nn.Module):
    """softmax(Q K^T / sqrt(d)) V with dropout on the probabilities, from the packed QKV tensor;
    ``causal``: query q sees keys <= q only."""

    def __init__(self, heads: int, p: float = 0.1, seed: int = 0, causal: bool = False):
        super().__init__()
        self.heads = heads
        self.p = p
        self.causal = bool(causal)
        self.seed = int(seed) & 0x7FFFFFFF
        self.step = None  # device int64 counter, set by the owning model (ops/layernorm.bump_step)

    def _kernel_ok(self, qkv) -> bool:
        B, S, E = qkv.shape
        return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and E % (3 * self.heads) == 0
                and E // (3 * self.heads) == 64 and S % 32 == 0 and 32 <= S <= 128)

    @staticmethod
    def long_kernel_shape_ok(S: int, head_dim: int) -> bool:
        """Shapes of the streaming kernels (attention_long.hip): head dim 64, S = 192, 256, .., 512."""
        return head_dim == 64 and 128 < S <= 512 and S % 64 == 0

    def _long_kernel_ok(self, qkv) -> bool:
        B, S, E = qkv.shape
        return (qkv.is_cuda and qkv.dtype == torch.bfloat16 and E % (3 * self.heads) == 0
                and self.long_kernel_shape_ok(S, E // (3 * self.heads)) and _feat("attn_long"))

    def forward(self, qkv, lens=None):
        p = self.p if self.training else 0.0
        if self._kernel_ok(qkv) or self._long_kernel_ok(qkv):
            return _AttnFn.apply(qkv, self, p, lens)
        return self._sdpa(qkv, lens, p)

    def _sdpa(self, qkv, lens, p):
        """``F.scaled_dot_product_attention`` on transposed views (what no kernel takes; tools/attn_bench.py --sdpa)."""
        B, S, E = qkv.shape
        H = self.heads
        q, k, v = qkv.view(B, S, 3, H, E // (3 * H)).permute(2, 0, 3, 1, 4).unbind(0)
        if lens is None:
            a = F.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=self.causal)
            return a.transpose(1, 2).reshape(B, S, E // 3)
        valid = torch.arange(S, device=qkv.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]
        row = valid[:, None, :, None]
        # padded rows never enter a product (where, not a multiply: 0 * NaN = NaN)
        q, k, v = (torch.where(row, t, torch.zeros((), dtype=t.dtype, device=t.device)) for t in (q, k, v))
        # padded queries see every key (their zero q gives a finite uniform row, also at L = 0) and
        # are multiplied by zero below
        mask = valid[:, None, None, :] | ~row
        if self.causal:  # key <= q and key < L; a padded query keeps key 0, so its row stays finite
            mask = mask & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=p) * row.to(q.dtype)
        return a.transpose(1, 2).reshape(B, S, E // 3)
