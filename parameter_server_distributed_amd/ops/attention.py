"""Multi-head self-attention on the fused gfx950 kernels of ``csrc/kernels/attention.hip`` (S <= 128)
and ``csrc/kernels/attention_long.hip`` (S in 192 .. 4096, a multiple of 64).

Input is the packed QKV projection output ``[B, S, 3*H*64]`` exactly as the QKV Linear writes it;
output is ``[B, S, H*64]`` exactly as the output projection reads it. Backward returns the packed
``dQKV``. Compared with ``F.scaled_dot_product_attention`` on q/k/v views this removes the
transpose copy of the output, the stack/cat of dq/dk/dv and the layout copy in backward. Up to
S = 128 the whole head runs out of LDS in one kernel per direction; from S = 192 to 4096 (steps of 64)
streaming kernels keep Q (backward: also K, V) fragments in registers and walk the other operand in
64-row chunks with an online softmax -- same layouts, ``lse``, ``lens``, dropout hash and QKV-bias
hand-over (feature ``attn_long``; off: those lengths take SDPA as well. S = 576 .. 4096 also needs the
feature ``attn_xlong``; off: S > 512 takes SDPA).

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

Packed documents pass ``doc_start`` (int32 ``[B, S]`` on qkv's device, ``doc_starts`` builds it):
``doc_start[b, t]`` is the index of the first token of the document token ``t`` belongs to. With
``causal=True`` query ``q`` sees key ``k`` iff both are of one document, ``k <= q`` and ``k < lens[b]`` --
for a well-formed row ``doc_start[b, q] <= k <= q``. The document copies of both kernel families skip
the 32-row blocks of other documents; entries at positions past a length are never read, the values
are clamped to ``[0, t]`` and only compared on the device. All zeros is bitwise the plain causal call.
With ``causal=False`` the kernels do not serve a ``doc_start``: the module then takes SDPA with the
symmetric same-document mask, and the native op raises. Arbitrary masks are not supported.

``FusedSelfAttention(..., causal=True, window=W)`` is causal sliding-window attention: query ``q`` sees key
``k`` iff ``max(doc_start[b, q], q - W + 1, 0) <= k <= q`` and ``k < lens[b]`` -- ``W`` keys with its own. The
streaming kernels have window copies (with or without a ``doc_start``) that skip the 32-row blocks out of
a window's reach; ``W >= S`` cuts nothing and takes exactly the path of a module without a window. The
whole-head kernels have none: S <= 128 with ``W < S`` takes SDPA with the band AND-ed into the mask. The
native ops take ``window`` last (0: off) and raise on a window without ``causal`` or at an S <= 128.

CPU tensors, other dtypes, head dims != 64 or S not in {32, 64, 96, 128} or {192, 256, .., 4096} use SDPA
-- the reference the tests compare against -- with the same length, causal, document and window
semantics.
"""
from __future__ import annotations


import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.config import feature as _feat
from .. import native


def doc_starts(doc_lens, S: int, device=None) -> torch.Tensor:
    """``doc_start`` (int32 ``[B, S]``) from per-row lists of document lengths, laid end to end from
    position 0. A row's documents may sum to less than ``S``: every remaining position is padding and
    gets its own index (a one-token document). Lengths must be positive and sum to at most ``S``."""
    out = torch.arange(S, dtype=torch.int32).repeat(len(doc_lens), 1)
    for b, row in enumerate(doc_lens):
        t = 0
        for n in row:
            n = int(n)
            if n < 1 or t + n > S:
                raise ValueError(f"row {b}: document lengths {list(row)} do not fit {S} positions")
            out[b, t:t + n] = t
            t += n
    return out.to(device) if device is not None else out


def check_doc_start(t: torch.Tensor) -> None:
    """Raise ``ValueError`` unless ``t`` is a well-formed ``doc_start``: int32 ``[B, S]``, every row
    non-decreasing, ``t[b, i] <= i`` (and >= 0) and ``t[b, t[b, i]] == t[b, i]``. Reads the tensor back
    (a device sync): for tests and debugging, never on the hot path."""
    if t.dim() != 2 or t.dtype != torch.int32:
        raise ValueError(f"doc_start must be an int32 [B, S] tensor, got {t.dtype} {tuple(t.shape)}")
    v = t.long()
    S = v.shape[1]
    idx = torch.arange(S, device=v.device)[None, :]
    if S and bool((v[:, 1:] < v[:, :-1]).any()):
        raise ValueError("doc_start: a row is not non-decreasing")
    if bool(((v < 0) | (v > idx)).any()):
        raise ValueError("doc_start: an entry is outside [0, t]")
    if not torch.equal(torch.gather(v, 1, v), v):
        raise ValueError("doc_start: doc_start[doc_start[t]] != doc_start[t] (a start that is not its own start)")


class _AttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, qkv, mod, p, lens=None, doc_start=None, window=None):
        # qkv straight from an MfmaLinear with a bias (ops/linear.py tags its output): backward also
        # sums dqkv's columns -- that Linear's bias gradient -- and hands it over
        src = getattr(qkv, "_psd_src", None) if _feat("attn_bias") else None
        ctx.src = src if (src is not None and src[0].bias is not None and src[0].act in (None, "none")
                          and src[0]._psd_tok == src[1]) else None
        qkv = qkv.contiguous()
        # window: None on every path that existed before it (no argument passed), else the W of the window copies
        ctx.win = () if window is None else (int(window),)
        o, lse = native().attn_fwd(qkv, mod.heads, p, mod.seed, mod.step, lens, 0, mod.causal, doc_start, *ctx.win)
        ctx.mod, ctx.p, ctx.lens, ctx.doc = mod, p, lens, doc_start
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
        dqkv = native().attn_bwd(do, qkv, o, lse, mod.heads, ctx.p, mod.seed, mod.step, db, ctx.lens, 0, mod.causal,
                                 ctx.doc, *ctx.win)
        if db is not None:
            ctx.src[0]._psd_bias_hand = (ctx.src[1], dqkv.data_ptr(), db)
        return dqkv, None, None, None, None, None


class FusedSelfAttention(nn.Module):
    """softmax(Q K^T / sqrt(d)) V with dropout on the probabilities, from the packed QKV tensor;
    ``causal``: query q sees keys <= q only; ``window=W`` (causal only): and keys > q - W only.
    ``forward(qkv, lens=None, doc_start=None)``: with a
    ``doc_start`` (packed documents, module docstring) a causal module runs the document copies of the
    kernels at the kernel shapes; a bidirectional one has no kernel for it and takes SDPA with the
    symmetric same-document mask."""

    def __init__(self, heads: int, p: float = 0.1, seed: int = 0, causal: bool = False, window: int | None = None):
        super().__init__()
        if window is not None:
            if int(window) < 1:
                raise ValueError(f"window must be >= 1 (the query's own key included) or None, got {window}")
            if not causal:
                raise ValueError("window needs causal=True: there is no symmetric window")
        self.heads = heads
        self.p = p
        self.causal = bool(causal)
        self.window = None if window is None else int(window)
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

    @staticmethod
    def xlong_kernel_shape_ok(S: int, head_dim: int) -> bool:
        """Shapes the streaming kernels serve past 512 (feature ``attn_xlong``): head dim 64, S = 576, 640, .., 4096."""
        return head_dim == 64 and 512 < S <= 4096 and S % 64 == 0

    def _long_kernel_ok(self, qkv) -> bool:
        B, S, E = qkv.shape
        if not (qkv.is_cuda and qkv.dtype == torch.bfloat16 and E % (3 * self.heads) == 0 and _feat("attn_long")):
            return False
        dh = E // (3 * self.heads)
        return self.long_kernel_shape_ok(S, dh) or (self.xlong_kernel_shape_ok(S, dh) and _feat("attn_xlong"))

    def forward(self, qkv, lens=None, doc_start=None):
        p = self.p if self.training else 0.0
        if self.window is not None and self.window < qkv.shape[1]:
            # a window that cuts something: the window copies of the streaming kernels, or SDPA with the mask
            if self._long_kernel_ok(qkv):
                return _AttnFn.apply(qkv, self, p, lens, doc_start, self.window)
            return self._sdpa(qkv, lens, p, doc_start, self.window)
        if (doc_start is None or self.causal) and (self._kernel_ok(qkv) or self._long_kernel_ok(qkv)):
            return _AttnFn.apply(qkv, self, p, lens, doc_start)
        return self._sdpa(qkv, lens, p, doc_start)

    def _sdpa(self, qkv, lens, p, doc_start=None, window=None):
        """``F.scaled_dot_product_attention`` on transposed views (what no kernel takes; tools/attn_bench.py --sdpa)."""
        B, S, E = qkv.shape
        H = self.heads
        q, k, v = qkv.view(B, S, 3, H, E // (3 * H)).permute(2, 0, 3, 1, 4).unbind(0)
        if lens is None and doc_start is None and window is None:
            a = F.scaled_dot_product_attention(q, k, v, dropout_p=p, is_causal=self.causal)
            return a.transpose(1, 2).reshape(B, S, E // 3)
        if lens is None:
            lens = torch.full((B,), S, dtype=torch.int32, device=qkv.device)
        valid = torch.arange(S, device=qkv.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]
        row = valid[:, None, :, None]
        # padded rows never enter a product (where, not a multiply: 0 * NaN = NaN)
        q, k, v = (torch.where(row, t, torch.zeros((), dtype=t.dtype, device=t.device)) for t in (q, k, v))
        # padded queries see every key (their zero q gives a finite uniform row, also at L = 0) and
        # are multiplied by zero below
        mask = valid[:, None, None, :] | ~row
        if self.causal:  # key <= q and key < L; a padded query keeps key 0, so its row stays finite
            mask = mask & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
        if doc_start is not None:  # valid queries see their own document only; padded ones stay as they were
            same = doc_start[:, None, :, None] == doc_start[:, None, None, :]
            mask = mask & (same | ~row)
        if window is not None:  # key > q - W (with the causal mask: W keys, the query's own included); padded
            idx = torch.arange(S, device=qkv.device)  # queries keep every key, as above
            mask = mask & ((idx[None, :] > idx[:, None] - int(window)) | ~row)
        a = F.scaled_dot_product_attention(q, k, v, attn_mask=mask, dropout_p=p) * row.to(q.dtype)
        return a.transpose(1, 2).reshape(B, S, E // 3)
