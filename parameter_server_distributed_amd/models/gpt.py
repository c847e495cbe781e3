"""GPT-1-shaped decoder language model (12 layers, hidden 768, 12 heads, FFN 3072, context 512) with
a next-token head over every position. Random init, synthetic token batches.

The block is ``BertLayer`` with ``causal=True``: post-LN, GELU FFN, every Linear an ``MfmaLinear`` and
the attention the causal instantiations of the fused gfx950 kernels (``ops/attention.py``; SDPA with
the same mask off-GPU). Deviations from the original GPT-1, stated here: the 40,478-token vocabulary
is padded to 40512 (a multiple of 64, for the GEMM tiles); the embeddings are ``FusedBertEmbeddings``
with all-zero token types, so the sum of the word and position rows (plus one constant type row) goes
through an embedding LayerNorm and dropout where GPT-1 has dropout only; and the LM head is untied
from the word embedding, for the reason ``models/bert.py`` gives (the PS data plane needs every weight
consumed by exactly one autograd node).

``pos="rope"`` replaces the learned absolute positions by rotary position embeddings: every block owns
a ``RotaryQK(heads, max_pos, rope_base)`` (``ops/rope.py``) between its QKV Linear and its attention, the
angle following the position inside the document (it restarts with ``doc_start``). One more deviation,
stated here: the embedding block is kept, fed all-zero position ids and given a one-row position table,
so the learned position signal becomes one constant row next to the constant type row. The rotary
tables are no part of the state, so one ``state_dict`` serves every ``max_pos``.

``arch="llama"`` replaces the block by ``LlamaLayer`` (``models/llama_block.py``): a pre-norm residual
stream, RMSNorm (eps 1e-6), a gated SiLU FFN of width ``ffn`` (default ``8/3 * hidden`` rounded up to a
multiple of 256: 2048 at 768, the GELU FFN's parameter count) and bias-free Linears, the LM head included;
the stack ends with a final ``norm_f``. The forward threads the residual stream and the last branch output
``(r, h)`` through the blocks. ``pos``, ``window``, padded batches and packed documents compose with it
unchanged. One more deviation, stated here: the embedding block is kept as it is -- ``FusedBertEmbeddings``
with its embedding LayerNorm (with a bias) and dropout -- where Llama feeds the bare word embedding into
the first block. ``fp8=True`` is not built for this block. ``arch="gpt"`` (the default) is the model above,
module for module.
"""
from __future__ import annotations


import torch
import torch.nn as nn

from ..ops.embedding import FusedBertEmbeddings
from ..ops.layernorm import bump_step
from ..ops.linear import MfmaLinear
from ..ops.loss import cross_entropy
from .bert import BertLayer, wire_fp8_handover

VOCAB = 40512


class GPTForLM(nn.Module):
    def __init__(self, layers=12, hidden=768, heads=12, vocab=VOCAB, max_pos=512, dropout=0.1, fp8=False,
                 window=None, pos="learned", rope_base=10000.0, arch="gpt", ffn=None):
        super().__init__()
        if pos not in ("learned", "rope"):
            raise ValueError(f"GPTForLM: pos must be 'learned' or 'rope', got {pos!r}")
        if arch not in ("gpt", "llama"):
            raise ValueError(f"GPTForLM: arch must be 'gpt' or 'llama', got {arch!r}")
        if arch == "llama" and fp8:
            raise ValueError("GPTForLM: fp8=True with arch='llama' is not built (the Llama block's Linears are bf16)")
        if arch == "gpt" and ffn is not None and int(ffn) != 4 * hidden:
            raise ValueError(f"GPTForLM: arch='gpt' has the fixed FFN width 4 * hidden = {4 * hidden}, got ffn={ffn}")
        self.vocab = vocab
        self.pos = pos
        self.arch = arch
        # pos="rope": the position table has one row, which every token reads (all-zero position ids)
        self.emb = FusedBertEmbeddings(vocab, hidden, 1 if pos == "rope" else max_pos, 2, eps=1e-12, p=dropout,
                                       seed=4242)
        # fp8: MX fp8 qkv / proj / ffn1 / ffn2 in every block (models/bert.py); the LM head stays bf16
        # window: every block attends to the last `window` keys only (sliding window, ops/attention.py)
        # rope: every block rotates its Q and K by the position inside the document (ops/rope.py)
        rope = (max_pos, rope_base) if pos == "rope" else None
        if arch == "llama":
            from ..ops.rmsnorm import FusedAddRMSNorm
            from .llama_block import LlamaLayer, default_ffn

            ffn = default_ffn(hidden) if ffn is None else int(ffn)
            self.layers = nn.ModuleList([LlamaLayer(hidden, heads, ffn, dropout, i, window=window, rope=rope)
                                         for i in range(layers)])
            # the last block's branch joins the stream here; seeds 2 * i + 1, 2 * i + 2 belong to block i
            self.norm_f = FusedAddRMSNorm(hidden, eps=1e-6, p=dropout, seed=2 * layers + 1)
            self.head = MfmaLinear(hidden, vocab, bias=False)
        else:
            self.layers = nn.ModuleList([BertLayer(hidden, heads, 4 * hidden, dropout, i, causal=True, fp8=fp8,
                                                   window=window, rope=rope) for i in range(layers)])
            wire_fp8_handover(self.layers)
            self.head = MfmaLinear(hidden, vocab)
        self.p = dropout
        # device step counter for the fused dropout masks (ops/layernorm.py)
        self.register_buffer("_psd_rng_step", torch.zeros(1, dtype=torch.int64), persistent=False)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.02)
                if m.bias is not None:
                    nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=0.02)

    def forward(self, batch):
        # (ids,) or, for a padded batch, (ids, lens): int32 [B] lengths, positions >= lens[b] are padding
        # that no attention key or query row reads. Packed documents: (ids, lens, doc_start), doc_start
        # int32 [B, S] (ops/attention.py): a token attends inside its own document only and its position
        # id restarts there, t - doc_start[b, t]. Logits of every position: [B*S, vocab]
        ids = batch[0]
        lens = batch[1] if len(batch) > 1 else None
        doc_start = batch[2] if len(batch) > 2 else None
        bump_step(self)
        pos_ids = None
        if self.pos == "rope":  # the blocks carry the position; the embedding adds its one constant row
            pos_ids = torch.zeros_like(ids)
        elif doc_start is not None:
            pos_ids = torch.arange(ids.shape[1], device=ids.device)[None, :] - doc_start.long()
        x = self.emb(ids, torch.zeros_like(ids), pos_ids)
        if self.arch == "llama":  # the residual stream r and the last branch output h, joined at each norm
            r, h = x, None
            for layer in self.layers:
                r, h = layer(r, h, lens, doc_start)
            x = self.norm_f(r, h)[1]
        else:
            for layer in self.layers:
                x = layer(x, lens, doc_start)
        return self.head(x.reshape(-1, x.shape[-1]))

    @staticmethod
    def loss(logits, labels):
        return cross_entropy(logits, labels)  # fused bf16 softmax-CE kernels (ops/loss.py)


def gpt_batch(batch: int, seq: int, vocab: int, device, seed: int = 0, min_len: int | None = None,
              docs: tuple[int, int] | None = None):
    """Synthetic language-model batch: random ids and the next-token labels ``[B*S]``,
    ``labels[b, s] = ids[b, s + 1]``; the last position has no next token and gets -100, which the loss
    ignores.

    With ``min_len`` the sequences are padded: lengths are uniform in [min_len, seq], ids past a length
    are 0, every position ``s >= L - 1`` gets label -100 and the batch tuple gains ``lens`` (int32 [B]).

    With ``docs=(lo, hi)`` every row is packed with documents of length uniform in [lo, hi], laid end to
    end; the last one is cut at ``seq``. No label crosses a boundary: each document's last token gets
    -100. Returns ``((ids, lens, doc_start), labels)`` with ``lens`` full and ``doc_start`` int32 [B, S]
    (ops/attention.doc_starts). Not with ``min_len``."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, vocab, (batch, seq), generator=g)
    if docs is not None:
        if min_len is not None:
            raise ValueError("gpt_batch: docs (packed rows) cannot be combined with min_len (padded rows)")
        lo, hi = int(docs[0]), int(docs[1])
        if not 1 <= lo <= hi:
            raise ValueError(f"docs must be (lo, hi) with 1 <= lo <= hi, got {docs}")
        from ..ops.attention import doc_starts

        rows = []
        for _ in range(batch):
            row, t = [], 0
            while t < seq:
                n = min(int(torch.randint(lo, hi + 1, (1,), generator=g)), seq - t)
                row.append(n)
                t += n
            rows.append(row)
        ds = doc_starts(rows, seq)
        labels = torch.full((batch, seq), -100, dtype=torch.long)
        labels[:, :-1] = ids[:, 1:]
        last = torch.ones(batch, seq, dtype=torch.bool)  # a document's last token: the next one starts anew
        last[:, :-1] = ds[:, 1:] != ds[:, :-1]
        labels[last] = -100
        lens = torch.full((batch,), seq, dtype=torch.int32)
        return (ids.to(device), lens.to(device), ds.to(device)), labels.reshape(-1).to(device)
    if min_len is None:
        lens = torch.full((batch,), seq, dtype=torch.long)
    else:
        if not 1 <= int(min_len) <= seq:
            raise ValueError(f"min_len must be in [1, {seq}], got {min_len}")
        lens = torch.randint(int(min_len), seq + 1, (batch,), generator=g)
        ids = ids * (torch.arange(seq)[None, :] < lens[:, None])
    labels = torch.full((batch, seq), -100, dtype=torch.long)
    labels[:, :-1] = ids[:, 1:]
    labels[torch.arange(seq)[None, :] >= lens[:, None] - 1] = -100
    labels = labels.reshape(-1).to(device)
    if min_len is None:
        return (ids.to(device),), labels
    return (ids.to(device), lens.to(torch.int32).to(device)), labels
