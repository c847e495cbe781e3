"""BERT-base (12 layers, hidden 768, 12 heads, FFN 3072) with the masked-LM head, for BASELINE.json
config 4 (BERT-base with the Adam update kernel). Random init, synthetic token batches.

Every Linear is an ``MfmaLinear`` (hand-written gfx950 MFMA GEMM forward + both backward GEMMs,
bias/GELU fused); attention is the fused gfx950 kernel of ``ops/attention.py`` (SDPA off-GPU).
Deviations from the original BERT, both standard in large-scale training and stated here: the
vocabulary is padded to 30528 (a multiple of 64, for the GEMM tiles) and the MLM decoder weight is
untied from the word embedding (the PS data plane overlaps each bucket's update with the rest of
backward, which requires every weight to be consumed by exactly one autograd node).
"""
from __future__ import annotations


import torch
import torch.nn as nn

from ..ops.attention import FusedSelfAttention
from ..ops.embedding import FusedBertEmbeddings
from ..ops.layernorm import FusedAddLayerNorm, bump_step
from ..ops.linear import MfmaLinear
from ..ops.loss import cross_entropy

VOCAB = 30528


class BertLayer(nn.Module):
    def __init__(self, hidden=768, heads=12, ffn=3072, dropout=0.1, index=0, causal=False, fp8=False, window=None,
                 rope=None):
        super().__init__()
        # rope: (max_pos, base) -- rotary position embedding of Q and K between the QKV Linear and the
        # attention (ops/rope.py); None: no such module, the path below is untouched
        self.rot = None
        if rope is not None:
            from ..ops.rope import RotaryQK

            self.rot = RotaryQK(heads, int(rope[0]), float(rope[1]))
        self.heads = heads
        # fp8: the four Linears run the MX fp8 recipe of ops/linear.py (fp8 forward and bwd-data, bf16
        # weight gradient); each LayerNorm writes the MX input of the Linear that reads its output
        # (ln1 -> ffn1 here, ln2 -> the next layer's qkv: wire_fp8_handover)
        f8 = "mx" if fp8 else False
        self.fp8 = bool(fp8)
        self.qkv = MfmaLinear(hidden, 3 * hidden, fp8=f8)
        # packed QKV in, [B, S, hidden] out: one fused kernel per direction (ops/attention.py)
        # window (causal only): sliding-window attention over the last `window` keys (ops/attention.py)
        self.attn = FusedSelfAttention(heads, p=dropout, seed=1000 + index, causal=causal, window=window)
        self.proj = MfmaLinear(hidden, hidden, fp8=f8)
        # LayerNorm(x + dropout(branch)) as one fused kernel family (ops/layernorm.py)
        self.ln1 = FusedAddLayerNorm(hidden, eps=1e-12, p=dropout, seed=2 * index + 1)
        self.ffn1 = MfmaLinear(hidden, ffn, act="gelu", fp8=f8)
        self.ffn2 = MfmaLinear(ffn, hidden, fp8=f8)
        # ffn1's output feeds only ffn2: ffn2's bwd-data GEMM applies the GELU backward and sums
        # ffn1's bias gradient in its epilogue (ops/linear.py)
        self.ffn2.psd_gelu_input_from(self.ffn1)
        self.ln2 = FusedAddLayerNorm(hidden, eps=1e-12, p=dropout, seed=2 * index + 2)
        if fp8:
            self.ln1.psd_mx_output_to(self.ffn1)
        self.p = dropout

    def forward(self, x, lens=None, doc_start=None):
        # each residual LayerNorm hands the gradient of its x input to the Linear that also reads x
        # (folded into that Linear's bwd-data GEMM, ops/layernorm.py)
        # doc_start: packed documents (ops/attention.py), passed on to the attention
        qkv = self.qkv(x)
        if self.rot is not None:  # rotated in place on the GPU; the QKV Linear then sums its own bias gradient
            qkv = self.rot(qkv, lens, doc_start)
        x = self.ln1(x, self.proj(self.attn(qkv, lens, doc_start)), x_grad_to=self.qkv)
        return self.ln2(x, self.ffn2(self.ffn1(x)), x_grad_to=self.ffn1)


def wire_fp8_handover(layers) -> None:
    """ln2 of each fp8 block writes the MX input of the next block's qkv (the last block's ln2 feeds a
    bf16 head: no hand-over)."""
    for prev, nxt in zip(layers, list(layers)[1:]):
        if prev.fp8 and nxt.fp8:
            prev.ln2.psd_mx_output_to(nxt.qkv)


class BertForMLM(nn.Module):
    def __init__(self, layers=12, hidden=768, heads=12, vocab=VOCAB, max_pos=512, dropout=0.1, fp8=False):
        super().__init__()
        self.vocab = vocab
        # dropout(LayerNorm(word + position + token type)) on one fused kernel each way, with the
        # word table's deterministic sorted-scatter gradient (ops/embedding.py)
        self.emb = FusedBertEmbeddings(vocab, hidden, max_pos, 2, eps=1e-12, p=dropout, seed=4242)
        # fp8: MX fp8 qkv / proj / ffn1 / ffn2 in every layer; the MLM head, the decoder and the
        # embeddings stay bf16
        self.layers = nn.ModuleList([BertLayer(hidden, heads, 4 * hidden, dropout, i, fp8=fp8) for i in range(layers)])
        wire_fp8_handover(self.layers)
        self.head = MfmaLinear(hidden, hidden, act="gelu")
        self.head_ln = nn.LayerNorm(hidden, eps=1e-12)
        self.decoder = MfmaLinear(hidden, vocab)
        self.p = dropout
        # device step counter for the fused LayerNorms' dropout masks (ops/layernorm.py)
        self.register_buffer("_psd_rng_step", torch.zeros(1, dtype=torch.int64), persistent=False)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)
            elif isinstance(m, nn.Embedding):
                nn.init.normal_(m.weight, std=0.02)

    def forward(self, batch):
        # (ids, types, mlm_pos) or, for a padded batch, (ids, types, mlm_pos, lens): int32 [B] lengths,
        # positions >= lens[b] are padding that no attention key or query row reads
        ids, types, mlm_pos = batch[:3]
        lens = batch[3] if len(batch) > 3 else None
        bump_step(self)
        x = self.emb(ids, types)
        for layer in self.layers:
            x = layer(x, lens)
        # MLM head only on the masked positions (max_predictions_per_seq per sequence, as in the
        # original BERT pre-training): 6-7x less head/decoder/softmax work than all tokens
        x = x.reshape(-1, x.shape[-1]).index_select(0, mlm_pos)
        return self.decoder(self.head_ln(self.head(x)))

    @staticmethod
    def loss(logits, labels):
        return cross_entropy(logits, labels)  # fused bf16 softmax-CE kernels (ops/loss.py)


def bert_batch(batch: int, seq: int, vocab: int, device, seed: int = 0, mask_prob: float = 0.15,
               min_len: int | None = None):
    """Synthetic pre-training batch: random ids, sentence-B types for the second half, and
    round(mask_prob * seq) masked positions per sequence (flat indices) with their labels.

    With ``min_len`` the sequences are padded: lengths are uniform in [min_len, seq], ids past a
    length are 0, the masked positions are drawn among the valid ones, and the batch tuple gains
    ``lens`` (int32 [B]). The prediction count per sequence stays round(mask_prob * seq) (the
    original BERT's max_predictions_per_seq): surplus slots point at position 0 with label -100,
    which the loss ignores."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, vocab, (batch, seq), generator=g)
    types = (torch.arange(seq)[None, :] >= seq // 2).long().expand(batch, seq).contiguous()
    npred = max(1, round(mask_prob * seq))
    if min_len is None:
        cols = torch.stack([torch.randperm(seq, generator=g)[:npred].sort().values for _ in range(batch)])
        flat = (cols + torch.arange(batch)[:, None] * seq).reshape(-1)
        labels = ids.reshape(-1)[flat]
        return (ids.to(device), types.to(device), flat.to(device)), labels.to(device)
    if not 1 <= int(min_len) <= seq:
        raise ValueError(f"min_len must be in [1, {seq}], got {min_len}")
    lens = torch.randint(int(min_len), seq + 1, (batch,), generator=g)
    ids = ids * (torch.arange(seq)[None, :] < lens[:, None])
    cols = torch.zeros(batch, npred, dtype=torch.long)
    used = torch.zeros(batch, npred, dtype=torch.bool)
    for b in range(batch):
        c = torch.randperm(int(lens[b]), generator=g)[:npred].sort().values
        cols[b, :c.numel()] = c
        used[b, :c.numel()] = True
    flat = (cols + torch.arange(batch)[:, None] * seq).reshape(-1)
    labels = torch.where(used.reshape(-1), ids.reshape(-1)[flat], torch.full_like(flat, -100))
    return (ids.to(device), types.to(device), flat.to(device), lens.to(torch.int32).to(device)), labels.to(device)
