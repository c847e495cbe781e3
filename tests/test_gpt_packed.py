"""Packed documents in the decoder LM (models/gpt.py): ``(ids, lens, doc_start)`` batches, position ids that
restart at each document (``FusedBertEmbeddings(pos_ids=...)``, kernels/layernorm.hip emb_ln_*) and labels
that never cross a boundary. The model-level statement: a packed row trains exactly like its documents
as separate padded rows."""
import math

import pytest
import torch

TINY = dict(layers=2, hidden=128, heads=2, vocab=256)


def test_gpt_batch_packs_documents():
    from parameter_server_distributed_amd.models.gpt import gpt_batch
    from parameter_server_distributed_amd.ops.attention import check_doc_start

    B, S, V = 5, 64, 50
    (ids, lens, doc), labels = gpt_batch(B, S, V, torch.device("cpu"), seed=3, docs=(3, 20))
    assert ids.shape == (B, S) and doc.shape == (B, S) and doc.dtype == torch.int32
    assert lens.dtype == torch.int32 and lens.tolist() == [S] * B
    check_doc_start(doc)
    labels = labels.view(B, S)
    first = torch.ones(B, S, dtype=torch.bool)
    first[:, 1:] = doc[:, 1:] != doc[:, :-1]
    last = torch.ones(B, S, dtype=torch.bool)
    last[:, :-1] = first[:, 1:]
    assert (labels[last] == -100).all()  # every document's last position, the row's last one included
    assert torch.equal(labels[:, :-1][~last[:, :-1]], ids[:, 1:][~last[:, :-1]])  # inside: the next token
    for b in range(B):  # document lengths in [lo, hi], the last one cut at S
        starts = first[b].nonzero().flatten().tolist() + [S]
        n = [e - s for s, e in zip(starts[:-1], starts[1:])]
        assert all(3 <= v <= 20 for v in n[:-1]) and 1 <= n[-1] <= 20 and len(n) > 1
    (ids2, lens2, doc2), labels2 = gpt_batch(B, S, V, torch.device("cpu"), seed=3, docs=(3, 20))
    assert torch.equal(ids, ids2) and torch.equal(doc, doc2) and torch.equal(labels.view(-1), labels2)
    (_, _, doc3), _ = gpt_batch(B, S, V, torch.device("cpu"), seed=4, docs=(3, 20))
    assert not torch.equal(doc, doc3)
    with pytest.raises(ValueError):
        gpt_batch(B, S, V, torch.device("cpu"), docs=(3, 20), min_len=5)
    with pytest.raises(ValueError):
        gpt_batch(B, S, V, torch.device("cpu"), docs=(0, 20))


def test_packed_row_trains_like_its_documents_as_padded_rows():
    """One packed row of three documents: the same summed token loss and parameter gradients as the three
    documents as three padded rows with ``lens`` (fp32 on the CPU, dropout 0)."""
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM
    from parameter_server_distributed_amd.ops.attention import doc_starts

    torch.manual_seed(0)
    S, n = 24, [7, 12, 5]
    m = GPTForLM(**TINY, max_pos=S, dropout=0.0)
    g = torch.Generator(device="cpu").manual_seed(1)
    ids = torch.randint(0, TINY["vocab"], (1, S), generator=g)
    doc = doc_starts([n], S)
    labels = torch.full((1, S), -100, dtype=torch.long)
    padded = torch.zeros(3, S, dtype=torch.long)
    plabels = torch.full((3, S), -100, dtype=torch.long)
    t = 0
    for i, k in enumerate(n):
        labels[0, t:t + k - 1] = ids[0, t + 1:t + k]
        padded[i, :k] = ids[0, t:t + k]
        plabels[i, :k - 1] = ids[0, t + 1:t + k]
        t += k
    count = int((labels >= 0).sum())
    assert count == sum(n) - 3 == int((plabels >= 0).sum())

    def grads(batch, lab):
        m.zero_grad(set_to_none=True)
        loss = m.loss(m(batch), lab.reshape(-1)) * count  # the summed token loss
        loss.backward()
        return loss.item(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}

    la, ga = grads((ids, torch.tensor([S], dtype=torch.int32), doc), labels)
    lb, gb = grads((padded, torch.tensor(n, dtype=torch.int32)), plabels)
    assert math.isfinite(la) and abs(la - lb) <= 1e-4 * abs(lb), (la, lb)
    assert ga.keys() == gb.keys() and len(ga) > 10
    for k in ga:
        assert (ga[k] - gb[k]).norm().item() <= 1e-4 * gb[k].norm().item() + 1e-12, k
    # and not like the row read as one document
    lc, _ = grads((ids,), labels)
    assert abs(lc - la) > 1e-3 * abs(la)

    spec = models.build("gpt_small", torch.device("cpu"), torch.float32, seq_len=32, pack_docs=(4, 12), **TINY)
    x, y = spec.make_batch(2, torch.device("cpu"))
    assert len(x) == 3 and x[2].shape == (2, 32)
    assert math.isfinite(spec.loss(spec.model(x), y).item())


# ------------------------------------------------------------------------------------------ GPU


@pytest.mark.gpu
def test_bert_embeddings_pos_ids_match_fp32(gpu):
    import torch.nn.functional as F

    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops import embedding
    from parameter_server_distributed_amd.ops.attention import doc_starts
    from parameter_server_distributed_amd.ops.embedding import FusedBertEmbeddings

    from test_layernorm import _mask

    torch.manual_seed(1)
    V, H, B, S, p = 1000, 768, 2, 64, 0.1
    assert V > embedding.SMALL_VOCAB
    emb = FusedBertEmbeddings(V, H, max_pos=64, p=p, seed=11).to(gpu)
    with torch.no_grad():
        for t in (emb.word.weight, emb.pos.weight, emb.tok_type.weight):
            t.normal_(0, 0.5)
        emb.ln.weight.uniform_(0.5, 1.5)
        emb.ln.bias.uniform_(-0.5, 0.5)
    emb.to(torch.bfloat16)
    step = torch.tensor([5], device=gpu, dtype=torch.int64)
    emb.step = step
    ids = torch.randint(0, V, (B, S), device=gpu)
    types = torch.randint(0, 2, (B, S), device=gpu)
    doc = doc_starts([[37, 1, 26]] * B, S, gpu)  # positions restart at 0, 37 and 38
    pos = torch.arange(S, device=gpu)[None, :] - doc.long()
    params = (emb.word.weight, emb.pos.weight, emb.tok_type.weight, emb.ln.weight, emb.ln.bias)
    calls = []
    orig = embedding._BertEmbLNFn.apply
    embedding._BertEmbLNFn.apply = lambda *a: calls.append(1) or orig(*a)
    try:
        y = emb(ids, types, pos)
    finally:
        embedding._BertEmbLNFn.apply = orig
    assert calls  # the fused kernels
    g = torch.randn(B, S, H, device=gpu).to(torch.bfloat16)
    y.backward(g)
    got = (y,) + tuple(t.grad.clone() for t in params)

    mask = _mask(native(), (B, S, H), p, 11, step, gpu)
    leaves = [t.detach().float().requires_grad_(True) for t in params]
    w, pt, tt, gm, bt = leaves
    x = F.embedding(ids, w) + F.embedding(pos, pt) + F.embedding(types, tt)
    yr = F.layer_norm(x, (H,), gm, bt, emb.ln.eps) * mask / (1 - p)
    yr.backward(g.float())
    for name, a, b in zip(("y", "word", "pos", "type", "gamma", "beta"), got, (yr,) + tuple(t.grad for t in leaves)):
        rel = ((a.float() - b).norm() / b.norm()).item()
        assert rel < 2e-2, (name, rel)
    assert got[2][37:].abs().sum().item() == 0  # no token has a position past the longest document

    def again(*pos_arg):
        for t in params:
            t.grad = None
        out = emb(ids, types, *pos_arg)
        out.backward(g)
        return (out,) + tuple(t.grad.clone() for t in params)

    assert all(torch.equal(a, b) for a, b in zip(again(pos), got))  # deterministic, the position scatter too
    ar = torch.arange(S, device=gpu)[None, :].expand(B, S).contiguous()
    plain = again()
    # (the position gradient too: the sorted scatter and the batch sum both round one fp32 sum of B = 2 rows)
    for name, a, b in zip(("y", "word", "pos", "type", "gamma", "beta"), again(ar), plain):
        assert torch.equal(a, b), name


@pytest.mark.gpu
def test_packed_gpt_step_on_the_kernels_matches_the_sdpa_path(gpu, monkeypatch):
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops import attention

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, layers=2, seq_len=256, pack_docs=(16, 96))
    m = spec.model
    for t in m.parameters():  # bf16 working weights, as the PS data planes give them
        t.data = t.data.to(torch.bfloat16)
    for mod in m.modules():  # dropout 0: the two paths draw different masks
        if isinstance(getattr(mod, "p", None), float):
            mod.p = 0.0
    x, y = spec.make_batch(4, gpu, seed=1)
    assert len(x) == 3 and x[2].dtype == torch.int32 and x[2].shape == (4, 256)
    probe = torch.empty(4, 256, 3 * 768, device=gpu, dtype=torch.bfloat16)
    assert m.layers[0].attn.causal and m.layers[0].attn._long_kernel_ok(probe)

    def run():
        calls = []
        orig = attention._AttnFn.apply
        attention._AttnFn.apply = lambda *a: calls.append(a[-1]) or orig(*a)
        try:
            m.zero_grad(set_to_none=True)
            logits = m(x)
            loss = spec.loss(logits, y)
            loss.backward()
        finally:
            attention._AttnFn.apply = orig
        return loss.float().item(), logits.detach().float(), calls

    la, logits, calls = run()
    assert len(calls) == 2 and all(c is x[2] for c in calls)  # both layers on the document kernels
    assert math.isfinite(la)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    assert not m.layers[0].attn._long_kernel_ok(probe)
    lb, logits_b, calls = run()
    assert not calls  # SDPA with the boolean mask
    monkeypatch.setenv("PSD_FEATURES", "")
    ulp = 2.0 ** (math.floor(math.log2(logits.abs().max().item())) - 7)  # one bf16 ulp at max|logit| (tests/test_gpt.py)
    print(f"loss kernels {la:.5f}, sdpa {lb:.5f}, ulp {ulp:.5f}")
    assert abs(la - lb) <= ulp, (la, lb, ulp)
