"""Packed documents in causal self-attention (``doc_start``; ops/attention.py, the DOCS copies of
kernels/attention.hip and attention_long.hip): query q sees key k iff both are of one document, k <= q
and k < the sequence's length.

The yardstick is the fp32 composite below: the ``_ref`` / ``_ref_lse`` of tests/test_attention_causal.py
with the same-document test applied to the valid rows, on the same input generators. Tolerances are the
project's own for these kernels: output and lse 2e-2, gradients 3e-2. A case whose gradient exceeds
3e-2 is allowed twice what the bf16 SDPA path measures with the same mask on the same inputs against
the same composite (_GRAD_TOL, profiles/attn_docs.md), never a figure taken from the kernels."""
import math

import pytest
import torch

from test_attention_causal import _assert_pad_zero, _documented_mask, _dout, _qkv, _valid


def _rows(docs, S):
    """Document lengths laid end to end and cut at S (a layout written for S = 128 also serves S = 64)."""
    out, t = [], 0
    for n in docs:
        if t >= S:
            break
        out.append(min(n, S - t))
        t += out[-1]
    return out


def _doc(docs, S, B, dev=None):
    from parameter_server_distributed_amd.ops.attention import doc_starts

    return doc_starts([_rows(docs, S)] * B, S, dev)


def _visible(qkv, lens, doc, causal=True):
    """[B, 1, q, key]: key < L, key <= q under the causal mask, and for a valid query the same document."""
    B, S, _ = qkv.shape
    valid = _valid(lens, S)
    vis = valid[:, None, None, :].expand(B, 1, S, S)
    if causal:
        vis = vis & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
    if doc is not None:
        vis = vis & ((doc[:, None, :, None] == doc[:, None, None, :]) | ~valid[:, None, :, None])
    return vis


def _ref(qkv, heads, lens=None, doc=None, mask=None, p=0.0, causal=True):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
    q, k, v = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    vis = _visible(qkv, lens, doc, causal)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~vis, float("-inf"))
    empty = (lens.clamp(0, S) == 0)[:, None, None, None]
    a = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * vis
    if mask is not None:
        a = a * mask / (1.0 - p)
    o = (a @ v) * valid[:, None, :, None]
    return o.transpose(1, 2).reshape(B, S, E // 3)


def _ref_lse(qkv, heads, lens=None, doc=None):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
    q, k, _ = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~_visible(qkv, lens, doc), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return torch.where(valid[:, None, :], lse, torch.zeros_like(lse))


# ------------------------------------------------------------------------------------------ CPU


def test_doc_starts_round_trip_and_malformed_rows_are_rejected():
    from parameter_server_distributed_amd.ops.attention import check_doc_start, doc_starts

    t = doc_starts([[5, 1, 20, 22], [48], [3, 4]], 48)
    assert t.dtype == torch.int32 and t.shape == (3, 48)
    assert t[0].tolist() == [0] * 5 + [5] + [6] * 20 + [26] * 22
    assert t[1].tolist() == [0] * 48
    assert t[2].tolist() == [0] * 3 + [3] * 4 + list(range(7, 48))  # the remainder: its own index
    check_doc_start(t)
    check_doc_start(torch.zeros(2, 8, dtype=torch.int32))
    for bad in ([0, 0, 2, 1], [0, 2, 2, 2], [-1, 0, 0, 0], [0, 0, 1, 1]):  # order, > t, < 0, not its own start
        with pytest.raises(ValueError):
            check_doc_start(torch.tensor([bad], dtype=torch.int32))
    with pytest.raises(ValueError):
        check_doc_start(torch.zeros(2, 8, dtype=torch.int64))
    with pytest.raises(ValueError):
        check_doc_start(torch.zeros(8, dtype=torch.int32))
    for bad in ([[0]], [[40, 9]]):
        with pytest.raises(ValueError):
            doc_starts(bad, 48)


def test_docs_cpu_module_matches_the_composite():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(0)
    H, S = 2, 48
    docs = [5, 1, 20, 22]
    qkv = torch.randn(4, S, 3 * H * 64)
    doc = _doc(docs, S, 4)
    m = FusedSelfAttention(H, p=0.0, causal=True).eval()
    torch.testing.assert_close(m(qkv, None, doc), _ref(qkv, H, None, doc), atol=1e-5, rtol=1e-5)
    assert not torch.allclose(m(qkv, None, doc), m(qkv), atol=1e-3)
    lens = torch.tensor([S, 17, 0, 1], dtype=torch.int32)
    out = m(qkv, lens, doc)
    torch.testing.assert_close(out, _ref(qkv, H, lens, doc), atol=1e-5, rtol=1e-5)
    assert (out[~_valid(lens, S)] == 0).all()
    # entries past a length change nothing
    junk = doc.clone()
    junk[~_valid(lens, S)] = 10**6
    assert torch.equal(m(qkv, lens, junk), out)
    # all zeros: one document per row
    torch.testing.assert_close(m(qkv, lens, torch.zeros_like(doc)), m(qkv, lens), atol=1e-6, rtol=1e-6)


def test_docs_cpu_packed_row_is_each_document_alone():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(1)
    H, S = 2, 48
    docs = [5, 1, 20, 22]
    qkv = torch.randn(2, S, 3 * H * 64)
    m = FusedSelfAttention(H, p=0.0, causal=True).eval()
    out = m(qkv, None, _doc(docs, S, 2))
    t = 0
    for n in docs:
        torch.testing.assert_close(out[:, t:t + n], m(qkv[:, t:t + n].contiguous()), atol=1e-5, rtol=1e-5)
        t += n


def test_docs_without_causal_raise_in_the_native_op_and_take_sdpa_in_the_module():
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(2)
    H, S = 2, 64
    qkv = torch.randn(2, S, 3 * H * 64)
    doc = _doc([37, 1, 26], S, 2)
    x = qkv.to(torch.bfloat16)
    with pytest.raises(RuntimeError, match="doc_start"):
        native().attn_fwd(x, H, 0.0, 1, None, None, 0, False, doc)
    with pytest.raises(RuntimeError, match="doc_start"):
        native().attn_bwd(x[:, :, :H * 64].contiguous(), x, x[:, :, :H * 64].contiguous(), torch.zeros(2, H, S),
                          H, 0.0, 1, None, None, None, 0, False, doc)
    b = FusedSelfAttention(H, p=0.0).eval()
    lens = torch.tensor([S, 40], dtype=torch.int32)
    for ln in (None, lens):
        torch.testing.assert_close(b(qkv, ln, doc), _ref(qkv, H, ln, doc, causal=False), atol=1e-5, rtol=1e-5)
    assert not torch.allclose(b(qkv, None, doc), b(qkv), atol=1e-3)


def test_bert_embeddings_pos_ids_cpu_composite():
    import torch.nn.functional as F

    from parameter_server_distributed_amd.ops.embedding import FusedBertEmbeddings

    torch.manual_seed(0)
    emb = FusedBertEmbeddings(100, 32, max_pos=16, p=0.0)
    ids = torch.randint(0, 100, (3, 9))
    types = torch.randint(0, 2, (3, 9))
    pos = torch.tensor([[0, 1, 2, 0, 1, 2, 3, 0, 1]] * 3)
    y = emb(ids, types, pos)
    x = emb.word.weight[ids] + emb.pos.weight[pos] + emb.tok_type.weight[types]
    torch.testing.assert_close(y, F.layer_norm(x, (32,), emb.ln.weight, emb.ln.bias, emb.ln.eps))
    y.sum().backward()
    assert emb.pos.weight.grad[4:].abs().sum() == 0 and emb.pos.weight.grad[:4].abs().sum() > 0
    assert torch.equal(emb(ids, types, torch.arange(9)[None].expand(3, 9).contiguous()), emb(ids, types))


# ------------------------------------------------------------------------------------------ GPU


def _run(C, qkv, do, H, lens, doc, p=0.0, seed=11, step=None, grid_cap=0, bias=None):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap, True, doc)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, bias, lens, grid_cap, True, doc)
    return o, lse, dqkv


def _takes_a_kernel(m, qkv):
    return m._kernel_ok(qkv) or m._long_kernel_ok(qkv)


# The layouts: the smallest places the kernels can go wrong.
#   whole head  boundaries off the 32-grid with a one-token document; boundaries on the grid (whole-block skips only)
#   S = 192     the last tile has 64 queries: waves 2, 3 without rows
#   S = 256     a document that starts mid-chunk (70: lanes of a computing wave that see no key) and one that
#               starts one past a tile boundary (129)
#   S = 512     one tile whose waves begin their chunk walk at different chunks
_LAYOUTS = [
    (64, [37, 1, 62, 28]), (128, [37, 1, 62, 28]),
    (64, [32, 32, 64]), (128, [32, 32, 64]),
    (192, [70, 59, 63]),
    (256, [70, 59, 71, 56]),
    (512, [5, 395, 112]),
]
_IDS = [f"S{s}-{'_'.join(map(str, d))}" for s, d in _LAYOUTS]

# (S, first document, with lengths) -> gradient tolerance: twice the bf16 SDPA path's measured error with the
# same mask on the same inputs (module docstring); every other case keeps 3e-2
# S = 128, [37, 1, 62, 28], with lengths: two elements of dQ in row 48 of the full-length sequence (the 11th
# token of the document that starts at 38) measures 0.0333; the bf16 SDPA path measures 0.0186 there
_GRAD_TOL = {(128, 37, True): 2 * 0.0186}


def _check_vs_fp32(gpu, S, docs, lens_t, seed):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention, check_doc_start

    B, H = 4, 2
    doc = _doc(docs, S, B, gpu)
    check_doc_start(doc)
    qkv = _qkv(B, S, H, gpu, seed).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    assert _takes_a_kernel(m, qkv)
    o = m(qkv, lens_t, doc)
    g = _dout(B, S, H, gpu, seed)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t, doc)
    orf.backward(g.float())
    print(f"S {S} docs {docs} lens {lens_t is not None}: max|dO| {(o.float() - orf).abs().max().item():.4f}, "
          f"max|ddQKV| {(qkv.grad.float() - qr.grad).abs().max().item():.4f} of {qr.grad.abs().max().item():.2f}")
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    gtol = _GRAD_TOL.get((S, docs[0], lens_t is not None), 3e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=gtol, rtol=gtol)
    o2, lse, dqkv = _run(native(), qkv.detach(), g, H, lens_t, doc)
    assert torch.equal(o2, o.detach()) and torch.equal(dqkv, qkv.grad)
    torch.testing.assert_close(lse, _ref_lse(qkv.detach().float(), H, lens_t, doc), atol=2e-2, rtol=2e-2)
    # and not the plain causal result
    assert not torch.equal(o2, native().attn_fwd(qkv.detach(), H, 0.0, 11, None, lens_t, 0, True)[0])
    return qkv.detach(), g, doc, o2, lse, dqkv


@pytest.mark.gpu
@pytest.mark.parametrize("S,docs", _LAYOUTS, ids=_IDS)
def test_docs_attention_matches_fp32(gpu, S, docs):
    _check_vs_fp32(gpu, S, docs, None, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("S,docs", _LAYOUTS, ids=_IDS)
def test_docs_varlen_matches_fp32_and_entries_past_a_length_are_not_read(gpu, C, S, docs):
    H = 2
    lens_t = torch.tensor([S - 23, 0, 1, S], device=gpu, dtype=torch.int32)  # S - 23 cuts a document
    qkv, g, doc, o, lse, dqkv = _check_vs_fp32(gpu, S, docs, lens_t, 2)
    _assert_pad_zero(lens_t, S, o, lse, dqkv)
    pad = ~_valid(lens_t, S)
    for junk_v in (10**6, -5):
        junk = doc.clone()
        junk[pad] = junk_v
        for p in (0.0, 0.1):
            step = torch.tensor([5], device=gpu, dtype=torch.int64)
            for a, b in zip(_run(C, qkv, g, H, lens_t, junk, p, step=step), _run(C, qkv, g, H, lens_t, doc, p, step=step)):
                assert torch.equal(a, b), (junk_v, p)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [128, 256])
def test_docs_every_token_its_own_document_is_exact(gpu, C, S):
    B, H = 2, 2
    qkv = _qkv(B, S, H, gpu, 3)
    do = _dout(B, S, H, gpu, 3)
    doc = torch.arange(S, device=gpu, dtype=torch.int32).repeat(B, 1)
    o, lse, dqkv = _run(C, qkv, do, H, None, doc)
    q5 = qkv.view(B, S, 3, H, 64)
    assert torch.equal(o.view(B, S, H, 64), q5[:, :, 2])
    assert torch.equal(dqkv.view(B, S, 3, H, 64)[:, :, 2], do.view(B, S, H, 64))
    sqq = (q5[:, :, 0].float() * q5[:, :, 1].float()).sum(-1) / 8.0  # [B, S, H]
    torch.testing.assert_close(lse, sqq.permute(0, 2, 1).contiguous(), atol=2e-2, rtol=2e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [128, 256])
def test_docs_all_zero_is_bitwise_the_causal_call(gpu, C, S, p):
    """Contract (b), bias partials included."""
    B, H = 4, 2
    qkv = _qkv(B, S, H, gpu, 4)
    do = _dout(B, S, H, gpu, 4)
    zero = torch.zeros(B, S, device=gpu, dtype=torch.int32)
    step = torch.tensor([7], device=gpu, dtype=torch.int64)
    for lens in (None, torch.tensor([S, S - 23, 0, 33], device=gpu, dtype=torch.int32)):
        ba, bb = (torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(2))
        o, lse = C.attn_fwd(qkv, H, p, 11, step, lens, 0, True)
        dqkv = C.attn_bwd(do, qkv, o, lse, H, p, 11, step, ba, lens, 0, True)
        got = _run(C, qkv, do, H, lens, zero, p, step=step, bias=bb)
        for a, b in zip(got + (bb,), (o, lse, dqkv, ba)):
            assert torch.equal(a, b)
        assert ba.abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("S,docs,k", [(128, [37, 1, 62, 28], 2), (256, [70, 59, 71, 56], 1)], ids=["S128", "S256"])
def test_docs_rows_do_not_depend_on_other_documents(gpu, C, S, docs, k):
    """Contract (a): other finite values in document k's rows of qkv and dO leave every other document's
    rows of O, lse and dQKV bit for bit."""
    B, H = 2, 2
    doc = _doc(docs, S, B, gpu)
    t0 = sum(docs[:k])
    t1 = t0 + docs[k]
    qkv = _qkv(B, S, H, gpu, 12)
    do = _dout(B, S, H, gpu, 12)
    q2, d2 = qkv.clone(), do.clone()
    q2[:, t0:t1] = _qkv(B, S, H, gpu, 13, scale=2.0)[:, t0:t1]
    d2[:, t0:t1] = _dout(B, S, H, gpu, 13)[:, t0:t1]
    keep = torch.ones(S, dtype=torch.bool, device=gpu)
    keep[t0:t1] = False
    lens_t = torch.tensor([S, S - 23], device=gpu, dtype=torch.int32)
    for lens in (None, lens_t):
        for p in (0.0, 0.1):
            step = torch.tensor([4], device=gpu, dtype=torch.int64)
            a = _run(C, qkv, do, H, lens, doc, p, step=step)
            b = _run(C, q2, d2, H, lens, doc, p, step=step)
            assert torch.equal(a[0][:, keep], b[0][:, keep])
            assert torch.equal(a[1][:, :, keep], b[1][:, :, keep])
            assert torch.equal(a[2][:, keep], b[2][:, keep])
            assert not torch.equal(a[0][:, ~keep], b[0][:, ~keep])  # the document itself did change
            assert all(torch.isfinite(t).all() for t in b)


@pytest.mark.gpu
@pytest.mark.parametrize("S,docs", [(128, [37, 1, 62, 28]), (256, [70, 59, 71, 56])], ids=["S128", "S256"])
def test_docs_dropout_is_the_documented_hash_over_the_visible_keys(gpu, C, S, docs):
    B, H, p, seed, stepv = 3, 2, 0.5, 11, 5
    step = torch.tensor([stepv], device=gpu, dtype=torch.int64)
    doc = _doc(docs, S, B, gpu)
    x = _qkv(B, S, H, gpu, 5, scale=0.5)
    g = _dout(B, S, H, gpu, 5)
    hashm = torch.from_numpy(_documented_mask(B, H, S, p, seed, stepv)).to(gpu)
    lens_t = torch.tensor([S, S // 2 + 5, 33], device=gpu, dtype=torch.int32)
    for lens in (None, lens_t):
        o, lse, dqkv = _run(C, x, g, H, lens, doc, p, seed=seed, step=step)
        xr = x.float().requires_grad_(True)
        orf = _ref(xr, H, lens, doc, hashm.float(), p)
        orf.backward(g.float())
        torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
        for a, b in zip(_run(C, x, g, H, lens, doc, p, seed=seed, step=step), (o, lse, dqkv)):
            assert torch.equal(a, b)
    _assert_pad_zero(lens_t, S, o, lse, dqkv)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S,docs", [(128, [37, 1, 62, 28]), (512, [5, 395, 112])], ids=["S128", "S512"])
def test_docs_results_do_not_depend_on_the_grid(gpu, C, S, docs, p):
    B, H = 4, 2
    doc = _doc(docs, S, B, gpu)
    lens_t = torch.tensor([S, S // 4 + 6, S - 31, 33], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 6)
    do = _dout(B, S, H, gpu, 6)
    step = torch.tensor([2], device=gpu, dtype=torch.int64)
    for lens in (lens_t, None):
        db = [torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(3)]
        want = _run(C, qkv, do, H, lens, doc, p, step=step, grid_cap=0, bias=db[0])
        for cap, out in zip((1, 3), db[1:]):
            for a, b in zip(_run(C, qkv, do, H, lens, doc, p, step=step, grid_cap=cap, bias=out), want):
                assert torch.equal(a, b), cap
            assert torch.equal(out, db[0])
    if p == 0.0:  # one workgroup walks every item: a stale read of the previous item's LDS would show here
        o, lse, dqkv = _run(C, qkv, do, H, lens_t, doc, grid_cap=1)
        xr = qkv.float().requires_grad_(True)
        orf = _ref(xr, H, lens_t, doc)
        orf.backward(do.float())
        torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)


@pytest.mark.gpu
@pytest.mark.parametrize("S,docs", [(128, [37, 1, 62, 28]), (256, [70, 59, 71, 56])], ids=["S128", "S256"])
def test_docs_bias_out_is_the_column_sum_of_dqkv(gpu, C, S, docs):
    H, B = 2, 4
    doc = _doc(docs, S, B, gpu)
    lens_t = torch.tensor([S, S - 23, 0, 33], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 7)
    do = _dout(B, S, H, gpu, 7)
    for p in (0.0, 0.1):
        step = torch.tensor([3], device=gpu, dtype=torch.int64)
        db = torch.empty(3 * H * 64, device=gpu, dtype=torch.float32)
        o, lse, dqkv = _run(C, qkv, do, H, lens_t, doc, p, step=step, bias=db)
        assert torch.equal(dqkv, _run(C, qkv, do, H, lens_t, doc, p, step=step)[2])
        want = dqkv.float().sum((0, 1))
        torch.testing.assert_close(db, want, rtol=1e-2, atol=1e-2 * float(want.abs().max()) + 1e-6)
        assert db.abs().max() > 0


@pytest.mark.gpu
def test_docs_routing_kernels_at_the_kernel_shapes_and_sdpa_elsewhere(gpu, C):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops import attention
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    B, H = 2, 2
    m = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    calls = []
    orig = attention._AttnFn.apply
    attention._AttnFn.apply = lambda *a: calls.append(a[-1]) or orig(*a)
    try:
        for S in (128, 256):
            doc = _doc([70, 59, 71, 56], S, B, gpu)
            qkv = _qkv(B, S, H, gpu, 8)
            assert _takes_a_kernel(m, qkv)
            o = m(qkv, None, doc)
            assert calls and calls[-1] is doc
            assert torch.equal(o, native().attn_fwd(qkv, H, 0.0, m.seed, None, None, 0, True, doc)[0])
        n = len(calls)
        S = 160
        doc = _doc([70, 59, 31], S, B, gpu)
        for lens_t in (None, torch.tensor([S, 75], device=gpu, dtype=torch.int32)):
            qkv = _qkv(B, S, H, gpu, 9).requires_grad_(True)
            assert not _takes_a_kernel(m, qkv)
            o = m(qkv, lens_t, doc)
            g = _dout(B, S, H, gpu, 9)
            o.backward(g)
            qr = qkv.detach().float().requires_grad_(True)
            orf = _ref(qr, H, lens_t, doc)
            orf.backward(g.float())
            torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
            torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
        assert len(calls) == n
    finally:
        attention._AttnFn.apply = orig
    # the kernels do not serve a bidirectional doc_start: the native op raises, the module takes SDPA
    qkv = _qkv(B, 128, H, gpu, 10)
    doc = _doc([37, 1, 62, 28], 128, B, gpu)
    with pytest.raises(RuntimeError, match="doc_start"):
        C.attn_fwd(qkv, H, 0.0, 1, None, None, 0, False, doc)
    b = FusedSelfAttention(H, p=0.0).to(gpu)
    torch.testing.assert_close(b(qkv, None, doc).float(), _ref(qkv.float(), H, None, doc, causal=False),
                               atol=2e-2, rtol=2e-2)
