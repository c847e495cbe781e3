"""Variable-length sequences in the fused self-attention (kernels/attention.hip, ops/attention.py) and
the BERT model: per-sequence lengths ``lens`` (int32 [B]), keys past a length get probability 0, rows
past it are exact zeros in O, lse and dQKV and are never read.

The fp32 yardstick is the composite ``_ref`` below; tolerances against it are those of
tests/test_attention.py for the same kernels (output 2e-2, gradients 3e-2)."""
import math

import pytest
import torch


def _valid(lens, S):
    return torch.arange(S, device=lens.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]


def _ref(qkv, heads, lens, mask=None, p=0.0):
    """fp32 attention from packed [B, S, 3*H*D] over keys < L only, output rows >= L zeroed; finite
    for L = 0 (a sequence without a valid key gets zero probabilities instead of softmax(-inf))."""
    B, S, E = qkv.shape
    D = E // (3 * heads)
    q, k, v = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    keym = valid[:, None, None, :]
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~keym, float("-inf"))
    empty = (lens.clamp(0, S) == 0)[:, None, None, None]
    a = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * keym
    if mask is not None:
        a = a * mask / (1.0 - p)
    o = (a @ v) * valid[:, None, :, None]
    return o.transpose(1, 2).reshape(B, S, E // 3)


def _ref_lse(qkv, heads, lens):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    q, k, _ = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~valid[:, None, None, :], float("-inf"))
    lse = torch.logsumexp(s, dim=-1)  # [B, H, S]
    return torch.where(valid[:, None, :], lse, torch.zeros_like(lse))


def _assert_pad_zero(lens, S, o, lse, dqkv):
    pad = ~_valid(lens, S)  # [B, S]
    assert (o[pad] == 0).all()
    assert (lse.transpose(1, 2)[pad] == 0).all()
    assert (dqkv[pad] == 0).all()  # q, k and v parts: the whole packed row


# ------------------------------------------------------------------------------------------ CPU


def test_varlen_cpu_fallback_matches_reference():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(0)
    lens = torch.tensor([16, 7, 0], dtype=torch.int32)
    qkv = torch.randn(3, 16, 3 * 2 * 8, requires_grad=True)
    m = FusedSelfAttention(2, p=0.1).eval()
    o = m(qkv, lens)
    g = torch.randn_like(o)
    o.backward(g)
    qr = qkv.detach().clone().requires_grad_(True)
    orf = _ref(qr, 2, lens)
    orf.backward(g)
    assert torch.isfinite(o).all() and torch.isfinite(qkv.grad).all()
    torch.testing.assert_close(o, orf, atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(qkv.grad, qr.grad, atol=1e-5, rtol=1e-5)
    pad = ~_valid(lens, 16)
    assert (o[pad] == 0).all() and (qkv.grad[pad] == 0).all()


def test_varlen_cpu_fallback_never_reads_padded_rows():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(1)
    lens = torch.tensor([16, 7, 0], dtype=torch.int32)
    qkv = torch.randn(3, 16, 3 * 2 * 8)
    bad = qkv.clone()
    bad[~_valid(lens, 16)] = float("nan")
    m = FusedSelfAttention(2, p=0.0).eval()
    assert torch.equal(m(bad, lens), m(qkv, lens))


def test_bert_batch_min_len():
    from parameter_server_distributed_amd.models.bert import bert_batch

    vocab, seq = 1000, 32
    (ids, types, pos, lens), labels = bert_batch(4, seq, vocab, "cpu", min_len=5)
    assert lens.dtype == torch.int32 and lens.shape == (4,)
    assert ((lens >= 5) & (lens <= seq)).all()
    valid = _valid(lens, seq)
    assert (ids[~valid] == 0).all()
    npred = round(0.15 * seq)
    assert pos.shape == labels.shape == (4 * npred,)  # max_predictions_per_seq slots per sequence
    seq_of = torch.arange(4).repeat_interleave(npred)
    assert (pos // seq == seq_of).all()
    real = labels >= 0
    assert real.any()
    assert valid.reshape(-1)[pos[real]].all()
    assert torch.equal(labels[real], ids.reshape(-1)[pos[real]])
    assert (labels[~real] == -100).all() and (pos[~real] % seq == 0).all()
    # short sequences: fewer valid positions than slots
    (ids, types, pos, lens), labels = bert_batch(6, seq, vocab, "cpu", seed=3, min_len=1)
    real = labels >= 0
    for b in range(6):
        n = int(real[b * npred:(b + 1) * npred].sum())
        assert n == min(npred, int(lens[b]))
        assert pos[b * npred:(b + 1) * npred][:n].unique().numel() == n
    with pytest.raises(ValueError):
        bert_batch(2, seq, vocab, "cpu", min_len=0)
    with pytest.raises(ValueError):
        bert_batch(2, seq, vocab, "cpu", min_len=seq + 1)


def test_bert_batch_without_min_len_is_unchanged():
    from parameter_server_distributed_amd.models.bert import bert_batch

    batch, seq, vocab, seed, mask_prob = 4, 32, 1000, 7, 0.15
    # the full-length formula as it was before lengths existed
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, vocab, (batch, seq), generator=g)
    types = (torch.arange(seq)[None, :] >= seq // 2).long().expand(batch, seq).contiguous()
    npred = max(1, round(mask_prob * seq))
    cols = torch.stack([torch.randperm(seq, generator=g)[:npred].sort().values for _ in range(batch)])
    flat = (cols + torch.arange(batch)[:, None] * seq).reshape(-1)
    labels = ids.reshape(-1)[flat]

    x, y = bert_batch(batch, seq, vocab, "cpu", seed)
    assert len(x) == 3
    for got, want in zip((*x, y), (ids, types, flat, labels)):
        assert got.dtype == want.dtype and torch.equal(got, want)
    x2, y2 = bert_batch(batch, seq, vocab, "cpu", seed, min_len=None)
    assert len(x2) == 3 and all(torch.equal(a, b) for a, b in zip((*x2, y2), (*x, y)))


def test_bert_cpu_variable_length_batch():
    from parameter_server_distributed_amd.models.bert import BertForMLM, bert_batch

    torch.manual_seed(2)
    vocab, seq = 512, 32
    model = BertForMLM(layers=2, hidden=128, heads=2, vocab=vocab, max_pos=64, dropout=0.0)
    (ids, types, pos, lens), labels = bert_batch(4, seq, vocab, "cpu", seed=1, min_len=5)
    assert (lens < seq).any()
    logits = model((ids, types, pos, lens))
    loss = model.loss(logits, labels)
    assert torch.isfinite(loss)
    loss.backward()
    grads = [p.grad for p in model.parameters() if p.grad is not None]
    assert grads and all(torch.isfinite(g).all() for g in grads)
    assert model.layers[0].qkv.weight.grad.abs().sum() > 0
    # other ids at the padded positions: no logit moves
    ids2 = ids.clone()
    pad = ~_valid(lens, seq)
    ids2[pad] = torch.randint(1, vocab, (int(pad.sum()),))
    with torch.no_grad():
        a = model((ids, types, pos, lens))
        b = model((ids2, types, pos, lens))
        c = model((ids2, types, pos))  # without lens the padding is attended to
    assert torch.equal(a, b)
    assert not torch.equal(a, c)


def test_model_zoo_passes_min_seq_len():
    from parameter_server_distributed_amd import models

    spec = models.build("bert_base", torch.device("cpu"), torch.float32, layers=1, hidden=64, heads=1, vocab=128,
                        seq_len=32, min_seq_len=4)
    x, y = spec.make_batch(3, "cpu")
    assert len(x) == 4 and x[3].dtype == torch.int32 and ((x[3] >= 4) & (x[3] <= 32)).all()
    spec = models.build("bert_base", torch.device("cpu"), torch.float32, layers=1, hidden=64, heads=1, vocab=128,
                        seq_len=32)
    assert len(spec.make_batch(3, "cpu")[0]) == 3


# ------------------------------------------------------------------------------------------ GPU


def _qkv(B, S, H, gpu, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16).to(gpu)


def _run(C, qkv, do, H, lens, p=0.0, seed=11, step=None, grid_cap=0):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, None, lens, grid_cap)
    return o, lse, dqkv


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("B,S,H", [(2, 128, 3), (3, 64, 2)])
def test_full_length_lens_is_the_full_length_kernel(gpu, C, B, S, H, p):
    qkv = _qkv(B, S, H, gpu, 1)
    do = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)
    step = torch.tensor([5], device=gpu, dtype=torch.int64)
    lens = torch.full((B,), S, device=gpu, dtype=torch.int32)
    want = _run(C, qkv, do, H, None, p, step=step)
    got = _run(C, qkv, do, H, lens, p, step=step)
    for a, b in zip(got, want):
        assert torch.equal(a, b)


_CASES = [
    (128, [128, 77, 1, 64]),
    (96, [5, 64, 96]),
    (64, [64, 33, 32]),
    (32, [32, 17, 1]),
    (64, [0, 200, -3]),  # clamps to [0, 64, 0]
]


@pytest.mark.gpu
@pytest.mark.parametrize("S,lens", _CASES, ids=[f"S{s}-{'_'.join(map(str, l))}" for s, l in _CASES])
def test_varlen_matches_fp32(gpu, S, lens):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    H, B = 2, len(lens)
    lens_t = torch.tensor(lens, device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 2).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0).to(gpu)
    assert m._kernel_ok(qkv)
    o = m(qkv, lens_t)
    g = torch.randn_like(o)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    # the raw op: lse over the valid keys, and exact zeros on every padded row
    from parameter_server_distributed_amd import native

    o2, lse, dqkv = _run(native(), qkv.detach(), g, H, lens_t)
    assert torch.equal(o2, o.detach()) and torch.equal(dqkv, qkv.grad)
    torch.testing.assert_close(lse, _ref_lse(qkv.detach().float(), H, lens_t), atol=2e-2, rtol=2e-2)
    _assert_pad_zero(lens_t, S, o2, lse, dqkv)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_padded_rows_are_never_read(gpu, C, p):
    S, H, lens = 128, 2, [128, 77, 1, 64, 0]
    B = len(lens)
    lens_t = torch.tensor(lens, device=gpu, dtype=torch.int32)
    pad = ~_valid(lens_t, S)
    qkv = _qkv(B, S, H, gpu, 3)
    do = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)
    qkv[pad] = 0
    do[pad] = 0
    step = torch.tensor([9], device=gpu, dtype=torch.int64)
    want = _run(C, qkv, do, H, lens_t, p, step=step)
    qn, dn = qkv.clone(), do.clone()
    qn[pad] = float("nan")
    dn[pad] = float("nan")
    o, lse = C.attn_fwd(qn, H, p, 11, step, lens_t)
    on = o.clone()
    on[pad] = float("nan")  # backward reads O too (D = rowsum(dO . O)): its padded rows as well
    dqkv = C.attn_bwd(dn, qn, on, lse, H, p, 11, step, None, lens_t)
    for a, b in zip((o, lse, dqkv), want):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_persistent_loop_leaves_no_stale_lds(gpu, C, reverse, p):
    """One or two workgroups walk all six items, a short one after a long one and the reverse: bitwise
    the results of one workgroup per item."""
    B, H, S = 3, 2, 128
    lens_t = torch.tensor([128, 40, 97], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 4)
    do = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)
    if reverse:
        qkv, do, lens_t = qkv.flip(0).contiguous(), do.flip(0).contiguous(), lens_t.flip(0).contiguous()
    step = torch.tensor([2], device=gpu, dtype=torch.int64)
    want = _run(C, qkv, do, H, lens_t, p, step=step, grid_cap=0)
    _assert_pad_zero(lens_t, S, *want)
    for cap in (1, 2):
        got = _run(C, qkv, do, H, lens_t, p, step=step, grid_cap=cap)
        for a, b in zip(got, want):
            assert torch.equal(a, b), cap
    # the same walk without lengths: grid_cap alone changes nothing either
    full = _run(C, qkv, do, H, None, p, step=step, grid_cap=0)
    for a, b in zip(_run(C, qkv, do, H, None, p, step=step, grid_cap=1), full):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_varlen_dropout_keeps_the_mask_bits(gpu, C):
    torch.manual_seed(5)
    B, S, H, D, p = 3, 64, 2, 64, 0.2
    lens_t = torch.tensor([64, 33, 17], device=gpu, dtype=torch.int32)
    step = torch.tensor([5], device=gpu, dtype=torch.int64)
    qkv = (torch.randn(B, S, 3, H, D, device=gpu) * 0.5).to(torch.bfloat16)
    # V = I per head: O = dropout(P), so the kernel reveals its own mask
    probe = qkv.clone()
    probe[:, :, 2] = torch.eye(S, D, device=gpu, dtype=torch.bfloat16)[None, :, None, :].expand(B, S, H, D)
    po, _ = C.attn_fwd(probe.view(B, S, -1), H, p, 11, step)
    pl, _ = C.attn_fwd(probe.view(B, S, -1), H, p, 11, step, lens_t)
    mask = (po.view(B, S, H, D).permute(0, 2, 1, 3) != 0)  # [B, H, q, key]
    mask_l = (pl.view(B, S, H, D).permute(0, 2, 1, 3) != 0)
    valid = _valid(lens_t, S)
    pair = (valid[:, None, :, None] & valid[:, None, None, :]).expand_as(mask)
    assert torch.equal(mask_l[pair], mask[pair])  # a length moves nobody's mask bits
    assert not mask_l[~pair].any()
    assert abs(mask[pair].float().mean().item() - (1 - p)) < 0.03

    x = qkv.view(B, S, -1).contiguous()
    g = torch.randn(B, S, H * D, device=gpu).to(torch.bfloat16)
    o, lse, dqkv = _run(C, x, g, H, lens_t, p, step=step)
    xr = x.float().requires_grad_(True)
    orf = _ref(xr, H, lens_t, mask.float(), p)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
    _assert_pad_zero(lens_t, S, o, lse, dqkv)


@pytest.mark.gpu
def test_qkv_bias_grad_hand_over_with_lens(gpu):
    """tests/test_attention.py's bias hand-over comparison on a padded batch: the padded rows of dQKV
    are zeros, so the column sums the attention backward hands over equal the Linear's own."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    torch.manual_seed(6)
    B, S, H = 4, 64, 2
    lens_t = torch.tensor([64, 33, 0, 17], device=gpu, dtype=torch.int32)
    lin = MfmaLinear(256, 3 * H * 64).to(gpu).to(torch.bfloat16)
    att = FusedSelfAttention(H, p=0.0).to(gpu)
    x0 = torch.randn(B, S, 256, device=gpu).to(torch.bfloat16)
    g = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)

    def run(hand):
        lin.weight.grad = lin.bias.grad = None
        x = x0.clone().requires_grad_(True)
        qkv = lin(x)
        if not hand:
            qkv = qkv * 1  # untagged: the Linear sums its own bias gradient
        att(qkv, lens_t).backward(g)
        return [t.float().clone() for t in (x.grad, lin.weight.grad, lin.bias.grad)]

    got, ref = run(True), run(False)
    assert lin._psd_bias_hand is None
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-2, atol=1e-2 * float(b.abs().max()) + 1e-6)
    assert got[2].abs().max() > 0


@pytest.mark.gpu
def test_graph_replay_sees_the_current_lens(gpu, C):
    B, S, H = 3, 64, 2
    qkv = _qkv(B, S, H, gpu, 7)
    do = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)
    lens_t = torch.tensor([64, 10, 33], device=gpu, dtype=torch.int32)
    first = _run(C, qkv, do, H, lens_t)  # eager once: code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _run(C, qkv, do, H, lens_t)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, first):
        assert torch.equal(a, b)
    lens_t.copy_(torch.tensor([5, 64, 0], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    want = _run(C, qkv, do, H, lens_t)
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], first[0])
    _assert_pad_zero(lens_t, S, *out)


@pytest.mark.gpu
def test_lens_argument_is_checked(gpu, C):
    qkv = _qkv(2, 32, 1, gpu, 8)
    for bad in (torch.tensor([32, 32], device=gpu),  # int64
                torch.tensor([32], device=gpu, dtype=torch.int32),  # numel != B
                torch.tensor([32, 32], dtype=torch.int32),  # host tensor
                torch.tensor([32, 1, 32, 1], device=gpu, dtype=torch.int32)[::2]):  # not contiguous
        with pytest.raises(RuntimeError):
            C.attn_fwd(qkv, 1, 0.0, 0, None, bad)


@pytest.mark.gpu
def test_trainer_captures_a_step_on_a_padded_bert_batch(gpu):
    """The trainer hands the batch tuple to the model whole, so the four-element padded batch goes
    through the eager and the captured step alike."""
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    torch.manual_seed(0)
    spec = models.build("bert_base", gpu, torch.bfloat16, layers=1, seq_len=64, min_seq_len=8)
    batch = spec.make_batch(4, gpu)
    assert len(batch[0]) == 4 and (batch[0][3] < 64).any()
    assert spec.model.layers[0].attn._kernel_ok(torch.empty(4, 64, 3 * 768, device=gpu, dtype=torch.bfloat16))
    ps = CollectivePS(spec.model, OptimConfig("adam", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    losses = [tr.step().float().item() for _ in range(5)]
    torch.cuda.synchronize()
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_long_sequences_take_the_masked_sdpa_path(gpu):
    """S > 128 stays on SDPA and gets the same length semantics there."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    B, S, H = 3, 160, 2
    lens_t = torch.tensor([160, 50, 0], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 9).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0).to(gpu)
    assert not m._kernel_ok(qkv)
    o = m(qkv, lens_t)
    g = torch.randn_like(o)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    pad = ~_valid(lens_t, S)
    assert (o[pad] == 0).all() and (qkv.grad[pad] == 0).all()
