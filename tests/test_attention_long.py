"""Streaming fused self-attention for S = 192 .. 512 (kernels/attention_long.hip, ops/attention.py):
the contracts of the whole-head kernels (tests/test_attention.py, tests/test_attention_varlen.py) at
the longer lengths -- fp32 match, ``lse``, ``lens``, the dropout hash, grid independence, the QKV-bias
hand-over, graph replay and the BERT step.

The yardsticks are the fp32 / fp64 composites below; tolerances are the project's own for these
kernels (output and lse 2e-2, gradients 3e-2). The forced-rescale test's gradient bound is
rtol 3e-2, atol 1e-2 * max|ref|: its 16x key rows put max|dQ| near 12, where bf16 rounding of P and dS
alone exceeds a plain 3e-2 (a bf16 emulation of the streaming numerics measured 0.06 against 0.12)."""
import math

import pytest
import torch


def _valid(lens, S):
    return torch.arange(S, device=lens.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]


def _ref(qkv, heads, lens=None, mask=None, p=0.0):
    """Attention in qkv's own precision from packed [B, S, 3*H*D] over keys < L only, output rows >= L
    zeroed; finite for L = 0."""
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
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


def _ref_lse(qkv, heads, lens=None):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
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


def test_long_kernel_shape_and_cpu_routing():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    ok = FusedSelfAttention.long_kernel_shape_ok
    assert [s for s in range(0, 1025, 32) if ok(s, 64)] == [192, 256, 320, 384, 448, 512]
    for s in (128, 160, 224, 576):
        assert not ok(s, 64)
    assert not ok(256, 32)
    torch.manual_seed(0)
    m = FusedSelfAttention(1, p=0.0).eval()
    qkv = torch.randn(2, 256, 3 * 64)
    assert not m._long_kernel_ok(qkv) and not m._kernel_ok(qkv)  # a CPU tensor never takes a kernel
    assert not m._long_kernel_ok(qkv.to(torch.bfloat16))
    lens = torch.tensor([256, 100], dtype=torch.int32)
    torch.testing.assert_close(m(qkv, lens), _ref(qkv, 1, lens), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(m(qkv), _ref(qkv, 1), atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------ GPU


def _qkv(B, S, H, gpu, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16).to(gpu)


def _dout(B, S, H, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16).to(gpu)


def _run(C, qkv, do, H, lens, p=0.0, seed=11, step=None, grid_cap=0):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, None, lens, grid_cap)
    return o, lse, dqkv


def _check_module_vs_fp32(gpu, B, S, H, lens_t, seed):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    qkv = _qkv(B, S, H, gpu, seed).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0).to(gpu)
    assert m._long_kernel_ok(qkv) and not m._kernel_ok(qkv)
    o = m(qkv, lens_t)
    g = _dout(B, S, H, gpu, seed)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    # the raw op: the module's results, and lse over the valid keys
    o2, lse, dqkv = _run(native(), qkv.detach(), g, H, lens_t)
    assert torch.equal(o2, o.detach()) and torch.equal(dqkv, qkv.grad)
    torch.testing.assert_close(lse, _ref_lse(qkv.detach().float(), H, lens_t), atol=2e-2, rtol=2e-2)
    return qkv.detach(), g, o2, lse, dqkv


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H", [(2, 192, 2), (1, 256, 1), (1, 320, 3), (2, 512, 2)])
def test_long_attention_matches_fp32(gpu, B, S, H):
    _check_module_vs_fp32(gpu, B, S, H, None, 1)


def _ref64(x, heads):
    """Full-tensor fp64 reference on the host: O and dQKV for the upstream gradient g."""
    xr = x.detach().double().cpu().requires_grad_(True)
    return xr, _ref(xr, heads)


@pytest.mark.gpu
@pytest.mark.parametrize("j", [250, 20, 131], ids=["last32", "first32", "key130"])
def test_online_softmax_rescale_is_forced(gpu, C, j):
    """Keys j, j-1, j-2 are 16x the queries 7, 100, 201: those rows' running max jumps by about 30
    at the chunk holding key j (a late chunk, the first one -- set once and never again --, or the
    third), so the rescale of l and of the O accumulators is exercised with a factor far from 1."""
    B, S, H = 2, 256, 2
    x = _qkv(B, S, H, gpu, 21, scale=0.5).view(B, S, 3, H, 64).clone()
    for i, r in enumerate((7, 100, 201)):
        x[:, j - i, 1] = (16 * x[:, r, 0].float()).to(torch.bfloat16)
    x = x.view(B, S, -1).contiguous()
    g = _dout(B, S, H, gpu, 21)
    o, lse, dqkv = _run(C, x, g, H, None)
    xr, orf = _ref64(x, H)
    orf.backward(g.double().cpu())
    s = (xr.detach().view(B, S, 3, H, 64)[:, 7, 0] * xr.detach().view(B, S, 3, H, 64)[:, j, 1]).sum(-1) / 8
    assert s.min() > 15, s  # the spike is there
    torch.testing.assert_close(o.double().cpu(), orf.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(lse.double().cpu(), _ref_lse(xr.detach(), H), atol=2e-2, rtol=2e-2)
    ref = xr.grad
    torch.testing.assert_close(dqkv.double().cpu(), ref, rtol=3e-2, atol=1e-2 * float(ref.abs().max()))


_CASES = [
    (192, [192, 129, 128, 65, 1, 0]),
    (512, [512, 385, 77, 700, -3]),  # clamps to [.., 512, 0]
]


@pytest.mark.gpu
@pytest.mark.parametrize("S,lens", _CASES, ids=[f"S{s}" for s, _ in _CASES])
def test_long_varlen_matches_fp32(gpu, C, S, lens):
    H, B = 2, len(lens)
    lens_t = torch.tensor(lens, device=gpu, dtype=torch.int32)
    qkv, g, o, lse, dqkv = _check_module_vs_fp32(gpu, B, S, H, lens_t, 2)
    _assert_pad_zero(lens_t, S, o, lse, dqkv)
    # all-S lens is bitwise the lens=None result
    full = torch.full((B,), S, device=gpu, dtype=torch.int32)
    for p in (0.0, 0.2):
        step = torch.tensor([5], device=gpu, dtype=torch.int64)
        for a, b in zip(_run(C, qkv, g, H, full, p, step=step), _run(C, qkv, g, H, None, p, step=step)):
            assert torch.equal(a, b), p


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_long_padded_rows_are_never_read(gpu, C, p):
    S, H, lens = 256, 2, [256, 130, 1, 0]
    B = len(lens)
    lens_t = torch.tensor(lens, device=gpu, dtype=torch.int32)
    pad = ~_valid(lens_t, S)
    qkv = _qkv(B, S, H, gpu, 3)
    do = _dout(B, S, H, gpu, 3)
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


def _np_mix32(h):
    import numpy as np

    h = h.astype(np.uint64) & 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    h ^= h >> 16
    return h


def _documented_mask(B, H, S, p, seed, stepv):
    """common.h drop_keep over idx = ((b*H + h)*S + q)*S + key with attn_key(seed, step) -> [B, H, q, key]."""
    import numpy as np

    key = int(_np_mix32(np.array([((seed * 0x27D4EB2F) ^ (stepv * 0x165667B1)) & 0xFFFFFFFF]))[0])
    idx = np.arange(B * H * S * S, dtype=np.uint64)
    pr = idx >> 1
    h = _np_mix32(np.uint64(key) ^ ((pr & 0xFFFFFFFF) * 0x9E3779B9 & 0xFFFFFFFF)
                  ^ (((pr >> 32) * 0x7F4A7C15) & 0xFFFFFFFF))
    bits = np.where(idx & 1, h >> 16, h & 0xFFFF)
    thresh = min(4294967295, int(np.floor(p * 4294967296.0)))
    return (bits >= (thresh >> 16)).reshape(B, H, S, S)


def _probe_mask(C, qkv5, H, p, seed, step, lens=None):
    """The forward's own keep-mask [B, H, q, key]: S/64 probe forwards, V = identity on one 64-key chunk
    and zero elsewhere, so O[q, d] = dropout(P)[q, 64 c + d]."""
    B, S = qkv5.shape[:2]
    parts = []
    for c in range(S // 64):
        probe = qkv5.clone()
        probe[:, :, 2] = 0
        probe[:, 64 * c:64 * (c + 1), 2] = torch.eye(64, device=qkv5.device, dtype=torch.bfloat16)[None, :, None, :]
        po, _ = C.attn_fwd(probe.view(B, S, -1), H, p, seed, step, lens)
        parts.append(po.view(B, S, H, 64).permute(0, 2, 1, 3) != 0)
    return torch.cat(parts, dim=-1)


@pytest.mark.gpu
def test_long_dropout_mask_is_the_documented_hash(gpu, C):
    B, S, H, p, seed, stepv = 3, 192, 2, 0.2, 11, 5
    step = torch.tensor([stepv], device=gpu, dtype=torch.int64)
    qkv5 = _qkv(B, S, H, gpu, 5, scale=0.5).view(B, S, 3, H, 64)
    mask = _probe_mask(C, qkv5, H, p, seed, step)
    want = torch.from_numpy(_documented_mask(B, H, S, p, seed, stepv)).to(gpu)
    assert torch.equal(mask, want), int((mask != want).sum())
    assert abs(mask.float().mean().item() - (1 - p)) < 0.02
    assert not torch.equal(_probe_mask(C, qkv5, H, p, seed, step + 1), mask)  # another step, another mask

    # forward and both backward passes under that mask
    x = qkv5.reshape(B, S, -1).contiguous()
    g = _dout(B, S, H, gpu, 5)
    o, lse, dqkv = _run(C, x, g, H, None, p, seed=seed, step=step)
    xr = x.float().requires_grad_(True)
    orf = _ref(xr, H, None, mask.float(), p)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)

    # with lengths the valid pairs keep their bits
    lens_t = torch.tensor([192, 100, 33], device=gpu, dtype=torch.int32)
    mask_l = _probe_mask(C, qkv5, H, p, seed, step, lens_t)
    valid = _valid(lens_t, S)
    pair = (valid[:, None, :, None] & valid[:, None, None, :]).expand_as(mask)
    assert torch.equal(mask_l[pair], mask[pair])
    assert not mask_l[~pair].any()
    o, lse, dqkv = _run(C, x, g, H, lens_t, p, seed=seed, step=step)
    xr = x.float().requires_grad_(True)
    orf = _ref(xr, H, lens_t, mask.float(), p)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
    _assert_pad_zero(lens_t, S, o, lse, dqkv)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_long_results_do_not_depend_on_the_grid(gpu, C, reverse, p):
    """One or two workgroups walk all twelve items, a short one after a long one and the reverse:
    bitwise the results of the launcher's own grid; and two identical calls are bitwise equal."""
    B, H, S = 3, 2, 256
    lens_t = torch.tensor([256, 70, 193], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 4)
    do = _dout(B, S, H, gpu, 4)
    if reverse:
        qkv, do, lens_t = qkv.flip(0).contiguous(), do.flip(0).contiguous(), lens_t.flip(0).contiguous()
    step = torch.tensor([2], device=gpu, dtype=torch.int64)
    for lens in (lens_t, None):
        want = _run(C, qkv, do, H, lens, p, step=step, grid_cap=0)
        if lens is not None:
            _assert_pad_zero(lens, S, *want)
        for cap in (1, 2):
            for a, b in zip(_run(C, qkv, do, H, lens, p, step=step, grid_cap=cap), want):
                assert torch.equal(a, b), cap
        for a, b in zip(_run(C, qkv, do, H, lens, p, step=step, grid_cap=0), want):
            assert torch.equal(a, b)
    # the bias partial sums as well
    o, lse = C.attn_fwd(qkv, H, p, 11, step, lens_t)
    db = [torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(3)]
    for cap, out in zip((0, 1, 2), db):
        C.attn_bwd(do, qkv, o, lse, H, p, 11, step, out, lens_t, cap)
    assert torch.equal(db[0], db[1]) and torch.equal(db[0], db[2])


@pytest.mark.gpu
def test_long_qkv_bias_grad_hand_over_with_lens(gpu):
    """tests/test_attention_varlen.py's bias hand-over comparison at S = 192 (two tiles per sequence,
    the second a 64-row one): the column sums the attention backward hands over equal the Linear's own."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    torch.manual_seed(6)
    B, S, H = 4, 192, 2
    lens_t = torch.tensor([192, 129, 0, 17], device=gpu, dtype=torch.int32)
    lin = MfmaLinear(256, 3 * H * 64).to(gpu).to(torch.bfloat16)
    att = FusedSelfAttention(H, p=0.0).to(gpu)
    x0 = torch.randn(B, S, 256, device=gpu).to(torch.bfloat16)
    g = torch.randn(B, S, H * 64, device=gpu).to(torch.bfloat16)
    assert att._long_kernel_ok(lin(x0))

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
def test_long_graph_replay_sees_the_current_lens(gpu, C):
    B, S, H = 3, 192, 2
    qkv = _qkv(B, S, H, gpu, 7)
    do = _dout(B, S, H, gpu, 7)
    lens_t = torch.tensor([192, 10, 130], device=gpu, dtype=torch.int32)
    first = _run(C, qkv, do, H, lens_t)  # eager once: code objects loaded before the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = _run(C, qkv, do, H, lens_t)
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(out, first):
        assert torch.equal(a, b)
    lens_t.copy_(torch.tensor([5, 192, 0], dtype=torch.int32))
    graph.replay()
    torch.cuda.synchronize()
    want = _run(C, qkv, do, H, lens_t)
    for a, b in zip(out, want):
        assert torch.equal(a, b)
    assert not torch.equal(out[0], first[0])
    _assert_pad_zero(lens_t, S, *out)


@pytest.mark.gpu
def test_trainer_captures_a_bert_step_at_seq_256(gpu):
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    torch.manual_seed(0)
    spec = models.build("bert_base", gpu, torch.bfloat16, layers=1, seq_len=256, min_seq_len=8)
    batch = spec.make_batch(2, gpu)
    assert len(batch[0]) == 4
    attn = spec.model.layers[0].attn
    probe = torch.empty(2, 256, 3 * 768, device=gpu, dtype=torch.bfloat16)
    assert attn._long_kernel_ok(probe) and not attn._kernel_ok(probe)
    ps = CollectivePS(spec.model, OptimConfig("adam", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    losses = [tr.step().float().item() for _ in range(5)]
    torch.cuda.synchronize()
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_feature_off_takes_sdpa(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    B, S, H = 2, 256, 2
    lens_t = torch.tensor([256, 50], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 9).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0).to(gpu)
    assert not m._long_kernel_ok(qkv) and not m._kernel_ok(qkv)
    o = m(qkv, lens_t)
    g = _dout(B, S, H, gpu, 9)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    monkeypatch.setenv("PSD_FEATURES", "")
    assert m._long_kernel_ok(qkv)
