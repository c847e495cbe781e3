"""The streaming attention kernels (kernels/attention_long.hip) at S = 576 .. 4096 (feature ``attn_xlong``):
every instantiation -- full, lengths, causal, documents -- with the contracts it has up to S = 512.

The yardstick is the fp32 composite below (the ``_ref`` / ``_ref_lse`` of tests/test_attention_docs.py with
an optional causal mask, written out here) on the same input generators (randn * 1.5). Tolerances are the
project's own for these kernels: output and lse 2e-2, gradients 3e-2."""
import math

import pytest
import torch


def _valid(lens, S):
    return torch.arange(S, device=lens.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]


def _full(qkv, lens):
    if lens is None:
        return torch.full((qkv.shape[0],), qkv.shape[1], device=qkv.device, dtype=torch.int32)
    return lens


def _visible(qkv, lens, causal, doc):
    """[B, 1, q, key]: key < L; causal: key <= q; documents: for a valid query key >= its document's start."""
    B, S, _ = qkv.shape
    valid = _valid(lens, S)
    idx = torch.arange(S, device=qkv.device)
    vis = valid[:, None, None, :].expand(B, 1, S, S)
    if causal:
        vis = vis & (idx[None, :] <= idx[:, None])[None, None]
    if doc is not None:
        lb = torch.minimum(doc.long().clamp(min=0), idx[None, :])
        vis = vis & ((idx[None, None, None, :] >= lb[:, None, :, None]) | ~valid[:, None, :, None])
    return vis


def _ref(qkv, heads, lens=None, causal=False, doc=None, mask=None, p=0.0):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    lens = _full(qkv, lens)
    q, k, v = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    vis = _visible(qkv, lens, causal, doc)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~vis, float("-inf"))
    empty = (lens.clamp(0, S) == 0)[:, None, None, None]
    a = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * vis
    if mask is not None:
        a = a * mask / (1.0 - p)
    o = (a @ v) * valid[:, None, :, None]
    return o.transpose(1, 2).reshape(B, S, E // 3)


def _ref_lse(qkv, heads, lens=None, causal=False, doc=None):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    lens = _full(qkv, lens)
    q, k, _ = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~_visible(qkv, lens, causal, doc), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return torch.where(valid[:, None, :], lse, torch.zeros_like(lse))


def _assert_pad_zero(lens, S, o, lse, dqkv):
    pad = ~_valid(lens, S)
    assert (o[pad] == 0).all()
    assert (lse.transpose(1, 2)[pad] == 0).all()
    assert (dqkv[pad] == 0).all()


# ------------------------------------------------------------------------------------------ CPU


def test_xlong_kernel_shapes_feature_and_cpu_routing():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention
    from parameter_server_distributed_amd.utils.config import FEATURES

    ok = FusedSelfAttention.xlong_kernel_shape_ok
    assert [s for s in range(0, 4225, 32) if ok(s, 64)] == list(range(576, 4097, 64))
    assert not ok(1024, 32) and not ok(4160, 64) and not ok(512, 64)
    long_ok = FusedSelfAttention.long_kernel_shape_ok  # unchanged
    assert [s for s in range(0, 4225, 32) if long_ok(s, 64)] == [192, 256, 320, 384, 448, 512]
    assert FEATURES["attn_xlong"][0] is True and "SDPA" in FEATURES["attn_xlong"][1]
    torch.manual_seed(0)
    m = FusedSelfAttention(1, p=0.0, causal=True).eval()
    qkv = torch.randn(1, 576, 3 * 64)
    assert not m._long_kernel_ok(qkv) and not m._kernel_ok(qkv)  # a CPU tensor never takes a kernel
    assert not m._long_kernel_ok(qkv.to(torch.bfloat16))
    lens = torch.tensor([300], dtype=torch.int32)
    torch.testing.assert_close(m(qkv, lens), _ref(qkv, 1, lens, causal=True), atol=1e-5, rtol=1e-5)


# ------------------------------------------------------------------------------------------ GPU


def _qkv(B, S, H, gpu, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16).to(gpu)


def _dout(B, S, H, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16).to(gpu)


def _run(C, qkv, do, H, lens, causal=False, doc=None, p=0.0, seed=11, step=None, grid_cap=0, bias=None):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap, causal, doc)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, bias, lens, grid_cap, causal, doc)
    return o, lse, dqkv


# a boundary off the 32-row grid and one document longer than 512; the remainder of a row is one more document
_DOCS = {576: [37, 539], 1024: [37, 1, 600, 386], 2048: [70, 1000, 978], 4096: [37, 1, 2000, 700, 1358]}


def _doc(S, B, dev):
    from parameter_server_distributed_amd.ops.attention import check_doc_start, doc_starts

    assert sum(_DOCS[S]) == S
    t = doc_starts([_DOCS[S]] * B, S, dev)
    check_doc_start(t)
    return t


def _check(gpu, C, B, S, H, lens, causal, doc, seed):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    qkv = _qkv(B, S, H, gpu, seed).requires_grad_(True)
    g = _dout(B, S, H, gpu, seed)
    m = FusedSelfAttention(H, p=0.0, causal=causal).to(gpu)
    assert m._long_kernel_ok(qkv) and not m._kernel_ok(qkv) and not m.long_kernel_shape_ok(S, 64)
    o = m(qkv, lens, doc)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens, causal, doc)
    orf.backward(g.float())
    tag = f"S {S} causal {causal} lens {None if lens is None else lens.tolist()} docs {doc is not None}"
    print(f"{tag}: max|dO| {(o.float() - orf).abs().max().item():.4f}, max|ddQKV| "
          f"{(qkv.grad.float() - qr.grad).abs().max().item():.4f} of {qr.grad.abs().max().item():.2f}")
    torch.testing.assert_close(o.float(), orf.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    o2, lse, dqkv = _run(C, qkv.detach(), g, H, lens, causal, doc)
    assert torch.equal(o2, o.detach()) and torch.equal(dqkv, qkv.grad)  # the module is the native op
    torch.testing.assert_close(lse, _ref_lse(qkv.detach().float(), H, lens, causal, doc), atol=2e-2, rtol=2e-2)
    if lens is not None:
        _assert_pad_zero(lens, S, o2, lse, dqkv)
        pad = ~_valid(lens, S)
        if pad.any():  # padded rows of qkv and dO are never read
            q2, g2 = qkv.detach().clone(), g.clone()
            q2[pad] = float("nan")
            g2[pad] = float("nan")
            for a, b in zip(_run(C, q2, g2, H, lens, causal, doc), (o2, lse, dqkv)):
                assert torch.equal(a, b)


_SHAPES = [(1, 576, 2), (2, 1024, 2), (1, 2048, 1), (1, 4096, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H", _SHAPES, ids=[f"S{s}" for _, s, _ in _SHAPES])
def test_xlong_full_and_lengths_match_fp32(gpu, C, B, S, H):
    """S = 576: a 64-row last tile and an odd chunk count; S = 4096: 64 chunks."""
    _check(gpu, C, B, S, H, None, False, None, 1)
    # a length inside the last tile, a multiple of 128, and an empty sequence (the other rows: another length)
    for L in (S - 23, S // 2 // 128 * 128, 0):
        lens = torch.tensor([L] + [S - 69] * (B - 1), device=gpu, dtype=torch.int32)
        _check(gpu, C, B, S, H, lens, False, None, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H", _SHAPES, ids=[f"S{s}" for _, s, _ in _SHAPES])
def test_xlong_causal_and_documents_match_fp32(gpu, C, B, S, H):
    _check(gpu, C, B, S, H, None, True, None, 3)
    _check(gpu, C, B, S, H, None, True, _doc(S, B, gpu), 4)
    lens = torch.tensor([S - 23] + [S // 2 // 128 * 128] * (B - 1), device=gpu, dtype=torch.int32)
    _check(gpu, C, B, S, H, lens, True, _doc(S, B, gpu), 5)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_xlong_results_do_not_depend_on_the_grid(gpu, C, p):
    B, H, S = 2, 2, 1024
    qkv = _qkv(B, S, H, gpu, 6)
    do = _dout(B, S, H, gpu, 6)
    lens_t = torch.tensor([S - 31, 330], device=gpu, dtype=torch.int32)
    doc = _doc(S, B, gpu)
    step = torch.tensor([2], device=gpu, dtype=torch.int64)
    for lens, causal, dc in ((None, False, None), (lens_t, False, None), (lens_t, True, None), (None, True, doc)):
        db = [torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(4)]
        want = _run(C, qkv, do, H, lens, causal, dc, p, step=step, grid_cap=0, bias=db[0])
        for cap, out in zip((1, 3, 0), db[1:]):  # one workgroup, three, and the launcher's own grid again
            for a, b in zip(_run(C, qkv, do, H, lens, causal, dc, p, step=step, grid_cap=cap, bias=out), want):
                assert torch.equal(a, b), cap
            assert torch.equal(out, db[0]), cap
        ref = want[2].float().sum((0, 1))  # the bias hand-over: the column sums of the dQKV written
        torch.testing.assert_close(db[0], ref, rtol=1e-2, atol=1e-2 * float(ref.abs().max()) + 1e-6)
        assert db[0].abs().max() > 0


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


def _probe_mask(C, qkv5, H, p, seed, step):
    """The forward's own keep-mask [B, H, q, key]: S/64 probe forwards, V = identity on one 64-key chunk
    and zero elsewhere, so O[q, d] = dropout(P)[q, 64 c + d]."""
    B, S = qkv5.shape[:2]
    parts = []
    for c in range(S // 64):
        probe = qkv5.clone()
        probe[:, :, 2] = 0
        probe[:, 64 * c:64 * (c + 1), 2] = torch.eye(64, device=qkv5.device, dtype=torch.bfloat16)[None, :, None, :]
        po, _ = C.attn_fwd(probe.view(B, S, -1), H, p, seed, step)
        parts.append(po.view(B, S, H, 64).permute(0, 2, 1, 3) != 0)
    return torch.cat(parts, dim=-1)


@pytest.mark.gpu
def test_xlong_dropout_mask_is_the_documented_hash(gpu, C):
    B, S, H, p, seed, stepv = 1, 1024, 2, 0.1, 11, 5
    step = torch.tensor([stepv], device=gpu, dtype=torch.int64)
    # scale 0.25: no probability of the 1024 underflows to a bf16 zero, so O != 0 is the keep bit
    qkv5 = _qkv(B, S, H, gpu, 5, scale=0.25).view(B, S, 3, H, 64)
    mask = _probe_mask(C, qkv5, H, p, seed, step)
    want = torch.from_numpy(_documented_mask(B, H, S, p, seed, stepv)).to(gpu)
    assert torch.equal(mask, want), int((mask != want).sum())
    assert abs(mask.float().mean().item() - (1 - p)) < 0.02
    x = qkv5.reshape(B, S, -1).contiguous()
    g = _dout(B, S, H, gpu, 5)
    lens_t = torch.tensor([S - 23], device=gpu, dtype=torch.int32)
    for lens, causal in ((None, False), (lens_t, True)):  # forward and both backward passes under that mask
        o, lse, dqkv = _run(C, x, g, H, lens, causal, None, p, seed=seed, step=step)
        xr = x.float().requires_grad_(True)
        orf = _ref(xr, H, lens, causal, None, mask.float(), p)
        orf.backward(g.float())
        torch.testing.assert_close(o.float(), orf.detach(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
        for a, b in zip(_run(C, x, g, H, lens, causal, None, p, seed=seed, step=step), (o, lse, dqkv)):
            assert torch.equal(a, b)  # two runs, the same bits


@pytest.mark.gpu
def test_xlong_feature_switches(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops import attention
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    B, S, H = 2, 1024, 2
    lens_t = torch.tensor([S, 300], device=gpu, dtype=torch.int32)
    m = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    g = _dout(B, S, H, gpu, 9)
    calls = []
    orig = attention._AttnFn.apply
    monkeypatch.setattr(attention._AttnFn, "apply", lambda *a: calls.append(1) or orig(*a))

    def run():
        qkv = _qkv(B, S, H, gpu, 9).requires_grad_(True)
        o = m(qkv, lens_t)
        o.backward(g)
        return o.detach().float(), qkv.grad.float()

    want = run()
    assert len(calls) == 1  # both features on: one call per forward
    qr = _qkv(B, S, H, gpu, 9).float().requires_grad_(True)
    orf = _ref(qr, H, lens_t, True)
    orf.backward(g.float())
    for feats in ("attn_xlong=0", "attn_long=0"):
        monkeypatch.setenv("PSD_FEATURES", feats)
        probe = _qkv(B, S, H, gpu, 9)
        assert not m._long_kernel_ok(probe) and not m._kernel_ok(probe)
        got = run()
        assert len(calls) == 1, feats  # SDPA on transposed views
        torch.testing.assert_close(got[0], orf.detach(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(got[1], qr.grad, atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(got[0], want[0], atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(got[1], want[1], atol=3e-2, rtol=3e-2)
    monkeypatch.setenv("PSD_FEATURES", "attn_xlong=0")
    assert m._long_kernel_ok(_qkv(B, 512, H, gpu, 9))  # attn_xlong leaves S <= 512 alone
    monkeypatch.setenv("PSD_FEATURES", "")
    assert m._long_kernel_ok(probe)


@pytest.mark.gpu
def test_gpt_step_at_seq_1024_on_the_kernels_matches_the_sdpa_path(gpu, monkeypatch):
    """tests/test_gpt_packed.py's comparison of the two paths, at S = 1024 (max_pos follows seq_len)."""
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops import attention

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, layers=1, vocab=2048, seq_len=1024)
    m = spec.model
    assert m.emb.pos.weight.shape[0] == 1024
    for t in m.parameters():  # bf16 working weights, as the PS data planes give them
        t.data = t.data.to(torch.bfloat16)
    for mod in m.modules():  # dropout 0: the two paths draw different masks
        if isinstance(getattr(mod, "p", None), float):
            mod.p = 0.0
    x, y = spec.make_batch(2, gpu, seed=1)
    probe = torch.empty(2, 1024, 3 * 768, device=gpu, dtype=torch.bfloat16)
    assert m.layers[0].attn.causal and m.layers[0].attn._long_kernel_ok(probe)

    def run():
        calls = []
        orig = attention._AttnFn.apply
        attention._AttnFn.apply = lambda *a: calls.append(1) or orig(*a)
        try:
            m.zero_grad(set_to_none=True)
            logits = m(x)
            loss = spec.loss(logits, y)
            loss.backward()
        finally:
            attention._AttnFn.apply = orig
        return loss.float().item(), logits.detach().float(), len(calls)

    la, logits, n = run()
    assert n == 1 and math.isfinite(la)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    lb, _, n = run()
    assert n == 0  # SDPA
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setenv("PSD_FEATURES", "")
    ulp = 2.0 ** (math.floor(math.log2(logits.abs().max().item())) - 7)  # one bf16 ulp at max|logit| (tests/test_gpt.py)
    print(f"loss kernels {la:.5f}, sdpa {lb:.5f}, ulp {ulp:.5f}")
    assert abs(la - lb) <= ulp, (la, lb, ulp)
