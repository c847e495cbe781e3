"""Causal sliding-window attention (``window=W``; ops/attention.py, the WINDOW copies of
kernels/attention_long.hip): query q of sequence b sees key k iff

    max(doc_start[b, q], q - W + 1, 0) <= k <= q   and   k < L,

W keys with the query's own. The yardstick is the fp32 composite below -- the ``_ref`` / ``_ref_lse`` of
tests/test_attention_docs.py with the lower bound in place of the document start, written out here -- on
the same input generators (randn * 1.5). Tolerances are the project's own for these kernels: output and
lse 2e-2, gradients 3e-2.

Two groups of cases of the fp32 match miss the gradient bound by one or two elements, as cases of
tests/test_attention_causal.py and tests/test_attention_docs.py do, and are treated as there (_grad_tol):
they allow twice what the module's bf16 SDPA path measures with the same mask on the same inputs against
the same composite, never a figure taken from the kernels. Measured on an MI355X as the smallest t that
passes atol = rtol = t:
  W = 33 (S = 192, 256 plain and with documents; S = 576, 1024 every variant): one element of dQ in a row
    with 33 keys (sequence 2 row 58 at S = 192, sequence 0 row 442 at S = 576 and 1024), 0.0317 (0.0351
    absolute); the bf16 SDPA path measures 0.0317 at the same element.
  S = 1024 with documents, every W but 1: one element of dV (sequence 3, row 589), 0.0305; the bf16 SDPA
    path measures 0.0305 there.
Both are the rounding of the bf16 gradient itself: over all 144 cases the SDPA path's figure equals the
kernels' to four digits (0.013 .. 0.0317), and every other case keeps 3e-2."""
import math

import pytest
import torch
import torch.nn.functional as F

TINY = dict(layers=2, hidden=128, heads=2, vocab=256)


def _valid(lens, S):
    return torch.arange(S, device=lens.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]


def _lower(B, S, doc, window, dev):
    """[B, S]: first key query q may see, max(doc[b, q] clamped to [0, q], q - W + 1, 0)."""
    idx = torch.arange(S, device=dev)
    lb = torch.zeros(B, S, dtype=torch.long, device=dev)
    if doc is not None:
        lb = torch.minimum(doc.long().clamp(min=0), idx[None, :])
    if window is not None:
        lb = torch.maximum(lb, (idx - int(window) + 1).clamp(min=0)[None, :])
    return lb


def _visible(qkv, lens, doc, window):
    """[B, 1, q, key]: key < L, key <= q, and for a valid query key >= its lower bound."""
    B, S, _ = qkv.shape
    valid = _valid(lens, S)
    idx = torch.arange(S, device=qkv.device)
    vis = valid[:, None, None, :] & (idx[None, :] <= idx[:, None])[None, None]
    lb = _lower(B, S, doc, window, qkv.device)
    return vis & ((idx[None, None, None, :] >= lb[:, None, :, None]) | ~valid[:, None, :, None])


def _full(qkv, lens):
    if lens is None:
        return torch.full((qkv.shape[0],), qkv.shape[1], device=qkv.device, dtype=torch.int32)
    return lens


def _ref(qkv, heads, lens=None, doc=None, window=None, mask=None, p=0.0):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    lens = _full(qkv, lens)
    q, k, v = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    vis = _visible(qkv, lens, doc, window)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~vis, float("-inf"))
    empty = (lens.clamp(0, S) == 0)[:, None, None, None]
    a = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * vis
    if mask is not None:
        a = a * mask / (1.0 - p)
    o = (a @ v) * valid[:, None, :, None]
    return o.transpose(1, 2).reshape(B, S, E // 3)


def _ref_lse(qkv, heads, lens=None, doc=None, window=None):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    lens = _full(qkv, lens)
    q, k, _ = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~_visible(qkv, lens, doc, window), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)
    return torch.where(valid[:, None, :], lse, torch.zeros_like(lse))


def _assert_pad_zero(lens, S, o, lse, dqkv):
    pad = ~_valid(lens, S)
    assert (o[pad] == 0).all()
    assert (lse.transpose(1, 2)[pad] == 0).all()
    assert (dqkv[pad] == 0).all()


def _rows(docs, S):
    """Document lengths laid end to end and cut at S; the remainder is one more document."""
    out, t = [], 0
    for n in docs:
        if t >= S:
            break
        out.append(min(n, S - t))
        t += out[-1]
    if t < S:
        out.append(S - t)
    return out


def _doc(docs, S, B, dev=None):
    from parameter_server_distributed_amd.ops.attention import doc_starts

    return doc_starts([_rows(docs, S)] * B, S, dev)


# ------------------------------------------------------------------------------------------ CPU

_CPU_W = (1, 2, 7, 32, 47, 48, 60)


@pytest.mark.parametrize("S", [48, 96])
def test_window_cpu_module_matches_the_composite(S):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(0)
    H, B = 2, 4
    qkv = torch.randn(B, S, 3 * H * 64)
    v = qkv.view(B, S, 3, H, 64)[:, :, 2].reshape(B, S, H * 64)
    doc = _doc([5, 1, 20, 22], S, B)
    lens = torch.tensor([S, 17, 0, 1], dtype=torch.int32)
    plain = FusedSelfAttention(H, p=0.0, causal=True).eval()
    for W in _CPU_W:
        m = FusedSelfAttention(H, p=0.0, causal=True, window=W).eval()
        assert m.window == W and plain.window is None
        for ln, dc in ((lens, None), (None, doc), (lens, doc), (None, None)):
            out = m(qkv, ln, dc)
            torch.testing.assert_close(out, _ref(qkv, H, ln, dc, W), atol=1e-5, rtol=1e-5)
            if ln is not None:
                assert (out[~_valid(ln, S)] == 0).all()
            if W >= S:  # no key is cut: the module without a window, bit for bit
                assert torch.equal(out, plain(qkv, ln, dc))
            elif W < 32:
                assert not torch.allclose(out, plain(qkv, ln, dc), atol=1e-3)
            if W == 1:  # every valid query sees itself alone
                want = v if ln is None else v * _valid(ln, S)[:, :, None]
                torch.testing.assert_close(out, want, atol=1e-6, rtol=1e-6)
        # entries of doc_start past a length change nothing
        junk = doc.clone()
        junk[~_valid(lens, S)] = 10**6
        assert torch.equal(m(qkv, lens, junk), m(qkv, lens, doc))


def test_window_argument_checks_and_the_gpt_model_on_the_cpu():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.bert import BertLayer
    from parameter_server_distributed_amd.models.gpt import GPTForLM, gpt_batch
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    for bad in (0, -3):
        with pytest.raises(ValueError, match="window"):
            FusedSelfAttention(2, causal=True, window=bad)
    with pytest.raises(ValueError, match="window"):
        FusedSelfAttention(2, causal=False, window=8)
    with pytest.raises(ValueError, match="window"):
        BertLayer(128, 2, 512, window=8)  # a bidirectional layer
    assert BertLayer(128, 2, 512, causal=True, window=8).attn.window == 8

    torch.manual_seed(0)
    S, W, B = 32, 5, 3
    m = GPTForLM(**TINY, max_pos=S, dropout=0.0, window=W).eval()
    assert all(layer.attn.window == W and layer.attn.causal for layer in m.layers)
    (ids,), _ = gpt_batch(B, S, TINY["vocab"], torch.device("cpu"), seed=2)
    with torch.no_grad():
        got = m((ids,))
    idx = torch.arange(S)
    band = (idx[None, :] <= idx[:, None]) & (idx[None, :] > idx[:, None] - W)
    assert band.sum(1).tolist() == [min(q + 1, W) for q in range(S)]

    def explicit(attn):
        def fwd(qkv, lens=None, doc_start=None):
            Bq, Sq, E = qkv.shape
            q, k, v = qkv.view(Bq, Sq, 3, attn.heads, 64).permute(2, 0, 3, 1, 4).unbind(0)
            a = F.scaled_dot_product_attention(q, k, v, attn_mask=band)
            return a.transpose(1, 2).reshape(Bq, Sq, E // 3)
        return fwd

    for layer in m.layers:
        layer.attn.forward = explicit(layer.attn)
    with torch.no_grad():
        want = m((ids,))
    torch.testing.assert_close(got, want, atol=1e-5, rtol=1e-5)
    torch.manual_seed(0)
    full = GPTForLM(**TINY, max_pos=S, dropout=0.0).eval()
    with torch.no_grad():
        assert not torch.allclose(full((ids,)), got, atol=1e-3)  # same weights (same seed), another mask

    spec = models.build("gpt_small", torch.device("cpu"), torch.float32, seq_len=32, window=6, pack_docs=(4, 12), **TINY)
    assert all(layer.attn.window == 6 for layer in spec.model.layers)
    x, y = spec.make_batch(2, torch.device("cpu"))
    assert math.isfinite(spec.loss(spec.model(x), y).item())
    assert models.build("gpt_small", torch.device("cpu"), torch.float32, seq_len=32, **TINY).model.layers[0].attn.window is None


# ------------------------------------------------------------------------------------------ GPU


def _qkv(B, S, H, gpu, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16).to(gpu)


def _dout(B, S, H, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16).to(gpu)


def _run(C, qkv, do, H, lens, doc, window, p=0.0, seed=11, step=None, grid_cap=0, bias=None):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap, True, doc, window)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, bias, lens, grid_cap, True, doc, window)
    return o, lse, dqkv


# documents with boundaries off the 32-row grid, some shorter and some longer than most of the windows
_DOCS = {192: [70, 59, 63], 256: [70, 59, 71, 56], 576: [5, 395, 112, 64], 1024: [37, 1, 530, 200, 256]}
_WINDOWS = (1, 31, 32, 33, 64, 100, 129, 200)


def _grad_tol(S, variant, W):
    """3e-2, or twice the bf16 SDPA path's measured error for the cases the module docstring lists."""
    if W == 33 and (S >= 576 or variant in ("plain", "docs")):
        return 2 * 0.0317
    if S == 1024 and "docs" in variant and W != 1:
        return 2 * 0.0305
    return 3e-2


def _variant(name, S, B, gpu):
    lens = torch.tensor([S - 23, 0, 1, S], device=gpu, dtype=torch.int32) if "lens" in name else None
    doc = _doc(_DOCS[S], S, B, gpu) if "docs" in name else None
    return lens, doc


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ["plain", "lens", "docs", "lens+docs"])
@pytest.mark.parametrize("S", [192, 256, 576, 1024])
def test_window_attention_matches_fp32(gpu, C, S, variant):
    B, H = 4, 2
    lens, doc = _variant(variant, S, B, gpu)
    qkv = _qkv(B, S, H, gpu, 1)
    do = _dout(B, S, H, gpu, 1)
    v = qkv.view(B, S, 3, H, 64)[:, :, 2].reshape(B, S, H * 64)
    valid = _valid(_full(qkv, lens), S)
    for W in _WINDOWS + (S - 1,):
        o, lse, dqkv = _run(C, qkv, do, H, lens, doc, W)
        qr = qkv.float().requires_grad_(True)
        orf = _ref(qr, H, lens, doc, W)
        orf.backward(do.float())
        print(f"S {S} {variant} W {W}: max|dO| {(o.float() - orf).abs().max().item():.4f}, max|ddQKV| "
              f"{(dqkv.float() - qr.grad).abs().max().item():.4f} of {qr.grad.abs().max().item():.2f}")
        torch.testing.assert_close(o.float(), orf.detach(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(lse, _ref_lse(qkv.float(), H, lens, doc, W), atol=2e-2, rtol=2e-2)
        gtol = _grad_tol(S, variant, W)
        torch.testing.assert_close(dqkv.float(), qr.grad, atol=gtol, rtol=gtol)
        if lens is not None:
            _assert_pad_zero(lens, S, o, lse, dqkv)
        if W == 1:  # one key with probability exactly 1
            assert torch.equal(o[valid], v[valid])


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [256, 576])
def test_window_at_least_s_is_bitwise_the_causal_call(gpu, C, S, p):
    """window > 0 always launches the window copies: with no key cut they give the causal (or document)
    copies' bits, bias partials included."""
    B, H = 4, 2
    qkv = _qkv(B, S, H, gpu, 4)
    do = _dout(B, S, H, gpu, 4)
    step = torch.tensor([7], device=gpu, dtype=torch.int64)
    for name in ("plain", "lens", "docs", "lens+docs"):
        lens, doc = _variant(name, S, B, gpu)
        ba = torch.empty(3 * H * 64, device=gpu, dtype=torch.float32)
        want = _run(C, qkv, do, H, lens, doc, 0, p, step=step, bias=ba)
        for W in (S, S + 7):
            bb = torch.empty(3 * H * 64, device=gpu, dtype=torch.float32)
            got = _run(C, qkv, do, H, lens, doc, W, p, step=step, bias=bb)
            for a, b in zip(got + (bb,), want + (ba,)):
                assert torch.equal(a, b), (name, W)
        assert ba.abs().max() > 0
        if doc is None:  # (no document of _DOCS is longer than S - 40)
            assert not torch.equal(_run(C, qkv, do, H, lens, doc, S - 40, p, step=step)[0], want[0])


@pytest.mark.gpu
def test_window_blocks_out_of_reach_are_never_multiplied(gpu, C):
    """Skipping, per 32-row block by the block's first query: NaN in K / V rows [64, 96) does not reach a
    32-query block whose first query q0 has q0 - W + 1 > 95; NaN in dO rows [512, 544) does not reach the
    dK / dV of a 32-key block with k0 + 31 < 512 - W + 1."""
    B, H, S, W = 1, 2, 1024, 128
    qkv = _qkv(B, S, H, gpu, 5)
    do = _dout(B, S, H, gpu, 5)
    o, lse, dqkv = _run(C, qkv, do, H, None, None, W)
    assert all(torch.isfinite(t).all() for t in (o, lse, dqkv))

    bad = qkv.clone()
    bad.view(B, S, 3, H, 64)[:, 64:96, 1:] = float("nan")
    o2, lse2, dqkv2 = _run(C, bad, do, H, None, None, W)
    q_first = 224  # the first multiple of 32 with q0 - 127 > 95
    assert q_first - W + 1 > 95 and q_first - 32 - W + 1 <= 95
    assert torch.equal(o2[:, q_first:], o[:, q_first:]) and torch.equal(lse2[:, :, q_first:], lse[:, :, q_first:])
    dq, dq2 = (t.view(B, S, 3, H, 64)[:, q_first:, 0] for t in (dqkv, dqkv2))
    assert torch.equal(dq2, dq)
    assert torch.isnan(o2[:, 64:96]).all()  # the probe is live: those queries see the keys

    bad_do = do.clone()
    bad_do[:, 512:544] = float("nan")
    dqkv3 = C.attn_bwd(bad_do, qkv, o, lse, H, 0.0, 11, None, None, None, 0, True, None, W)
    k_end = 384  # key blocks [k0, k0 + 32) with k0 + 31 < 512 - 127 = 385: k0 <= 352
    assert k_end - 1 < 512 - W + 1 <= k_end + 31
    kv, kv3 = (t.view(B, S, 3, H, 64)[:, :k_end, 1:] for t in (dqkv, dqkv3))
    assert torch.equal(kv3, kv)
    assert torch.isnan(dqkv3.view(B, S, 3, H, 64)[:, 512 - W + 1:544, 1:]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("t", [37, 200, 333])
def test_window_rows_do_not_depend_on_keys_before_the_window(gpu, C, t):
    """Other finite values in rows < t of qkv leave row q of O and lse bit for bit for every q with
    q - W + 1 >= t -- also where t and q are on no block boundary."""
    B, H, S, W = 2, 2, 576, 100
    qkv = _qkv(B, S, H, gpu, 6)
    q2 = qkv.clone()
    q2[:, :t] = _qkv(B, S, H, gpu, 7, scale=2.0)[:, :t]
    lens_t = torch.tensor([S, S - 23], device=gpu, dtype=torch.int32)
    for lens in (None, lens_t):
        for p in (0.0, 0.1):
            step = torch.tensor([4], device=gpu, dtype=torch.int64)
            a = C.attn_fwd(qkv, H, p, 11, step, lens, 0, True, None, W)
            b = C.attn_fwd(q2, H, p, 11, step, lens, 0, True, None, W)
            q_first = t + W - 1
            assert torch.equal(a[0][:, q_first:], b[0][:, q_first:])
            assert torch.equal(a[1][:, :, q_first:], b[1][:, :, q_first:])
            assert not torch.equal(a[0][:, q_first - 1], b[0][:, q_first - 1])  # that row sees key t - 1
            assert torch.isfinite(b[0]).all()


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


def _probe_mask(C, qkv5, H, p, seed, step, lens, doc, window):
    """The forward's own keep-mask [B, H, q, key]: S/64 probe forwards, V = identity on one 64-key chunk
    and zero elsewhere, so O[q, d] = dropout(P)[q, 64 c + d] (zero at a key the query does not see)."""
    B, S = qkv5.shape[:2]
    parts = []
    for c in range(S // 64):
        probe = qkv5.clone()
        probe[:, :, 2] = 0
        probe[:, 64 * c:64 * (c + 1), 2] = torch.eye(64, device=qkv5.device, dtype=torch.bfloat16)[None, :, None, :]
        po, _ = C.attn_fwd(probe.view(B, S, -1), H, p, seed, step, lens, 0, True, doc, window)
        parts.append(po.view(B, S, H, 64).permute(0, 2, 1, 3) != 0)
    return torch.cat(parts, dim=-1)


@pytest.mark.gpu
def test_window_dropout_grid_determinism_and_bias(gpu, C):
    B, H, S, W, p, seed, stepv = 3, 2, 576, 100, 0.1, 11, 5
    step = torch.tensor([stepv], device=gpu, dtype=torch.int64)
    x = _qkv(B, S, H, gpu, 8, scale=0.5)
    g = _dout(B, S, H, gpu, 8)
    doc = _doc(_DOCS[S], S, B, gpu)
    lens_t = torch.tensor([S, S // 2 + 5, 33], device=gpu, dtype=torch.int32)
    hashm = torch.from_numpy(_documented_mask(B, H, S, p, seed, stepv)).to(gpu)
    # the kept set is the documented mask restricted to the visible keys
    mask = _probe_mask(C, x.view(B, S, 3, H, 64), H, p, seed, step, lens_t, doc, W)
    vis = _visible(x, lens_t, doc, W) & _valid(lens_t, S)[:, None, :, None]
    vis = vis.expand_as(mask)
    assert torch.equal(mask[vis], hashm[vis]), int((mask[vis] != hashm[vis]).sum())
    assert not mask[~vis].any()
    assert abs(mask[vis].float().mean().item() - (1 - p)) < 0.02
    for lens, dc in ((None, None), (lens_t, None), (None, doc), (lens_t, doc)):
        db = [torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(4)]
        o, lse, dqkv = _run(C, x, g, H, lens, dc, W, p, seed=seed, step=step, bias=db[0])
        xr = x.float().requires_grad_(True)
        orf = _ref(xr, H, lens, dc, W, hashm.float(), p)
        orf.backward(g.float())
        torch.testing.assert_close(o.float(), orf.detach(), atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
        # one workgroup, three, the launcher's own grid again: the same bits, bias partials included
        for cap, out in zip((1, 3, 0), db[1:]):
            for a, b in zip(_run(C, x, g, H, lens, dc, W, p, seed=seed, step=step, grid_cap=cap, bias=out), (o, lse, dqkv)):
                assert torch.equal(a, b), cap
            assert torch.equal(out, db[0]), cap
        want = dqkv.float().sum((0, 1))
        torch.testing.assert_close(db[0], want, rtol=1e-2, atol=1e-2 * float(want.abs().max()) + 1e-6)
        assert db[0].abs().max() > 0
    _assert_pad_zero(lens_t, S, o, lse, dqkv)


@pytest.mark.gpu
def test_window_argument_errors_of_the_native_op(gpu, C):
    H = 2
    qkv = _qkv(1, 256, H, gpu, 9)
    o, lse = C.attn_fwd(qkv, H, 0.0, 1, None, None, 0, True)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_fwd(qkv, H, 0.0, 1, None, None, 0, True, None, -1)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_fwd(qkv, H, 0.0, 1, None, None, 0, False, None, 16)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_bwd(o, qkv, o, lse, H, 0.0, 1, None, None, None, 0, True, None, -1)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_bwd(o, qkv, o, lse, H, 0.0, 1, None, None, None, 0, False, None, 16)
    small = _qkv(1, 128, H, gpu, 9)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_fwd(small, H, 0.0, 1, None, None, 0, True, None, 16)
    o, lse = C.attn_fwd(small, H, 0.0, 1, None, None, 0, True)
    with pytest.raises(RuntimeError, match="window"):
        C.attn_bwd(o, small, o, lse, H, 0.0, 1, None, None, None, 0, True, None, 16)
    # the keyword, last
    a = C.attn_fwd(qkv, H, 0.0, 1, causal=True, window=64)
    assert torch.equal(a[0], C.attn_fwd(qkv, H, 0.0, 1, None, None, 0, True, None, 64)[0])


class _Spy:
    """The native module with attn_fwd's positional arguments recorded."""

    def __init__(self, real, calls):
        self._real, self._calls = real, calls

    def __getattr__(self, name):
        fn = getattr(self._real, name)
        if name != "attn_fwd":
            return fn
        return lambda *a: self._calls.append(a) or fn(*a)


@pytest.mark.gpu
def test_window_module_routing(gpu, monkeypatch):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops import attention
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    B, H = 2, 2
    fn_calls, nat_calls = [], []
    orig = attention._AttnFn.apply
    real = native()
    monkeypatch.setattr(attention._AttnFn, "apply", lambda *a: fn_calls.append(a) or orig(*a))
    monkeypatch.setattr(attention, "native", lambda: _Spy(real, nat_calls))

    # S = 128: the whole-head kernels have no window copies
    qkv = _qkv(B, 128, H, gpu, 10).requires_grad_(True)
    lens = torch.tensor([128, 75], device=gpu, dtype=torch.int32)
    m = FusedSelfAttention(H, p=0.0, causal=True, window=32).to(gpu)
    o = m(qkv, lens)
    g = _dout(B, 128, H, gpu, 10)
    o.backward(g)
    assert not fn_calls and not nat_calls
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens, None, 32)
    orf.backward(g.float())
    torch.testing.assert_close(o.float(), orf.detach(), atol=2e-2, rtol=2e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)

    # S = 256, W = 64: one call, the window last
    qkv = _qkv(B, 256, H, gpu, 11)
    m = FusedSelfAttention(H, p=0.0, causal=True, window=64).to(gpu)
    o = m(qkv)
    assert len(fn_calls) == 1 and len(nat_calls) == 1 and nat_calls[0][-1] == 64 and len(nat_calls[0]) == 10
    assert torch.equal(o, real.attn_fwd(qkv, H, 0.0, m.seed, None, None, 0, True, None, 64)[0])
    torch.testing.assert_close(o.float(), _ref(qkv.float(), H, None, None, 64), atol=2e-2, rtol=2e-2)

    # no window, and a window that cuts nothing: today's call, no window argument
    for w in (None, 256, 300):
        del nat_calls[:]
        m = FusedSelfAttention(H, p=0.0, causal=True, window=w).to(gpu)
        o = m(qkv)
        assert len(nat_calls) == 1 and len(nat_calls[0]) == 9, w
        assert torch.equal(o, real.attn_fwd(qkv, H, 0.0, m.seed, None, None, 0, True)[0])

    # features off: SDPA with the mask
    monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    del nat_calls[:]
    m = FusedSelfAttention(H, p=0.0, causal=True, window=64).to(gpu)
    torch.testing.assert_close(m(qkv).float(), _ref(qkv.float(), H, None, None, 64), atol=2e-2, rtol=2e-2)
    assert not nat_calls
