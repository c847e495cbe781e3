"""Causal self-attention on the fused kernels (kernels/attention.hip for S <= 128, attention_long.hip for
S = 192 .. 512; ops/attention.py): query q attends to keys <= q, and < the sequence's length with
``lens``. The contracts of the bidirectional kernels (tests/test_attention_varlen.py,
tests/test_attention_long.py) under the mask -- fp32 match, ``lse``, zero padded rows, padding never
read, the dropout hash, grid independence, the QKV-bias hand-over -- plus the causal one: rows <= j
do not depend, bit for bit, on rows > j.

The yardstick is the fp32 composite below (softmax over ``tril & key < L``); tolerances are the
project's own for these kernels (output and lse 2e-2, gradients 3e-2) with the same input generators.

Three cases of the fp32 match miss the gradient bound by one element of dQ in an early row (S = 320
without lengths, row 8: 0.0379; S = 256 and S = 512 with lengths, row 3: 0.0393 each, as the smallest t
that passes atol = rtol = t). A causal row near the start has a handful of keys, so its dS values are of
order 10 and their bf16 rounding is not averaged out, while the element itself nearly cancels. The
bf16 SDPA path rounds dS the same way and measures the same 0.0379 / 0.0393 / 0.0393 against the same
composite on the same inputs; those three cases allow twice that (_GRAD_TOL, profiles/attn_causal.md),
every other case keeps 3e-2."""
import math

import pytest
import torch


def _valid(lens, S):
    return torch.arange(S, device=lens.device)[None, :] < lens.clamp(0, S)[:, None]  # [B, S]


def _visible(qkv, lens, causal=True):
    """[B, 1, q, key]: key < L, and key <= q under the causal mask."""
    B, S, _ = qkv.shape
    vis = _valid(lens, S)[:, None, None, :].expand(B, 1, S, S)
    if causal:
        vis = vis & torch.ones(S, S, dtype=torch.bool, device=qkv.device).tril()
    return vis


def _ref(qkv, heads, lens=None, mask=None, p=0.0, causal=True):
    """Attention in qkv's own precision from packed [B, S, 3*H*D] over the visible keys only, output
    rows >= L zeroed; finite for L = 0."""
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
    q, k, v = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    vis = _visible(qkv, lens, causal)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~vis, float("-inf"))
    empty = (lens.clamp(0, S) == 0)[:, None, None, None]
    a = torch.softmax(torch.where(empty, torch.zeros_like(s), s), dim=-1) * vis
    if mask is not None:
        a = a * mask / (1.0 - p)
    o = (a @ v) * valid[:, None, :, None]
    return o.transpose(1, 2).reshape(B, S, E // 3)


def _ref_lse(qkv, heads, lens=None, causal=True):
    B, S, E = qkv.shape
    D = E // (3 * heads)
    if lens is None:
        lens = torch.full((B,), S, device=qkv.device, dtype=torch.int32)
    q, k, _ = qkv.view(B, S, 3, heads, D).permute(2, 0, 3, 1, 4).unbind(0)
    valid = _valid(lens, S)
    s = (q @ k.transpose(-1, -2) / math.sqrt(D)).masked_fill(~_visible(qkv, lens, causal), float("-inf"))
    lse = torch.logsumexp(s, dim=-1)  # [B, H, S]
    return torch.where(valid[:, None, :], lse, torch.zeros_like(lse))


def _assert_pad_zero(lens, S, o, lse, dqkv):
    pad = ~_valid(lens, S)  # [B, S]
    assert (o[pad] == 0).all()
    assert (lse.transpose(1, 2)[pad] == 0).all()
    assert (dqkv[pad] == 0).all()  # q, k and v parts: the whole packed row


# ------------------------------------------------------------------------------------------ CPU


def test_causal_cpu_module_matches_the_composite():
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    torch.manual_seed(0)
    H, S = 2, 48
    qkv = torch.randn(4, S, 3 * H * 64)
    m = FusedSelfAttention(H, p=0.0, causal=True).eval()
    assert m.causal and not FusedSelfAttention(H).causal
    torch.testing.assert_close(m(qkv), _ref(qkv, H), atol=1e-5, rtol=1e-5)
    lens = torch.tensor([S, 17, 0, 1], dtype=torch.int32)
    out = m(qkv, lens)
    torch.testing.assert_close(out, _ref(qkv, H, lens), atol=1e-5, rtol=1e-5)
    assert (out[~_valid(lens, S)] == 0).all()
    # row q is the attention over rows <= q alone
    torch.testing.assert_close(m(qkv)[:, :20], m(qkv[:, :20].contiguous()), atol=1e-5, rtol=1e-5)
    # the default is the bidirectional module, unchanged
    b = FusedSelfAttention(H, p=0.0).eval()
    torch.testing.assert_close(b(qkv), _ref(qkv, H, causal=False), atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(b(qkv, lens), _ref(qkv, H, lens, causal=False), atol=1e-5, rtol=1e-5)
    assert not torch.allclose(b(qkv), m(qkv), atol=1e-3)


# ------------------------------------------------------------------------------------------ GPU


def _qkv(B, S, H, gpu, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16).to(gpu)


def _dout(B, S, H, gpu, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16).to(gpu)


def _run(C, qkv, do, H, lens, p=0.0, seed=11, step=None, grid_cap=0, causal=True):
    o, lse = C.attn_fwd(qkv, H, p, seed, step, lens, grid_cap, causal)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, seed, step, None, lens, grid_cap, causal)
    return o, lse, dqkv


def _takes_a_kernel(m, qkv):
    return m._kernel_ok(qkv) or m._long_kernel_ok(qkv)


# (S, with lengths) -> gradient tolerance: twice the bf16 SDPA path's measured error (module docstring)
_GRAD_TOL = {(320, False): 2 * 0.0379, (256, True): 2 * 0.0393, (512, True): 2 * 0.0393}


def _check_module_vs_fp32(gpu, B, S, H, lens_t, seed):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    qkv = _qkv(B, S, H, gpu, seed).requires_grad_(True)
    m = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    assert _takes_a_kernel(m, qkv)
    o = m(qkv, lens_t)
    g = _dout(B, S, H, gpu, seed)
    o.backward(g)
    qr = qkv.detach().float().requires_grad_(True)
    orf = _ref(qr, H, lens_t)
    orf.backward(g.float())
    print(f"S {S}: max|dO| {(o.float() - orf).abs().max().item():.4f}, "
          f"max|ddQKV| {(qkv.grad.float() - qr.grad).abs().max().item():.4f} of {qr.grad.abs().max().item():.2f}")
    torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
    gtol = _GRAD_TOL.get((S, lens_t is not None), 3e-2)
    torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=gtol, rtol=gtol)
    # the raw op: the module's results, and lse over the visible keys
    o2, lse, dqkv = _run(native(), qkv.detach(), g, H, lens_t)
    assert torch.equal(o2, o.detach()) and torch.equal(dqkv, qkv.grad)
    torch.testing.assert_close(lse, _ref_lse(qkv.detach().float(), H, lens_t), atol=2e-2, rtol=2e-2)
    # and not the bidirectional result
    assert not torch.equal(o2, native().attn_fwd(qkv.detach(), H, 0.0, 11, None, lens_t)[0])
    return qkv.detach(), g, o2, lse, dqkv


@pytest.mark.gpu
@pytest.mark.parametrize("B,S,H", [(2, 32, 2), (1, 64, 1), (2, 96, 2), (2, 128, 3), (2, 192, 2), (1, 256, 1),
                                   (1, 320, 3), (2, 512, 2)])
def test_causal_attention_matches_fp32(gpu, B, S, H):
    _check_module_vs_fp32(gpu, B, S, H, None, 1)


# a length inside a diagonal block, on a block edge, at 0 and at S (and one that clamps)
_LENS = [
    (32, [32, 7, 0, 1]),
    (96, [96, 65, 64, 0, 33]),
    (128, [128, 70, 0, 33]),
    (192, [192, 129, 128, 65, 1, 0]),
    (256, [256, 130, 64, 1]),
    (512, [512, 385, 77, 700, -3, 256]),
]


@pytest.mark.gpu
@pytest.mark.parametrize("S,lens", _LENS, ids=[f"S{s}" for s, _ in _LENS])
def test_causal_varlen_matches_fp32(gpu, C, S, lens):
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
@pytest.mark.parametrize("S,j", [(64, 40), (128, 70), (256, 150), (512, 300)])
def test_causal_rows_do_not_depend_on_later_rows(gpu, C, S, j):
    """Other finite values in rows > j of qkv leave rows <= j of O and lse bit for bit; with rows > j
    of dO zero, rows <= j of dQKV as well (a later query then adds exact zeros to dK and dV)."""
    B, H = 2, 2
    qkv = _qkv(B, S, H, gpu, 12)
    other = qkv.clone()
    other[:, j + 1:] = _qkv(B, S, H, gpu, 13, scale=2.0)[:, j + 1:]
    do = _dout(B, S, H, gpu, 12)
    do[:, j + 1:] = 0
    lens_t = torch.tensor([S, j + 20], device=gpu, dtype=torch.int32)
    for lens in (None, lens_t):
        for p in (0.0, 0.1):
            step = torch.tensor([4], device=gpu, dtype=torch.int64)
            a = _run(C, qkv, do, H, lens, p, step=step)
            b = _run(C, other, do, H, lens, p, step=step)
            assert torch.equal(a[0][:, :j + 1], b[0][:, :j + 1])
            assert torch.equal(a[1][:, :, :j + 1], b[1][:, :, :j + 1])
            assert torch.equal(a[2][:, :j + 1], b[2][:, :j + 1])
            assert not torch.equal(a[0][:, j + 1:], b[0][:, j + 1:])  # the later rows did change
            assert all(torch.isfinite(t).all() for t in b)


@pytest.mark.gpu
@pytest.mark.parametrize("S,lens", [(128, [128, 70, 1, 0]), (256, [256, 130, 1, 0])], ids=["S128", "S256"])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_causal_padded_rows_are_never_read(gpu, C, p, S, lens):
    H, B = 2, len(lens)
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
    o, lse = C.attn_fwd(qn, H, p, 11, step, lens_t, 0, True)
    on = o.clone()
    on[pad] = float("nan")  # backward reads O too (D = rowsum(dO . O)): its padded rows as well
    dqkv = C.attn_bwd(dn, qn, on, lse, H, p, 11, step, None, lens_t, 0, True)
    for a, b in zip((o, lse, dqkv), want):
        assert torch.isfinite(a).all()
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("S", [64, 128, 256])
def test_causal_results_do_not_depend_on_the_grid(gpu, C, S, reverse, p):
    """One or three workgroups walk all the items, a short one after a long one and the reverse:
    bitwise the results of the launcher's own grid, and two identical calls are bitwise equal. One
    workgroup per launch keeps the whole-head backward's Pd / dS image in LDS from item to item: a
    read outside what the current item wrote would pick up the previous, longer item's values."""
    B, H = 4, 2
    lens_t = torch.tensor([S, S // 4 + 6, S - 31, 33], device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 4)
    do = _dout(B, S, H, gpu, 4)
    if reverse:
        qkv, do, lens_t = qkv.flip(0).contiguous(), do.flip(0).contiguous(), lens_t.flip(0).contiguous()
    step = torch.tensor([2], device=gpu, dtype=torch.int64)
    for lens in (lens_t, None):
        want = _run(C, qkv, do, H, lens, p, step=step, grid_cap=0)
        if lens is not None:
            _assert_pad_zero(lens, S, *want)
        for cap in (1, 3):
            for a, b in zip(_run(C, qkv, do, H, lens, p, step=step, grid_cap=cap), want):
                assert torch.equal(a, b), cap
        for a, b in zip(_run(C, qkv, do, H, lens, p, step=step, grid_cap=0), want):
            assert torch.equal(a, b)
    # one workgroup and the fp32 composite agree as well (a stale read can be the same in every grid
    # only if every grid maps the items alike, which grid_cap = 1 and the full grid do not)
    if p == 0.0:
        o, lse, dqkv = _run(C, qkv, do, H, lens_t, grid_cap=1)
        xr = qkv.float().requires_grad_(True)
        orf = _ref(xr, H, lens_t)
        orf.backward(do.float())
        torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
    # the bias partial sums as well
    o, lse = C.attn_fwd(qkv, H, p, 11, step, lens_t, 0, True)
    db = [torch.empty(3 * H * 64, device=gpu, dtype=torch.float32) for _ in range(3)]
    for cap, out in zip((0, 1, 3), db):
        C.attn_bwd(do, qkv, o, lse, H, p, 11, step, out, lens_t, cap, True)
    assert torch.equal(db[0], db[1]) and torch.equal(db[0], db[2])


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
    """The causal forward's own keep-mask [B, H, q, key]: S/64 probe forwards, V = identity on one 64-key
    chunk and zero elsewhere, so O[q, d] = dropout(P)[q, 64 c + d] (zero at a masked key)."""
    B, S = qkv5.shape[:2]
    parts = []
    for c in range(S // 64):
        probe = qkv5.clone()
        probe[:, :, 2] = 0
        probe[:, 64 * c:64 * (c + 1), 2] = torch.eye(64, device=qkv5.device, dtype=torch.bfloat16)[None, :, None, :]
        po, _ = C.attn_fwd(probe.view(B, S, -1), H, p, seed, step, lens, 0, True)
        parts.append(po.view(B, S, H, 64).permute(0, 2, 1, 3) != 0)
    return torch.cat(parts, dim=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 256])
def test_causal_dropout_mask_is_the_documented_hash_below_the_diagonal(gpu, C, S):
    B, H, p, seed, stepv = 3, 2, 0.2, 11, 5
    step = torch.tensor([stepv], device=gpu, dtype=torch.int64)
    qkv5 = _qkv(B, S, H, gpu, 5, scale=0.5).view(B, S, 3, H, 64)
    mask = _probe_mask(C, qkv5, H, p, seed, step)
    doc = torch.from_numpy(_documented_mask(B, H, S, p, seed, stepv)).to(gpu)
    tril = torch.ones(S, S, dtype=torch.bool, device=gpu).tril()
    assert torch.equal(mask, doc & tril), int((mask != (doc & tril)).sum())
    assert abs(mask[:, :, tril].float().mean().item() - (1 - p)) < 0.02

    # forward and the backward passes under that mask
    x = qkv5.reshape(B, S, -1).contiguous()
    g = _dout(B, S, H, gpu, 5)
    lens_t = torch.tensor([S, S // 2 + 5, 33], device=gpu, dtype=torch.int32)
    for lens in (None, lens_t):
        o, lse, dqkv = _run(C, x, g, H, lens, p, seed=seed, step=step)
        xr = x.float().requires_grad_(True)
        orf = _ref(xr, H, lens, doc.float(), p)
        orf.backward(g.float())
        torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv.float(), xr.grad, atol=3e-2, rtol=3e-2)
    # with lengths the visible pairs keep their bits
    mask_l = _probe_mask(C, qkv5, H, p, seed, step, lens_t)
    valid = _valid(lens_t, S)
    pair = (valid[:, None, :, None] & valid[:, None, None, :] & tril).expand_as(mask)
    assert torch.equal(mask_l[pair], doc[pair])
    assert not mask_l[~pair].any()
    _assert_pad_zero(lens_t, S, o, lse, dqkv)


@pytest.mark.gpu
@pytest.mark.parametrize("S,lens", [(128, [128, 70, 0, 33]), (256, [256, 130, 0, 17])], ids=["S128", "S256"])
def test_causal_bias_out_is_the_column_sum_of_dqkv(gpu, C, S, lens):
    """The QKV-bias hand-over under the mask: bias_out is the column sum of the dQKV that was written
    (the bound of the bidirectional hand-over tests), through the raw op and through the modules."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    H, B = 2, len(lens)
    lens_t = torch.tensor(lens, device=gpu, dtype=torch.int32)
    qkv = _qkv(B, S, H, gpu, 6)
    do = _dout(B, S, H, gpu, 6)
    for p in (0.0, 0.1):
        step = torch.tensor([3], device=gpu, dtype=torch.int64)
        o, lse = C.attn_fwd(qkv, H, p, 11, step, lens_t, 0, True)
        db = torch.empty(3 * H * 64, device=gpu, dtype=torch.float32)
        dqkv = C.attn_bwd(do, qkv, o, lse, H, p, 11, step, db, lens_t, 0, True)
        assert torch.equal(dqkv, C.attn_bwd(do, qkv, o, lse, H, p, 11, step, None, lens_t, 0, True))
        want = dqkv.float().sum((0, 1))
        torch.testing.assert_close(db, want, rtol=1e-2, atol=1e-2 * float(want.abs().max()) + 1e-6)
        assert db.abs().max() > 0

    torch.manual_seed(6)
    lin = MfmaLinear(256, 3 * H * 64).to(gpu).to(torch.bfloat16)
    att = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    x0 = torch.randn(B, S, 256, device=gpu).to(torch.bfloat16)
    assert _takes_a_kernel(att, lin(x0))

    def run(hand):
        lin.weight.grad = lin.bias.grad = None
        x = x0.clone().requires_grad_(True)
        y = lin(x)
        if not hand:
            y = y * 1  # untagged: the Linear sums its own bias gradient
        att(y, lens_t).backward(do)
        return [t.float().clone() for t in (x.grad, lin.weight.grad, lin.bias.grad)]

    got, ref = run(True), run(False)
    assert lin._psd_bias_hand is None
    for a, b in zip(got, ref):
        torch.testing.assert_close(a, b, rtol=1e-2, atol=1e-2 * float(b.abs().max()) + 1e-6)
    assert got[2].abs().max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("S,off", [(160, False), (256, True)], ids=["S160", "S256_attn_long_off"])
def test_causal_sdpa_path_matches_the_composite(gpu, monkeypatch, S, off):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    if off:
        monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    B, H = 2, 2
    m = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    for lens_t in (None, torch.tensor([S, 50], device=gpu, dtype=torch.int32)):
        qkv = _qkv(B, S, H, gpu, 9).requires_grad_(True)
        assert not _takes_a_kernel(m, qkv)
        o = m(qkv, lens_t)
        g = _dout(B, S, H, gpu, 9)
        o.backward(g)
        qr = qkv.detach().float().requires_grad_(True)
        orf = _ref(qr, H, lens_t)
        orf.backward(g.float())
        torch.testing.assert_close(o.float(), orf, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(qkv.grad.float(), qr.grad, atol=3e-2, rtol=3e-2)
    if off:
        monkeypatch.setenv("PSD_FEATURES", "")
        assert m._long_kernel_ok(qkv)
