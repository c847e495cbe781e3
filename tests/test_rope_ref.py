"""Rotary position embeddings on the CPU (ops/rope.py): the composite ``rope_ref`` against an independent
complex formulation in fp64, the relative-position property, the pass-through contracts, the argument
errors and the decoder LM with ``pos="rope"``.

Bounds. The tables are the fp64 cos / sin rounded once to fp32, so each entry is off by at most 2^-25
(half an fp32 ulp below 1); an fp64 evaluation on them is then off by at most 2^-25 (|x1| + |x2|) per
element. The checks allow 2^-22 (|x1| + |x2|): a factor of two over the fp32 rounding 2^-23, per element,
and the same figure scaled by the pair products for a score q . k.

The helpers at the top are shared with tests/test_rope.py (the kernel's tests)."""
import math

import pytest
import torch

EPS = 2.0 ** -22


def _tables(P, device=None):
    from parameter_server_distributed_amd.ops.rope import rope_tables

    return rope_tables(P, device=device)


def _halves(qkv, H):
    """(x1, x2) of the Q and K heads: [B, S, 2H, 32] each."""
    B, S, E = qkv.shape
    qk = qkv[:, :, :2 * E // 3].reshape(B, S, 2 * H, 64)
    return qk[..., :32], qk[..., 32:]


def _doc_rows(S):
    """Document lengths [5, 59, 1, 100, ...] laid end to end and cut at S (the rest is one document)."""
    out, t = [], 0
    for n in (5, 59, 1, 100, 10**9):
        if t >= S:
            break
        out.append(min(n, S - t))
        t += out[-1]
    return out


def _docs(B, S, device=None):
    from parameter_server_distributed_amd.ops.attention import doc_starts

    return doc_starts([_doc_rows(S)] * B, S, device)


def _positions(B, S, doc, device):
    t = torch.arange(S, device=device)[None, :].expand(B, S)
    return t if doc is None else t - torch.minimum(doc.long().clamp(min=0), t)


def _bits(t):
    return t.contiguous().view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()])


def rope_error(got, x, H, cos, sin, lens=None, doc=None, inverse=False):
    """Worst error / bound over the Q and K elements of ``got`` (bf16) against ``rope_ref`` in fp64 on the same
    bf16 input ``x`` and the same fp32 tables: bound = 2^-8 |ref64| (half a bf16 ulp, the rule of
    tests/test_row_kernels_fp64.py) + 2^-20 (|x1 c| + |x2 s|) (eight fp32 ulps of the two product magnitudes
    of the element, for the contraction freedom). Returns (worst ratio, its error, its bound)."""
    from parameter_server_distributed_amd.ops.rope import rope_ref

    B, S, E = x.shape
    ref = rope_ref(x.double(), H, cos, sin, lens, doc, inverse)
    pos = _positions(B, S, doc, x.device)
    c = cos.double()[pos][:, :, None, :]
    s = sin.double()[pos][:, :, None, :]
    x1, x2 = _halves(x.double(), H)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(), (x2 * c).abs() + (x1 * s).abs()], dim=-1).reshape(B, S, -1)
    refqk = ref[:, :, :2 * E // 3]
    err = (got[:, :, :2 * E // 3].double() - refqk).abs()
    bound = 2.0 ** -8 * refqk.abs() + 2.0 ** -20 * mag
    assert bool(torch.isfinite(err).all())
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
    i = int(ratio.argmax())
    return float(ratio.reshape(-1)[i]), float(err.reshape(-1)[i]), float(bound.reshape(-1)[i])


# ------------------------------------------------------------------------------------------ the composite


def test_rope_ref_matches_the_complex_formulation_in_fp64():
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(0)
    B, S, H = 2, 40, 2
    x = torch.randn(B, S, 3 * H * 64, dtype=torch.float64)
    cos, sin = _tables(S)
    assert cos.dtype == torch.float32 and cos.shape == (S, 32) and sin.shape == (S, 32)
    theta = torch.tensor(10000.0, dtype=torch.float64) ** (-torch.arange(32, dtype=torch.float64) / 32.0)
    ang = torch.arange(S, dtype=torch.float64)[:, None] * theta[None, :]
    x1, x2 = _halves(x, H)
    for inverse in (False, True):
        z = torch.complex(x1, x2) * torch.polar(torch.ones_like(ang), -ang if inverse else ang)[None, :, None, :]
        got1, got2 = _halves(rope_ref(x, H, cos, sin, inverse=inverse), H)
        bound = EPS * (x1.abs() + x2.abs())
        assert bool(((got1 - z.real).abs() <= bound).all()) and bool(((got2 - z.imag).abs() <= bound).all())
        assert float((got1 - x1).abs().max()) > 0.1  # and it did rotate
    y = rope_ref(x, H, cos, sin)
    assert y.dtype == torch.float64 and y.data_ptr() != x.data_ptr()  # out of place
    # fp32 input: fp32 maths, fp32 out, close to the fp64 result
    y32 = rope_ref(x.float(), H, cos, sin)
    assert y32.dtype == torch.float32
    torch.testing.assert_close(y32.double(), y, atol=1e-5, rtol=1e-5)


def test_scores_depend_on_the_relative_position_only():
    """One head, S = 96: a document of 32 rows at row offset 0 against the same rows at offset d. Read as one
    long document the copy sits at positions d .. d + 31, and every score q_m . k_n must not move; with a
    doc_start that restarts the positions at d the rotated rows themselves are those of offset 0, bit for bit."""
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(1)
    S, H, n = 96, 1, 32
    cos, sin = _tables(S)
    docx = torch.randn(1, n, 3 * 64, dtype=torch.float64)

    def scores(y):
        q, k = y[0, :, :64], y[0, :, 64:128]
        return q @ k.t()

    base = torch.zeros(1, S, 3 * 64, dtype=torch.float64)
    base[:, :n] = docx
    ya = rope_ref(base, H, cos, sin, doc_start=torch.zeros(1, S, dtype=torch.int32))[:, :n]
    q1, q2 = docx[0, :, :32].abs(), docx[0, :, 32:64].abs()
    k1, k2 = docx[0, :, 64:96].abs(), docx[0, :, 96:128].abs()
    bound = EPS * ((q1 + q2) @ (k1 + k2).t())  # the element bound, scaled by the pair products of a score
    for d in (1, 31, 64):
        xb = torch.zeros(1, S, 3 * 64, dtype=torch.float64)
        xb[:, d:d + n] = docx
        yb = rope_ref(xb, H, cos, sin)[:, d:d + n]
        assert float((yb - ya).abs().max()) > 0.1  # other angles ...
        diff = (scores(yb) - scores(ya)).abs()
        assert bool((diff <= bound).all()), (d, float((diff / bound).max()))  # ... the same scores
        doc = torch.arange(S, dtype=torch.int32)[None, :].clone()
        doc[:, d:d + n] = d
        assert torch.equal(rope_ref(xb, H, cos, sin, doc_start=doc)[:, d:d + n], ya)
    # and the scores do depend on m - n: shifting only the keys changes them
    xk = torch.zeros(1, S, 3 * 64, dtype=torch.float64)
    xk[:, :n, :64] = docx[:, :, :64]
    xk[:, 1:n + 1, 64:128] = docx[:, :, 64:128]
    yk = rope_ref(xk, H, cos, sin)
    moved = yk[0, :n, :64] @ yk[0, 1:n + 1, 64:128].t()
    assert float((moved - scores(ya)).abs().max()) > 0.1


def test_inverse_after_forward_returns_the_input():
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(2)
    B, S, H = 3, 70, 2
    x = torch.randn(B, S, 3 * H * 64, dtype=torch.float64)
    cos, sin = _tables(128)  # P > S
    lens = torch.tensor([S, 33, 0], dtype=torch.int32)
    doc = _docs(B, S)
    for ln, dc in ((None, None), (lens, doc), (None, doc)):
        back = rope_ref(rope_ref(x, H, cos, sin, ln, dc), H, cos, sin, ln, dc, inverse=True)
        x1, x2 = _halves(x, H)
        b1, b2 = _halves(back, H)
        bound = EPS * (x1.abs() + x2.abs())
        assert bool(((b1 - x1).abs() <= bound).all()) and bool(((b2 - x2).abs() <= bound).all())


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32, torch.bfloat16])
def test_position_zero_rows_and_v_are_bitwise_unchanged(dtype):
    from parameter_server_distributed_amd.ops.attention import doc_starts
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(3)
    B, S, H = 2, 64, 2
    x = torch.randn(B, S, 3 * H * 64).to(dtype)
    x[0, 5, 3] = -0.0
    cos, sin = _tables(S)
    doc = doc_starts([[5, 59], [64]], S)
    for inverse in (False, True):
        y = rope_ref(x, H, cos, sin, None, doc, inverse)
        assert y.dtype == dtype
        assert torch.equal(_bits(y[:, :, 2 * H * 64:]), _bits(x[:, :, 2 * H * 64:]))
        for b, t in ((0, 0), (0, 5), (1, 0)):
            assert torch.equal(_bits(y[b, t]), _bits(x[b, t]))
        assert not torch.equal(y[0, 6], x[0, 6]) and not torch.equal(y[1, 5], x[1, 5])
        plain = rope_ref(x, H, cos, sin, inverse=inverse)
        assert torch.equal(_bits(plain[:, 0]), _bits(x[:, 0])) and not torch.equal(plain[0, 5], x[0, 5])
    # all zeros is the call without a doc_start
    assert torch.equal(_bits(rope_ref(x, H, cos, sin, None, torch.zeros(B, S, dtype=torch.int32))),
                       _bits(rope_ref(x, H, cos, sin)))


def test_rows_past_a_length_keep_their_bits_with_nan_in_them():
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(4)
    S, H = 48, 2
    lens = torch.tensor([0, 1, S - 1, S, S + 7, -3], dtype=torch.int32)
    B = lens.numel()
    x = torch.randn(B, S, 3 * H * 64).to(torch.bfloat16)
    pad = torch.arange(S)[None, :] >= lens.clamp(0, S)[:, None]
    x[pad] = float("nan")
    cos, sin = _tables(S)
    doc = _docs(B, S)
    junk = doc.clone()
    junk[pad] = 2**30
    for dc in (None, doc, junk):
        y = rope_ref(x, H, cos, sin, lens, dc)
        assert torch.equal(_bits(y[pad]), _bits(x[pad]))
        assert bool(torch.isfinite(y[~pad].float()).all())
        assert not torch.equal(y[3, 1:], x[3, 1:])
    assert torch.equal(_bits(rope_ref(x, H, cos, sin, lens, junk)), _bits(rope_ref(x, H, cos, sin, lens, doc)))
    junk[pad] = -5
    assert torch.equal(_bits(rope_ref(x, H, cos, sin, lens, junk)), _bits(rope_ref(x, H, cos, sin, lens, doc)))


def test_fp32_composite_contracted_or_not_meets_the_kernel_conditions():
    """The two conditions tests/test_rope.py puts on the kernel, met by the reference alone: the fp32 composite
    as written (two products, one subtraction, each rounded) and with the contraction a compiler may apply
    (one product rounded, then a fused multiply-add, emulated exactly in fp64) both stay inside the fp64
    bound, and they agree bitwise on at least 99 % of the elements."""
    from parameter_server_distributed_amd.ops.rope import rope_ref

    torch.manual_seed(0)
    for (B, S, H) in ((2, 64, 2), (3, 200, 12)):
        x = torch.randn(B, S, 3 * H * 64).to(torch.bfloat16)
        cos, sin = _tables(S)
        doc = _docs(B, S)
        for inverse in (False, True):
            plain = rope_ref(x, H, cos, sin, None, doc, inverse)
            x1, x2 = _halves(x.double(), H)
            pos = _positions(B, S, doc, x.device)
            c = cos.double()[pos][:, :, None, :]
            s = sin.double()[pos][:, :, None, :] * (-1.0 if inverse else 1.0)
            # a 24 x 24-bit product is exact in fp64; the other product is rounded to fp32 first
            y1 = (x1 * c - (x2 * s).float().double()).float()
            y2 = (x2 * c + (x1 * s).float().double()).float()
            fused = torch.cat([y1, y2], dim=-1).to(torch.bfloat16).reshape(B, S, 2 * H * 64)
            fused = torch.where((pos != 0)[:, :, None], fused, x[:, :, :2 * H * 64])
            fused = torch.cat([fused, x[:, :, 2 * H * 64:]], dim=-1)
            for name, got in (("plain", plain), ("fused", fused)):
                ratio, err, bound = rope_error(got, x, H, cos, sin, None, doc, inverse)
                assert ratio <= 1.0, (name, ratio, err, bound)
            same = float((_bits(plain) == _bits(fused)).float().mean())
            assert same >= 0.99, same


# ------------------------------------------------------------------------------------------ module and model


def test_value_errors():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM
    from parameter_server_distributed_amd.ops.rope import RotaryQK, rope_ref, rope_tables

    for bad in (0, -4):
        with pytest.raises(ValueError, match="max_pos"):
            rope_tables(bad)
    with pytest.raises(ValueError, match="base"):
        rope_tables(8, base=0.0)
    rot = RotaryQK(2, 32)
    assert rot.cos.shape == (32, 32) and rot.cos.dtype == torch.float32
    rot(torch.randn(1, 32, 3 * 2 * 64))
    with pytest.raises(ValueError, match="max_pos"):
        rot(torch.randn(1, 33, 3 * 2 * 64))
    with pytest.raises(ValueError, match="qkv"):
        rot(torch.randn(1, 32, 3 * 2 * 32))  # head dim 32
    with pytest.raises(ValueError):
        rope_ref(torch.randn(1, 40, 3 * 2 * 64), 2, rot.cos, rot.sin)  # a table with fewer than S rows
    for bad in ("alibi", None, "Rope"):
        with pytest.raises(ValueError, match="pos"):
            GPTForLM(layers=1, hidden=128, heads=2, vocab=64, max_pos=16, pos=bad)
    with pytest.raises(ValueError, match="pos"):
        models.build("gpt_small", torch.device("cpu"), torch.float32, layers=1, hidden=128, heads=2, vocab=64,
                     seq_len=16, pos="sinusoidal")


def test_rotary_module_is_the_composite_on_the_cpu_and_owns_no_state():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.rope import RotaryQK, rope_ref

    torch.manual_seed(5)
    B, S, H = 2, 24, 2
    rot = RotaryQK(H, 32, base=500.0)
    assert rot.state_dict() == {} and not list(rot.parameters())
    x = torch.randn(B, S, 3 * H * 64, requires_grad=True)
    lens = torch.tensor([S, 9], dtype=torch.int32)
    doc = _docs(B, S)
    y = rot(x, lens, doc)
    assert torch.equal(y, rope_ref(x.detach(), H, rot.cos, rot.sin, lens, doc)) and y.data_ptr() != x.data_ptr()
    assert not hasattr(y, "_psd_src")
    g = torch.randn_like(y)
    y.backward(g)
    # the backward of an orthogonal map is its inverse, and passed-through rows pass the gradient through
    torch.testing.assert_close(x.grad, rope_ref(g, H, rot.cos, rot.sin, lens, doc, inverse=True), atol=1e-6, rtol=1e-6)
    # prepare() keeps the tables fp32, and a dtype cast of the module rebuilds them instead of rounding them
    m = models.prepare(RotaryQK(H, 32), torch.device("cpu"), torch.bfloat16)
    assert m.cos.dtype == torch.float32
    m = RotaryQK(H, 32, base=500.0).to(torch.bfloat16)
    assert m.cos.dtype == torch.float32 and torch.equal(m.cos, rot.cos) and m.state_dict() == {}


def test_bert_layer_with_rope_and_without():
    from parameter_server_distributed_amd.models.bert import BertLayer
    from parameter_server_distributed_amd.ops.rope import RotaryQK

    torch.manual_seed(6)
    plain = BertLayer(128, 2, 256, 0.0)
    assert plain.rot is None and not any("rot" in k for k in plain.state_dict())
    layer = BertLayer(128, 2, 256, 0.0, rope=(64, 10000.0))  # bidirectional: allowed at the layer level
    assert isinstance(layer.rot, RotaryQK) and layer.rot.max_pos == 64
    assert layer.state_dict().keys() == plain.state_dict().keys()
    layer.load_state_dict(plain.state_dict())
    x = torch.randn(2, 16, 128)
    assert not torch.allclose(layer(x), plain(x), atol=1e-4)


def test_two_layer_gpt_with_rope_runs_forward_and_backward():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM, gpt_batch

    torch.manual_seed(7)
    tiny = dict(layers=2, hidden=128, heads=2, vocab=256)
    m = GPTForLM(**tiny, max_pos=48, dropout=0.0, pos="rope", rope_base=1000.0)
    assert m.emb.pos.weight.shape == (1, 128)
    assert all(layer.rot is not None and layer.rot.base == 1000.0 and layer.rot.max_pos == 48 for layer in m.layers)
    ref = GPTForLM(**tiny, max_pos=48, dropout=0.0)
    assert ref.emb.pos.weight.shape == (48, 128) and all(layer.rot is None for layer in ref.layers)
    assert m.state_dict().keys() == ref.state_dict().keys()  # no table in the state
    for kw in (dict(docs=(5, 20)), dict(min_len=20), dict()):
        x, y = gpt_batch(3, 48, tiny["vocab"], torch.device("cpu"), seed=1, **kw)
        m.zero_grad(set_to_none=True)
        loss = m.loss(m(x), y)
        loss.backward()
        assert math.isfinite(loss.item())
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in m.parameters())
    # the position signal is in the blocks: swapping two rows' contents changes the logits of later rows
    ids = x[0].clone()
    a = m((ids,)).view(3, 48, -1)
    ids2 = ids.clone()
    ids2[:, [3, 4]] = ids[:, [4, 3]]
    b = m((ids2,)).view(3, 48, -1)
    assert torch.allclose(a[:, :3], b[:, :3], atol=1e-5) and not torch.allclose(a[:, 10], b[:, 10], atol=1e-4)
    # one state for every context length
    longer = GPTForLM(**tiny, max_pos=96, dropout=0.0, pos="rope", rope_base=1000.0)
    longer.load_state_dict(m.state_dict())
    x2, y2 = gpt_batch(2, 96, tiny["vocab"], torch.device("cpu"), seed=2)
    assert math.isfinite(longer.loss(longer(x2), y2).item())
    torch.testing.assert_close(longer((ids,)).view(3, 48, -1), a, atol=1e-5, rtol=1e-5)
    spec = models.build("gpt_small", torch.device("cpu"), torch.float32, seq_len=32, pos="rope", rope_base=500.0,
                        pack_docs=(4, 12), **tiny)
    assert spec.model.emb.pos.weight.shape[0] == 1 and spec.model.layers[0].rot.base == 500.0
    xb, yb = spec.make_batch(2, torch.device("cpu"))
    assert math.isfinite(spec.loss(spec.model(xb), yb).item())
