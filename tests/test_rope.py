"""The rotary position embedding kernel (csrc/kernels/rope.hip, native ``rope_``) and ``RotaryQK`` on the GPU.

Accuracy is measured against ``rope_ref`` evaluated in fp64 on the same bf16 inputs and the same fp32
tables: per element |got - ref64| <= 2^-8 |ref64| + 2^-20 (|x1 c| + |x2 s|) -- half a bf16 ulp, the rule of
tests/test_row_kernels_fp64.py, plus eight fp32 ulps of the product magnitudes for the contraction freedom
-- and at least 99 % of the elements equal ``rope_ref`` run in fp32 on the GPU bit for bit (1 % is left for
where the bf16 rounding tips). tests/test_rope_ref.py shows on the CPU that the fp32 composite, contracted
or not, meets both conditions by itself. Each case prints one ROWERR line (recorded in profiles/rope.md).

Shapes: (2, 64, 2) the small base case; (3, 200, 12) S no multiple of 32 and 96 lanes per row, so rows
straddle waves; (1, 4096, 1) the table's last row. Each runs with ``blocks`` = 0 and with 1 and 3, which
make the grid-stride loop wrap.

The module and model comparisons run the same chain with ``PSD_FEATURES=rope=0`` -- the composite, with
the same attention and GEMM kernels -- as the yardstick. Tolerances are the project's own: output 2e-2,
gradients 3e-2 and a column sum 1e-2 (relative to its largest entry) from tests/test_attention_docs.py; the
loss within one bf16 ulp at max|logit| from tests/test_gpt_packed.py, whose 2e-2 relative norm also serves
the parameter gradients."""
import math

import pytest
import torch

from test_rope_ref import _bits, _doc_rows, _docs, _tables, rope_error

pytestmark = pytest.mark.gpu

SHAPES = [(2, 64, 2), (3, 200, 12), (1, 4096, 1)]
IDS = ["B2-S64-H2", "B3-S200-H12", "B1-S4096-H1"]


def _x(B, S, H, gpu, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(B, S, 3 * H * 64, generator=g).to(torch.bfloat16).to(gpu)


def _lens(B, S, gpu):
    return torch.tensor([S - 23, 1, S, 0, S // 2][:B], device=gpu, dtype=torch.int32)


_SHARED = {}


def _case(gpu, shape):
    """Input, tables, lens, doc_start and the blocks = 0 results of one shape, computed once and never changed."""
    if shape not in _SHARED:
        from parameter_server_distributed_amd import native

        B, S, H = shape
        x = _x(B, S, H, gpu)
        cos, sin = _tables(S, gpu)
        lens, doc = _lens(B, S, gpu), _docs(B, S, gpu)
        out = {}
        for inverse in (False, True):
            out[("plain", inverse)] = native().rope_(x.clone(), H, cos, sin, None, None, inverse, 0)
            out[("docs", inverse)] = native().rope_(x.clone(), H, cos, sin, lens, doc, inverse, 0)
        _SHARED[shape] = (x, cos, sin, lens, doc, out)
    return _SHARED[shape]


@pytest.mark.parametrize("blocks", [0, 1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rope_kernel_matches_fp64_and_does_not_depend_on_the_grid(gpu, C, shape, blocks):
    from parameter_server_distributed_amd.ops.rope import rope_ref

    B, S, H = shape
    x, cos, sin, lens, doc, want = _case(gpu, shape)
    cells = []
    for inverse in (False, True):
        for name, ln, dc in (("plain", None, None), ("docs", lens, doc)):
            buf = x.clone()
            got = C.rope_(buf, H, cos, sin, ln, dc, inverse, blocks)
            assert got.data_ptr() == buf.data_ptr()  # in place, the same tensor back
            assert torch.equal(_bits(got), _bits(want[(name, inverse)])), (name, inverse, blocks)  # grid, and run to run
            ratio, err, bound = rope_error(got, x, H, cos, sin, ln, dc, inverse)
            ref32 = rope_ref(x, H, cos, sin, ln, dc, inverse)
            same = float((_bits(got) == _bits(ref32)).float().mean())
            cells.append(f"{name}{' inv' if inverse else ''} {err:.3e} / {bound:.3e} = {ratio:.3f}, bitwise {same:.5f}")
            assert ratio <= 1.0, (name, inverse, ratio, err, bound)
            assert same >= 0.99, (name, inverse, same)
            assert not torch.equal(got, x)
    print(f"ROWERR rope B{B} S{S} H{H} blocks {blocks} | " + " | ".join(cells))


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rope_v_is_never_read_or_written(gpu, C, shape):
    B, S, H = shape
    x, cos, sin, lens, doc, want = _case(gpu, shape)
    xn = x.clone()
    xn[:, :, 2 * H * 64:] = float("nan")
    for name, ln, dc in (("plain", None, None), ("docs", lens, doc)):
        got = C.rope_(xn.clone(), H, cos, sin, ln, dc, False, 0)
        assert torch.equal(_bits(got[:, :, 2 * H * 64:]), _bits(xn[:, :, 2 * H * 64:]))
        assert bool(torch.isfinite(got[:, :, :2 * H * 64].float()).all())
        assert torch.equal(got[:, :, :2 * H * 64], want[(name, False)][:, :, :2 * H * 64])


@pytest.mark.parametrize("blocks", [0, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rope_rows_past_a_length_keep_their_bits(gpu, C, shape, blocks):
    """lens = [0, 1, S - 1, S, S + 9, -2] (clamped on the device): rows >= L hold NaN and keep their bits; their
    doc_start entries, set to 2^30 or -5, are clamped at most, never an index: the results are bitwise those
    with well-formed entries."""
    _, S, H = shape
    lens = torch.tensor([0, 1, S - 1, S, S + 9, -2], device=gpu, dtype=torch.int32)
    B = lens.numel()
    x = _x(B, S, H, gpu, seed=1)
    pad = torch.arange(S, device=gpu)[None, :] >= lens.clamp(0, S)[:, None]
    x[pad] = float("nan")
    cos, sin = _tables(S, gpu)
    doc = _docs(B, S, gpu)
    for inverse in (False, True):
        plain = C.rope_(x.clone(), H, cos, sin, lens, None, inverse, blocks)
        assert torch.equal(_bits(plain[pad]), _bits(x[pad]))
        assert bool(torch.isfinite(plain[~pad].float()).all())
        assert not torch.equal(plain[3, 1:], x[3, 1:]) and not torch.equal(plain[2, 1:S - 1], x[2, 1:S - 1])
        # L = S and L = S + 9 (clamped to S) are whole rows
        assert torch.equal(plain[3:5], C.rope_(x[3:5].clone(), H, cos, sin, None, None, inverse, blocks))
        want = C.rope_(x.clone(), H, cos, sin, lens, doc, inverse, blocks)
        assert torch.equal(_bits(want[pad]), _bits(x[pad]))
        for junk_v in (2**30, -5):
            junk = doc.clone()
            junk[pad] = junk_v
            assert torch.equal(_bits(C.rope_(x.clone(), H, cos, sin, lens, junk, inverse, blocks)), _bits(want))
    # a doc_start is valid without lens as well, and junk anywhere is clamped to [0, t]
    y = _x(2, S, H, gpu, seed=2)
    wild = torch.full((2, S), 2**30, device=gpu, dtype=torch.int32)
    wild[1] = -5
    got = C.rope_(y.clone(), H, cos, sin, None, wild, False, blocks)
    assert torch.equal(got[0], y[0])  # clamped to t: every row at position 0
    assert torch.equal(got[1], C.rope_(y[1:2].clone(), H, cos, sin, None, None, False, blocks)[0])  # clamped to 0


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rope_position_zero_rows_and_all_zero_doc_start(gpu, C, shape):
    from parameter_server_distributed_amd.ops.attention import doc_starts

    _, S, H = shape
    B = 2
    x = _x(B, S, H, gpu, seed=3)
    cos, sin = _tables(S, gpu)
    rows = [[5, 59] + ([S - 64] if S > 64 else []), _doc_rows(S)]
    doc = doc_starts(rows, S, gpu)
    for inverse in (False, True):
        got = C.rope_(x.clone(), H, cos, sin, None, doc, inverse, 0)
        for b, row in enumerate(rows):
            t = 0
            for n in row:  # the first token of each document is at position 0: unchanged bit for bit
                assert torch.equal(_bits(got[b, t]), _bits(x[b, t])), (b, t)
                if n > 1:
                    assert not torch.equal(got[b, t + 1], x[b, t + 1])
                t += n
        # a document rotates like the same rows at the start of a sequence
        alone = C.rope_(x[:, 5:64].clone(), H, cos, sin, None, None, inverse, 0)
        assert torch.equal(got[0, 5:64], alone[0])
        zero = torch.zeros(B, S, device=gpu, dtype=torch.int32)
        assert torch.equal(_bits(C.rope_(x.clone(), H, cos, sin, None, zero, inverse, 0)),
                           _bits(C.rope_(x.clone(), H, cos, sin, None, None, inverse, 0)))


def test_rope_argument_errors_name_the_argument(gpu, C):
    B, S, H = 2, 64, 2
    x = _x(B, S, H, gpu)
    cos, sin = _tables(S, gpu)
    lens = torch.full((B,), S, device=gpu, dtype=torch.int32)
    doc = torch.zeros(B, S, device=gpu, dtype=torch.int32)
    before = x.clone()

    def bad(match, *args):
        with pytest.raises(RuntimeError, match=match):
            C.rope_(*args)

    bad("qkv", x.float(), H, cos, sin)  # dtype
    bad("qkv", x[:, :, :3 * H * 64 - 8], H, cos, sin)  # non-contiguous
    bad("qkv", x.transpose(0, 1), H, cos, sin)
    bad("qkv", x.cpu(), H, cos.cpu(), sin.cpu())
    bad("qkv.*head dim 64", x, 4, cos, sin)  # head dim 32
    bad("qkv.*head dim 64", x.view(B * S, -1), H, cos, sin)
    bad("heads", x, 0, cos, sin)
    bad("cos", x, H, cos[:S - 1], sin)  # fewer than S rows
    bad("sin", x, H, cos, sin[:S - 1])
    bad("cos", x, H, cos.double(), sin)
    bad("sin", x, H, cos, sin.to(torch.bfloat16))
    bad("cos", x, H, cos[:, :16], sin)
    bad("sin", x, H, cos, sin.cpu())
    bad("lens", x, H, cos, sin, lens.long())
    bad("lens", x, H, cos, sin, lens[:1])
    bad("lens", x, H, cos, sin, lens.cpu())
    bad("lens", x, H, cos, sin, lens.view(B, 1))
    bad("doc_start", x, H, cos, sin, None, doc.long())
    bad("doc_start", x, H, cos, sin, None, doc[:, :S - 1])
    bad("doc_start", x, H, cos, sin, lens, doc.cpu())
    bad("doc_start", x, H, cos, sin, lens, doc.view(-1))
    bad("blocks", x, H, cos, sin, None, None, False, -1)
    assert torch.equal(x, before)  # nothing ran
    # S = 1 and a table longer than S are served
    one = C.rope_(x[:, :1].contiguous(), H, cos, sin)
    assert torch.equal(one, x[:, :1])


def test_rope_is_legal_under_stream_capture(gpu, C):
    B, S, H = 3, 200, 12
    x0 = _x(B, S, H, gpu, seed=4)
    cos, sin = _tables(S, gpu)
    lens, doc = _lens(B, S, gpu), _docs(B, S, gpu)
    fwd = C.rope_(x0.clone(), H, cos, sin, lens, doc, False, 0)
    eager = C.rope_(fwd.clone(), H, cos, sin, lens, doc, True, 0)
    buf, mid = x0.clone(), torch.empty_like(x0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):  # warm-up outside the capture
        C.rope_(buf, H, cos, sin, lens, doc, False, 0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        C.rope_(buf, H, cos, sin, lens, doc, False, 0)
        mid.copy_(buf)
        C.rope_(buf, H, cos, sin, lens, doc, True, 0)
    for _ in range(2):
        buf.copy_(x0)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(_bits(mid), _bits(fwd)) and torch.equal(_bits(buf), _bits(eager))


# ------------------------------------------------------------------------------------------ autograd


def _chain(gpu, B, S, H, lens, doc, seed):
    """x -> MfmaLinear (bias) -> RotaryQK -> FusedSelfAttention(causal) -> backward of a fixed dO. Returns O,
    dqkv at the Linear's output (unrotated), the Linear's weight and bias gradients, and whether the tensor
    the attention got was the Linear's own output."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention
    from parameter_server_distributed_amd.ops.linear import MfmaLinear
    from parameter_server_distributed_amd.ops.rope import RotaryQK

    g = torch.Generator(device="cpu").manual_seed(seed)
    hidden = H * 64
    lin = MfmaLinear(hidden, 3 * hidden).to(gpu).to(torch.bfloat16)
    with torch.no_grad():
        lin.weight.copy_(torch.randn(3 * hidden, hidden, generator=g) * hidden ** -0.5)
        lin.bias.copy_(torch.randn(3 * hidden, generator=g) * 0.1)
    rot = RotaryQK(H, 256).to(gpu)
    attn = FusedSelfAttention(H, p=0.0, causal=True).to(gpu)
    x = torch.randn(B, S, hidden, generator=g).to(torch.bfloat16).to(gpu).requires_grad_(True)
    do = torch.randn(B, S, hidden, generator=g).to(torch.bfloat16).to(gpu)
    kept = {}
    y = lin(x)
    ptr = y.data_ptr()
    y.register_hook(lambda gr: kept.__setitem__("dqkv", gr.detach().clone()))
    r = rot(y, lens, doc)
    assert not hasattr(r, "_psd_src")
    assert attn._kernel_ok(r) or attn._long_kernel_ok(r)
    o = attn(r, lens, doc)
    o.backward(do)
    return (o.detach(), kept["dqkv"], lin.weight.grad.clone(), lin.bias.grad.clone(), x.grad.clone(),
            r.data_ptr() == ptr)


@pytest.mark.parametrize("S", [192, 64])
def test_rotary_module_through_attention_matches_the_composite_chain(gpu, monkeypatch, S):
    """Also the test of the bias hand-over: the QKV Linear's bias gradient must be the column sums of the
    unrotated dqkv. A ``_psd_src`` tag left on the rotated tensor would let the attention hand over the sums
    of the dQKV it wrote, before the inverse rotation, under the same data pointer."""
    B, H = 2, 2
    lens = torch.tensor([S, S - 23], device=gpu, dtype=torch.int32)
    doc = _docs(B, S, gpu)
    for ln, dc in ((None, None), (lens, doc)):
        monkeypatch.setenv("PSD_FEATURES", "")
        got = _chain(gpu, B, S, H, ln, dc, seed=S)
        monkeypatch.setenv("PSD_FEATURES", "rope=0")
        want = _chain(gpu, B, S, H, ln, dc, seed=S)
        monkeypatch.setenv("PSD_FEATURES", "")
        assert got[5] and not want[5]  # in place on the Linear's output / the composite's copy
        o, dqkv, dw, db, dx = (t.float() for t in got[:5])
        o_r, dqkv_r, dw_r, db_r, dx_r = (t.float() for t in want[:5])
        print(f"S {S} lens/docs {ln is not None}: max|dO| {(o - o_r).abs().max():.4f} "
              f"max|ddqkv| {(dqkv - dqkv_r).abs().max():.4f} max|ddW| {(dw - dw_r).abs().max():.4f} of "
              f"{dw_r.abs().max():.2f} max|ddb| {(db - db_r).abs().max():.4f} of {db_r.abs().max():.2f}")
        torch.testing.assert_close(o, o_r, atol=2e-2, rtol=2e-2)
        torch.testing.assert_close(dqkv, dqkv_r, atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(dx, dx_r, atol=3e-2, rtol=3e-2)
        torch.testing.assert_close(dw, dw_r, rtol=1e-2, atol=1e-2 * float(dw_r.abs().max()))
        torch.testing.assert_close(db, db_r, rtol=1e-2, atol=1e-2 * float(db_r.abs().max()))
        sums = dqkv.sum((0, 1))  # fp32 column sums of the unrotated dqkv
        torch.testing.assert_close(db, sums, rtol=1e-2, atol=1e-2 * float(sums.abs().max()) + 1e-6)
        assert float(sums[:2 * H * 64].abs().max()) > 0  # Q and K columns carry gradient
        if ln is not None:
            pad = torch.arange(S, device=gpu)[None, :] >= ln[:, None]
            assert bool((dqkv[pad] == 0).all())


def test_rotary_module_gradient_out_of_place_on_request_and_for_other_layouts(gpu):
    from parameter_server_distributed_amd.ops.rope import RotaryQK, rope_ref

    B, S, H = 2, 64, 2
    rot = RotaryQK(H, 64).to(gpu)
    x = _x(B, S, H, gpu, seed=5)
    g = _x(B, S, H, gpu, seed=6)
    want = rope_ref(g.double(), H, rot.cos, rot.sin, inverse=True)

    def grad_of(make_g, in_place):
        rot.grad_in_place = in_place
        leaf = x.clone().requires_grad_(True)
        y = rot(leaf * 1)
        gg = make_g()
        keep = gg.clone()
        y.backward(gg)
        rot.grad_in_place = True
        return leaf.grad, gg, keep

    dx, gg, keep = grad_of(lambda: g.clone(), True)
    torch.testing.assert_close(dx.double(), want, atol=2e-2, rtol=2e-2)
    dx2, gg2, keep2 = grad_of(lambda: g.clone(), False)
    assert torch.equal(dx2, dx) and torch.equal(gg2, keep2)  # rotated into a copy: the gradient handed in is intact
    # a leaf that requires grad is rotated into a copy as well, and keeps its values
    leaf = x.clone().requires_grad_(True)
    y = rot(leaf)
    assert torch.equal(leaf.detach(), x) and not torch.equal(y.detach(), x)
    y.backward(g.clone())
    assert torch.equal(leaf.grad, dx)


# ------------------------------------------------------------------------------------------ model

TINY = dict(layers=2, hidden=128, heads=2, vocab=512)


def _model(gpu, max_pos, pos="rope"):
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    torch.manual_seed(0)
    m = models.prepare(GPTForLM(**TINY, max_pos=max_pos, pos=pos, dropout=0.0), gpu, torch.bfloat16)
    for t in m.parameters():  # bf16 working weights, as the PS data planes give them
        t.data = t.data.to(torch.bfloat16)
    return m


@pytest.mark.parametrize("kw", [dict(docs=(20, 90)), dict(min_len=100)], ids=["docs", "padded"])
def test_gpt_rope_step_on_the_kernel_matches_the_composite(gpu, monkeypatch, kw):
    from parameter_server_distributed_amd.models.gpt import gpt_batch
    from parameter_server_distributed_amd.ops import rope

    m = _model(gpu, 256)
    assert m.emb.pos.weight.shape[0] == 1 and m.layers[0].rot.cos.dtype == torch.float32
    x, y = gpt_batch(2, 192, TINY["vocab"], gpu, seed=1, **kw)

    def run():
        calls = []
        orig = rope._RopeFn.apply
        rope._RopeFn.apply = lambda *a: calls.append(1) or orig(*a)
        try:
            m.zero_grad(set_to_none=True)
            logits = m(x)
            loss = m.loss(logits, y)
            loss.backward()
        finally:
            rope._RopeFn.apply = orig
        return loss.float().item(), logits.detach().float(), {k: p.grad.float().clone() for k, p in m.named_parameters()}, calls

    la, logits, ga, calls = run()
    assert len(calls) == 2 and math.isfinite(la)  # both blocks on the kernel
    monkeypatch.setenv("PSD_FEATURES", "rope=0")
    lb, _, gb, calls = run()
    monkeypatch.setenv("PSD_FEATURES", "")
    assert not calls
    ulp = 2.0 ** (math.floor(math.log2(logits.abs().max().item())) - 7)  # one bf16 ulp at max|logit| (tests/test_gpt.py)
    print(f"loss kernel {la:.5f}, composite {lb:.5f}, ulp {ulp:.5f}")
    assert abs(la - lb) <= ulp, (la, lb, ulp)
    assert ga.keys() == gb.keys() and len(ga) == 5 + 12 * 2 + 2
    for k in ga:
        assert bool(torch.isfinite(ga[k]).all()), k
        rel = ((ga[k] - gb[k]).norm() / gb[k].norm().clamp_min(1e-30)).item()
        assert rel < 2e-2, (k, rel)


def test_gpt_rope_one_state_dict_serves_two_context_lengths(gpu):
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    a = _model(gpu, 128)
    state = a.state_dict()
    assert not any("cos" in k or "sin" in k or "rot" in k for k in state)
    b = _model(gpu, 256)
    with torch.no_grad():
        for p in b.parameters():
            p.add_(1.0)
    b.load_state_dict(state)  # strict: no table in the state
    for m, S in ((a, 128), (b, 256)):
        x, y = gpt_batch(2, S, TINY["vocab"], gpu, seed=2)
        loss = m.loss(m(x), y)
        loss.backward()
        assert math.isfinite(loss.float().item())
    x, _ = gpt_batch(2, 128, TINY["vocab"], gpu, seed=3)
    assert torch.equal(a(x), b(x))  # the same weights, the same first 128 table rows
    with pytest.raises(ValueError, match="max_pos"):
        a(gpt_batch(1, 192, TINY["vocab"], gpu, seed=2)[0])


def test_gpt_learned_positions_keep_their_state_dict(gpu):
    m = _model(gpu, 256, pos="learned")
    want = {"emb.word.weight": (512, 128), "emb.pos.weight": (256, 128), "emb.tok_type.weight": (2, 128),
            "emb.ln.weight": (128,), "emb.ln.bias": (128,), "head.weight": (512, 128), "head.bias": (512,)}
    for i in range(2):
        for k, s in (("qkv", (384, 128)), ("proj", (128, 128)), ("ffn1", (512, 128)), ("ffn2", (128, 512)),
                     ("ffn2._psd_gelu_from", (512, 128))):
            want[f"layers.{i}.{k}.weight"] = s
            want[f"layers.{i}.{k}.bias"] = s[:1]
        for k in ("ln1", "ln2"):
            want[f"layers.{i}.{k}.weight"] = want[f"layers.{i}.{k}.bias"] = (128,)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert all(layer.rot is None for layer in m.layers)
