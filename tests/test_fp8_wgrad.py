"""The MX fp8 weight gradient of the fp8 Linear layers (feature ``fp8_wgrad``, default off): the split-K
block-scaled GEMM ``gemm_fp8_splitk_`` (kernels/gemm.hip, MX with MODE 1) on its own, and
``MfmaLinear(fp8="mx")`` computing dW = dq(q_t(dy')) dq(q_t(x))^T with both operands e4m3 and the MX blocks
along the tokens -- against fp64 emulations of the very operand bytes, exact on small integers, into the
grad sinks, with its fallbacks, and through the BERT / GPT models, the captured step and a 100-step fit."""
import math

import pytest
import torch
import torch.nn.functional as F

ON = "linear_tune=0,fp8_wgrad=1"
OFF = "linear_tune=0,fp8_wgrad=0"


def _bf16_params(m):
    for p in m.parameters():  # bf16 weights (the PS data plane's working copy)
        p.data = p.data.to(torch.bfloat16)
    return m


def _dq(q, s):
    from parameter_server_distributed_amd.ops import dequantize_mx_ref

    return dequantize_mx_ref(q, s.flatten())


# ---------------------------------------------------------------------------------------- CPU
def test_fp8_wgrad_is_a_feature_and_defaults_to_off(monkeypatch):
    from parameter_server_distributed_amd.ops.fp8_common import FP8_CALLS
    from parameter_server_distributed_amd.utils.config import FEATURES, feature

    assert FEATURES["fp8_wgrad"][0] is False and isinstance(FEATURES["fp8_wgrad"][1], str)
    monkeypatch.setenv("PSD_FEATURES", "")
    assert feature("fp8_wgrad") is False
    monkeypatch.setenv("PSD_FEATURES", "fp8_wgrad=1")
    assert feature("fp8_wgrad") is True
    assert FP8_CALLS["lin_wgrad"] >= 0


@pytest.mark.parametrize("act", [None, "gelu"])
def test_mx_linear_on_the_host_is_still_f_linear(act, monkeypatch):
    from parameter_server_distributed_amd.ops.fp8_common import FP8_CALLS
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    monkeypatch.setenv("PSD_FEATURES", "fp8_wgrad=1")
    torch.manual_seed(0)
    lin = MfmaLinear(128, 256, act=act, fp8="mx")
    ref = torch.nn.Linear(128, 256)
    ref.load_state_dict(lin.state_dict())
    x = torch.randn(128, 128)
    before = dict(FP8_CALLS)
    xa, xb = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    y, want = lin(xa), ref(xb)
    if act == "gelu":
        want = F.gelu(want, approximate="tanh")
    assert torch.equal(y, want)
    g = torch.randn_like(want)
    y.backward(g)
    want.backward(g)
    assert torch.equal(lin.weight.grad, ref.weight.grad) and torch.equal(xa.grad, xb.grad)
    assert FP8_CALLS == before


# ---------------------------------------------------------------------------------------- GPU: native GEMM
# (M, N, K). The first: a partial row tile (136 = 128 + 8), a partial column tile (264 = 256 + 8) and three
# K-tiles, so splits = 2 gives one split of two K-tiles and one of a single K-tile (the start-up path that
# stages its only K-tile twice) and splits = 3 three single-tile splits; the second: whole tiles, eight
# K-tiles, where splits = 0 picks two and splits = 3 rounds k_per_split up (384, 384, 256).
GEMM_SHAPES = [(136, 264, 384), (256, 384, 1024)]
SPLITS = [0, 1, 2, 3]


def _int_operands(M, N, K, gpu, seed=0):
    """|v| <= 3: exact in e4m3 with unit block scales."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    b = torch.randint(-3, 4, (N, K), generator=g).float()
    unit = lambda r: torch.full((r, K // 32), 127, dtype=torch.uint8, device=gpu)  # noqa: E731
    return a, b, a.to(torch.float8_e4m3fn).to(gpu), b.to(torch.float8_e4m3fn).to(gpu), unit(M), unit(N)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_fp8_splitk_is_exact_on_small_integers(gpu, C, shape):
    M, N, K = shape
    a, b, aq, bq, sa, sb = _int_operands(M, N, K, gpu)
    want = a @ b.t()  # |sum| <= 9 K: exact in fp32
    outs = []
    for s in SPLITS:
        out = torch.full((M, N), float("nan"), device=gpu, dtype=torch.float32)
        C.gemm_fp8_splitk_(aq, bq, sa, sb, out, False, 1.0, s)
        torch.testing.assert_close(out.cpu(), want, rtol=0, atol=0)
        outs.append(out)
    assert all(torch.equal(outs[0], o) for o in outs[1:])
    # accumulate onto an integer-valued out with scale 0.5: halves, still exact
    g = torch.Generator().manual_seed(9)
    base = torch.randint(-64, 65, (M, N), generator=g).float()
    for s in SPLITS:
        out = base.to(gpu)
        C.gemm_fp8_splitk_(aq, bq, sa, sb, out, True, 0.5, s)
        torch.testing.assert_close(out.cpu(), base + 0.5 * want, rtol=0, atol=0)
    assert 1 <= C.gemm_fp8_splits(M, N, K) <= max(1, K // 512)


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", GEMM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gemm_fp8_splitk_matches_the_emulation(gpu, C, shape, out_dtype):
    """Gaussian operands with per-row magnitudes 2^-6 .. 2^6 against the float64 product of
    dequantize_mx_ref of the very bytes passed in: elementwise |got - ref| <= K 2^-23 (|dqA| |dqB|^T), the
    worst case of a length-K fp32 accumulation with one extra bit for a truncating accumulator; a bf16 out
    adds one bf16 rounding, 2^-8 |ref|."""
    from parameter_server_distributed_amd.ops import quantize_mx_ref

    M, N, K = shape
    g = torch.Generator().manual_seed(M + N + K)
    ops = []
    for rows in (M, N):
        v = torch.randn(rows, K, generator=g) * torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g).float())
        ops.append(quantize_mx_ref(v.to(torch.bfloat16)))
    (aq, sa), (bq, sb) = ops
    A, B = _dq(aq, sa).double(), _dq(bq, sb).double()
    ref = A @ B.t()
    bound = K * 2.0 ** -23 * (A.abs() @ B.abs().t())
    if out_dtype == torch.bfloat16:
        bound = bound + 2.0 ** -8 * ref.abs()
    dev = lambda q, s, r: (q.to(gpu), s.view(r, K // 32).to(gpu))  # noqa: E731
    (aq, sa), (bq, sb) = dev(aq, sa, M), dev(bq, sb, N)
    for s in SPLITS:
        out = torch.empty(M, N, device=gpu, dtype=out_dtype)
        C.gemm_fp8_splitk_(aq, bq, sa, sb, out, False, 1.0, s)
        err = (out.double().cpu() - ref).abs()
        print(f"gemm_fp8_splitk {shape} {out_dtype} splits {s}: max err / bound "
              f"{float((err / bound.clamp_min(1e-300)).max()):.4f}, relative L2 {float(err.norm() / ref.norm()):.3e}")
        assert bool((err <= bound).all()), float((err - bound).max())


@pytest.mark.gpu
@pytest.mark.parametrize("out_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_gemm_fp8_splitk_writes_nothing_outside_out(gpu, C, out_dtype):
    M, N, K = GEMM_SHAPES[0]
    a, b, aq, bq, sa, sb = _int_operands(M, N, K, gpu, seed=3)
    pad = 4096
    for s in (0, 2, 3):
        buf = torch.full((M * N + 2 * pad,), -7.0, device=gpu, dtype=out_dtype)
        out = buf[pad:pad + M * N].view(M, N)
        C.gemm_fp8_splitk_(aq, bq, sa, sb, out, False, 1.0, s)
        torch.testing.assert_close(out.float().cpu(), (a @ b.t()).to(out_dtype).float(), rtol=0, atol=0)
        raw = buf.view(torch.uint8).view(-1, buf.element_size())
        sentinel = torch.full((1,), -7.0, device=gpu, dtype=out_dtype).view(torch.uint8)
        assert bool((raw[:pad] == sentinel).all()) and bool((raw[pad + M * N:] == sentinel).all())


@pytest.mark.gpu
def test_gemm_fp8_splitk_refuses_what_is_outside_its_contract(gpu, C):
    M, N, K = 128, 256, 256
    _, _, aq, bq, sa, sb = _int_operands(M, N, K, gpu)
    out = torch.full((M, N), -7.0, device=gpu, dtype=torch.float32)
    C.gemm_fp8_splitk_(aq, bq, sa, sb, out, False, 1.0, 2)  # the contract itself
    out.fill_(-7.0)
    one = torch.ones(1, device=gpu)
    wide = torch.full((M, 2 * N), -7.0, device=gpu, dtype=torch.float32)
    k192 = lambda q: q[:, :192].contiguous()  # noqa: E731
    s192 = lambda s: s[:, :6].contiguous()  # noqa: E731
    bad = [
        lambda: C.gemm_fp8_splitk_(aq.view(torch.uint8).view(torch.float8_e5m2), bq, sa, sb, out, False, 1.0, 2),
        lambda: C.gemm_fp8_splitk_(aq, bq, one, one, out, False, 1.0, 2),  # per-tensor fp32 scales
        lambda: C.gemm_fp8_splitk_(k192(aq), k192(bq), s192(sa), s192(sb), out, False, 1.0, 2),  # K = 192
        lambda: C.gemm_fp8_splitk_(aq, bq, sa, sb, wide[:, :N], False, 1.0, 2),  # a non-contiguous out
        lambda: C.gemm_fp8_splitk_(aq, bq, sa.cpu(), sb.cpu(), out, False, 1.0, 2),  # host scales
        lambda: C.gemm_fp8_splitk_(aq, bq, sa, sb, out[:, :N - 8].contiguous(), False, 1.0, 2),  # a mis-shaped out
    ]
    for call in bad:
        with pytest.raises(RuntimeError):
            call()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all()) and bool((wide == -7.0).all())  # nothing was launched


# ---------------------------------------------------------------------------------------- GPU: module
LIN_SHAPES = [(384, 384, 128), (256, 768, 384)]  # (tokens, in, out): three and two K-tiles of tokens


def _act(z, act):
    return F.gelu(z, approximate="tanh") if act == "gelu" else z


def _pair(gpu, K, N, act, ints=False, seed=0):
    """An ``fp8="mx"`` Linear and a bf16 one with the same weights."""
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    torch.manual_seed(seed)
    l8 = _bf16_params(MfmaLinear(K, N, act=act, fp8="mx").to(gpu))
    with torch.no_grad():
        if ints:
            l8.weight.copy_(torch.randint(-3, 4, (N, K)).float())
            l8.bias.zero_()
        else:
            l8.weight.copy_(torch.randn(N, K) * 0.05)
            l8.bias.copy_(torch.randn(N) * 0.5)
    lb = _bf16_params(MfmaLinear(K, N, act=act).to(gpu))
    lb.load_state_dict(l8.state_dict())
    return l8, lb


def _calls():
    from parameter_server_distributed_amd.ops.fp8_common import FP8_CALLS

    return FP8_CALLS


@pytest.mark.gpu
@pytest.mark.parametrize("act", [None, "gelu"], ids=["none", "gelu"])
@pytest.mark.parametrize("shape", LIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mx_linear_weight_gradient_matches_the_mx_emulation(gpu, C, shape, act, monkeypatch):
    """weight.grad against dq(q_t(dy')) dq(q_t(x))^T in float64 on the host from quantize_mx_ref of the
    transposed copies: |got - ref| <= tokens 2^-23 (|A| |B|^T) + 2^-8 |ref| (the GEMM test's bound plus the
    bf16 rounding of the stored gradient); exactly one fp8 weight-gradient launch per backward; the bias
    and input gradients bitwise those of the run with fp8_wgrad off."""
    from parameter_server_distributed_amd.ops import quantize_mx_ref

    monkeypatch.setenv("PSD_FEATURES", ON)
    M, K, N = shape
    l8, _ = _pair(gpu, K, N, act)
    torch.manual_seed(1)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(M, N, device=gpu).to(torch.bfloat16)
    before = dict(_calls())
    y = l8(x)
    if act == "gelu":  # dy' from the kernel the backward itself runs
        dyp = torch.empty_like(dy)
        C.gelu_bwd_colsum_(dy, l8._psd_gelu_pre, dyp, torch.empty(N, device=gpu, dtype=torch.bfloat16), False)
    else:
        dyp = dy
    y.backward(dy)
    assert _calls()["lin_wgrad"] == before["lin_wgrad"] + 1
    assert _calls()["lin_dgrad"] == before["lin_dgrad"] + 1
    gq, sg = quantize_mx_ref(dyp.cpu().t().contiguous())
    xq, sx = quantize_mx_ref(x.detach().cpu().t().contiguous())
    A, B = _dq(gq, sg).double(), _dq(xq, sx).double()
    ref = A @ B.t()
    bound = M * 2.0 ** -23 * (A.abs() @ B.abs().t()) + 2.0 ** -8 * ref.abs()
    assert l8.weight.grad.dtype == torch.bfloat16 and l8.weight.grad.shape == (N, K)
    err = (l8.weight.grad.double().cpu() - ref).abs()
    print(f"fp8 wgrad {shape} act {act}: max err / bound {float((err / bound.clamp_min(1e-300)).max()):.4f}, "
          f"relative L2 vs the emulation {float(err.norm() / ref.norm()):.3e}")
    assert bool((err <= bound).all()), float((err - bound).max())
    got = (x.grad.clone(), l8.bias.grad.clone())
    # the same step with the feature off: the counter rests, dx and db keep their bits
    monkeypatch.setenv("PSD_FEATURES", OFF)
    x.grad = None
    l8.zero_grad(set_to_none=True)
    mid = dict(_calls())
    l8(x).backward(dy)
    assert _calls()["lin_wgrad"] == mid["lin_wgrad"] and _calls()["lin_dgrad"] == mid["lin_dgrad"] + 1
    assert torch.equal(x.grad, got[0]) and torch.equal(l8.bias.grad, got[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", LIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mx_linear_weight_gradient_is_exact_on_small_integers(gpu, shape, monkeypatch):
    """|v| <= 3 is exact in e4m3 with unit block scales: weight.grad is bf16(di^T xi)."""
    monkeypatch.setenv("PSD_FEATURES", ON)
    M, K, N = shape
    l8, _ = _pair(gpu, K, N, None, ints=True)
    g = torch.Generator().manual_seed(5)
    xi = torch.randint(-3, 4, (M, K), generator=g).float()
    di = torch.randint(-3, 4, (M, N), generator=g).float()
    x = xi.to(gpu, torch.bfloat16).requires_grad_(True)
    before = _calls()["lin_wgrad"]
    l8(x).backward(di.to(gpu, torch.bfloat16))
    assert _calls()["lin_wgrad"] == before + 1
    torch.testing.assert_close(l8.weight.grad.float().cpu(), (di.t() @ xi).to(torch.bfloat16).float(), rtol=0, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("sink_dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_mx_linear_weight_gradient_lands_in_the_grad_sink(gpu, sink_dtype, monkeypatch):
    """With a ``_psd_grad_sink`` (the PS data plane's hook) the GEMM's reduce writes the view it returns,
    in the view's dtype, and nothing beside it. A bf16 view is adopted as weight.grad (no second tensor);
    an fp32 view holds the unrounded sums (autograd casts what it hands the bf16 parameter)."""
    monkeypatch.setenv("PSD_FEATURES", ON)
    M, K, N = LIN_SHAPES[0]
    l8, _ = _pair(gpu, K, N, None, ints=True)
    g = torch.Generator().manual_seed(6)
    xi = torch.randint(-3, 4, (M, K), generator=g).float()
    di = torch.randint(-3, 4, (M, N), generator=g).float()
    pad = 1024
    buf = torch.full((N * K + 2 * pad,), -7.0, device=gpu, dtype=sink_dtype)
    view = buf[pad:pad + N * K].view(N, K)
    asked = []

    def sink(p):
        asked.append(p)
        return view.view(view.shape) if p is l8.weight else None

    l8._psd_grad_sink = sink
    before = _calls()["lin_wgrad"]
    l8(xi.to(gpu, torch.bfloat16)).backward(di.to(gpu, torch.bfloat16))
    assert _calls()["lin_wgrad"] == before + 1 and any(p is l8.weight for p in asked)
    want = di.t() @ xi
    torch.testing.assert_close(view.float().cpu(), want.to(sink_dtype).float(), rtol=0, atol=0)
    assert bool((buf[:pad] == -7.0).all()) and bool((buf[pad + N * K:] == -7.0).all())
    if sink_dtype == torch.bfloat16:
        assert l8.weight.grad.data_ptr() == view.data_ptr()
    else:
        torch.testing.assert_close(l8.weight.grad.float().cpu(), want.to(torch.bfloat16).float(), rtol=0, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [None, "gelu"], ids=["none", "gelu"])
def test_mx_linear_weight_gradient_fallbacks_are_the_bf16_bits(gpu, C, act, monkeypatch):
    """136 tokens (no multiple of 128) with the feature on, and 256 tokens with it off: the bf16 weight
    gradient runs, the counter rests, and the bits are a bf16 MfmaLinear's from the same x and dy'."""
    for feats, M in ((ON, 136), (OFF, 256)):
        monkeypatch.setenv("PSD_FEATURES", feats)
        K, N = 256, 256
        l8, _ = _pair(gpu, K, N, act)
        _, lb = _pair(gpu, K, N, None)  # same weights (same seed), no activation
        torch.manual_seed(2)
        x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
        dy = torch.randn(M, N, device=gpu).to(torch.bfloat16)
        before = dict(_calls())
        x8 = x.clone().requires_grad_(True)
        y = l8(x8)
        if act == "gelu":
            dyp = torch.empty_like(dy)
            db_want = torch.empty(N, device=gpu, dtype=torch.bfloat16)
            C.gelu_bwd_colsum_(dy, l8._psd_gelu_pre, dyp, db_want, False)
        else:
            dyp = dy
        y.backward(dy)
        assert _calls()["lin_wgrad"] == before["lin_wgrad"]
        assert _calls()["lin_dgrad"] == before["lin_dgrad"] + 1
        xb = x.clone().requires_grad_(True)
        lb(xb).backward(dyp)
        assert torch.equal(l8.weight.grad, lb.weight.grad)
        assert torch.equal(l8.bias.grad, db_want if act == "gelu" else lb.bias.grad)


@pytest.mark.gpu
def test_mx_linear_with_fp8_wgrad_against_fp32_linear(gpu, monkeypatch):
    """The shape and bounds of test_mx_linear_against_fp32_linear (256 tokens, 512 -> 384, GELU): relative
    L2 of dW against an fp32 nn.Linear < 0.08 (the emulation of the recipe alone gives 0.038 there)."""
    monkeypatch.setenv("PSD_FEATURES", ON)
    l8, _ = _pair(gpu, 512, 384, "gelu")
    ref = torch.nn.Linear(512, 384).to(gpu)
    with torch.no_grad():
        ref.weight.copy_(l8.weight.float())
        ref.bias.copy_(l8.bias.float())
    torch.manual_seed(0)
    x = torch.randn(256, 512, device=gpu)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    before = _calls()["lin_wgrad"]
    y = l8(xb)
    yr = F.gelu(ref(xr), approximate="tanh")
    g = torch.randn_like(yr)
    y.backward(g.to(torch.bfloat16))
    yr.backward(g)
    assert _calls()["lin_wgrad"] == before + 1
    rel = float((y.detach().float() - yr.detach()).norm() / yr.detach().norm())
    relx = float((xb.grad.float() - xr.grad).norm() / xr.grad.norm())
    relw = float((l8.weight.grad.float() - ref.weight.grad).norm() / ref.weight.grad.norm())
    print(f"MX fp8 Linear with fp8_wgrad vs fp32: relative L2 y {rel:.4f} dx {relx:.4f} dW {relw:.4f}")
    assert rel < 0.06, rel
    assert relx < 0.08 and relw < 0.08, (relx, relw)


# ---------------------------------------------------------------------------------------- GPU: models
SIZES = dict(layers=2, hidden=768, heads=12, vocab=2048)
SEQ, BATCH = 32, 4  # 128 tokens: one K-tile, one split


def _build(name, gpu, fp8, seed=0, **kw):
    from parameter_server_distributed_amd import models

    torch.manual_seed(seed)
    spec = models.build(name, gpu, torch.bfloat16, fp8=fp8, **{**SIZES, "seq_len": SEQ, **kw})
    _bf16_params(spec.model).train()
    return spec


def _grads(spec, batch):
    x, y = batch
    spec.model.zero_grad(set_to_none=True)
    loss = spec.loss(spec.model(x), y)
    loss.backward()
    return float(loss.detach().float()), {n: p.grad.float().clone() for n, p in spec.model.named_parameters()}


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bert_base", "gpt_small"])
def test_fp8_transformer_step_runs_the_fp8_weight_gradients(gpu, name, monkeypatch):
    """One forward / backward of the 2-layer model with fp8=True and fp8_wgrad on: 8 fp8 weight gradients
    beside the 8 forward and 8 bwd-data GEMMs; the gradients against the fp8=False model at the bounds of
    test_fp8_transformer_step_runs_the_fp8_linears_and_tracks_bf16 (cosine > 0.9, norm ratio in (0.8, 1.25))."""
    monkeypatch.setenv("PSD_FEATURES", ON)
    s8 = _build(name, gpu, True)
    sb = _build(name, gpu, False)
    sb.model.load_state_dict(s8.model.state_dict())
    batch = s8.make_batch(BATCH, gpu)
    before = dict(_calls())
    loss8, g8 = _grads(s8, batch)
    for k in ("lin_fwd", "lin_dgrad", "lin_wgrad"):
        assert _calls()[k] - before[k] == 8, (k, _calls()[k] - before[k])
    lossb, gb = _grads(sb, batch)
    assert _calls()["lin_wgrad"] - before["lin_wgrad"] == 8  # the bf16 model launches none
    assert math.isfinite(loss8) and all(bool(torch.isfinite(g).all()) for g in g8.values())
    dot = sum(float((g8[n] * gb[n]).sum()) for n in gb)
    n8 = sum(float(g.pow(2).sum()) for g in g8.values()) ** 0.5
    nb = sum(float(g.pow(2).sum()) for g in gb.values()) ** 0.5
    print(f"{name} fp8 + fp8_wgrad vs bf16 first-step gradient: cosine {dot / (n8 * nb):.4f}, "
          f"norm ratio {n8 / nb:.4f}, loss {loss8:.4f} vs {lossb:.4f}")
    assert dot / (n8 * nb) > 0.9, dot / (n8 * nb)
    assert 0.8 < n8 / nb < 1.25, n8 / nb


@pytest.mark.gpu
def test_trainer_captures_the_fp8_gpt_step_with_fp8_wgrad(gpu, monkeypatch):
    """The fp8 weight gradient reads nothing from the device on the host: the Trainer captures the step,
    and the captured run's losses are finite and fall (test_trainer_captures_the_fp8_gpt_step with the
    feature on)."""
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    monkeypatch.setenv("PSD_FEATURES", ON)
    spec = _build("gpt_small", gpu, True, min_seq_len=8)
    batch = spec.make_batch(BATCH, gpu)
    ps = CollectivePS(spec.model, OptimConfig("adamw", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    before = _calls()["lin_wgrad"]
    losses = [tr.step().float().item() for _ in range(5)]
    torch.cuda.synchronize()
    assert _calls()["lin_wgrad"] > before
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses


@pytest.mark.gpu
def test_fp8_wgrad_tiny_bert_100_step_convergence(gpu, monkeypatch):
    """test_fp8_tiny_bert_100_step_convergence with a third arm: 100 AdamW steps of a tiny BERT on a fixed
    synthetic batch set from the same init and batch order -- bf16, MX fp8 Linears, and MX fp8 Linears
    with the fp8 weight gradient (1,024 tokens per step). Every arm fits the set (last-10 mean loss < 0.5x
    the first-5 mean) and each fp8 arm's mean loss over the run is within 10 % of the bf16 run's."""
    curves = {}
    arms = {"bf16": (False, "fp8_wgrad=0"), "fp8": (True, "fp8_wgrad=0"), "fp8+wgrad": (True, "fp8_wgrad=1")}
    counts = {}
    for arm, (fp8, feats) in arms.items():
        monkeypatch.setenv("PSD_FEATURES", feats)
        before = dict(_calls())
        spec = _build("bert_base", gpu, fp8, layers=2, hidden=256, heads=4, vocab=512, seq_len=64)
        batches = [spec.make_batch(16, gpu, seed=s) for s in range(4)]
        opt = torch.optim.AdamW(spec.model.parameters(), lr=1e-3)
        L = []
        for i in range(100):
            x, y = batches[i % len(batches)]
            opt.zero_grad(set_to_none=True)
            loss = spec.loss(spec.model(x), y)
            loss.backward()
            opt.step()
            L.append(loss.detach().float())
        curves[arm] = [float(v) for v in torch.stack(L).cpu()]
        counts[arm] = {k: _calls()[k] - before[k] for k in ("lin_fwd", "lin_dgrad", "lin_wgrad")}
    assert counts["bf16"] == {"lin_fwd": 0, "lin_dgrad": 0, "lin_wgrad": 0}
    assert counts["fp8"] == {"lin_fwd": 800, "lin_dgrad": 800, "lin_wgrad": 0}
    assert counts["fp8+wgrad"] == {"lin_fwd": 800, "lin_dgrad": 800, "lin_wgrad": 800}
    avg = lambda L, a, b: sum(L[a:b]) / (b - a)  # noqa: E731
    print("; ".join(f"{arm}: first-5 {avg(L, 0, 5):.4f} mean {avg(L, 0, 100):.4f} last-10 {avg(L, 90, 100):.4f}"
                    for arm, L in curves.items()))
    for L in curves.values():
        assert all(math.isfinite(v) for v in L)
        assert avg(L, 90, 100) < 0.5 * avg(L, 0, 5), (avg(L, 0, 5), avg(L, 90, 100))
    lb = curves["bf16"]
    for arm in ("fp8", "fp8+wgrad"):
        assert abs(avg(curves[arm], 0, 100) - avg(lb, 0, 100)) <= 0.10 * avg(lb, 0, 100), arm
