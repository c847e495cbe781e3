"""MX fp8 Linear layers (``MfmaLinear(fp8="mx")``, ops/linear.py) and the BERT / GPT models built with
``fp8=True``: the forward and bwd-data GEMMs against fp32 emulations of the MX operands, the bf16 weight
and bias gradients against the bf16 module's bits, the fused LayerNorm's MX hand-over, the fallbacks, and
the models through the eager, the PS and the captured step."""
import math

import pytest
import torch
import torch.nn.functional as F


def _bf16_params(m):
    for p in m.parameters():  # bf16 weights (the PS data plane's working copy)
        p.data = p.data.to(torch.bfloat16)
    return m


# ---------------------------------------------------------------------------------------- CPU
def test_fp8_mode_is_validated():
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    for ok in (False, True, "mx"):
        assert MfmaLinear(128, 128, fp8=ok).fp8 == ok
    assert MfmaLinear(128, 128).fp8 is False
    for bad in ("nope", "MX", 1, None, "fp8"):
        with pytest.raises(ValueError):
            MfmaLinear(128, 128, fp8=bad)


@pytest.mark.parametrize("act", [None, "gelu"])
def test_mx_linear_on_the_host_is_f_linear(act):
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    torch.manual_seed(0)
    lin = MfmaLinear(128, 256, act=act, fp8="mx")
    x = torch.randn(5, 128)
    want = F.linear(x, lin.weight, lin.bias)
    if act == "gelu":
        want = F.gelu(want, approximate="tanh")
    assert torch.equal(lin(x), want)


def test_build_marks_the_encoder_linears_and_wires_the_layernorms():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    cpu = torch.device("cpu")
    for name in ("bert_base", "gpt_small"):
        kw = dict(layers=2, hidden=256, heads=4, vocab=512)
        m8 = models.build(name, cpu, torch.float32, fp8=True, **kw).model
        mx = sorted(n for n, m in m8.named_modules() if isinstance(m, MfmaLinear) and m.fp8 == "mx")
        assert mx == sorted(f"layers.{i}.{n}" for i in range(2) for n in ("qkv", "proj", "ffn1", "ffn2"))
        rest = [m for n, m in m8.named_modules() if isinstance(m, MfmaLinear) and n not in mx]
        assert rest and all(m.fp8 is False for m in rest)  # the MLM head / decoder / LM head
        l0, l1 = m8.layers
        assert l0.ln1._psd_mx_to is l0.ffn1 and l1.ln1._psd_mx_to is l1.ffn1
        assert l0.ln2._psd_mx_to is l1.qkv and l1.ln2._psd_mx_to is None
        # fp8=False builds the model as before
        a = models.build(name, cpu, torch.float32, **kw).model
        b = models.build(name, cpu, torch.float32, fp8=False, **kw).model
        for m in (a, b):
            assert all(x.fp8 is False for x in m.modules() if isinstance(x, MfmaLinear))
            assert all(layer.ln1._psd_mx_to is None and layer.ln2._psd_mx_to is None for layer in m.layers)
        shapes = [[(n, tuple(p.shape)) for n, p in m.named_parameters()] for m in (a, b, m8)]
        assert shapes[0] == shapes[1] == shapes[2]
        assert [n for n, _ in a.named_modules()] == [n for n, _ in m8.named_modules()]


def test_fp8_ln_handover_is_a_feature():
    from parameter_server_distributed_amd.utils.config import FEATURES

    assert FEATURES["fp8_ln_handover"][0] is True


# ---------------------------------------------------------------------------------------- GPU: LayerNorm
@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
def test_layernorm_writes_the_consumers_mx_operand(gpu, C, p, monkeypatch):
    from parameter_server_distributed_amd.ops import quantize_mx
    from parameter_server_distributed_amd.ops.handover import Q8Pending
    from parameter_server_distributed_amd.ops.layernorm import FusedAddLayerNorm
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    torch.manual_seed(3)
    H, M = 768, 64
    ln = _bf16_params(FusedAddLayerNorm(H, p=p, seed=7).to(gpu)).train()
    with torch.no_grad():
        ln.weight.copy_(0.5 + torch.rand(H))
        ln.bias.copy_(0.3 * torch.randn(H))
    cons = _bf16_params(MfmaLinear(H, 256, fp8="mx").to(gpu))
    ln.psd_mx_output_to(cons)
    assert "_psd_mx_to" not in dict(ln.named_modules())  # a reference, not a submodule
    # rows of very different magnitude: the block scales differ along the row
    x = (torch.randn(M, H, device=gpu) * torch.exp2(torch.randint(-4, 5, (1, H), device=gpu).float())).to(torch.bfloat16)
    h = torch.randn(M, H, device=gpu).to(torch.bfloat16)
    y = ln(x, h)
    rec = cons._psd_q8_pending
    assert isinstance(rec, Q8Pending) and rec.t.data_ptr() == y.data_ptr() and rec.t.shape == y.shape
    q, s = quantize_mx(y.detach())
    assert torch.equal(rec.scales.flatten(), s)
    assert torch.equal(rec.q.view(torch.uint8), q.view(torch.uint8))
    # y, s, mean, rstd: bitwise those of the call without the MX outputs
    plain = C.ln_fwd(x, h, ln.weight, ln.bias, ln.eps, p, ln.seed, None)
    q8 = torch.empty(M, H, device=gpu, dtype=torch.float8_e4m3fn)
    sc8 = torch.empty(M * H // 32, device=gpu, dtype=torch.uint8)
    both = C.ln_fwd(x, h, ln.weight, ln.bias, ln.eps, p, ln.seed, None, q8, sc8)
    for a, b in zip(plain, both):
        assert torch.equal(a, b)
    assert torch.equal(both[0], y.detach()) and torch.equal(q8.view(torch.uint8), q.view(torch.uint8))
    # the consumer takes the record for exactly that tensor, once
    before = cons.psd_mx_handovers
    cons(y)
    assert cons.psd_mx_handovers == before + 1 and cons._psd_q8_pending is None
    ln(x, h)
    cons(y.clone())  # another tensor: the record is dropped, not used
    assert cons.psd_mx_handovers == before + 1 and cons._psd_q8_pending is None
    # feature off: no record
    monkeypatch.setenv("PSD_FEATURES", "fp8_ln_handover=0")
    ln(x, h)
    assert cons._psd_q8_pending is None


# ---------------------------------------------------------------------------------------- GPU: Linear
SHAPES = [(136, 256, 256), (256, 768, 384)]  # (M, K, N): a partial row tile at the smallest sensible K; BERT's K


def _dq(q, s):
    from parameter_server_distributed_amd.ops import dequantize_mx_ref

    return dequantize_mx_ref(q, s.flatten())


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


@pytest.mark.gpu
@pytest.mark.parametrize("act", [None, "gelu"], ids=["none", "gelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mx_linear_forward_and_dx_match_the_mx_emulation(gpu, C, shape, act, monkeypatch):
    """y against act(dq(q(x)) dq(q(W))^T + b) and dx against dq(q_e5m2(dy')) dq(q_t(W))^T in fp32 on the
    host (rtol = atol = 1e-2, the bound of test_gemm_fp8_quantized_matches_dequant_reference for the same
    kernel); with a handed-over residual gradient dx is that product added onto it, one bf16 rounding."""
    from parameter_server_distributed_amd.ops import conv as conv_ops
    from parameter_server_distributed_amd.ops import quantize_mx_ref

    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    M, K, N = shape
    l8, _ = _pair(gpu, K, N, act)
    torch.manual_seed(1)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16).requires_grad_(True)
    dy = torch.randn(M, N, device=gpu).to(torch.bfloat16)
    before = dict(conv_ops.FP8_CALLS)
    y = l8(x)
    xq, sx = quantize_mx_ref(x.detach().cpu())
    wq, sw = quantize_mx_ref(l8.weight.detach().cpu())
    want = _act(_dq(xq, sx) @ _dq(wq, sw).t() + l8.bias.detach().float().cpu(), act)
    torch.testing.assert_close(y.detach().float().cpu(), want, rtol=1e-2, atol=1e-2)
    # dy' (the gradient after the activation backward) from the kernel the backward itself runs
    if act == "gelu":
        dyp = torch.empty_like(dy)
        C.gelu_bwd_colsum_(dy, l8._psd_gelu_pre, dyp, torch.empty(N, device=gpu, dtype=torch.bfloat16), False)
    else:
        dyp = dy
    y.backward(dy)
    assert conv_ops.FP8_CALLS["lin_fwd"] == before["lin_fwd"] + 1
    assert conv_ops.FP8_CALLS["lin_dgrad"] == before["lin_dgrad"] + 1
    assert conv_ops.FP8_CALLS["ps_weights"] == before["ps_weights"]
    gq, sg = quantize_mx_ref(dyp.cpu(), e5m2=True)
    tq, st = quantize_mx_ref(l8.weight.detach().t().contiguous().cpu())
    want_dx = _dq(gq, sg) @ _dq(tq, st).t()
    torch.testing.assert_close(x.grad.float().cpu(), want_dx, rtol=1e-2, atol=1e-2)
    # the residual hand-over: the same product added onto the handed-over gradient
    dx0 = x.grad.clone()
    x.grad = None
    y = l8(x)
    handed = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    l8._psd_pending_dx.append((l8._psd_tok, handed.clone()))
    y.backward(dy)
    torch.testing.assert_close(x.grad, (handed.float() + dx0.float()).to(torch.bfloat16), rtol=2.0 ** -7, atol=0)
    assert not l8._psd_pending_dx and not l8._psd_gelu_hands


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mx_linear_is_exact_on_small_integers(gpu, shape):
    """|v| <= 3 is exact in e4m3 and e5m2 with unit block scales: y and dx are the exact products."""
    M, K, N = shape
    l8, _ = _pair(gpu, K, N, None, ints=True)
    g = torch.Generator().manual_seed(5)
    xi = torch.randint(-3, 4, (M, K), generator=g).float()
    di = torch.randint(-3, 4, (M, N), generator=g).float()
    x = xi.to(gpu, torch.bfloat16).requires_grad_(True)
    # fp32 output through the native op (bf16 cannot hold every sum): the module's operands, its GEMM
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops import quantize_mx, quantize_mx_t

    wf = l8.weight.detach().float().cpu()
    out = torch.empty(M, N, device=gpu, dtype=torch.float32)
    xq, sx = quantize_mx(x.detach())
    wq, sw = quantize_mx(l8.weight.detach())
    native().gemm_fp8_(xq, wq, sx, sw, out)
    torch.testing.assert_close(out.cpu(), xi @ wf.t(), rtol=0, atol=0)
    dq, ds = quantize_mx(di.to(gpu, torch.bfloat16), e5m2=True)
    tq, ts = quantize_mx_t(l8.weight.detach())
    dxo = torch.empty(M, K, device=gpu, dtype=torch.float32)
    native().gemm_fp8_(dq, tq, ds, ts, dxo)
    torch.testing.assert_close(dxo.cpu(), di @ wf, rtol=0, atol=0)
    # and through the module: the exact products rounded to bf16 once
    y = l8(x)
    y.backward(di.to(gpu, torch.bfloat16))
    torch.testing.assert_close(y.detach().float().cpu(), (xi @ wf.t()).to(torch.bfloat16).float(), rtol=0, atol=0)
    torch.testing.assert_close(x.grad.float().cpu(), (di @ wf).to(torch.bfloat16).float(), rtol=0, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("act", [None, "gelu"], ids=["none", "gelu"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_mx_linear_weight_and_bias_gradients_are_the_bf16_bits(gpu, C, shape, act, monkeypatch):
    """dW and db stay bf16 on the saved bf16 x and dy': with linear_tune off, bitwise what a bf16
    MfmaLinear produces from the same x and dy' (for GELU dy' depends on the fp8 pre-activation, so
    the bf16 module is given that dy' directly)."""
    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    M, K, N = shape
    l8, _ = _pair(gpu, K, N, act)
    _, lb = _pair(gpu, K, N, None)  # same weights (same seed), no activation
    torch.manual_seed(2)
    x = torch.randn(M, K, device=gpu).to(torch.bfloat16)
    dy = torch.randn(M, N, device=gpu).to(torch.bfloat16)
    x8 = x.clone().requires_grad_(True)
    y = l8(x8)
    if act == "gelu":
        dyp = torch.empty_like(dy)
        db_want = torch.empty(N, device=gpu, dtype=torch.bfloat16)
        C.gelu_bwd_colsum_(dy, l8._psd_gelu_pre, dyp, db_want, False)
    else:
        dyp = dy
    y.backward(dy)
    xb = x.clone().requires_grad_(True)
    lb(xb).backward(dyp)
    assert torch.equal(l8.weight.grad, lb.weight.grad)
    assert torch.equal(l8.bias.grad, db_want if act == "gelu" else lb.bias.grad)


@pytest.mark.gpu
def test_mx_linear_against_fp32_linear(gpu):
    """Relative L2 of y, dx, dW against an fp32 nn.Linear, at the bounds test_mfma_linear_fp8_forward_backward
    sets for the per-tensor stub on the same shape: 0.06 forward, 0.08 gradients."""
    l8, _ = _pair(gpu, 512, 384, "gelu")
    ref = torch.nn.Linear(512, 384).to(gpu)
    with torch.no_grad():
        ref.weight.copy_(l8.weight.float())
        ref.bias.copy_(l8.bias.float())
    torch.manual_seed(0)
    x = torch.randn(256, 512, device=gpu)
    xb = x.to(torch.bfloat16).requires_grad_(True)
    xr = x.clone().requires_grad_(True)
    y = l8(xb)
    yr = F.gelu(ref(xr), approximate="tanh")
    g = torch.randn_like(yr)
    y.backward(g.to(torch.bfloat16))
    yr.backward(g)
    rel = float((y.detach().float() - yr.detach()).norm() / yr.detach().norm())
    relx = float((xb.grad.float() - xr.grad).norm() / xr.grad.norm())
    relw = float((l8.weight.grad.float() - ref.weight.grad).norm() / ref.weight.grad.norm())
    print(f"MX fp8 Linear vs fp32: relative L2 y {rel:.4f} dx {relx:.4f} dW {relw:.4f}")
    assert rel < 0.06, rel
    assert relx < 0.08 and relw < 0.08, (relx, relw)


@pytest.mark.gpu
def test_mx_linear_outside_the_contract_runs_the_bf16_path(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops import conv as conv_ops

    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    l8, lb = _pair(gpu, 192, 256, "gelu")  # K % 128 != 0
    torch.manual_seed(4)
    x = torch.randn(64, 192, device=gpu).to(torch.bfloat16)
    dy = torch.randn(64, 256, device=gpu).to(torch.bfloat16)
    before = dict(conv_ops.FP8_CALLS)
    outs = []
    for lin in (l8, lb):
        xi = x.clone().requires_grad_(True)
        y = lin(xi)
        y.backward(dy)
        outs.append((y.detach(), xi.grad, lin.weight.grad, lin.bias.grad))
    assert conv_ops.FP8_CALLS == before
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    # feature fp8_compute off: the same for a shape inside the contract
    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0,fp8_compute=0")
    l8, lb = _pair(gpu, 256, 256, None)
    xi = torch.randn(64, 256, device=gpu).to(torch.bfloat16)
    assert torch.equal(l8(xi), lb(xi)) and conv_ops.FP8_CALLS == before


# ---------------------------------------------------------------------------------------- GPU: models
SIZES = dict(layers=2, hidden=768, heads=12, vocab=2048)
SEQ, BATCH = 32, 4


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
def test_fp8_transformer_step_runs_the_fp8_linears_and_tracks_bf16(gpu, name):
    """One forward / backward of the 2-layer model with fp8=True: 8 fp8 forward and 8 fp8 bwd-data GEMMs
    (every encoder Linear's input needs a gradient: the embeddings train), the LayerNorm hand-over taken
    by ffn1 of each layer and by layer 2's qkv, finite loss and gradients; the gradients against the
    fp8=False model on the same weights, batch and dropout step at the bounds of
    test_fp8_wide_resnet_tracks_bf16 (cosine > 0.9, norm ratio in (0.8, 1.25))."""
    from parameter_server_distributed_amd.ops import conv as conv_ops

    s8 = _build(name, gpu, True)
    sb = _build(name, gpu, False)
    sb.model.load_state_dict(s8.model.state_dict())
    batch = s8.make_batch(BATCH, gpu)
    lins = [(i, n, getattr(layer, n)) for i, layer in enumerate(s8.model.layers) for n in ("qkv", "proj", "ffn1", "ffn2")]
    took0 = {(i, n): m.psd_mx_handovers for i, n, m in lins}
    before = dict(conv_ops.FP8_CALLS)
    loss8, g8 = _grads(s8, batch)
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 8
    assert conv_ops.FP8_CALLS["lin_dgrad"] - before["lin_dgrad"] == 8
    took = {k: m.psd_mx_handovers - took0[k] for (i, n, m), k in zip(lins, took0)}
    assert took == {(i, n): int(n == "ffn1" or (n == "qkv" and i == 1)) for i, n, _ in lins}, took
    assert all(m._psd_q8_pending is None and not m._psd_gelu_hands and not m._psd_pending_dx for _, _, m in lins)
    lossb, gb = _grads(sb, batch)
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 8  # the bf16 model launches none
    assert math.isfinite(loss8) and all(bool(torch.isfinite(g).all()) for g in g8.values())
    dot = sum(float((g8[n] * gb[n]).sum()) for n in gb)
    n8 = sum(float(g.pow(2).sum()) for g in g8.values()) ** 0.5
    nb = sum(float(g.pow(2).sum()) for g in gb.values()) ** 0.5
    print(f"{name} fp8 vs bf16 first-step gradient: cosine {dot / (n8 * nb):.4f}, norm ratio {n8 / nb:.4f}, "
          f"loss {loss8:.4f} vs {lossb:.4f}")
    assert dot / (n8 * nb) > 0.9, dot / (n8 * nb)
    assert 0.8 < n8 / nb < 1.25, n8 / nb


@pytest.mark.gpu
def test_fp8_bert_padded_rows_do_not_reach_valid_rows(gpu):
    """MX blocks run along K inside one row, so GEMM rows stay independent: a NaN planted in a padded
    row of the input embeddings changes no valid row of the encoder output."""
    spec = _build("bert_base", gpu, True)
    m = spec.model.eval()
    lens = torch.tensor([32, 20, 9, 1], device=gpu, dtype=torch.int32)
    valid = torch.arange(SEQ, device=gpu)[None, :] < lens[:, None]
    x = torch.randn(BATCH, SEQ, SIZES["hidden"], device=gpu).to(torch.bfloat16)
    bad = x.clone()
    bad[~valid] = float("nan")
    outs = []
    with torch.no_grad():
        for t in (x, bad):
            for layer in m.layers:
                t = layer(t, lens)
            outs.append(t)
    assert bool(torch.isfinite(outs[0][valid]).all())
    assert torch.equal(outs[0][valid], outs[1][valid])


@pytest.mark.gpu
@pytest.mark.parametrize("plane", ["collective", "async"])
def test_fp8_bert_reads_the_published_mx_weights(gpu, plane):
    """World-1 PS with pull_dtype="fp8": every fp8 Linear forward reads the MX copy the data plane
    published (8 per step), the published weights and the loss stay finite."""
    from parameter_server_distributed_amd.ops import conv as conv_ops
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.async_ps import AsyncPS
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

    spec = _build("bert_base", gpu, True)
    x, y = spec.make_batch(BATCH, gpu)
    cfg = OptimConfig("adam", lr=1e-4)
    if plane == "async":
        ps = AsyncPS(spec.model, cfg, staleness=0, bucket_mb=8, device=gpu, pull_dtype="fp8")
    else:
        ps = CollectivePS(spec.model, cfg, staleness=0, bucket_mb=8, device=gpu, pull_dtype="fp8")
    try:
        assert ps.pull_mx
        losses = []
        for _ in range(3):
            before = dict(conv_ops.FP8_CALLS)
            ps.begin_step()
            loss = spec.loss(spec.model(x), y)
            loss.backward()
            ps.finish_step()
            losses.append(float(loss.detach().float()))
            assert conv_ops.FP8_CALLS["ps_weights"] - before["ps_weights"] == 8
            assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 8
        if plane == "async":
            ps.drain()
            ps.begin_step()
        torch.cuda.synchronize()
        assert all(math.isfinite(v) for v in losses), losses
        for m in spec.model.modules():
            if getattr(m, "fp8", None) == "mx":
                q, s = m._psd_w8(m.weight)
                assert bool(torch.isfinite(q.float()).all()) and bool(torch.isfinite(m.weight.float()).all())
    finally:
        if plane == "async":
            ps.close()


@pytest.mark.gpu
def test_trainer_captures_the_fp8_gpt_step(gpu, monkeypatch):
    """The fp8 path reads nothing from the device on the host: the Trainer captures the step, and the
    captured run's losses are finite, fall (what test_trainer_captures_a_gpt_step_at_seq_256 asks of the
    bf16 model) and follow an eager run of the same steps (same kernels, same counter-based dropout
    masks: 2 % covers the bf16 loss rounding, 2^-8, through five optimizer steps)."""
    from parameter_server_distributed_amd.ops import conv as conv_ops
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")  # same GEMM kernels in both runs
    runs = {}
    for graph in (False, True):
        spec = _build("gpt_small", gpu, True, min_seq_len=8)
        batch = spec.make_batch(BATCH, gpu)
        ps = CollectivePS(spec.model, OptimConfig("adamw", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
        tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=graph, graph_warmup=2)
        before = conv_ops.FP8_CALLS["lin_fwd"]
        runs[graph] = [tr.step().float().item() for _ in range(5)]
        torch.cuda.synchronize()
        assert conv_ops.FP8_CALLS["lin_fwd"] > before
        if graph:
            assert tr.graphs and tr.graph_error is None, tr.graph_error
    losses = runs[True]
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    for a, b in zip(runs[False], losses):
        assert abs(a - b) <= 0.02 * abs(a), runs


@pytest.mark.gpu
def test_fp8_tiny_bert_100_step_convergence(gpu):
    """100 AdamW steps of a tiny BERT (hidden 256: the torch LayerNorm fallback and the stand-alone
    quantise passes) on a fixed synthetic batch set, MX fp8 Linears vs bf16 from the same init and batch
    order: both fit the set (last-10 mean loss < 0.5x the first-5 mean) and the fp8 mean loss over the run
    is within 10 % of the bf16 run's (the form of test_fp8_wide_resnet_300_step_convergence)."""
    from parameter_server_distributed_amd.ops import conv as conv_ops

    curves = {}
    before = dict(conv_ops.FP8_CALLS)
    for fp8 in (False, True):
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
        curves[fp8] = [float(v) for v in torch.stack(L).cpu()]
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 100 * 8
    assert conv_ops.FP8_CALLS["lin_dgrad"] - before["lin_dgrad"] == 100 * 8
    avg = lambda L, a, b: sum(L[a:b]) / (b - a)  # noqa: E731
    lb, l8 = curves[False], curves[True]
    print(f"bf16: first-5 {avg(lb, 0, 5):.4f} mean {avg(lb, 0, 100):.4f} last-10 {avg(lb, 90, 100):.4f}; "
          f"fp8: first-5 {avg(l8, 0, 5):.4f} mean {avg(l8, 0, 100):.4f} last-10 {avg(l8, 90, 100):.4f}")
    for L in (lb, l8):
        assert all(math.isfinite(v) for v in L)
        assert avg(L, 90, 100) < 0.5 * avg(L, 0, 5), (avg(L, 0, 5), avg(L, 90, 100))
    assert abs(avg(l8, 0, 100) - avg(lb, 0, 100)) <= 0.10 * avg(lb, 0, 100)
