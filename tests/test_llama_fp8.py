"""The fp8 Llama block (``GPTForLM(arch="llama", fp8="mx")``): the MX operands the fused RMSNorm / SwiGLU kernels
write as side outputs -- bitwise ``quantize_mx_ref`` of the bf16 tensor the same launch stores, every other output
bitwise the plain launch's -- and the block through one step: the hand-overs taken, the feature flag changing no
bit, the gradients against the bf16 block."""
import math

import pytest
import torch

from test_fp8_linear import BATCH, SEQ, SIZES, _bf16_params, _grads
from test_gpt import TINY


def _scaled(gen, rows, cols, gpu):
    """randn with the columns scaled by 2^randint(-4, 5) (the block scales differ along a row), bf16."""
    s = torch.exp2(torch.randint(-4, 5, (1, cols), generator=gen).float())
    return (torch.randn(rows, cols, generator=gen) * s).to(torch.bfloat16).to(gpu)


def _same_as_ref(t, q8, sc8, e5m2):
    """q8 / sc8 are quantize_mx_ref of the bf16 tensor t, and so is the GPU quantize_mx."""
    from parameter_server_distributed_amd.ops import quantize_mx, quantize_mx_ref

    q, s = quantize_mx_ref(t.cpu(), e5m2)
    assert bool(torch.isfinite(t.float()).all()) and 127 in s.tolist() and len(set(s.tolist())) > 1
    for qq, ss in ((q8, sc8), quantize_mx(t, e5m2)):
        assert torch.equal(ss.flatten().cpu(), s)
        assert torch.equal(qq.view(torch.uint8).cpu(), q.view(torch.uint8))


def _mx_out(t, e5m2):
    return (torch.empty(t.shape, device=t.device, dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn),
            torch.empty(t.numel() // 32, device=t.device, dtype=torch.uint8))


def _rms_inputs(rows, H, gpu):
    g = torch.Generator().manual_seed(rows * 7 + H)
    r, h, dy, drn = (_scaled(g, rows, H, gpu) for _ in range(4))
    for t in (r, h, dy, drn):
        t[min(1, rows - 1), 32:64] = 0  # an all-zero block of y and of dh: the unit scale
    gamma = (0.5 + torch.rand(H, generator=g)).to(torch.bfloat16).to(gpu)
    return r, h, dy, drn, gamma


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("rows", [5, 8197])  # a partial workgroup; 5 waves take a second row
@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_forward_writes_the_mx_copy_of_y(gpu, C, H, rows, with_h, p):
    r, h, _, _, gamma = _rms_inputs(rows, H, gpu)
    h = h if with_h else None
    plain = C.rms_fwd(r, h, gamma, 1e-6, p, 11, None)
    q8, sc8 = _mx_out(r, False)
    both = C.rms_fwd(r, h, gamma, 1e-6, p, 11, None, q8, sc8)
    for a, b in zip(plain, both):  # r_new, y, rstd
        assert torch.equal(a, b)
    _same_as_ref(both[1], q8, sc8, False)


@pytest.mark.gpu
@pytest.mark.parametrize("with_drn", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.1])  # dh is dr itself / a tensor of its own
@pytest.mark.parametrize("rows", [5, 70])  # 70: 3 workgroups, a wave visits several rows
@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_backward_writes_the_e5m2_copy_of_dh(gpu, C, H, rows, p, with_drn):
    r, h, dy, drn, gamma = _rms_inputs(rows, H, gpu)
    drn = drn if with_drn else None
    r_new, _, rstd = C.rms_fwd(r, h, gamma, 1e-6, p, 11, None)
    plain = C.rms_bwd(dy, drn, r_new, rstd, gamma, p, 11, None, True, None)
    q8, sc8 = _mx_out(r, True)
    dr, dh, dg = C.rms_bwd(dy, drn, r_new, rstd, gamma, p, 11, None, True, None, q8, sc8)
    assert (dh.data_ptr() == dr.data_ptr()) == (p == 0.0)
    for a, b in zip(plain, (dr, dh, dg)):
        assert torch.equal(a, b)
    _same_as_ref(dh, q8, sc8, True)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [3, 67])
@pytest.mark.parametrize("F", [32, 96])  # one block per row; L = 12: the walk's remainder path
def test_swiglu_writes_the_mx_copies_of_a_and_dgu(gpu, C, F, T):
    g = torch.Generator().manual_seed(F + T)
    gu, da = _scaled(g, T, 2 * F, gpu), _scaled(g, T, F, gpu)
    gu[1, F:F + 32] = 0  # an all-zero block of a,
    da[1, :32] = 0  # and of both halves of dgu
    a, dgu = C.swiglu_fwd(gu, 0), C.swiglu_bwd(da, gu, 0)
    for blocks in (1, 0):  # one workgroup: the loop wraps, the last pass is partial
        q8, sc8 = _mx_out(a, False)
        assert torch.equal(C.swiglu_fwd(gu, blocks, q8, sc8), a)
        _same_as_ref(a, q8, sc8, False)
        q8, sc8 = _mx_out(dgu, True)
        assert torch.equal(C.swiglu_bwd(da, gu, blocks, q8, sc8), dgu)
        _same_as_ref(dgu, q8, sc8, True)  # [T, 2F]: the gate and the up half, blocks inside each
    # F % 32 != 0 with MX outputs: refused before any launch
    gu, da = _scaled(g, T, 2 * 48, gpu), _scaled(g, T, 48, gpu)
    q8 = torch.full((T, 48), 0.5, device=gpu).to(torch.float8_e4m3fn)
    with pytest.raises(RuntimeError, match="q8_out"):
        C.swiglu_fwd(gu, 0, q8, torch.zeros(T * 48 // 32, device=gpu, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="q8_out"):
        C.swiglu_bwd(da, gu, 0, *_mx_out(gu, True))
    assert bool((q8.float() == 0.5).all())


def _llama(gpu, fp8):
    from parameter_server_distributed_amd import models

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, fp8=fp8, arch="llama", pos="rope", seq_len=SEQ, **SIZES)
    _bf16_params(spec.model).train()
    return spec


@pytest.mark.gpu
def test_fp8_llama_step_takes_the_handovers_and_tracks_bf16(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops import conv as conv_ops

    s8, s8off, sb = _llama(gpu, "mx"), _llama(gpu, "mx"), _llama(gpu, False)
    for s in (s8off, sb):
        s.model.load_state_dict(s8.model.state_dict())
    batch = s8.make_batch(BATCH, gpu)

    def lins(spec):
        return {(i, n): getattr(layer, n) for i, layer in enumerate(spec.model.layers)
                for n in ("qkv", "proj", "gate_up", "down")}

    # linear_tune off throughout: the same GEMM kernels in every run (a shape's first call also times the candidates)
    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    before = dict(conv_ops.FP8_CALLS)
    torch.manual_seed(1)  # pos="rope": the embedding block is the composite, whose dropout is torch's
    loss8, g8 = _grads(s8, batch)
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 8
    assert conv_ops.FP8_CALLS["lin_dgrad"] - before["lin_dgrad"] == 8
    assert {k: m.psd_mx_handovers for k, m in lins(s8).items()} == {k: int(k[1] != "proj") for k in lins(s8)}
    assert {k: m.psd_mx_grad_handovers for k, m in lins(s8).items()} == {k: int(k[1] != "qkv") for k in lins(s8)}
    assert all(m._psd_q8_pending is None and m._psd_dq8_pending is None for m in lins(s8).values())
    # feature off: stand-alone quantise passes, the same bits
    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0,fp8_llama_handover=0")
    torch.manual_seed(1)
    loss_off, g_off = _grads(s8off, batch)
    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 16
    assert all(m.psd_mx_handovers == 0 and m.psd_mx_grad_handovers == 0 for m in lins(s8off).values())
    assert loss_off == loss8 and all(torch.equal(g8[n], g_off[n]) for n in g8)
    # against the bf16 block: the bounds of test_fp8_transformer_step_runs_the_fp8_linears_and_tracks_bf16
    torch.manual_seed(1)
    lossb, gb = _grads(sb, batch)
    assert conv_ops.FP8_CALLS["lin_fwd"] - before["lin_fwd"] == 16  # the bf16 model launches none
    assert math.isfinite(loss8) and all(bool(torch.isfinite(g).all()) for g in g8.values())
    dot = sum(float((g8[n] * gb[n]).sum()) for n in gb)
    n8 = sum(float(g.pow(2).sum()) for g in g8.values()) ** 0.5
    nb = sum(float(g.pow(2).sum()) for g in gb.values()) ** 0.5
    print(f"llama fp8 vs bf16 first-step gradient: cosine {dot / (n8 * nb):.4f}, norm ratio {n8 / nb:.4f}, "
          f"loss {loss8:.4f} vs {lossb:.4f}")
    assert dot / (n8 * nb) > 0.9, dot / (n8 * nb)
    assert 0.8 < n8 / nb < 1.25, n8 / nb


def test_fp8_llama_builds_and_runs_on_the_host():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    cpu = torch.device("cpu")
    kw = dict(seq_len=16, arch="llama", pos="rope", **TINY)
    s8 = models.build("gpt_small", cpu, torch.float32, fp8="mx", **kw)
    sb = models.build("gpt_small", cpu, torch.float32, **kw)
    assert list(s8.model.state_dict()) == list(sb.model.state_dict())
    mx = sorted(n for n, m in s8.model.named_modules() if isinstance(m, MfmaLinear) and m.fp8 == "mx")
    assert mx == sorted(f"layers.{i}.{n}" for i in range(TINY["layers"]) for n in ("qkv", "proj", "gate_up", "down"))
    l0, l1 = s8.model.layers[0], s8.model.layers[1]
    assert l0.norm1._psd_mx_to is l0.qkv and l0.act._psd_mxg_to is l0.gate_up and l0.norm2._psd_mxg_to is l0.proj
    assert l1.norm1._psd_mxg_to is l0.down and l0.norm1._psd_mxg_to is None
    # on the host the Linears are F.linear and the norm / activation the composites: the bf16 model's numbers
    sb.model.load_state_dict(s8.model.state_dict())
    batch = s8.make_batch(2, cpu)
    torch.manual_seed(1)  # the composites' dropout is torch's
    l8, g8 = _grads(s8, batch)
    torch.manual_seed(1)
    lb, gb = _grads(sb, batch)
    assert math.isfinite(l8) and l8 == lb and all(torch.equal(g8[n], gb[n]) for n in g8)
    with pytest.raises(ValueError, match="fp8"):
        GPTForLM(**TINY, arch="llama", fp8="bogus")
    assert GPTForLM(**TINY, fp8="mx").layers[0].qkv.fp8 == "mx"  # arch="gpt": what True means
