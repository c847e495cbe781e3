"""The Llama-style block on the kernels (models/llama_block.py, ``GPTForLM(arch="llama")``): a two-layer
stack against the same chain with ``PSD_FEATURES=rmsnorm=0,swiglu=0`` -- the composites, with the same GEMM
and attention kernels -- the whole model's causality and a few optimizer steps, and a captured Trainer step
whose norm-weight gradients arrive through the PS grad sink.

Tolerances are the project's own (tests/test_rope.py): output 2e-2, input and parameter gradients 3e-2,
relative to the tensor's largest entry; causality within one bf16 ulp at max|logit| (tests/test_gpt.py)."""
import math

import pytest
import torch

from test_gpt import _later_ids_changed

pytestmark = pytest.mark.gpu

HIDDEN, HEADS, FFN = 768, 12, 2048


def _stack(gpu, S):
    from parameter_server_distributed_amd.models.llama_block import LlamaLayer

    torch.manual_seed(0)
    layers = torch.nn.ModuleList([LlamaLayer(HIDDEN, HEADS, FFN, 0.0, i, rope=(S, 10000.0)) for i in range(2)])
    for m in layers.modules():
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.normal_(m.weight, std=0.02)
    with torch.no_grad():
        for layer in layers:
            layer.norm1.weight.uniform_(0.5, 1.5)
            layer.norm2.weight.uniform_(0.5, 1.5)
    return layers.to(gpu).to(torch.bfloat16).train()


def _run(layers, x, cr, ch, lens):
    for p in layers.parameters():
        p.grad = None
    leaf = x.clone().requires_grad_(True)
    r, h = leaf, None
    for layer in layers:
        r, h = layer(r, h, lens)
    ((r.float() * cr).sum() + (h.float() * ch).sum()).backward()
    out = {"r": r.detach().float(), "h": h.detach().float(), "dx": leaf.grad.float()}
    out.update({"d" + k: p.grad.float().clone() for k, p in layers.named_parameters()})
    return out


@pytest.mark.parametrize("S", [64, 256])
def test_llama_stack_matches_the_composite_chain(gpu, monkeypatch, S):
    from parameter_server_distributed_amd.ops import rmsnorm, swiglu

    B = 2
    layers = _stack(gpu, S)
    g = torch.Generator(device=gpu).manual_seed(S)
    x = torch.randn(B, S, HIDDEN, device=gpu, generator=g).to(torch.bfloat16)
    cr = torch.randn(B, S, HIDDEN, device=gpu, generator=g)
    ch = torch.randn(B, S, HIDDEN, device=gpu, generator=g)
    lens = torch.tensor([S, S - 23], device=gpu, dtype=torch.int32)
    calls = {"rms": 0, "act": 0}
    orig_r, orig_s = rmsnorm._AddRMSFn.apply, swiglu._SwigluFn.apply
    monkeypatch.setattr(rmsnorm._AddRMSFn, "apply", lambda *a: (calls.__setitem__("rms", calls["rms"] + 1), orig_r(*a))[1])
    monkeypatch.setattr(swiglu._SwigluFn, "apply", lambda *a: (calls.__setitem__("act", calls["act"] + 1), orig_s(*a))[1])
    monkeypatch.setenv("PSD_FEATURES", "")
    got = _run(layers, x, cr, ch, lens)
    assert calls == {"rms": 4, "act": 2}  # every norm site and both activations on the kernels
    monkeypatch.setenv("PSD_FEATURES", "rmsnorm=0,swiglu=0")
    want = _run(layers, x, cr, ch, lens)
    monkeypatch.setenv("PSD_FEATURES", "")
    assert calls == {"rms": 4, "act": 2}  # the composites
    assert got.keys() == want.keys() and len(got) == 3 + 2 * 6
    for k in got:
        assert bool(torch.isfinite(got[k]).all()), k
        top = float(want[k].abs().max())
        err = float((got[k] - want[k]).abs().max())
        tol = 2e-2 if k in ("r", "h") else 3e-2
        print(f"S {S} {k}: max|diff| {err:.4e} of max|ref| {top:.4e} ({err / top:.2e})")
        assert top > 0 and err <= tol * top, (k, err, top)


def _model(gpu, S):
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    torch.manual_seed(0)
    m = GPTForLM(layers=2, vocab=2048, max_pos=S, arch="llama", pos="rope").to(gpu).to(torch.bfloat16)
    probe = torch.empty(2, S, 3 * HIDDEN, device=gpu, dtype=torch.bfloat16)
    attn = m.layers[0].attn
    assert attn.causal and (attn._kernel_ok(probe) if S <= 128 else attn._long_kernel_ok(probe))
    r = torch.empty(2, S, HIDDEN, device=gpu, dtype=torch.bfloat16)
    assert m.norm_f._kernel_ok(r, r) and m.layers[0].norm1._kernel_ok(r, None)
    return m


@pytest.mark.parametrize("S,j", [(64, 37), (256, 150)])
def test_llama_model_is_causal_on_the_kernels(gpu, S, j):
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    B = 2
    m = _model(gpu, S).eval()
    (ids,), _ = gpt_batch(B, S, m.vocab, gpu, seed=3)
    with torch.no_grad():
        a = m((ids,)).float().view(B, S, -1)
        b = m((_later_ids_changed(ids, j, m.vocab),)).float().view(B, S, -1)
    ulp = 2.0 ** (math.floor(math.log2(a.abs().max().item())) - 7)  # one bf16 ulp at max|logit|
    assert (a[:, :j + 1] - b[:, :j + 1]).abs().max().item() <= ulp
    assert (a[:, j + 1:] - b[:, j + 1:]).abs().max().item() > ulp


@pytest.mark.parametrize("S", [64, 256])
def test_llama_model_trains(gpu, S):
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    m = _model(gpu, S).train()
    x, y = gpt_batch(4, S, m.vocab, gpu, seed=4, min_len=S // 2)
    opt = torch.optim.AdamW(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(5):
        opt.zero_grad(set_to_none=True)
        loss = m.loss(m(x), y)
        loss.backward()
        opt.step()
        losses.append(loss.float().item())
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses


def test_trainer_captures_a_llama_step_at_seq_256(gpu):
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.ops.rmsnorm import FusedAddRMSNorm
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, arch="llama", pos="rope", layers=1, vocab=2048, seq_len=256,
                        min_seq_len=8)
    batch = spec.make_batch(2, gpu)
    assert len(batch[0]) == 2
    norms = [m for m in spec.model.modules() if isinstance(m, FusedAddRMSNorm)]
    assert len(norms) == 3
    ps = CollectivePS(spec.model, OptimConfig("adamw", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
    # the norm weights are sink parameters of the flat binding: their gradient is written by rms_bwd's finalize
    assert all(id(n.weight) in ps.flat.direct and n._psd_grad_sink == ps.flat.sink for n in norms)
    r = torch.empty(2, 256, HIDDEN, device=gpu, dtype=torch.bfloat16)
    assert all(n._kernel_ok(r, r) for n in norms)  # bf16 working weights: the kernels take every site
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    losses = [tr.step().float().item() for _ in range(5)]
    torch.cuda.synchronize()
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
    flat = ps.grads_flat
    lo, hi = flat.data_ptr(), flat.data_ptr() + flat.numel() * flat.element_size()
    for n in norms:
        gview = n.weight.grad
        assert gview is not None and lo <= gview.data_ptr() < hi  # the view of the flat buffer the kernel wrote
        assert gview.data_ptr() == ps.flat.grad_views[id(n.weight)].data_ptr()
        # (5 steps at lr 1e-4 stay below half a bf16 ulp of the working weight 1.0: the gradient is what shows)
        assert bool(torch.isfinite(gview.float()).all()) and bool((gview != 0).any())
