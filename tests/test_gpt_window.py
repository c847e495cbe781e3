"""The decoder LM with a sliding window (``models.build("gpt_small", ..., window=W)``, models/gpt.py): every
block's attention runs the window copies of the streaming kernels, plain and with packed documents. The
comparisons are those of tests/test_gpt_packed.py (kernel path against the SDPA path, within one bf16 ulp
of the largest logit) and tests/test_gpt.py (a trainer step captured in a graph)."""
import math

import pytest
import torch


def _build(gpu, bf16_weights, **kw):
    from parameter_server_distributed_amd import models

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, layers=2, vocab=2048, seq_len=256, window=64, **kw)
    m = spec.model
    if bf16_weights:  # bf16 working weights, as the PS data planes give them (the trainer test has a PS)
        for t in m.parameters():
            t.data = t.data.to(torch.bfloat16)
    for mod in m.modules():  # dropout 0: the two paths draw different masks, and a replay another one
        if isinstance(getattr(mod, "p", None), float):
            mod.p = 0.0
    attn = m.layers[0].attn
    probe = torch.empty(2, 256, 3 * 768, device=gpu, dtype=torch.bfloat16)
    assert attn.causal and attn.window == 64 and attn._long_kernel_ok(probe)
    return spec


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [None, (16, 96)], ids=["plain", "packed"])
def test_windowed_gpt_step_on_the_kernels_matches_the_sdpa_path(gpu, monkeypatch, pack):
    from parameter_server_distributed_amd.ops import attention

    spec = _build(gpu, True, **({} if pack is None else {"pack_docs": pack}))
    m = spec.model
    x, y = spec.make_batch(4, gpu, seed=1)
    assert len(x) == (1 if pack is None else 3)

    def run():
        calls = []
        orig = attention._AttnFn.apply
        attention._AttnFn.apply = lambda *a: calls.append(a) or orig(*a)
        try:
            m.zero_grad(set_to_none=True)
            logits = m(x)
            loss = spec.loss(logits, y)
            loss.backward()
        finally:
            attention._AttnFn.apply = orig
        return loss.float().item(), logits.detach().float(), calls

    la, logits, calls = run()
    assert len(calls) == 2 and all(c[-1] == 64 for c in calls)  # both layers on the window kernels
    if pack is not None:
        assert all(c[-2] is x[2] for c in calls)
    assert math.isfinite(la)
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setenv("PSD_FEATURES", "attn_long=0")
    lb, _, calls = run()
    assert not calls  # SDPA with the boolean mask
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in m.parameters())
    monkeypatch.setenv("PSD_FEATURES", "")
    ulp = 2.0 ** (math.floor(math.log2(logits.abs().max().item())) - 7)  # one bf16 ulp at max|logit| (tests/test_gpt.py)
    print(f"loss kernels {la:.5f}, sdpa {lb:.5f}, ulp {ulp:.5f}")
    assert abs(la - lb) <= ulp, (la, lb, ulp)


@pytest.mark.gpu
@pytest.mark.parametrize("pack", [None, (16, 96)], ids=["plain", "packed"])
def test_trainer_captures_a_windowed_gpt_step(gpu, pack):
    """Learning rate 0 and dropout 0: every step computes the same loss, so the captured step, replayed
    twice, must give the eager step's (within one bf16 ulp of it: the loss is a bf16 value)."""
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    spec = _build(gpu, False, **({} if pack is None else {"pack_docs": pack}))
    batch = spec.make_batch(2, gpu)
    ps = CollectivePS(spec.model, OptimConfig("adamw", lr=0.0, weight_decay=0.0), staleness=0, bucket_mb=8, device=gpu)
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    eager = [tr.step().float().item() for _ in range(2)]  # (two eager steps: the Linear tuner settles in the first)
    torch.cuda.synchronize()
    assert not tr.graphs and math.isfinite(eager[0]) and abs(eager[1] - eager[0]) <= 2.0 ** -7 * abs(eager[0])
    eager = eager[0]
    replays = []
    for _ in range(2):
        replays.append(tr.step().float().item())
        torch.cuda.synchronize()
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    print(f"eager {eager:.6f}, replays {replays}")
    for v in replays:
        assert abs(v - eager) <= 2.0 ** -7 * abs(eager), (eager, replays)
