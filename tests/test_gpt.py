"""The GPT-1-shaped decoder (models/gpt.py): the synthetic batch, causality of the whole model (a
token cannot see a later one) on the CPU composite path and on the fused causal attention kernels, a few
optimizer steps and a captured Trainer step."""
import math

import pytest
import torch

TINY = dict(layers=2, hidden=128, heads=2, vocab=512)


def test_gpt_batch_shifts_the_labels_and_pads():
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    cpu = torch.device("cpu")
    (ids,), labels = gpt_batch(3, 16, 100, cpu, seed=1)
    assert ids.shape == (3, 16) and ids.dtype == torch.long and labels.shape == (48,)
    lab = labels.view(3, 16)
    assert torch.equal(lab[:, :-1], ids[:, 1:])
    assert (lab[:, -1] == -100).all()
    assert int(ids.min()) >= 0 and int(ids.max()) < 100

    (ids, lens), labels = gpt_batch(64, 16, 100, cpu, seed=2, min_len=1)
    assert lens.dtype == torch.int32 and lens.shape == (64,)
    assert int(lens.min()) >= 1 and int(lens.max()) <= 16 and lens.unique().numel() > 4
    lab = labels.view(64, 16)
    pos = torch.arange(16)[None, :]
    L = lens.long()[:, None]
    assert (ids[pos >= L] == 0).all()
    assert (lab[pos >= L - 1] == -100).all()
    keep = pos < L - 1
    assert torch.equal(lab[keep], torch.roll(ids, -1, 1)[keep])
    (ids2, lens2), labels2 = gpt_batch(64, 16, 100, cpu, seed=2, min_len=1)
    assert torch.equal(ids, ids2) and torch.equal(lens, lens2) and torch.equal(labels, labels2)
    with pytest.raises(ValueError):
        gpt_batch(2, 16, 100, cpu, min_len=17)


def _later_ids_changed(ids, j, vocab):
    other = ids.clone()
    other[:, j + 1:] = (ids[:, j + 1:] + 1 + torch.arange(ids.shape[1] - j - 1, device=ids.device)) % vocab
    return other


def test_tiny_gpt_is_causal_on_cpu():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import GPTForLM, gpt_batch

    torch.manual_seed(0)
    B, S, j = 2, 64, 37
    m = GPTForLM(**TINY, max_pos=S).eval()
    assert all(layer.attn.causal for layer in m.layers)
    (ids,), _ = gpt_batch(B, S, TINY["vocab"], torch.device("cpu"), seed=3)
    with torch.no_grad():
        a = m((ids,)).view(B, S, -1)
        b = m((_later_ids_changed(ids, j, TINY["vocab"]),)).view(B, S, -1)
    assert a.shape == (B, S, TINY["vocab"])
    torch.testing.assert_close(a[:, :j + 1], b[:, :j + 1], atol=1e-5, rtol=0)
    assert (a[:, j + 1:] - b[:, j + 1:]).abs().max() > 1e-3
    # padded: the same holds, and a shorter length changes nothing before it
    lens = torch.tensor([S, j + 1], dtype=torch.int32)
    with torch.no_grad():
        c = m((ids, lens)).view(B, S, -1)
    torch.testing.assert_close(c[:, :j + 1], a[:, :j + 1], atol=1e-5, rtol=0)

    spec = models.build("gpt_small", torch.device("cpu"), torch.float32, seq_len=S, **TINY)
    assert spec.name == "gpt_small" and "gpt_small" in models.MODELS and spec.sample_desc == "sequences"
    x, y = spec.make_batch(2, torch.device("cpu"))
    assert len(x) == 1 and x[0].shape == (2, S)
    out = spec.model(x)
    assert out.shape == (2 * S, TINY["vocab"])
    loss = spec.loss(out, y)
    loss.backward()
    assert math.isfinite(loss.item()) and abs(loss.item() - math.log(TINY["vocab"])) < 1.0
    assert all(p.grad is not None for p in spec.model.parameters() if p is not spec.model.emb.tok_type.weight)
    padded = models.build("gpt", torch.device("cpu"), torch.float32, seq_len=S, min_seq_len=5, **TINY)
    x, y = padded.make_batch(4, torch.device("cpu"))
    assert len(x) == 2 and x[1].dtype == torch.int32
    assert math.isfinite(padded.loss(padded.model(x), y).item())


def _tiny_gpu(gpu, S):
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    torch.manual_seed(0)
    m = GPTForLM(**TINY, max_pos=S).to(gpu).to(torch.bfloat16)
    probe = torch.empty(2, S, 3 * TINY["hidden"], device=gpu, dtype=torch.bfloat16)
    attn = m.layers[0].attn
    assert attn.causal and (attn._kernel_ok(probe) if S <= 128 else attn._long_kernel_ok(probe))
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("S,j", [(64, 37), (256, 150)])
def test_tiny_gpt_is_causal_on_the_kernels(gpu, S, j):
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    B = 2
    m = _tiny_gpu(gpu, S).eval()
    (ids,), _ = gpt_batch(B, S, TINY["vocab"], gpu, seed=3)
    with torch.no_grad():
        a = m((ids,)).float().view(B, S, -1)
        b = m((_later_ids_changed(ids, j, TINY["vocab"]),)).float().view(B, S, -1)
    ulp = 2.0 ** (math.floor(math.log2(a.abs().max().item())) - 7)  # one bf16 ulp at max|logit|
    assert (a[:, :j + 1] - b[:, :j + 1]).abs().max().item() <= ulp
    assert (a[:, j + 1:] - b[:, j + 1:]).abs().max().item() > ulp


@pytest.mark.gpu
@pytest.mark.parametrize("S", [64, 256])
def test_tiny_gpt_trains(gpu, S):
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    m = _tiny_gpu(gpu, S).train()
    x, y = gpt_batch(4, S, TINY["vocab"], gpu, seed=4, min_len=S // 2)
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


@pytest.mark.gpu
def test_trainer_captures_a_gpt_step_at_seq_256(gpu):
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.ops.optim import OptimConfig
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    torch.manual_seed(0)
    spec = models.build("gpt_small", gpu, torch.bfloat16, layers=1, vocab=2048, seq_len=256, min_seq_len=8)
    batch = spec.make_batch(2, gpu)
    assert len(batch[0]) == 2
    attn = spec.model.layers[0].attn
    probe = torch.empty(2, 256, 3 * 768, device=gpu, dtype=torch.bfloat16)
    assert attn.causal and attn._long_kernel_ok(probe) and not attn._kernel_ok(probe)
    ps = CollectivePS(spec.model, OptimConfig("adamw", lr=1e-4), staleness=0, bucket_mb=8, device=gpu)
    tr = Trainer(spec.model, spec.loss, ps, batch, use_graph=True, graph_warmup=2)
    losses = [tr.step().float().item() for _ in range(5)]
    torch.cuda.synchronize()
    assert tr.graphs and tr.graph_error is None, tr.graph_error
    assert all(math.isfinite(v) for v in losses), losses
    assert losses[-1] < losses[0], losses
