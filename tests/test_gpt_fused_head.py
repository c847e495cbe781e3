"""``GPTForLM(fused_head=True)``: hidden states out of ``forward``, the loss through ``head_loss`` -- the same
model, state and loss as the default mode (exactly on the host, where both take the composite; within the
kernels' derived bounds on the device)."""
import pytest
import torch

TINY = dict(layers=2, hidden=128, heads=2, vocab=256)


def _pair(**kw):
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    out = []
    for fused in (False, True):
        torch.manual_seed(0)
        out.append(GPTForLM(**TINY, max_pos=64, dropout=0.0, fused_head=fused, **kw))
    return out


def test_fused_head_is_the_same_model_on_the_host():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    m, mf = _pair()
    sd, sdf = m.state_dict(), mf.state_dict()
    assert list(sd) == list(sdf) and all(torch.equal(sd[k], sdf[k]) for k in sd)
    batch, y = gpt_batch(2, 32, TINY["vocab"], "cpu", seed=3, min_len=9)
    h = mf(batch)
    assert h.shape == (64, TINY["hidden"]) and mf.logits(h).shape == (64, TINY["vocab"])
    loss, loss_f = m.loss(m(batch), y), mf.head_loss(h, y)
    assert torch.equal(loss, loss_f)
    loss_f.backward()
    assert all(p.grad is not None for p in mf.parameters())

    cpu = torch.device("cpu")
    spec = models.build("gpt", cpu, torch.float32, seq_len=32, fused_head=True, **TINY)
    x, y = spec.make_batch(2, cpu)
    assert spec.model.fused_head and spec.loss == spec.model.head_loss
    assert torch.isfinite(spec.loss(spec.model(x), y))
    assert not models.build("gpt", cpu, torch.float32, seq_len=32, **TINY).model.fused_head


@pytest.mark.gpu
@pytest.mark.parametrize("arch,min_len", [("gpt", None), ("llama", None), ("gpt", 20)])
def test_fused_head_matches_the_logits_path_on_the_device(gpu, arch, min_len):
    """Both heads against the fp64 loss and head weight gradient of the (shared) bf16 hidden states. The fused
    loss within the kernel's loss_row bound averaged over the rows; the logits path adds the bf16 rounding of
    its stored logits, at most 2^-9 max|z| on the lse and on the label logit of a row each. Weight gradients:
    2^-8 |g_ref| + 2^-8 |dZ_ref|^T |h| (tests/test_lmhead_xent.py)."""
    from parameter_server_distributed_amd.models.gpt import gpt_batch

    m, mf = (t.to(gpu).to(torch.bfloat16) for t in _pair(arch=arch))
    batch, y = gpt_batch(2, 64, TINY["vocab"], gpu, seed=5, min_len=min_len)
    h = mf(batch)
    loss_f, loss = mf.head_loss(h, y), m.loss(m(batch), y)
    assert "LinearXent" in type(loss_f.grad_fn).__name__
    loss_f.backward()
    loss.backward()

    hd, wd = h.detach().double(), mf.head.weight.detach().double()
    bias = mf.head.bias
    assert (bias is None) == (arch == "llama")
    z = hd @ wd.T + (0 if bias is None else bias.detach().double())
    absz = hd.abs() @ wd.abs().T + (0 if bias is None else bias.detach().double().abs())
    ok = y >= 0
    assert 0 < int(ok.sum()) < y.numel()
    lse = torch.logsumexp(z, 1)
    onehot = torch.zeros_like(z)
    onehot[ok, y[ok]] = 1
    ref = ((lse - (z * onehot).sum(1)) * ok).sum() / ok.sum()
    lim = 2 * TINY["hidden"] * 2.0 ** -23 * absz.max() + 2.0 ** -22 * (1 + lse.abs().max())
    assert abs(loss_f.double() - ref) <= lim + 2.0 ** -22 * ref
    assert abs(loss.double() - ref) <= lim + 2.0 ** -22 * ref + 2.0 ** -8 * z.abs().max()
    dz = (torch.softmax(z, 1) - onehot) * ok[:, None] / ok.sum()
    dw, A = dz.T @ hd, dz.abs().T @ hd.abs()
    for mod in (mf, m):
        err = (mod.head.weight.grad.double() - dw).abs()
        assert (err <= 2.0 ** -8 * dw.abs() + 2.0 ** -8 * A).all(), (err - 2.0 ** -8 * A).max()
    assert all(p.grad is not None for p in mf.parameters())
