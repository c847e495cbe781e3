"""The Llama-style block off the GPU: ``GPTForLM(arch="llama")`` on the torch composites (causality, the
loss at initialisation, gradients, no bias inside the blocks or the head, the argument errors), the
composites' gradients against finite differences in fp64, and ``arch="gpt"`` left as it was."""
import math

import pytest
import torch

from test_gpt import TINY, _later_ids_changed


def _tiny_llama(S, **kw):
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    torch.manual_seed(0)
    return GPTForLM(**TINY, max_pos=S, arch="llama", pos="rope", **kw)


def test_tiny_llama_is_causal_on_cpu():
    from parameter_server_distributed_amd.models.gpt import gpt_batch
    from parameter_server_distributed_amd.models.llama_block import LlamaLayer

    B, S, j = 2, 64, 37
    m = _tiny_llama(S).eval()
    assert all(isinstance(layer, LlamaLayer) and layer.attn.causal and layer.rot is not None for layer in m.layers)
    (ids,), _ = gpt_batch(B, S, TINY["vocab"], torch.device("cpu"), seed=3)
    with torch.no_grad():
        a = m((ids,)).view(B, S, -1)
        b = m((_later_ids_changed(ids, j, TINY["vocab"]),)).view(B, S, -1)
    assert a.shape == (B, S, TINY["vocab"])
    torch.testing.assert_close(a[:, :j + 1], b[:, :j + 1], atol=1e-5, rtol=0)
    assert (a[:, j + 1:] - b[:, j + 1:]).abs().max() > 1e-3
    # padded: a shorter length changes nothing before it
    lens = torch.tensor([S, j + 1], dtype=torch.int32)
    with torch.no_grad():
        c = m((ids, lens)).view(B, S, -1)
    torch.testing.assert_close(c[:, :j + 1], a[:, :j + 1], atol=1e-5, rtol=0)


def test_tiny_llama_loss_gradients_and_no_bias():
    from parameter_server_distributed_amd import models

    S = 64
    cpu = torch.device("cpu")
    torch.manual_seed(0)
    spec = models.build("gpt_small", cpu, torch.float32, seq_len=S, arch="llama", pos="rope", **TINY)
    m = spec.model
    assert m.arch == "llama" and m.layers[0].down.in_features == 512  # 8/3 * 128 rounded up to 256s
    x, y = spec.make_batch(2, cpu)
    out = m(x)
    assert out.shape == (2 * S, TINY["vocab"])
    # bump_step pointed every norm site at the model's device step counter and advanced it
    assert all(n.step is m._psd_rng_step for n in (m.norm_f, m.layers[0].norm1, m.layers[1].norm2))
    assert int(m._psd_rng_step) == 1
    loss = spec.loss(out, y)
    loss.backward()
    assert math.isfinite(loss.item()) and abs(loss.item() - math.log(TINY["vocab"])) < 1.0
    missing = [n for n, p in m.named_parameters() if p.grad is None]
    assert not missing, missing
    biased = [n for n, _ in m.named_parameters()
              if n.endswith(".bias") and (n.startswith("layers.") or n.startswith("head.") or n.startswith("norm_f."))]
    assert not biased, biased
    names = {n for n, _ in m.named_parameters()}
    assert {"layers.0.norm1.weight", "layers.1.norm2.weight", "layers.0.gate_up.weight", "norm_f.weight",
            "head.weight"} <= names
    wide = models.build("gpt", cpu, torch.float32, seq_len=S, arch="llama", ffn=256, **TINY).model
    assert wide.layers[0].gate_up.out_features == 512 and wide.layers[0].rot is None


def test_llama_argument_errors():
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    with pytest.raises(ValueError, match="arch"):
        GPTForLM(**TINY, arch="bogus")
    with pytest.raises(ValueError, match="not built"):
        GPTForLM(**TINY, arch="llama", fp8=True)


def test_arch_gpt_is_the_model_built_without_the_argument():
    from parameter_server_distributed_amd.models.gpt import GPTForLM

    torch.manual_seed(0)
    a = GPTForLM(**TINY, max_pos=64)
    torch.manual_seed(0)
    b = GPTForLM(**TINY, max_pos=64, arch="gpt")
    sa, sb = a.state_dict(), b.state_dict()
    assert list(sa.keys()) == list(sb.keys())
    assert all(torch.equal(sa[k], sb[k]) for k in sa)
    assert [n for n, _ in a.named_modules()] == [n for n, _ in b.named_modules()]


@pytest.mark.parametrize("with_h", [True, False])
def test_add_rmsnorm_ref_gradcheck(with_h):
    from parameter_server_distributed_amd.ops.rmsnorm import add_rmsnorm_ref

    g = torch.Generator().manual_seed(1)
    r = torch.randn(3, 16, dtype=torch.float64, generator=g, requires_grad=True)
    h = torch.randn(3, 16, dtype=torch.float64, generator=g, requires_grad=True) if with_h else None
    w = (torch.rand(16, dtype=torch.float64, generator=g) + 0.5).requires_grad_()
    if with_h:
        assert torch.autograd.gradcheck(lambda r, h, w: add_rmsnorm_ref(r, h, w, 1e-6, 0.0, False), (r, h, w))
    else:
        assert torch.autograd.gradcheck(lambda r, w: add_rmsnorm_ref(r, None, w, 1e-6, 0.0, False)[1], (r, w))
        assert add_rmsnorm_ref(r, None, w)[0] is r


def test_add_rmsnorm_ref_formula_and_module():
    from parameter_server_distributed_amd.ops.rmsnorm import FusedAddRMSNorm, add_rmsnorm_ref

    g = torch.Generator().manual_seed(2)
    r, h = torch.randn(5, 16, generator=g), torch.randn(5, 16, generator=g)
    w = torch.rand(16, generator=g) + 0.5
    r_new, y = add_rmsnorm_ref(r, h, w, 1e-6, 0.1, False)
    assert torch.equal(r_new, r + h)
    want = r_new * torch.rsqrt((r_new * r_new).mean(-1, keepdim=True) + 1e-6) * w
    torch.testing.assert_close(y, want, rtol=1e-6, atol=1e-6)
    mod = FusedAddRMSNorm(16, p=0.5).eval()
    assert [n for n, _ in mod.named_parameters()] == ["weight"] and bool((mod.weight == 1).all())
    assert mod.psd_direct_grad_params() == [mod.weight]
    r2, y2 = mod(r, h)  # eval: no dropout
    torch.testing.assert_close(y2, add_rmsnorm_ref(r, h, mod.weight)[1])
    assert mod(r)[0] is r


def test_swiglu_ref_gradcheck():
    from parameter_server_distributed_amd.ops.swiglu import SwiGLU, swiglu_ref

    g = torch.Generator().manual_seed(3)
    gu = torch.randn(3, 16, dtype=torch.float64, generator=g, requires_grad=True)  # F = 8
    assert swiglu_ref(gu).shape == (3, 8)
    assert torch.autograd.gradcheck(swiglu_ref, (gu,))
    x = gu.detach()
    sig = torch.sigmoid(x[:, :8])
    torch.testing.assert_close(swiglu_ref(x), x[:, :8] * sig * x[:, 8:])
    torch.testing.assert_close(SwiGLU()(x.float()), swiglu_ref(x.float()))
    with pytest.raises(ValueError):
        swiglu_ref(torch.zeros(2, 7))


def test_features_default_on():
    from parameter_server_distributed_amd.utils.config import FEATURES, feature

    assert "rmsnorm" in FEATURES and "swiglu" in FEATURES
    assert feature("rmsnorm") and feature("swiglu")
