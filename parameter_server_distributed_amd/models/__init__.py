"""Model zoo for the BASELINE.json configs (random init, synthetic data of the real shapes).

``build(name, ...)`` returns a ``ModelSpec`` with the module, a synthetic-batch factory, the loss and
the sample unit used for throughput (images or sequences).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable

import torch
import torch.nn as nn
import torch.nn.functional as F

from .mlp import MLP, synthetic_mnist
from .resnet import ResNet, resnet50, resnet101, wide_resnet101_2

__all__ = ["MLP", "ResNet", "resnet50", "resnet101", "wide_resnet101_2", "build", "ModelSpec", "MODELS"]


@dataclass
class ModelSpec:
    name: str
    model: nn.Module
    make_batch: Callable[[int, torch.device], tuple]
    loss: Callable
    sample_desc: str
    channels_last: bool = False
    tied_weights: bool = False


def _ce(out, y):
    from ..ops.loss import cross_entropy  # fused bf16 kernels on the GPU, fp32 F.cross_entropy elsewhere

    return cross_entropy(out, y)


def _image_batch(size: int, classes: int, dtype, channels_last: bool):
    def make(batch: int, device, seed: int = 0):
        g = torch.Generator(device="cpu").manual_seed(seed)
        x = torch.randn(batch, 3, size, size, generator=g).to(device=device, dtype=dtype)
        if channels_last:
            x = x.contiguous(memory_format=torch.channels_last)
        y = torch.randint(0, classes, (batch,), generator=g).to(device)
        return x, y

    return make


def prepare(model: nn.Module, device, dtype=torch.bfloat16, channels_last: bool = False) -> nn.Module:
    """Move to device, cast *buffers* (BN running stats) to the compute dtype, NHWC weights.

    Parameters stay fp32 here: the PS data plane takes the fp32 values as the master copy and
    re-points ``.data`` at its flat bf16 working buffer.
    """
    model = model.to(device)
    if channels_last:
        model = model.to(memory_format=torch.channels_last)
    for m in model.modules():
        if getattr(m, "_psd_fp32_buffers", False):
            continue
        for k, b in list(m._buffers.items()):
            if b is not None and b.is_floating_point():
                m._buffers[k] = b.to(dtype)
    return model


def build(name: str, device, dtype=torch.bfloat16, num_classes: int | None = None, **kw) -> ModelSpec:
    name = name.lower().replace("-", "_")
    if name in ("resnet50", "resnet101", "wide_resnet101_2", "wrn101"):
        ctor = {"resnet50": resnet50, "resnet101": resnet101, "wide_resnet101_2": wide_resnet101_2,
                "wrn101": wide_resnet101_2}[name]
        cls = num_classes or 1000
        size = kw.get("image_size", 224)
        cl = device.type == "cuda" if isinstance(device, torch.device) else str(device).startswith("cuda")
        m = prepare(ctor(cls, fp8=bool(kw.get("fp8", False))), device, dtype, channels_last=cl)
        return ModelSpec(name, m, _image_batch(size, cls, dtype, cl), _ce, "images", channels_last=cl)
    if name == "mlp":
        m = prepare(MLP(hidden=kw.get("hidden", 512)), device, dtype)

        def make(batch, device, seed=0):
            return synthetic_mnist(batch, device, dtype, seed)

        return ModelSpec(name, m, make, _ce, "images")
    if name in ("bert_base", "bert"):
        from .bert import BertForMLM, bert_batch

        m = prepare(BertForMLM(**{k: v for k, v in kw.items() if k in ("layers", "hidden", "heads", "vocab")},
                               fp8=bool(kw.get("fp8", False))), device, dtype)
        seq = kw.get("seq_len", 128)
        min_len = kw.get("min_seq_len")  # padded batches with lengths in [min_seq_len, seq_len]

        def make(batch, device, seed=0):
            return bert_batch(batch, seq, m.vocab, device, seed, min_len=min_len)

        return ModelSpec(name, m, make, m.loss, "sequences")
    if name in ("gpt_small", "gpt"):
        from .gpt import GPTForLM, gpt_batch

        seq = kw.get("seq_len", 512)
        m = prepare(GPTForLM(**{k: v for k, v in kw.items() if k in ("layers", "hidden", "heads", "vocab")},
                             max_pos=max(512, seq), fp8=bool(kw.get("fp8", False)), window=kw.get("window"),
                             pos=kw.get("pos", "learned"), rope_base=kw.get("rope_base", 10000.0),
                             arch=kw.get("arch", "gpt"), ffn=kw.get("ffn")),
                    device, dtype)
        min_len = kw.get("min_seq_len")  # padded batches with lengths in [min_seq_len, seq_len]
        pack = kw.get("pack_docs")  # (lo, hi): rows packed with documents of lengths in [lo, hi]

        def make(batch, device, seed=0):
            return gpt_batch(batch, seq, m.vocab, device, seed, min_len=min_len, docs=pack)

        return ModelSpec("gpt_small", m, make, m.loss, "sequences")
    raise KeyError(f"unknown model {name!r}; available: {MODELS}")


MODELS = ["mlp", "resnet50", "resnet101", "wide_resnet101_2", "bert_base", "gpt_small"]
