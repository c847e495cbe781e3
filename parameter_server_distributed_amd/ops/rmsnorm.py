"""The pre-norm residual step of a Llama-style block, ``r_new = r + dropout(h)``, ``y = RMSNorm(r_new)``,
on the fused gfx950 kernels of ``csrc/kernels/rmsnorm.hip`` (one pass forward, one pass backward + the
tiny fixed-order ``dgamma`` finalize).

``rstd = rsqrt(mean(r_new^2) + eps)`` is taken from the bf16-rounded ``r_new`` -- the value that is stored
and carried on as the residual stream -- and ``y = r_new * rstd * weight``; there is no bias and no mean.
The module returns both: ``r_new`` goes on to the next residual step, ``y`` into the block's branch.

Dropout masks come from LayerNorm's counter-based hash of (per-site seed, device step counter, element)
(``ops/layernorm.py``): regenerated in backward instead of stored, fresh on every replay of a captured
graph. The weight gradient goes straight into the PS flat-gradient buffer when the data plane installed a
grad sink.

CPU tensors, other dtypes or hidden sizes, and feature ``rmsnorm`` off use the composite
``add_rmsnorm_ref`` -- the reference the tests compare against.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import native
from ..utils.config import feature as _feat


def add_rmsnorm_ref(r, h, weight, eps: float = 1e-6, p: float = 0.0, training: bool = False):
    """The torch composite with the semantics of the kernels, on any device and dtype: ``(r_new, y)`` with
    ``r_new = r + dropout(h)`` in ``r``'s dtype (``r`` itself for ``h=None``), the statistics from that
    rounded ``r_new`` in fp32 (fp64 for an fp64 ``r``) and one rounding of ``y``. The dropout is torch's."""
    r_new = r if h is None else r + F.dropout(h, p, training)
    mt = torch.float64 if r.dtype == torch.float64 else torch.float32
    x = r_new.to(mt)
    rstd = torch.rsqrt((x * x).mean(-1, keepdim=True) + eps)
    return r_new, (x * rstd * weight.to(mt)).to(r.dtype)


class _AddRMSFn(torch.autograd.Function):
    """``(r, h) -> (r_new, y)`` with both outputs differentiable, or -- for ``h=None`` -- ``r -> y`` alone:
    ``r`` is then the residual stream itself and its other uses are left to autograd, which costs one
    gradient add in the model's first norm only. Saves ``r_new``, ``rstd`` and ``gamma``, nothing else."""

    @staticmethod
    def forward(ctx, r, h, weight, mod, p):
        shp = r.shape
        r_new, y, rstd = native().rms_fwd(r.contiguous(), None if h is None else h.contiguous(), weight, mod.eps, p,
                                          mod.seed, mod.step)
        ctx.mod, ctx.p, ctx.had_h = mod, p, h is not None
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(r_new, rstd, weight)
        if h is None:
            return y.view(shp)
        return r_new.view(shp), y.view(shp)

    @staticmethod
    def backward(ctx, *grads):
        r_new, rstd, w = ctx.saved_tensors
        mod = ctx.mod
        dr_new, dy = grads if ctx.had_h else (None, grads[0])
        if dy is None:  # y unused: only the residual stream's gradient passes through
            dy = torch.zeros_like(r_new)
        sink = getattr(mod, "_psd_grad_sink", None)
        dgo = sink(mod.weight) if sink is not None else None
        dr, dh, dg = native().rms_bwd(dy.contiguous().view(r_new.shape),
                                      None if dr_new is None else dr_new.contiguous().view(r_new.shape), r_new, rstd,
                                      w, ctx.p, mod.seed, mod.step, ctx.had_h, dgo)
        return dr, dh, dg, None, None


class FusedAddRMSNorm(nn.Module):
    """``forward(r, h=None) -> (r_new, y)``: the residual add (with dropout on the branch ``h``) and the
    RMSNorm of the new residual stream in one fused kernel family on MI355X. The weight, initialised to
    ones, is the only parameter."""

    def __init__(self, hidden: int, eps: float = 1e-6, p: float = 0.1, seed: int = 0):
        super().__init__()
        self.hidden = int(hidden)
        self.eps = float(eps)
        self.p = p
        self.seed = int(seed) & 0x7FFFFFFF
        self.step = None  # device int64 counter, set by the owning model (ops.layernorm.bump_step)
        self.weight = nn.Parameter(torch.ones(self.hidden))

    def extra_repr(self) -> str:
        return f"{self.hidden}, eps={self.eps}, p={self.p}"

    def psd_direct_grad_params(self):
        return [self.weight]

    def _kernel_ok(self, r, h) -> bool:
        return (r.is_cuda and r.dtype == torch.bfloat16 and r.shape[-1] == self.hidden and self.hidden in (768, 1024)
                and self.weight.dtype == torch.bfloat16 and self.weight.device == r.device
                and (h is None or (h.dtype == torch.bfloat16 and h.shape == r.shape and h.device == r.device)))

    def forward(self, r, h=None):
        p = self.p if self.training else 0.0
        if _feat("rmsnorm") and self._kernel_ok(r, h):
            if h is None:
                return r, _AddRMSFn.apply(r, None, self.weight, self, 0.0)
            return _AddRMSFn.apply(r, h, self.weight, self, p)
        return add_rmsnorm_ref(r, h, self.weight, self.eps, p, self.training)
