"""What the ResNet convolutions and BNs hand each other through module attributes: the records, the
one "is this record for exactly this tensor" test, and the small idioms every backward repeated.

A producer leaves a record on the consumer's module (``_psd_*`` attributes, wired by name in
models/resnet.py); the consumer takes it once (``take``) and uses it only if it was made for exactly
the tensor it was given. The records are NamedTuples: they index and unpack as the tuples they replace.

Identity modes (``same(a, b, strides)``). Equal memory can carry different strides where a dimension
has size 1, so the two modes differ and each site keeps the one it always had:
  data_ptr + shape + stride   conv._take_q8, conv._take_dq8 (Q8Pending), conv._bn_bwd_fusion (BnFwd, read
                              only), bn._stats_args (StatsPending)
  data_ptr + shape            _Conv1x1Fn.backward (FoldPending; a mismatch raises) and the BwdPre reads of
                              bn._FusedBNFn / bn._BNAddBNReluFn / tail._TailFn / tail._DualTailFn backward
  bn._fold_target compares the (data_ptr, shape) pair stored in ``_psd_fold_out`` (no tensor is kept).
"""
from __future__ import annotations

from typing import Any, NamedTuple

import torch

from ..utils.config import feature as _feat


class BnFwd(NamedTuple):
    """``bn._psd_fwd``: a ReLU BN's forward, for the consumer convolution's bwd-data epilogue. ``x`` None:
    the BN input was never stored; ``mbits``: a residual BN's ReLU bit-mask; ``xd`` / ``mean_d``: the
    downsample BN's input and mean of a dual tail."""
    y: Any
    x: Any
    mean: Any
    ss: Any
    mbits: Any
    xd: Any = None
    mean_d: Any = None


class BwdPre(NamedTuple):
    """``bn._psd_bwd_pre``: the masked gradient a conv bwd-data epilogue wrote, with the BN's backward
    partials (``part_d``: the downsample BN's, convn mode 3)."""
    g: Any
    part: Any
    rows: int
    part_d: Any = None


class FoldPending(NamedTuple):
    """``conv._psd_fold_pending``: what replaces the BN input gradient (dy = A g + B y + C) in the
    convolution's backward; ``P``: the fold wgrad products already taken."""
    g: Any
    coef: Any
    y: Any
    P: Any = None


class StatsPending(NamedTuple):
    """``bn._psd_stats_pending``: the statistics partials a convolution epilogue reduced for ``y``."""
    y: Any
    part: Any
    rows: int


class Q8Pending(NamedTuple):
    """``_psd_q8_pending`` / ``_psd_dq8_pending``: the MX fp8 copy ``q`` (+ E8M0 ``scales``) of ``t``."""
    t: Any
    q: Any
    scales: Any


def same(a: torch.Tensor, b: torch.Tensor, strides: bool) -> bool:
    """``a`` is exactly ``b``'s memory and shape (and, with ``strides``, its strides)."""
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and (not strides or a.stride() == b.stride())


def take(mod, attr: str, t: torch.Tensor, strides: bool, mismatch: str | None = None):
    """Consume the record on ``mod.<attr>``: cleared, then returned if it was made for ``t`` (its first
    field, compared by ``same``), else None -- or a RuntimeError(``mismatch``) where one is given."""
    rec = getattr(mod, attr, None) if mod is not None else None
    if rec is None:
        return None
    setattr(mod, attr, None)
    if same(rec[0], t, strides):
        return rec
    if mismatch is not None:
        raise RuntimeError(mismatch)
    return None


class StridedDr:
    """A residual-branch gradient handed to a BN (``_psd_pending_dr``) by a stride-2 1x1 (downsample)
    convolution, kept on its quarter grid: ``t4`` = dY . W of the strided positions, [N, C, H/2, W/2]
    channels_last. The full-size gradient is zero except at even (h, w); the consumer convolution's
    bwd-data epilogue adds it there (kernels/convn.hip bwd mode 5) and only other consumers build the
    full tensor (``full``)."""

    def __init__(self, t4: torch.Tensor, H: int, W: int):
        self.t4, self.H, self.W = t4, H, W

    def full(self) -> torch.Tensor:
        n, c = self.t4.shape[:2]
        out = torch.zeros(n, self.H, self.W, c, device=self.t4.device, dtype=self.t4.dtype).permute(0, 3, 1, 2)
        out[:, :, ::2, ::2] = self.t4
        return out


def take_dr(t):
    """A pending residual gradient as a full-size tensor (StridedDr materialised)."""
    return t.full() if isinstance(t, StridedDr) else t


def pop_dr(mod):
    """The newest gradient queued on ``mod._psd_pending_dr`` as a full-size tensor, or None."""
    pend = getattr(mod, "_psd_pending_dr", None)
    return take_dr(pend.pop()) if pend else None


def route_res_grad(resid_to, g):
    """A residual-branch gradient: queued on the BN that produced the residual (None returned), or
    returned for autograd."""
    if resid_to is None:
        return g
    resid_to._psd_pending_dr.append(g)
    return None


def sinks(mod):
    """(dgamma_out, dbeta_out): the PS data plane's gradient views of a BN's weight and bias."""
    sink = getattr(mod, "_psd_grad_sink", None)
    return (sink(mod.weight), sink(mod.bias)) if sink is not None else (None, None)


def bn_momentum(mod) -> float:
    return mod.momentum if mod.momentum is not None else 0.1


def fold_v() -> int:
    """convw variant of the fold / Gram launches: 1 = the two-stage ring at two workgroups per CU."""
    return 1 if _feat("convw_fold2") else 0


def dual_from_fold(pre: BwdPre, w3, a2, wd, xin, x, gamma3, mean3, invstd3, r, gamma_d, mean_d, invstd_d,
                   sinks3, sinks_d):
    """Both BNs of a downsample tail from the fold products. The consumer's bwd-data epilogue reduced
    (sum g, -mean3 sum g) for the masked gradient ``pre.g``; sum g y3 = sum_i W3 (g^T a2) and
    sum g yd = sum_i Wd (g^T x_in) come from the two fold wgrads taken here (handed on as ``Ps``, not
    retaken), and the downsample BN's sums derive from bn3's sum g (same g). ``x`` / ``r``: the BN inputs
    where they were stored, else g. Returns (Ps, dg3, db3, dgd, dbd, coef, coef_d)."""
    from .. import native

    C = native()
    g, part, rows = pre.g, pre.part, pre.rows
    if part.shape[0] <= rows:
        raise RuntimeError("psd dual tail: the partials buffer has no row for sum g y")
    Ps = []
    for wt, inp in ((w3, a2), (wd, xin)):
        P = torch.empty(C.convw_fold_rows(wt.shape[0], wt.shape[1]), inp.shape[1], device=g.device,
                        dtype=torch.float32)
        if not C.convw_(g, inp, P, 1, 1, 1, 0, variant=fold_v(), fold=True):
            raise RuntimeError("psd dual tail: convw_ declined the fold wgrad")
        Ps.append(P)
    part_d = torch.empty(2, part.shape[-1], device=part.device, dtype=torch.float32)
    C.bnfold_rowdot(Ps[0], w3, part[rows])
    C.bnfold_rowdot(Ps[1], wd, part_d)
    _, _, dg3, db3, dgd, dbd, coef, coef_d = C.bn_bwd_dual_pre(
        g, x, gamma3, mean3, invstd3, part, part_d, rows + 1, r, gamma_d, mean_d, invstd_d, *sinks3, *sinks_d,
        fold=True, fold_d=True, derive_d=True)
    return Ps, dg3, db3, dgd, dbd, coef, coef_d
