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

The transformer side (the second section below) hands tensors between the Linear, norm, SwiGLU and attention
Functions in the same way, with one more key: every forward of an ``MfmaLinear`` takes a fresh token
(``_psd_tok``), and a record made for a Linear's backward carries the token of the forward it belongs to, so a
backward that never ran (an exception, ``autograd.grad`` on a partial graph) leaves nothing a later step takes.

  attribute         record          producers               consumer              identity rule            a miss
  out._psd_src      LinearSrc       _LinearFn.forward       layernorm, attention  linear_src: the tag's    no hand-over is made:
  (on the tensor)   (lin, tok)      (tag_output; rope       (bias_src); rmsnorm,  token is the Linear's    the consumer runs its
                                    drops it, drop_tag)     swiglu                latest, + the caller's   own pass
                                                            (mx_grad_token);      predicate
                                                            linear (GELU fusion)
  _psd_q8_pending   Q8Pending       layernorm, rmsnorm,     _LinearFn.forward     data_ptr + shape +       quantize_mx(x)
                    (t, q, scales)  swiglu fwd (leave_q8)   (take)                stride of x
  _psd_dq8_pending  Q8Pending       rmsnorm, swiglu bwd     _LinearFn.backward    tok + data_ptr + shape   quantize_mx(dy', e5m2)
                    with its tok    (mx_grad_gate,          (take_dq8)            of dy
                                    leave_dq8)
  _psd_bias_hand    BiasHand        layernorm, attention    _LinearFn.backward    tok + data_ptr of dy'    colsum_(dy')
                    (tok, ptr, db)  bwd (hand_bias)         (take_bias)
  _psd_pending_dx   [PendingDx]     layernorm bwd           _LinearFn.backward    tok, newest first        dx is the GEMM's alone
                    (tok, g)        (queue_dx)              (take_dx)
  _psd_gelu_hands   {tok: (g, db)}  linear._gelu_dgrad      _LinearFn.backward    tok, then data_ptr of    none: the Linear's own
                    private to      (the consumer Linear's  (linear._take_gelu)   dy (another dy raises)   GELU backward
                    ops/linear.py   bwd-data epilogue)
Every take clears what it read, on a miss as on a hit. A convolution's ``_psd_dq8_pending`` is the same Q8Pending
without a token (ops/conv.py, ops/bn.py: the first section's ``take``).
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
    """``_psd_q8_pending`` / ``_psd_dq8_pending``: the MX fp8 copy ``q`` (+ E8M0 ``scales``) of ``t``; ``tok``: on
    a Linear's ``_psd_dq8_pending``, the token of the forward whose backward it is for."""
    t: Any
    q: Any
    scales: Any
    tok: Any = None


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


def grad_out(mod, param, like=None):
    """Where a backward writes ``param``'s gradient: the view the PS data plane's grad sink on ``mod`` returns for
    it (straight into the flat-gradient buffer), else None -- or, with ``like``, a fresh tensor shaped like it."""
    sink = getattr(mod, "_psd_grad_sink", None)
    out = sink(param) if sink is not None else None
    return torch.empty_like(like) if out is None and like is not None else out


def sinks(mod):
    """(dgamma_out, dbeta_out): the PS data plane's gradient views of a BN's weight and bias."""
    return grad_out(mod, mod.weight), grad_out(mod, mod.bias)


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


# ---------------------------------------------------------------------------------------------
# the transformer side: MfmaLinear <-> LayerNorm / RMSNorm / SwiGLU / attention (the table in the module docstring)


class LinearSrc(NamedTuple):
    """``out._psd_src``: the tag on an ``MfmaLinear``'s output tensor -- the module and that forward's token."""
    lin: Any
    tok: int


class BiasHand(NamedTuple):
    """``lin._psd_bias_hand``: the bias gradient ``db`` a consumer's backward summed over the columns of the
    Linear's output gradient, the tensor it wrote at ``ptr``."""
    tok: int
    ptr: int
    db: Any


class PendingDx(NamedTuple):
    """An entry of ``lin._psd_pending_dx``: the other gradient ``g`` of the Linear's input (a residual LayerNorm's)."""
    tok: Any
    g: Any


def tag_output(lin, out: torch.Tensor, tok: int) -> None:
    """Tag ``out`` as the output of ``lin``'s forward ``tok`` (on the Python tensor object: a view or a copy has none)."""
    out._psd_src = LinearSrc(lin, tok)


def drop_tag(out: torch.Tensor) -> None:
    """``out`` was updated in place (ops/rope.py): it is no longer what the Linear wrote."""
    if hasattr(out, "_psd_src"):
        del out._psd_src


def linear_src(out, lin=None):
    """The LinearSrc tag of ``out`` if the latest forward of the Linear it names -- ``lin``, where one is given --
    produced exactly this tensor, else None."""
    src = getattr(out, "_psd_src", None)
    fresh = src is not None and (lin is None or src.lin is lin) and src.lin._psd_tok == src.tok
    return src if fresh else None


def bias_src(out):
    """``linear_src(out)`` if that Linear has a bias and no activation: its output gradient is then the gradient
    the consumer's backward writes, whose column sums are the bias gradient (``hand_bias``); else None."""
    src = linear_src(out)
    return src if src is not None and src.lin.bias is not None and src.lin.act in (None, "none") else None


def mx_grad_token(lin, out):
    """The forward token of the fp8 Linear ``lin`` if ``out`` is the output of its latest forward and that forward
    ran the MX recipe -- then a fused backward that computes ``out``'s gradient may leave its MX e5m2 copy for
    ``lin`` (``mx_grad_gate``, ``leave_dq8``) -- else None."""
    src = linear_src(out, lin) if lin is not None else None
    return src.tok if src is not None and lin._psd_ran_mx else None


def forward_token(lin):
    """The token of ``lin``'s latest forward (None: it has not run, or there is no ``lin``)."""
    return getattr(lin, "_psd_tok", None)


def mx_pair(shape, device, e5m2: bool = False):
    """The MX side outputs of a launch that stores a bf16 tensor of ``shape``: its fp8 copy (e4m3, or e5m2 for a
    gradient) and one E8M0 scale per 32 elements."""
    q = torch.empty(tuple(shape), dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn, device=device)
    return q, torch.empty(q.numel() // 32, dtype=torch.uint8, device=device)


def leave_q8(cons, t: torch.Tensor, q, scales) -> None:
    """Leave the MX e4m3 copy of ``t`` on the Linear ``cons`` that reads ``t`` next."""
    cons._psd_q8_pending = Q8Pending(t, q, scales)


def mx_grad_gate(tok) -> bool:
    """Whether a fused backward writes the MX e5m2 copy of the gradient it hands a Linear: ``tok`` is that Linear's
    ``mx_grad_token`` and its bwd-data GEMM will read such a copy (with ``fp8_wgrad`` the dual quantiser makes it)."""
    return bool(tok is not None and _feat("fp8_llama_handover") and _feat("fp8_dgrad") and not _feat("fp8_wgrad"))


def leave_dq8(lin, tok, dy: torch.Tensor, q, scales) -> None:
    """Leave the MX e5m2 copy of ``dy``, the gradient of ``lin``'s forward ``tok``, for ``lin``'s backward -- keyed
    by the [tokens, out] view that backward compares."""
    lin._psd_dq8_pending = Q8Pending(dy.view(-1, dy.shape[-1]), q, scales, tok)


def hand_bias(src: LinearSrc, dy: torch.Tensor, db) -> None:
    """Hand ``src.lin`` its bias gradient ``db``, the column sums of its output gradient ``dy``."""
    src.lin._psd_bias_hand = BiasHand(src.tok, dy.data_ptr(), db)


def queue_dx(lin, tok, g: torch.Tensor) -> None:
    """Queue ``g``, the other gradient of the input of ``lin``'s forward ``tok``, for ``lin``'s bwd-data GEMM."""
    lin._psd_pending_dx.append(PendingDx(tok, g))


def take_dq8(mod, tok: int, dy2: torch.Tensor):
    """Consume ``mod._psd_dq8_pending`` (cleared): the Q8Pending if it carries the forward token ``tok`` and was
    made for exactly ``dy2`` (data_ptr and shape), else None."""
    pend = take(mod, "_psd_dq8_pending", dy2, strides=False)
    return pend if pend is not None and pend.tok == tok else None


def take_bias(mod, tok: int, dy2: torch.Tensor):
    """Consume ``mod._psd_bias_hand`` (cleared): the BiasHand if it carries the forward token ``tok`` and was summed
    from exactly ``dy2`` (data_ptr), else None."""
    bh = getattr(mod, "_psd_bias_hand", None)
    mod._psd_bias_hand = None
    return bh if bh is not None and bh[0] == tok and bh[1] == dy2.data_ptr() else None


def take_dx(mod, tok: int):
    """Consume ``mod._psd_pending_dx`` (emptied): the newest gradient queued for the forward token ``tok``, else
    None; entries of other tokens -- left by a backward that never ran -- are dropped."""
    pend = mod._psd_pending_dx
    got = next((g for t, g in reversed(pend) if t == tok), None)
    pend.clear()
    return got
