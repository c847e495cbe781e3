"""Linear layer on the hand-written MFMA GEMM (csrc/kernels/gemm.hip).

forward   y  = act(x W^T + b)     NT GEMM, bias + ReLU/GELU fused in the epilogue (GELU keeps the
                                  pre-activation for backward)
backward  dx = dy' W              NN GEMM (W read N-major through ds_read_b64_tr_b16: no transpose)
          dW = dy'^T x            TN split-K GEMM, reduced straight into the PS flat-gradient
                                  buffer when the data plane installed a grad sink
          db = colsum(dy')        column-sum kernel (also into the sink); for GELU the activation
                                  backward and this column sum are one pass (gelu_bwd_colsum_)

fp8, MX recipe (``MfmaLinear(..., fp8="mx")``; the encoder / decoder Linears of BERT and GPT built with
``fp8=True``): forward y = act(q(x) q(W)^T + b) and bwd-data dx = q_e5m2(dy') q_t(W) on the block-scaled
v_mfma_scale_f32_16x16x128_f8f6f4 (``gemm_fp8_``, 2x the bf16 MFMA rate) with OCP MX operands, one E8M0
scale per 32 K-elements; the weight and bias gradients stay bf16 on the saved bf16 x and dy', through the
routes and grad sinks of the bf16 path -- unless feature ``fp8_wgrad`` (default off) is on and tokens % 128
== 0: then dW = q_t(dy') q_t(x)^T, both operands e4m3 with blocks of 32 along the tokens (K = tokens), on
the split-K form of the same MFMA kernel (``gemm_fp8_splitk_``: fp32 slabs, deterministic reduce), written
where the bf16 route writes (the grad sink's bf16 / fp32 view, else a fresh bf16 tensor). The bias gradient
stays as it is.
  q(x)     the MX e4m3 copy the producing fused LayerNorm wrote (ops/layernorm.py psd_mx_output_to,
           feature ``fp8_ln_handover``) or the Llama block's fused RMSNorm / SwiGLU wrote (ops/rmsnorm.py,
           ops/swiglu.py, feature ``fp8_llama_handover``), else one ``quantize_mx`` pass
  q(W)     the MX e4m3 copy the PS data plane published (``pull_dtype="fp8"``, the ``_psd_w8`` hook of
           parallel/flat.py), else one ``quantize_mx`` pass
  q_t(W)   ``quantize_mx_t``: W^T [in, out] with blocks along ``out`` in one pass over the bf16 W
           (kernels/fp8_t.hip); q_e5m2(dy') the MX e5m2 copy the fused RMSNorm / SwiGLU backward that produced
           dy' wrote (``psd_mx_grad_to``; not with ``fp8_wgrad``), else one ``quantize_mx`` pass (feature
           ``fp8_dgrad``; off: bf16 dgrad)
  q_t(dy') with ``fp8_wgrad``: the transposed e4m3 half of one ``quantize_mx_dual`` pass over dy' whose e5m2
           row half (bitwise ``quantize_mx``'s) feeds bwd-data, else ``quantize_mx_t(dy')``; q_t(x) one
           ``quantize_mx_t`` pass over the saved bf16 x
Applies when in_features % 128 == 0, out_features % 128 == 0 and feature ``fp8_compute`` is on; any other
call of the module runs the bf16 path below. A residual LayerNorm's handed-over gradient is added after
the fp8 bwd-data GEMM (no beta = 1 epilogue), and the GELU-backward epilogue fusion is not taken (the
e5m2-A kernel has no activation epilogue): the producing GELU Linear runs ``gelu_bwd_colsum_``.

fp8, per-tensor stub (``fp8=True``): the forward GEMM alone on OCP e4m3 operands with per-tensor amax
scaling (x and W quantised each step by the amax / quant kernels); the backward GEMMs stay bf16. Needs
in_features % 128 == 0. No model uses it.

Per-shape routing (ops/autotune.py): for bf16 the forward, dgrad and wgrad GEMMs are each timed
once against hipBLASLt (torch.addmm / mm; bias + activation then run as separate passes) and the
faster path is kept. Measured on BERT-base (M = 8192 tokens) hipBLASLt wins most forward / dgrad
shapes, the split-K MFMA wgrad writing straight into the PS gradient buffer stays competitive.
Feature ``linear_tune`` off pins everything to the MFMA kernels.

Hand-overs (ops/handover.py holds the records, the tag on the output and every validity test; its docstring
has the table): the forward takes the MX copy of x its producer left; the backward takes the MX copy of dy,
the bias gradient a consumer LayerNorm / attention summed, a residual LayerNorm's gradient of x and the GELU
hand-over of the consumer Linear (private to this file), then runs four steps -- activation backward, bwd-data,
weight gradient, bias gradient (``_act_backward``, ``_bwd_data``, ``_weight_grad``, ``_bias_grad``).

CPU tensors (and non-bf16 / unaligned shapes) use ``F.linear`` -- the reference the tests compare
against.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..utils.config import feature as _feat
from .. import native
from . import autotune as _at
from .fp8_common import FP8_CALLS, mx_weight
from .handover import grad_out, linear_src, tag_output, take, take_bias, take_dq8, take_dx

ACTS = {None: 0, "none": 0, "relu": 1, "gelu": 2}


def _ok(x: torch.Tensor, w: torch.Tensor) -> bool:
    return (x.is_cuda and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and w.shape[0] % 8 == 0
            and w.shape[1] % 8 == 0)


def _route(key: tuple, mfma, blas, out: torch.Tensor | None = None, extra: dict | None = None):
    """The fastest of the MFMA kernel(s) and hipBLASLt for this GEMM shape (ops/autotune.py); ``out``
    is the buffer every candidate writes (validated against each other on the first call);
    ``extra``: more MFMA candidates by name (e.g. "mfma_ct", the 192 x 256 transposed-store tile)."""
    if not _feat("linear_tune"):
        return mfma
    probe = (lambda: out) if out is not None else None
    cands = {"mfma": mfma, **(extra or {}), "blas": blas}
    return cands[_at.choose(("linear",) + key, cands, "mfma", probe)]


def _ct(A, B, out, bias=None, act=0, aux=None):
    """Y = B A^T (+bias)(act) on the 192 x 256 transposed-store tile (kernels/gemm.hip CT): for 768-wide
    outputs 512 tiles = 2.0 rounds on 256 CUs where the 256 x 256 tile makes 384 = 1.5 rounds."""
    if not native().gemm_ct_(A, B, out, bias, act, aux):
        raise _at.Declined("192x256 transposed-store GEMM: shape outside the kernel's contract")


def _dgrad_route(key: tuple, dy2: torch.Tensor, w: torch.Tensor, dx: torch.Tensor):
    """dX = dY . W on the fastest of: the MFMA GEMM with W read N-major (NN), the MFMA GEMM on a
    transposed copy of W (NT: both operands K-major, the kernel's fastest layout; the copy is
    |W| bytes), or hipBLASLt -- timed and validated once per shape (ops/autotune.py)."""
    C = native()

    def nn_():
        C.gemm_(dy2, w, True, False, dx)

    def nt_():
        C.gemm_(dy2, w.t().contiguous(), True, True, dx)

    def blas():
        torch.mm(dy2, w, out=dx)

    def sk():  # split-K (fp32 slabs + reduce): a long K over few output tiles (the MLM head's dgrad,
        # K = 30,528 against 19 x 3 256-tiles, ran one K-loop per tile on 57 of 256 CUs)
        C.gemm_splitk_(dy2, w, True, False, dx)

    def ct():  # dX = dY W on the 192 x 256 transposed-store tile: A = W^T [in, out], B = dY [tokens, out]
        _ct(w.t().contiguous(), dy2, dx)

    if not _feat("linear_tune"):
        return nn_
    cands = {"mfma": nn_, "mfma_t": nt_, "mfma_ct": ct, "blas": blas}
    if dy2.shape[1] >= 4096 and dy2.shape[1] % 64 == 0:
        cands["mfma_sk"] = sk
    return cands[_at.choose(("linear",) + key, cands, "mfma", lambda: dx)]


def _gelu_dgrad(ctx, dy2, w, pre, M: int, K: int, N: int):
    """Bwd-data GEMM with the producing GELU Linear's backward in its epilogue: g = dY W * gelu'(pre)
    and that Linear's bias gradient (into its grad sink when the data plane installed one), handed
    over with the producer's forward token. Returns g, or None when the kernel declines the shape
    (nothing ran)."""
    C = native()
    src = ctx.gelu_src
    g = torch.empty(M, K, dtype=dy2.dtype, device=dy2.device)
    db = (grad_out(src, src.bias, like=src.bias) if src.bias is not None
          else torch.empty(K, dtype=w.dtype, device=w.device))

    def nn_():
        if not C.gemm_gelu_bwd_(dy2, w, True, False, pre, g, db):
            raise _at.Declined("gelu-bwd GEMM (NN)")

    def nt_():
        if not C.gemm_gelu_bwd_(dy2, w.t().contiguous(), True, True, pre, g, db):
            raise _at.Declined("gelu-bwd GEMM (NT)")

    try:
        fn = {"nn": nn_, "nt": nt_}[_at.choose(("linear", "dgrad_gelu", M, K, N), {"nn": nn_, "nt": nt_}, "nn",
                                              lambda: g)]
        fn()
    except _at.Declined:
        return None
    # keyed by the producer's forward token: its backward must find exactly this hand-over (a
    # fused gradient consumed as an ordinary one would apply GELU' twice)
    src._psd_gelu_hands[ctx.gelu_tok] = (g, db if src.bias is not None else None)
    return g


def _take_gelu(mod, tok: int):
    """Consume ``mod``'s GELU hand-over of the forward token ``tok`` -- (pre-activation gradient, bias gradient)
    from the consumer Linear's bwd-data epilogue (``_gelu_dgrad``) -- or None; older ones, left by a backward that
    never ran, are dropped."""
    hands = mod._psd_gelu_hands
    hand = hands.pop(tok, None)
    for t in [t for t in hands if t < tok]:
        del hands[t]
    return hand


def _act_backward(ctx, dy2, keep, hand):
    """dy' = the gradient before the activation, and the bias gradient where the same pass sums it (else None)."""
    if hand is not None:
        if ctx.act != 2 or hand[0].data_ptr() != dy2.data_ptr():
            raise RuntimeError(
                "psd MfmaLinear: the consumer fused this GELU's backward (psd_gelu_input_from) but the "
                "gradient reaching it is not the handed-over one -- the GELU output has another consumer")
        # the consumer's bwd-data GEMM already applied this GELU's backward and summed the bias
        # gradient (gemm_gelu_bwd_): dy IS the pre-activation gradient
        return dy2, hand[1]
    if ctx.act == 1:
        return dy2 * (keep.view(dy2.shape) > 0), None
    if ctx.act == 2 and ctx.has_bias and ctx.needs_input_grad[2] and dy2.shape[1] % 8 == 0:
        # GELU backward and the bias gradient in one pass over dy / pre (kernels/gemm.hip)
        db = grad_out(ctx.mod, ctx.mod.bias, like=ctx.mod.bias)
        g = torch.empty_like(dy2)
        native().gelu_bwd_colsum_(dy2, keep, g, db, False)
        return g, db
    if ctx.act == 2:
        return torch.ops.aten.gelu_backward(dy2, keep, approximate="tanh"), None
    return dy2, None


def _bwd_data(ctx, dy2, x2, w, pre_src, got, dq8, wgrad8: bool):
    """dx = dy' W, and [q_t(dy') [out, tokens] e4m3, its scales] where the dual quantiser made them for the fp8
    weight gradient (else None). ``got``: x's other gradient (a residual LayerNorm's, ops/layernorm.py); ``dq8``:
    the MX e5m2 copy of dy' its producer left."""
    (M, K), N = x2.shape, w.shape[0]
    dyT8 = None
    if ctx.mx and _feat("fp8_dgrad"):
        from . import quantize_mx, quantize_mx_dual, quantize_mx_t

        # dx = q_e5m2(dy') . q_t(W): A = dy' [M, out] e5m2, B = W^T [in, out] e4m3, MX blocks along out
        if wgrad8:  # one read of dy' for both of its MX copies; the row half is bitwise quantize_mx's
            dyq, sdy, *dyT8 = quantize_mx_dual(dy2, e5m2_row=True, e5m2_t=False)
        elif dq8 is not None:
            dyq, sdy = dq8.q.view(dy2.shape), dq8.scales
            ctx.mod.psd_mx_grad_handovers += 1
        else:
            dyq, sdy = quantize_mx(dy2, e5m2=True)
        wtq, swt = quantize_mx_t(w)
        dx = torch.empty(x2.shape, dtype=dy2.dtype, device=dy2.device)
        native().gemm_fp8_(dyq, wtq, sdy, swt, dx)
        FP8_CALLS["lin_dgrad"] += 1
        if got is not None:  # added after the GEMM (no beta = 1 fp8 epilogue)
            dx = got.view(M, K).add_(dx)
    elif got is not None:  # accumulated by the GEMM
        dx = got.view(M, K)
        dx.addmm_(dy2, w)
    else:
        dx = _gelu_dgrad(ctx, dy2, w, pre_src, M, K, N) if ctx.gelu_src is not None else None
        if dx is None:
            dx = torch.empty(x2.shape, dtype=dy2.dtype, device=dy2.device)
            _dgrad_route(("dgrad", M, K, N), dy2, w, dx)()
    return dx.view(ctx.in_shape), dyT8


def _weight_grad(ctx, dy2, x2, w, wgrad8: bool, dyT8):
    """dW = dy'^T x into the grad sink's view of the weight, else a fresh tensor. ``dyT8``: q_t(dy') and its scales
    from the bwd-data step, where it made them."""
    C = native()
    dw = grad_out(ctx.mod, ctx.mod.weight, like=w)
    if wgrad8:
        from . import quantize_mx_t

        # dW = q_t(dy') . q_t(x)^T: A = dy'^T [out, tokens], B = x^T [in, tokens], both e4m3, K = tokens
        dyT, sdyT = dyT8 or quantize_mx_t(dy2)
        xT, sxT = quantize_mx_t(x2)
        C.gemm_fp8_splitk_(dyT, xT, sdyT, sxT, dw, False, 1.0, 0)
        FP8_CALLS["lin_wgrad"] += 1
    else:
        _route(("wgrad", *x2.shape, w.shape[0]), lambda: C.gemm_splitk_(dy2, x2, False, False, dw, False, 1.0, 0),
               lambda: torch.mm(dy2.t(), x2, out=dw), dw)()
    return dw


def _bias_grad(ctx, dy2, db, hand):
    """db = colsum(dy'): ``db`` where the activation backward summed it, else the consumer's ``hand`` (summed by a
    LayerNorm's or the attention's backward, ops/layernorm.py, ops/attention.py), else the column-sum kernel."""
    if db is None and hand is not None:
        db = hand.db
    if db is None and ctx.has_bias and ctx.needs_input_grad[2]:
        db = grad_out(ctx.mod, ctx.mod.bias, like=ctx.mod.bias)
        native().colsum_(dy2, db, False)
    return db


class _LinearFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, mod):
        C = native()
        shp = x.shape
        x2 = x.reshape(-1, shp[-1]).contiguous()
        M, N = x2.shape[0], weight.shape[0]
        # the returned tensor owns the buffer and the GEMMs write its [M, N] view: autograd forbids a consumer's
        # in-place update (ops/rope.py rotates the QKV output) on a view made inside a Function
        out = torch.empty(*shp[:-1], N, dtype=x.dtype, device=x.device)
        y = out.view(M, N)
        act = ACTS[mod.act]
        aux = torch.empty_like(y) if act == 2 else None
        use_mx = mod.fp8 == "mx" and mod.psd_mx_input_ok(x2.shape[1])
        if use_mx:
            from . import quantize_mx

            # the MX copy of exactly this x from the producing LayerNorm, else quantised here
            rec = take(mod, "_psd_q8_pending", x, strides=True)
            if rec is not None:
                xq, sx = rec.q.view(x2.shape), rec.scales
                mod.psd_mx_handovers += 1
            else:
                xq, sx = quantize_mx(x2)
            wq, sw = mx_weight(mod, weight)
            C.gemm_fp8_(xq, wq, sx, sw, y, bias, act, aux)
            FP8_CALLS["lin_fwd"] += 1
        elif mod.fp8 is True and x2.shape[1] % 128 == 0:
            from . import quantize_fp8

            xq, sx = quantize_fp8(x2)
            wq, sw = quantize_fp8(weight)
            C.gemm_fp8_(xq, wq, sx, sw, y, bias, act, aux)
        else:
            def mfma():
                C.gemm_(x2, weight, True, True, y, bias, act, aux)

            def blas():
                pre = aux if act == 2 else y
                if bias is not None:
                    torch.addmm(bias, x2, weight.t(), out=pre)
                else:
                    torch.mm(x2, weight.t(), out=pre)
                if act == 1:
                    torch.relu_(y)
                elif act == 2:
                    torch.ops.aten.gelu.out(aux, approximate="tanh", out=y)

            _route(("fwd", M, x2.shape[1], N, act, bias is not None), mfma, blas, y,
                   {"mfma_ct": lambda: _ct(weight, x2, y, bias, act, aux)})()
        ctx.act = act
        ctx.mod = mod
        ctx.mx = use_mx
        # per-forward token: a residual LayerNorm that hands this forward's input gradient over
        # records it, and backward only takes a hand-over carrying its own token (a backward that
        # stopped between the two -- an exception, autograd.grad on a partial graph -- can never
        # leave a stale gradient for the next step)
        ctx.tok = mod._psd_tok = getattr(mod, "_psd_tok", 0) + 1
        mod._psd_ran_mx = use_mx  # of this forward: what a producer of dy's MX copy asks (handover.mx_grad_token)
        ctx.has_bias = bias is not None
        ctx.in_shape = shp
        # GELU hand-over (MfmaLinear.psd_gelu_input_from): this Linear's bwd-data GEMM applies the
        # producing GELU Linear's activation backward in its epilogue when x is that Linear's output
        # of the current forward
        src = getattr(mod, "_psd_gelu_from", None)
        # (not on the MX fp8 path: the e5m2-A GEMM has no activation epilogue, so no hand-over is made and
        # the producer runs gelu_bwd_colsum_ itself)
        fuse = (src is not None and not use_mx and _feat("gelu_fuse") and linear_src(x, src) is not None
                and getattr(src, "_psd_gelu_pre", None) is not None)
        ctx.gelu_src = src if fuse else None
        ctx.gelu_tok = src._psd_tok if fuse else None
        pre_src = src._psd_gelu_pre if fuse else None
        # (ReLU keeps the output itself, not its [M, N] view: a saved view made under no_grad cannot be unpacked
        # once an in-place op -- the library route's relu_ -- has touched it)
        ctx.save_for_backward(x2, weight, out if act == 1 else aux, pre_src)
        tag_output(mod, out, ctx.tok)  # for the consumers that hand this Linear's backward something (ops/handover.py)
        if act == 2:
            mod._psd_gelu_pre = aux  # what a fused consumer's backward reads (also saved in this ctx)
        return out

    @staticmethod
    def backward(ctx, dy):
        x2, w, keep, pre_src = ctx.saved_tensors
        mod, tok = ctx.mod, ctx.tok
        dy2 = dy.reshape(-1, w.shape[0]).contiguous()
        # what the consumers of this forward's output left for this backward (ops/handover.py): each is taken --
        # and cleared -- once, and used only for this forward's token and exactly this dy
        dq8 = take_dq8(mod, tok, dy2)
        dy2, db = _act_backward(ctx, dy2, keep, _take_gelu(mod, tok))
        got, bias_hand = take_dx(mod, tok), take_bias(mod, tok, dy2)  # (the bias hand-over is of dy')
        # fp8 weight gradient (feature fp8_wgrad): MX blocks run along the tokens, whole 128-wide K-tiles
        wgrad8 = ctx.mx and ctx.needs_input_grad[1] and x2.shape[0] % 128 == 0 and _feat("fp8_wgrad")
        dx, dyT8 = _bwd_data(ctx, dy2, x2, w, pre_src, got, dq8, wgrad8) if ctx.needs_input_grad[0] else (None, None)
        if ctx.gelu_src is not None and ctx.gelu_src._psd_gelu_pre is pre_src:
            ctx.gelu_src._psd_gelu_pre = None  # not kept alive between steps
        dw = _weight_grad(ctx, dy2, x2, w, wgrad8, dyT8) if ctx.needs_input_grad[1] else None
        return dx, dw, _bias_grad(ctx, dy2, db, bias_hand), None


class MfmaLinear(nn.Linear):
    """``nn.Linear`` (+ fused activation) running on the gfx950 MFMA GEMM for bf16 device tensors."""

    def __init__(self, in_features, out_features, bias=True, act=None, device=None, dtype=None, fp8=False):
        super().__init__(in_features, out_features, bias=bias, device=device, dtype=dtype)
        if not (fp8 is False or fp8 is True or (isinstance(fp8, str) and fp8 == "mx")):
            raise ValueError(f"MfmaLinear: fp8 must be False, True (per-tensor, forward only) or 'mx', got {fp8!r}")
        self.act = act
        self.fp8 = fp8
        self._psd_q8_pending = None  # ops.handover.Q8Pending of the input, left by the producing LayerNorm
        self.psd_mx_handovers = 0  # forwards that took it (tests / logs)
        self._psd_dq8_pending = None  # Q8Pending of dy with this forward's token, from the fused backward that made dy
        self.psd_mx_grad_handovers = 0  # backwards that took it
        self._psd_ran_mx = False  # whether the latest forward ran the MX recipe
        self._psd_pending_dx: list = []  # ops.handover.PendingDx: gradients of the input from a residual LayerNorm
        self._psd_gelu_from = None  # psd_gelu_input_from: the GELU Linear whose output is this one's input
        self._psd_gelu_hands: dict = {}  # forward token -> (pre-activation gradient, bias gradient) from the consumer
        self._psd_gelu_pre = None
        self._psd_bias_hand = None  # ops.handover.BiasHand from a consumer LayerNorm / attention

    def psd_gelu_input_from(self, src: "MfmaLinear") -> None:
        """Declare that this Linear's input is ``src``'s GELU output and nothing else reads it: the
        bwd-data GEMM here then returns d(pre-activation) with the GELU backward and src's bias
        gradient fused in its epilogue (src's backward skips both). Only valid when src's output
        has no other consumer (e.g. BERT's FFN: ffn2(ffn1(x)))."""
        assert src.act == "gelu"
        self._psd_gelu_from = src

    def psd_takes_pending_dx(self, x) -> bool:
        """True when this module's forward on ``x`` ran the autograd Function whose backward folds a
        handed-over input gradient into its bwd-data GEMM."""
        return _ok(x, self.weight) and x.shape[-1] == self.in_features

    def psd_direct_grad_params(self):
        return [p for p in (self.weight, self.bias) if p is not None]

    def psd_mx_input_ok(self, in_features: int) -> bool:
        """True when a bf16 device input of ``in_features`` columns runs the MX fp8 recipe here (else
        the bf16 path): what the forward and the LayerNorm that would hand its MX operand over ask."""
        w = self.weight
        return (self.fp8 == "mx" and w.is_cuda and w.dtype == torch.bfloat16 and in_features == self.in_features
                and self.in_features % 128 == 0 and self.out_features % 128 == 0 and _feat("fp8_compute"))

    def forward(self, x):
        if _ok(x, self.weight):
            return _LinearFn.apply(x, self.weight, self.bias, self)
        y = F.linear(x, self.weight.to(x.dtype), None if self.bias is None else self.bias.to(x.dtype))
        if self.act == "relu":
            y = F.relu(y)
        elif self.act == "gelu":
            y = F.gelu(y, approximate="tanh")
        return y
