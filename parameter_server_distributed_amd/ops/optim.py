"""Fused parameter-server optimizer (gfx950 kernel ``csrc/kernels/optim.hip``).

One kernel pass per flat shard does: sum of K gradient sources (K = 1 after an RCCL
reduce-scatter, K = #pushes for inbox-style shards) -> scale (1/W) -> SGD / momentum / Adam /
AdamW update of the fp32 master -> bf16 working copy for the all-gather.

Reference parity: ``ParameterServerCore::aggregate_gradients`` applies ``p -= g`` with lr fixed at 1
(src/parameter_server.cpp:77-91, "can add learning rate here" at :87). ``OptimConfig(kind="sgd",
lr=1.0)`` reproduces it; the other kinds match ``torch.optim.SGD/Adam/AdamW`` (tested against them).

Layer-wise optimizers (gfx950 kernels ``csrc/kernels/optim_lw.hip``): with a ``LayerTable`` -- the
tensor boundaries of the flat range -- the apply is segmented per tensor. ``lars`` and ``lamb`` scale
each tensor's update by a trust ratio from whole-tensor norms (norm pass, finalize, apply: three
launches), and ``exclude_1d`` keeps weight decay (and the trust ratio) off tensors of ndim <= 1
(BatchNorm / LayerNorm weights, biases) for any kind.

Per-step scalars (lr, grad scale, step count, Adam bias corrections) live in a 32-byte device
struct (``OptimDyn``) so a captured hipGraph replays with the current values.
"""
from __future__ import annotations

import math
from dataclasses import asdict, dataclass

import torch

from .. import native

KINDS = {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 3, "lars": 4, "lamb": 5}
LAYERWISE = ("lars", "lamb")


@dataclass
class OptimConfig:
    kind: str = "momentum"
    lr: float = 0.1
    momentum: float = 0.9
    dampening: float = 0.0
    nesterov: bool = False
    weight_decay: float = 0.0
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    maximize: bool = False
    trust_coef: float = 0.001  # LARS eta (lamb ignores it)
    # tensors of ndim <= 1 take no weight decay and no trust ratio; None: True for lars / lamb, else False
    exclude_1d: bool | None = None
    # global-norm gradient clipping, per push (async plane): each worker's gradient is scaled by
    # min(1, clip_norm / (||g||_2 + 1e-6)) before the round is averaged; 0: off
    clip_norm: float = 0.0

    def __post_init__(self):
        if self.kind not in KINDS:
            raise ValueError(f"unknown optimizer kind {self.kind!r}; expected one of {sorted(KINDS)}")
        if self.kind == "momentum" and self.momentum == 0.0:
            self.kind = "sgd"
        if self.exclude_1d is None:
            self.exclude_1d = self.kind in LAYERWISE
        self.exclude_1d = bool(self.exclude_1d)
        self.clip_norm = float(self.clip_norm)
        if not math.isfinite(self.clip_norm) or self.clip_norm < 0.0:
            raise ValueError(f"clip_norm must be finite and >= 0 (0: no clipping), got {self.clip_norm}")

    @property
    def code(self) -> int:
        return KINDS[self.kind]

    @property
    def num_states(self) -> int:
        return {"sgd": 0, "momentum": 1, "adam": 2, "adamw": 2, "lars": 1, "lamb": 2}[self.kind]

    @property
    def needs_layers(self) -> bool:
        """The apply needs the tensor boundaries (a ``LayerTable``)."""
        return self.kind in LAYERWISE or self.exclude_1d

    def to_dict(self):
        return asdict(self)


class OptimDyn:
    """Device-resident per-step scalars: ``[lr, grad_scale, bc1, bc2, step, pad x3]`` (32 B)."""

    def __init__(self, device, lr: float, grad_scale: float = 1.0):
        self.t = torch.zeros(8, dtype=torch.int32, device=device)
        self._f = self.t.view(torch.float32)
        self.set(lr=lr, grad_scale=grad_scale)

    def set(self, lr: float | None = None, grad_scale: float | None = None):
        vals = self.t.detach().cpu()
        fv = vals.view(torch.float32)
        if lr is not None:
            fv[0] = lr
        if grad_scale is not None:
            fv[1] = grad_scale
        self.t.copy_(vals)

    @property
    def step(self) -> int:
        return int(self.t[4].item())

    @property
    def lr(self) -> float:
        return float(self._f[0].item())


class LayerTable:
    """Tensor boundaries of one contiguous flat range, as the segmented kernels read them.

    ``tensors``: ``[(offset, numel, ndim)]`` in buffer order, offsets relative to the range, the first
    at 0 and every one on an ``align``-element boundary (64: the flat layouts of the data planes).
    ``n``: the length of the range. A segment runs from one tensor's start to the next tensor's
    start, so the alignment padding (zero weight, zero gradient) belongs to the tensor in front of
    it and contributes nothing. With ``exclude_1d`` tensors of ndim <= 1 get ``wd_mult`` 0 and
    ``adapt`` 0. Segments are cut into chunks of <= 8192 elements numbered from the segment start.

    Owns every device tensor of the table -- segment starts, per-segment ``wd_mult`` / ``adapt``, the
    chunk table, the per-chunk partials and the per-segment ratio -- allocated once here, so an
    apply allocates nothing and stays legal under stream capture."""

    def __init__(self, tensors, n: int, exclude_1d: bool, device, align: int = 64):
        tensors = [(int(o), int(k), int(d)) for (o, k, d) in tensors]
        if not tensors:
            raise ValueError("LayerTable needs at least one tensor")
        self.tensors = tensors
        self.n = int(n)
        self.exclude_1d = bool(exclude_1d)
        self.device = torch.device(device)
        try:
            self.t = native().lw_table_build([o for o, _, _ in tensors], [k for _, k, _ in tensors],
                                             [d for _, _, d in tensors], self.n, self.exclude_1d, int(align),
                                             str(self.device))
        except RuntimeError as e:  # a bad layout is the caller's value error
            raise ValueError(str(e).split("\n")[0]) from None
        (self.meta, self.seg_start, self.seg_chunk, self.wd_mult, self.adapt, self.chunk_seg, self.chunk_off,
         self.partials, self.ratio) = self.t

    @classmethod
    def for_range(cls, layout, lo: int, hi: int, exclude_1d: bool, device, align: int = 64) -> "LayerTable":
        """The table of ``[lo, hi)`` of a flat buffer from its ``[(offset, numel, ndim)]`` layout
        (absolute offsets); ``lo`` must be a tensor start."""
        inside = [(o - lo, k, d) for (o, k, d) in layout if lo <= o < hi]
        if not inside or inside[0][0] != 0:
            raise ValueError(f"range [{lo}, {hi}) does not start on a tensor start")
        return cls(inside, hi - lo, exclude_1d, device, align)

    @property
    def num_segments(self) -> int:
        return len(self.tensors)


def fused_apply_(cfg: OptimConfig, dyn: OptimDyn, master: torch.Tensor, grads, state1=None, state2=None,
                 shadow=None, advance: bool = True, layers: LayerTable | None = None, grid_cap: int = 0,
                 scales=None, mx_scales=None) -> None:
    """In-place fused update of ``master`` from the sum of ``grads`` (list or tensor). ``layers``:
    the ``LayerTable`` of ``master``'s range -- required for lars / lamb and with ``exclude_1d``,
    rejected otherwise (a table that changes nothing would only hide a configuration mistake).
    ``scales``: one fp32 tensor per gradient source on ``master``'s device (element 0 is used): the
    update then sees ``grad_scale * sum_k scales[k] * grads[k]``, multiplied inside the same kernel
    pass (the per-push clipping coefficients of the async plane). ``None``: the unscaled kernels.
    ``mx_scales``: the gradient sources are MX e4m3 payloads (``float8_e4m3fn`` or uint8, a multiple
    of 32 elements) and ``mx_scales[k]`` holds source k's uint8 E8M0 bytes ``[n / 32]``: the update
    sees the sum of ``q * 2^(byte - 127)``, dequantised inside the same pass (the async plane's fp8
    gradient push). One entry per source, or ``None`` for plain bf16 / fp32 sources."""
    C = native()
    if isinstance(grads, torch.Tensor):
        grads = [grads]
    scales = _check_scales(scales, len(grads))
    mx_scales = _check_scales(mx_scales, len(grads), "mx_scales")
    if cfg.needs_layers and layers is None:
        raise ValueError(f"optimizer {cfg.kind!r} (exclude_1d={cfg.exclude_1d}) needs the tensor boundaries: pass "
                         f"layers=LayerTable(...)")
    if not cfg.needs_layers and layers is not None:
        raise ValueError(f"optimizer {cfg.kind!r} with exclude_1d=False takes no layer table")
    if layers is not None and layers.n != master.numel():
        raise ValueError(f"layer table built for {layers.n} elements, master has {master.numel()}")
    if layers is not None and layers.exclude_1d != cfg.exclude_1d:
        raise ValueError(f"layer table built with exclude_1d={layers.exclude_1d}, config has {cfg.exclude_1d}")
    if advance:
        C.optim_advance_(dyn.t, cfg.beta1, cfg.beta2)
    if layers is None:
        C.fused_apply_(master, list(grads), state1, state2, shadow, dyn.t, cfg.code, cfg.momentum, cfg.dampening,
                       cfg.nesterov, cfg.weight_decay, cfg.beta1, cfg.beta2, cfg.eps, cfg.maximize, grid_cap, scales,
                       mx_scales)
    else:
        C.fused_apply_lw_(master, list(grads), state1, state2, shadow, dyn.t, cfg.code, cfg.momentum, cfg.dampening,
                          cfg.nesterov, cfg.weight_decay, cfg.beta1, cfg.beta2, cfg.eps, cfg.maximize, cfg.trust_coef,
                          layers.t, grid_cap, scales, mx_scales)


def _check_scales(scales, k: int, what: str = "scales") -> list:
    """``[]`` for no scales, else one tensor per source; a partial list is the caller's mistake."""
    if scales is None:
        return []
    scales = list(scales)
    if len(scales) != k or any(s is None for s in scales):
        raise ValueError(f"{what} must hold one tensor for each of the {k} gradient sources (or be None), got "
                         f"{sum(s is not None for s in scales)} of {len(scales)} set")
    return scales


def multi_reduce_(out: torch.Tensor, srcs, scale: float = 1.0, scales=None, mx_scales=None) -> None:
    """``out = scale * sum_k srcs[k]``, or with ``scales`` ``scale * sum_k scales[k] * srcs[k]``;
    with ``mx_scales`` the sources are MX e4m3 payloads and their E8M0 bytes (see ``fused_apply_``)."""
    srcs = list(srcs)
    native().multi_reduce_(out, srcs, scale, _check_scales(scales, len(srcs)),
                           _check_scales(mx_scales, len(srcs), "mx_scales"))


def push_quant_mx_(x: torch.Tensor, q: torch.Tensor, scales: torch.Tensor, blocks_per_seg: int = 0,
                   residual: torch.Tensor | None = None) -> None:
    """The fp8 gradient push's quantiser on one contiguous range: ``x`` (bf16 / fp32, a multiple of
    32 elements) -> ``q`` (``float8_e4m3fn`` or uint8 like ``x``) and ``scales`` (uint8 ``[n / 32]``),
    OCP MX e4m3 with the scale and rounding of ``quantize_mx_ref``. Unlike ``quant_mx_`` a NaN or
    +-inf element becomes the e4m3 NaN byte 0x7F (its block takes the unit scale 127), so a diverged
    gradient reaches the owner as NaN. GPU: the quantising scatter kernel of the async push
    (``csrc/kernels/xfer.hip``) with ``blocks_per_seg`` workgroups (0: the transport's default; the
    bytes do not depend on it). CPU tensors take the host implementation.
    ``residual`` (error feedback; contiguous fp32 ``[n]`` on ``x``'s device, 16-byte aligned on the
    GPU): the quantised value is ``v = fp32(x) + residual`` and ``residual`` becomes
    ``v - dq(q, scales)`` in place, 0 where ``v`` is NaN or +-inf -- ``ops.push_quant_mx_ef_ref``,
    bit for bit; on the GPU inside the same kernel pass."""
    native().push_quant_mx_(x, q, scales, int(blocks_per_seg), residual)


def clip_chunks(n: int) -> int:
    """Elements of the ``partials`` scratch ``grad_clip_coef_`` needs for ``n`` gradient elements."""
    return max(1, (int(n) + 8191) // 8192)


def grad_clip_coef_(flat: torch.Tensor, clip_norm: float, out: torch.Tensor, partials: torch.Tensor,
                    grid_cap: int = 0) -> None:
    """``out[1] = n = ||flat||_2`` and ``out[0] = c = min(1, clip_norm / (n + 1e-6))`` (the formula of
    ``torch.nn.utils.clip_grad_norm_``; a non-finite norm propagates) of a flat bf16 / fp32 gradient
    buffer, on the current stream (gfx950 kernels ``csrc/kernels/clip.hip``: a streaming pass with
    one fp32 partial per 8192 elements, then one workgroup that adds them in fp64). ``out``: fp32,
    at least 2 elements (the async plane passes its 256-byte push-scalar block); ``partials``: fp32
    scratch of ``clip_chunks(n)`` elements. No allocation, no sync; the result's bits do not depend
    on ``grid_cap``."""
    native().grad_clip_coef_(flat, float(clip_norm), out, partials, grid_cap)


def advance_(cfg: OptimConfig, dyn: OptimDyn) -> None:
    native().optim_advance_(dyn.t, cfg.beta1, cfg.beta2)


def apply_no_advance_(cfg: OptimConfig, dyn: OptimDyn, master, grads, state1=None, state2=None, shadow=None):
    fused_apply_(cfg, dyn, master, grads, state1, state2, shadow, advance=False)
