"""A model bound to flat parameter / gradient buffers: what the two PS data planes share.

Both planes (``collective_ps.CollectivePS``, ``async_ps.AsyncPS``) lay the model's parameters out in
one flat buffer (reverse registration order, 64-element aligned), point ``p.data`` / ``p.grad`` at
views of it, hand grad sinks to the fused modules, launch a bucket once its last gradient has
arrived, and map to and from the canonical layout of the elastic runtime. Each plane computes its
own layout (offsets are written into checkpoint manifests); ``FlatBinding`` does the rest.
"""
from __future__ import annotations

import torch
import torch.nn as nn

ALIGN = 64  # elements: every tensor starts 128-B aligned in the bf16 buffers


def _round(x: int, a: int) -> int:
    return (x + a - 1) // a * a


def zero_plan(spans, total: int, max_ranges: int = 8):
    """Ranges of a flat gradient buffer to zero before a step: the merged ``(offset, numel)`` spans of
    the parameters whose gradients are *accumulated* into their views (everything but the grad-sink
    params, whose kernels overwrite their views). ``None`` (zero the whole buffer in one launch)
    when that is most of the buffer or would take more than ``max_ranges`` launches. BERT-base:
    the embeddings only, 24M of 110M elements."""
    merged = []
    for off, n in sorted(spans):
        if merged and off <= merged[-1][0] + merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], off + n - merged[-1][0])
        else:
            merged.append([off, n])
    if len(merged) > max_ranges or sum(n for _, n in merged) > total // 2:
        return None
    return [tuple(r) for r in merged]


def zero_grads_(flat: torch.Tensor, plan) -> None:
    if plan is None:
        flat.zero_()
        return
    for off, n in plan:
        flat.narrow(0, off, n).zero_()


def install_fp8_weights(model: nn.Module, resolve) -> None:
    """Give every fp8 module (``fp8 = True``) a ``_psd_w8(w2)`` hook that returns the MX e4m3 copy
    of its weight the data plane pulled with the bf16 working copy -- views (q [Cout, K], E8M0
    scales [Cout*K/32]) into the flat fp8 buffers -- or None when the weight is not in them.
    ``resolve()`` -> (q_flat, scale_flat, params_flat) of the current working buffers (AsyncPS
    alternates two)."""
    for m in model.modules():
        w = getattr(m, "weight", None)
        if not getattr(m, "fp8", False) or not isinstance(w, nn.Parameter):
            continue

        def pub(w2, m=m):
            bufs = resolve()
            if bufs is None:
                return None
            qf, sf, pf = bufs
            wt = m.weight
            off = (wt.data_ptr() - pf.data_ptr()) // wt.element_size()
            n = wt.numel()
            if off < 0 or off + n > pf.numel() or off % 32 or n % 32 or w2.numel() != n:
                return None
            return qf.narrow(0, off, n).view(w2.shape), sf.narrow(0, off // 32, n // 32)

        m._psd_w8 = pub


def _flat_view(flat: torch.Tensor, off: int, p: torch.Tensor) -> torch.Tensor:
    """View of ``flat[off:off+numel]`` with the same shape *and strides* as ``p`` (channels_last
    conv weights stay channels_last)."""
    n = p.numel()
    seg = flat.narrow(0, off, n)
    if p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last) and not p.is_contiguous():
        o, i, kh, kw = p.shape
        return seg.view(o, kh, kw, i).permute(0, 3, 1, 2)
    return seg.view(p.shape)


def spread_owners(num_shards: int, world: int) -> list[int]:
    """Default placement: P shards spread evenly over the node (2 of 8 -> ranks 0 and 4)."""
    if not 1 <= num_shards <= world:
        raise ValueError(f"num_shards must be in [1, world={world}], got {num_shards}")
    return [k * world // num_shards for k in range(num_shards)]


class FlatBinding:
    """``model`` bound to flat buffers of ``total`` elements by ``layout``, the plane's list of
    ``(name, param, offset, numel)``. Modules that can write their parameter gradients straight into
    the flat gradient buffer (``psd_direct_grad_params()``: fused BN, linear, layer norm) get a grad
    sink; their params keep ``.grad = None`` so autograd adopts the written view instead of
    launching an accumulate kernel."""

    def __init__(self, model: nn.Module, layout: list, total: int):
        self.model, self.layout, self.total = model, layout, total
        self.direct = set()
        for m in model.modules():
            if hasattr(m, "psd_direct_grad_params"):
                self.direct.update(id(dp) for dp in m.psd_direct_grad_params() if dp is not None and dp.requires_grad)
                m._psd_grad_sink = self.sink
        self.direct_params = [p for (_, p, _o, _n) in layout if id(p) in self.direct]
        # grad-sink views are overwritten every step: only the accumulated ones need zeroing (a sink
        # param that gets no gradient in a step is zeroed when its bucket is flushed)
        self.zero_plan = zero_plan([(o, n) for (_, p, o, n) in layout if id(p) not in self.direct], total)
        self.arrived: set = set()
        self.grad_views = None  # {id(p): view} into the current gradient buffer
        self._views = {}  # per gradient buffer (AsyncPS alternates two)
        self.hooks = []

    # ------------------------------------------------------------------ views
    def initial(self, device) -> torch.Tensor:
        """fp32 staging of the parameters' current values, in the flat layout."""
        init = torch.zeros(self.total, dtype=torch.float32, device=device)
        for _, p, o, _n in self.layout:
            _flat_view(init, o, p).copy_(p.detach().float())
        return init

    def bind_params(self, flat: torch.Tensor):
        for _, p, o, _n in self.layout:
            p.data = _flat_view(flat, o, p)

    def bind_grads(self, flat: torch.Tensor):
        """Make ``flat`` the current gradient buffer: ``p.grad`` views of it (built once per buffer),
        None for the sink params."""
        if id(flat) not in self._views:
            self._views[id(flat)] = (flat, {id(p): _flat_view(flat, o, p) for (_, p, o, _n) in self.layout})
        self.grad_views = views = self._views[id(flat)][1]
        for _, p, _o, _n in self.layout:
            p.grad = None if id(p) in self.direct else views[id(p)]

    def sink(self, p):
        """Flat-gradient view a fused op may write ``p``'s gradient into (or None)."""
        if id(p) not in self.direct:
            return None
        v = self.grad_views[id(p)]
        # a fresh view (refcount 1) so autograd's AccumulateGrad adopts it instead of cloning
        return v.view(v.shape)

    # ------------------------------------------------------------------ zeroing and arrival
    def watch(self, launch, overlap: bool = True):
        """Call ``launch(bucket)`` for each bucket (``set_buckets``) once its last gradient has
        arrived (``overlap``), else at ``launch_ready(flush=True)``."""
        self._launch, self.overlap = launch, overlap
        self.hooks = [p.register_post_accumulate_grad_hook(self.on_grad) for _, p, _o, _n in self.layout]

    def set_buckets(self, buckets: list):
        """``buckets``: the plane's, in launch order, each with ``.params``, ``.pending``, ``.index``."""
        self.buckets = buckets
        self._p2b = {id(p): b for b in buckets for (_, p, _o, _n) in b.params}
        self._next = 0

    def begin(self, grads: torch.Tensor):
        """Before forward: zero the accumulated ranges of ``grads``, reset the arrival bookkeeping."""
        zero_grads_(grads, self.zero_plan)
        self.arrived = set()
        for b in self.buckets:
            b.pending = len(b.params)
        self._next = 0

    def on_grad(self, p):
        self.arrived.add(id(p))
        if id(p) in self.direct:
            v = self.grad_views[id(p)]
            if p.grad is not None and p.grad.data_ptr() != v.data_ptr():
                v.copy_(p.grad)  # producer did not use the sink (reference / CPU path)
        self._p2b[id(p)].pending -= 1
        if self.overlap:
            self.launch_ready()

    def launch_ready(self, flush: bool = False):
        """Launch strictly in bucket order, so every rank enqueues the same sequence (an out-of-order
        ready bucket waits for its predecessors). ``flush``: also the buckets whose hooks did not all
        fire; the sink views no kernel wrote are zeroed first."""
        while self._next < len(self.buckets) and (flush or self.buckets[self._next].pending <= 0):
            b = self.buckets[self._next]
            if b.pending > 0 and self.zero_plan is not None:  # flushed with gradients missing
                for _, p, _o, _n in b.params:
                    if id(p) in self.direct and id(p) not in self.arrived:
                        self.grad_views[id(p)].zero_()
            self._launch(b)
            self._next += 1

    # ------------------------------------------------------------------ canonical layout
    def canon_index(self):
        """(flat offset, canonical offset, numel) per parameter, canonical = model.named_parameters
        order without padding -- a layout independent of world size, shard count and buckets."""
        where = {id(p): (o, n) for (_, p, o, n) in self.layout}
        out, c = [], 0
        for _, p in self.model.named_parameters():
            if id(p) in where:
                o, n = where[id(p)]
                out.append((o, c, n))
                c += n
        return out, c

    def to_canonical(self, full: torch.Tensor) -> torch.Tensor:
        idx, n = self.canon_index()
        canon = torch.empty(n, dtype=torch.float32, device=full.device)
        for o, c, k in idx:
            canon.narrow(0, c, k).copy_(full.narrow(0, o, k))
        return canon

    def from_canonical(self, canon: torch.Tensor, key: str) -> torch.Tensor:
        idx, n = self.canon_index()
        if canon.numel() != n:
            raise ValueError(f"canonical {key} has {canon.numel()} elements, model has {n}")
        full = torch.zeros(self.total, dtype=torch.float32, device=canon.device)
        for o, c, k in idx:
            full.narrow(0, o, k).copy_(canon.narrow(0, c, k))
        return full

    def num_params(self) -> int:
        return sum(n for (_, _, _, n) in self.layout)

    def param_meta(self, params=None) -> list:
        """``(name, shape, offset, numel)`` of ``params`` (default: the whole layout), for manifests."""
        return [(n, list(p.shape), o, k) for (n, p, o, k) in (self.layout if params is None else params)]

    # ------------------------------------------------------------------ release
    def release(self, detach: bool = False):
        """Remove the grad hooks and the sinks this binding installed (a later plane's stay);
        ``detach``: the parameters also leave the flat buffers, keeping their values."""
        for h in self.hooks:
            h.remove()
        self.hooks = []
        for m in self.model.modules():
            if getattr(m, "_psd_grad_sink", None) == self.sink:
                del m._psd_grad_sink
        if detach:
            for p in self.model.parameters():
                p.grad = None
                p.data = p.data.clone()
