"""Asynchronous parameter server: apply-on-arrival with a stale-synchronous bound, over peer memory.

The collective data plane (``collective_ps.CollectivePS``) moves every rank in lock-step: its
"asynchrony" is a fixed S-step gradient delay. This one is the real thing (BASELINE.json config 3,
SURVEY 7.5.2): each PS shard applies each worker's push the moment it lands, versions advance per
push, and a worker blocks only when it would lead the slowest worker by more than S steps.

Per step of a worker (``begin_step`` / grad hooks / ``finish_step``):

  pull    SSP wait (every worker's clock at every shard >= step - S), then DMA-copy each shard's
          latest published snapshot into the working weights (pinned while the copy runs)
  fwd/bwd on the current stream; as each gradient bucket completes (post-accumulate-grad hook) its
          slices are DMA-copied over xGMI straight into this worker's inbox slot on the owning GPU
          (comm stream, overlapped with the rest of backward)
  commit  once the copies have landed, a message (step, pulled versions) is posted to each shard's
          single-producer ring in the shared control block

The owner's native engine thread (``csrc/async_ps.cpp``) applies each message with the fused gfx950
optimizer kernel, writes the bf16 snapshot
into a free publish buffer and advances the shard version, the worker's clock and the staleness
histogram (staleness = shard version at apply - version the gradient was computed on).

Optimizer semantics (``semantics``):

  "round" (default): K-batch asynchronous SGD with K = W. Each shard takes the pushes
          in arrival order, from whichever workers, and every K of them make ONE optimizer step on
          their average with the synchronous hyperparameters (the K inbox slots are summed inside
          the fused apply kernel; above 16, in groups of 16 into fp32 partials first). A worker's clock advances when the round holding its push has
          been applied. At SSP bound 0 the rounds are exactly the synchronous steps (a worker
          cannot push step t+1 before every step-t push is applied), so the trajectory equals the
          synchronous one; at S >= 1 a round may mix steps (stale gradients, bounded by S).
  "push": every push is applied on arrival as its own step, with the per-push hyperparameters of
          ``csrc/async_hyper.h`` (SGD grad x 1/W; momentum beta^(1/W) and a rescaled lr; Adam/AdamW
          beta^(1/W), lr/W), which keep the synchronous per-round EMA horizons and steady-state
          displacement -- lower latency, approximate. Both are pinned against the synchronous
          trajectory in tests/test_async_ps.py.

Gradient clipping (``OptimConfig.clip_norm > 0``) is per push: the buckets leave raw while backward
runs; ``finish_step`` then runs the norm pass over the whole flat gradient (``grad_clip_coef_``,
csrc/kernels/clip.hip), sends the resulting 256-byte scalar block after the buckets
(``engine.push_scalars``, same transport, ahead of the commit) and the owner's fused apply multiplies
each source of a round by its worker's coefficient ``min(1, clip_norm / (||g|| + 1e-6))`` in the
pass that sums them. ``grad_norm()`` reports the last step's (norm, coefficient).

Gradient push compression (``push_dtype="fp8"``): a push carries the gradient as OCP MX e4m3, one
E8M0 scale byte per 32 consecutive elements of the flat gradient buffer (blocks numbered from its
element 0; every shard, bucket and tensor boundary is a multiple of 64 elements, so no block
straddles one), with the scale and rounding of ``ops.quantize_mx_ref``. An inbox slot is then
``shard_len`` payload bytes followed by ``shard_len / 32`` scale bytes. The owner's update of a round
uses ``grad_scale * sum_k c_k * dq(q_k)``, ``dq`` the blockwise ``q * 2^(scale - 127)`` in fp32, in
the same source order and with the same additions as the bf16 push -- weight decay, momentum, Adam
moments, LARS / LAMB norms and the clip coefficients all see the dequantised sum. The clip norm is
that of the gradient BEFORE quantisation (the norm pass runs over the worker's raw buffer). A NaN or
+-inf gradient element arrives as NaN (e4m3 byte 0x7F). The bytes do not depend on the grid, on
``xfer_blocks`` or on the transport. No e5m2, no stochastic rounding.

Error feedback (``push_error_feedback=True``, fp8 push only): each worker keeps ONE fp32 residual
``r`` of ``total`` elements, laid out like the flat gradient buffer, zero at the start
(``push_residual``). A push of ``[lo, hi)`` quantises ``v = fp32(g) + r`` instead of ``g`` and leaves
``r = v - dq(q(v))`` behind, in place, in the kernel pass that quantises (exact in fp32: ``dq``
scales by a power of two); a NaN / +-inf element of ``v`` travels as NaN and its residual becomes 0.
Reference: ``ops.push_quant_mx_ef_ref``. The wire format, the slot size and the owner's apply are
untouched: the owner cannot tell whether feedback is on. A component too small for its block's
scale is no longer dropped on every step: it accumulates in ``r`` until it crosses half a quantum.
With clipping the norm is still that of the raw ``g`` (the residual is not in the norm pass): the
owner computes ``c_k * dq(q(g + r))``, the chosen approximation. Pushes of one range are
stream-ordered (``_resid_on``). The self-test and the probes push through the feedback path and
leave the residual zero. Checkpoints carry each worker's residual (``save`` / ``load``); the elastic
re-shard and crash restore (``canonical_state`` / ``load_canonical_state``) drop it.

Layout: the parameters live in one flat working buffer (``.data`` views, reverse registration
order, 64-element aligned) split into P contiguous shards (cut at the nearest tensor starts when the
optimizer needs tensor boundaries: lars, lamb, ``exclude_1d``; each owner then applies with the
layer table of its shard, csrc/kernels/optim_lw.hip; round semantics only for lars / lamb);
gradients alternate between two flat buffers so the next step never waits for the previous step's push copies. One node, one process
per GPU (the control block is POSIX shared memory); ``device=cpu`` runs the identical protocol on
host shared memory (CPU CI / gloo plumbing).

Reference parity: ``ParameterServerCore::receive_gradients`` (src/parameter_server.cpp:18-75)
buffers every push and applies only at the all-worker barrier (:37); there is no async mode and no
version, so none of this has a counterpart beyond the push/pull/apply roles.
"""
from __future__ import annotations

import os
import time
import uuid
from dataclasses import dataclass, field

import torch
import torch.distributed as dist
import torch.nn as nn

from .. import native
from ..ops import dequantize_mx_ref, quantize_mx_ref
from ..ops.optim import LAYERWISE, LayerTable, OptimConfig, OptimDyn, clip_chunks, grad_clip_coef_
from ..utils.config import fault, feature
from .flat import ALIGN, FlatBinding, _round, install_fp8_weights, spread_owners


def snap_bounds(total: int, P: int, starts: list[int]) -> list[int]:
    """Shard boundaries on tensor starts: for each ideal cut ``total * k / P`` the nearest tensor
    start, strictly increasing (a cut never takes a start an earlier cut took, and leaves one for
    every later cut). ``starts``: the tensors' offsets in increasing order, the first 0."""
    if P > len(starts):
        raise ValueError(f"{P} shards cut on tensor starts need at least {P} tensors, the model has {len(starts)}")
    bounds, prev = [0], 0
    for k in range(1, P):
        ideal = total * k // P
        cand = range(prev + 1, len(starts) - (P - 1 - k))
        prev = min(cand, key=lambda i: (abs(starts[i] - ideal), i))
        bounds.append(starts[prev])
    return bounds + [total]


class _NoTransport:
    """The async plane moves tensors by peer-memory DMA, not through a Transport; ``abort`` is the
    hook a failure detector (runtime/elastic.py _Watchdog) calls to fail every blocked wait."""

    name = "ipc"
    capturable = False

    def __init__(self, ps=None):
        self.ps = ps

    def abort(self):
        if self.ps is not None and self.ps.engine is not None:
            self.ps.engine.inject_error("aborted by a failure detector (a peer was declared dead)")


@dataclass
class _Bucket:
    index: int
    params: list = field(default_factory=list)  # (name, param, offset, numel)
    lo: int = 0
    hi: int = 0
    pending: int = 0


def _store_and_group():
    if dist.is_available() and dist.is_initialized():
        return dist.distributed_c10d._get_default_store(), dist.get_rank(), dist.get_world_size()
    return dist.HashStore(), 0, 1


class AsyncPS:
    def __init__(self, model: nn.Module, optim: OptimConfig, num_shards: int | None = None, staleness: int = 1,
                 bucket_mb: float = 16.0, device: torch.device | None = None, ps_ranks: list[int] | None = None,
                 worker_ranks: list[int] | None = None, param_dtype: torch.dtype = torch.bfloat16, nbuf: int = 4,
                 timeout_s: float | None = None, overlap: bool = True, store=None, log: bool = False,
                 semantics: str = "round", pull_dtype: str = "bf16", schedule: str = "free", xfer: str = "auto",
                 push_dtype: str = "bf16", push_error_feedback: bool = False):
        """``semantics``: "round" (K-batch async, default) or "push" (apply-on-arrival with the
        per-push hyperparameters of csrc/async_hyper.h); see the module docstring.
        ``schedule`` "fixed" ("round" semantics only): round r holds exactly every worker's step-r
        push and the pull of step t takes exactly version max(t - S, 0) -- every gradient is
        S rounds stale whatever the timing, so an S >= 1 run is bit-for-bit reproducible and equals
        synchronous SGD with S-step-delayed gradients (csrc/async_ps.h set_fixed_schedule). "free"
        (default): rounds in arrival order, pulls of the latest admissible snapshot.
        ``pull_dtype`` "fp8" (the Wide-ResNet fp8-weights config): each owner also publishes the MX
        e4m3 copy of its snapshot (one E8M0 scale per 32 elements, quantised from the fp32 master
        right after the apply, csrc/async_ps.cpp quant_publish); workers pull 1.03 bytes/parameter
        instead of 2, dequantise the bf16 working copy locally and hand the e4m3 weights + scales to
        the fp8 convolutions (no per-step weight quantisation on the worker).
        ``xfer`` (GPU): how pushes and pulls cross to the owners' memory -- "kernel": one scatter /
        gather kernel per bucket push / pull that reads or writes every owner's peer-mapped memory
        at once, one xGMI link per owner (kernels/xfer.hip); "copy": one hipMemcpyAsync per shard
        (one link at a time); "auto" (default): the kernel, falling back to the copies (on every
        rank together, logged in ``xfer_mode``) if its start-up self-test fails.
        ``push_dtype`` "fp8": a worker's gradient crosses to the owners as OCP MX e4m3 -- one E8M0
        scale byte per 32 consecutive elements of the flat gradient buffer, 33/32 bytes per element
        instead of 2 -- quantised inside the push (the scatter kernel, csrc/kernels/xfer.hip; with
        ``xfer="copy"`` into a staging buffer first; on the host for ``device=cpu``), and the owner's
        fused apply dequantises the inbox slots as it sums them (module docstring). "bf16" (default):
        the raw gradient, exactly as before.
        ``push_error_feedback`` (``push_dtype="fp8"`` only): each worker keeps what the quantiser
        dropped in one fp32 residual laid out like the flat gradient buffer (``push_residual``) and
        adds it to the next gradient before quantising, inside the same push kernel (module
        docstring). Off (default): every push discards its quantisation error."""
        if push_dtype not in ("bf16", "fp8"):
            raise ValueError(f"push_dtype must be bf16 or fp8, got {push_dtype!r}")
        if push_error_feedback and push_dtype != "fp8":
            raise ValueError(f"push_error_feedback=True needs push_dtype='fp8' (a {push_dtype} push drops nothing to "
                             f"feed back)")
        self.push_dtype = push_dtype
        self.push_mx = push_dtype == "fp8"
        self.push_error_feedback = bool(push_error_feedback)
        if xfer not in ("auto", "kernel", "copy"):
            raise ValueError(f"xfer must be auto, kernel or copy, got {xfer!r}")
        if semantics not in ("round", "push"):
            raise ValueError(f"semantics must be 'round' or 'push', got {semantics!r}")
        if semantics == "push" and optim.kind in LAYERWISE:
            raise ValueError(f"optimizer {optim.kind!r} takes whole rounds (the trust ratio is a property of the "
                             f"round's gradient): semantics='push' is not supported with it, use 'round'")
        self.xfer = xfer
        self.model = model
        self.cfg = optim
        st, self.rank, self.world = _store_and_group()
        self.store = store or st
        self.t = _NoTransport(self)
        self.worker_ranks = list(worker_ranks) if worker_ranks is not None else list(range(self.world))
        self.is_worker = self.rank in self.worker_ranks
        self.W = len(self.worker_ranks)
        self.owners = list(ps_ranks) if ps_ranks is not None else spread_owners(num_shards or self.world, self.world)
        self.P = len(self.owners)
        self.my_shards = [k for k, r in enumerate(self.owners) if r == self.rank]
        self.S = int(staleness)
        self.overlap = overlap
        self.device = device or next(model.parameters()).device
        self.is_cuda = self.device.type == "cuda"
        if param_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError("AsyncPS publishes bf16 or fp32 weights")
        if pull_dtype not in ("bf16", "fp8"):
            raise ValueError(f"pull_dtype must be bf16 or fp8, got {pull_dtype}")
        self.pull_mx = pull_dtype == "fp8" and param_dtype == torch.bfloat16 and self.is_cuda
        self.param_dtype = param_dtype
        self.step_idx = 0
        if schedule not in ("free", "fixed") or (schedule == "fixed" and semantics != "round"):
            raise ValueError(f"schedule must be 'free' or 'fixed' (fixed: round semantics), got {schedule!r}")
        self.schedule = schedule
        if schedule == "fixed":
            nbuf = max(nbuf, self.S + 2)  # the last S + 1 versions stay published
        self.pulled = [0] * self.P
        timeout_s = float(os.environ.get("PSD_ASYNC_TIMEOUT", timeout_s or 600.0))

        # ---- flat layout (same conventions as CollectivePS: reverse registration, 64-aligned)
        params = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        params.reverse()
        off = 0
        layout = []
        for n, p in params:
            layout.append((n, p, off, p.numel()))
            off += _round(p.numel(), ALIGN)
        total = _round(max(off, ALIGN), self.P * ALIGN)
        self.total = total
        # P contiguous shards, 64-element aligned, balanced by size
        if optim.needs_layers:
            # per-tensor norms / decay flags: a tensor must not straddle two owners, so the cuts move
            # to the nearest tensor starts (the apply's result does not depend on where they fall)
            bounds = snap_bounds(total, self.P, [o for (_n, _p, o, _k) in layout])
        else:
            bounds = [_round(total * k // self.P, ALIGN) for k in range(self.P)] + [total]
        self.shard_off = bounds[:-1]
        self.shard_len = [bounds[k + 1] - bounds[k] for k in range(self.P)]

        dev = self.device
        self._layout = layout
        self.flat = FlatBinding(model, layout, total)
        self._zero_plan = self.flat.zero_plan
        self._build_buckets(bucket_mb)
        init = self.flat.initial(dev)
        # working weights: with S >= 1 two buffers alternate per step, so the pull of step t+1 (DMA
        # from the owners' publish buffers) runs on a side stream while step t computes
        # (world 1: the pull is one local device copy, so pulling straight into the working weights at
        # the step start costs less than the prefetch + working-buffer copy -- feature async_direct_pull)
        self.prefetch = self.S >= 1 and not (self.world == 1 and feature("async_direct_pull"))
        self.pbufs = [init.to(param_dtype)]
        if self.prefetch:
            self.pbufs.append(self.pbufs[0].clone())
        # the model's parameters view ONE working buffer; each step copies its pulled buffer into it
        # on the compute stream (_to_work: a ~70 us device copy for BERT-base) instead of re-pointing
        # every parameter from Python (~200 `p.data =` per step: ~1 ms of host time at the step
        # boundary, where the GPU waited for it -- profiles/r5/bert_base_b256_r5_kernels.md)
        self.pwork = self.pbufs[0].clone() if self.prefetch else self.pbufs[0]
        self.cb = 0
        # MX pull targets (one per working buffer): e4m3 [total] + E8M0 scales [total / 32]
        self.q8s = [torch.zeros(total, dtype=torch.float8_e4m3fn, device=dev) for _ in self.pbufs] if self.pull_mx else []
        self.sc8s = [torch.full((total // 32,), 127, dtype=torch.uint8, device=dev) for _ in self.pbufs] \
            if self.pull_mx else []
        self.grads = [torch.zeros(total, dtype=param_dtype, device=dev) for _ in range(2)]
        self.gb = 0
        # error feedback of the fp8 push: ONE residual per worker (the gradient buffers alternate, the
        # residual does not), read and rewritten in place by the launch that quantises a range. Pushes
        # of one range must therefore be stream-ordered: _resid_stream is the stream of the last launch
        # that touched the residual, and _resid_on orders a launch on another stream behind it.
        self.push_residual = torch.zeros(total, dtype=torch.float32, device=dev) \
            if self.push_error_feedback and self.is_worker else None
        self._resid_stream = None
        # per-push global-norm clipping (OptimConfig.clip_norm > 0): the push scalars -- 256-byte
        # blocks [c, ||g||, 0...] -- alternate with the gradient buffers (step t-2's push may still be
        # reading the other one); one scratch of per-chunk partial sums. Off: nothing is allocated.
        self.clip = optim.clip_norm > 0
        self.scal = [torch.zeros(64, dtype=torch.float32, device=dev) for _ in range(2)] if self.clip else []
        self.clip_partials = torch.zeros(clip_chunks(total), dtype=torch.float32, device=dev) if self.clip else None
        self._last_scal = None
        f32 = dict(dtype=torch.float32, device=dev)
        # per-push hyperparameters (module docstring)
        self.semantics = semantics
        # K = W: every round completes (a cap below W would strand a partial round at W > 16 and
        # hold a worker's clock back forever); the engine pre-reduces above 16 sources
        self.round = self.W if semantics == "round" else 1
        if semantics == "push":
            self.hyper = native().async_hyper(optim.code, self.W, optim.momentum, optim.beta1, optim.beta2,
                                              optim.weight_decay)
        else:
            self.hyper = dict(lr_factor=1.0, grad_scale=1.0 / self.round, momentum=optim.momentum, beta1=optim.beta1,
                              beta2=optim.beta2, weight_decay=optim.weight_decay)
        self.master, self.state1, self.state2, self.dyn = {}, {}, {}, {}
        for k in self.my_shards:
            self.master[k] = init.narrow(0, self.shard_off[k], self.shard_len[k]).clone()
            if optim.num_states >= 1:
                self.state1[k] = torch.zeros(self.shard_len[k], **f32)
            if optim.num_states >= 2:
                self.state2[k] = torch.zeros(self.shard_len[k], **f32)
            self.dyn[k] = OptimDyn(dev, lr=optim.lr * self.hyper["lr_factor"], grad_scale=self.hyper["grad_scale"])
        del init
        # one layer table per owned shard (tensor boundaries relative to the shard's start)
        self.layers = {}
        if optim.needs_layers:
            flat = [(o, k, p.dim()) for (_n, p, o, k) in layout]
            for k in self.my_shards:
                self.layers[k] = LayerTable.for_range(flat, self.shard_off[k], self.shard_off[k] + self.shard_len[k],
                                                      optim.exclude_1d, dev, ALIGN)

        self.flat.bind_params(self.pwork)
        self.flat.bind_grads(self.grads[self.gb])
        self.flat.watch(self._push, overlap)
        if self.is_cuda:
            # ONE push stream: HIP maps a process's streams onto GPU_MAX_HW_QUEUES = 4 hardware
            # queues, and compute + engine apply + push + pull already take four -- a fifth stream
            # shares a queue with one of them and serialises behind its work (ResNet-50 b1024 async
            # S = 1: 91-95 ms/step with two push streams vs 78 ms synchronous,
            # profiles/async_push_streams_r4.md). The owners' links overlap inside one launch
            # instead (kernels/xfer.hip).
            self.comm_stream = torch.cuda.Stream(device=dev)
            self.pull_stream = torch.cuda.Stream(device=dev)
            self.push_done = [None, None]
            self.step_done = [None, None]  # end of a step's work on the compute stream, per buffer
            self.pull_done = [None, None]
        self._prefetched = None  # (step, pulled versions) of the pull issued ahead

        # ---- native engine: control block (rank 0 creates), memory exchange, initial publish
        # instance sequence number from the store itself (a per-rank counter key): every rank
        # agrees on it for any store lifetime -- an id(store)-keyed local count could collide when
        # a freed elastic generation's store address is reused on some ranks only
        n = int(self.store.add(f"psd/async/seq/{self.rank}", 1))
        key = f"psd/async/{n}"
        if self.rank == 0:
            self.store.set(f"{key}/shm", f"/psd_{os.getpid()}_{uuid.uuid4().hex[:12]}")
        shm = self.store.get(f"{key}/shm").decode()
        C = native()
        devidx = dev.index if (self.is_cuda and dev.index is not None) else (torch.cuda.current_device()
                                                                            if self.is_cuda else -1)
        if self.rank != 0:
            self.store.wait([f"{key}/ctl"])
        self.engine = C.AsyncEngine(self.rank, self.world, self.owners, self.worker_ranks, self.shard_off,
                                    self.shard_len, self.S, nbuf, shm, self.rank == 0, devidx, timeout_s,
                                    torch.finfo(param_dtype).bits // 8, self.pull_mx, self.clip, self.push_mx,
                                    cached_local=feature("async_cached_local"),
                                    apply_background=feature("async_apply_background"))
        if self.rank == 0:
            self.store.set(f"{key}/ctl", b"1")
        try:
            self._connect(key, optim, log)
        except Exception:
            # release this rank's shared memory / IPC mappings before the (collective) error escapes
            self.engine.stop()
            self.engine.close_peers()
            self.engine.free_local()
            self.engine = None
            raise
        self.tracer = None
        self.closed = False
        self._ckpt_seq = 0
        if self.pull_mx:  # the fp8 convolutions read the pulled e4m3 weights of the current buffer
            install_fp8_weights(model, lambda: (self.q8s[self.cb], self.sc8s[self.cb], self.pwork))

    def _connect(self, key, optim, log):
        """Exchange memory descriptors, map the peers, publish version 0, self-test, start."""
        self._key = key
        self.store.set(f"{key}/desc/{self.rank}", self.engine.local_desc())
        err = ""
        try:
            for r in range(self.world):
                self.engine.attach_peer(r, self.store.get(f"{key}/desc/{r}"))
        except Exception as e:  # noqa: BLE001 -- reported collectively below
            err = f"rank {self.rank}: {e}"
        self._agree("attach", err)
        for k in self.my_shards:
            h = self.hyper
            self.engine.set_shard_state(k, self.master[k], self.state1.get(k), self.state2.get(k), self.dyn[k].t,
                                        optim.code, h["momentum"], optim.dampening, optim.nesterov,
                                        h["weight_decay"], h["beta1"], h["beta2"], optim.eps)
            if k in self.layers:
                self.engine.set_shard_layers(k, self.layers[k].t, optim.trust_coef)
            self.engine.publish_initial(k)
        self.engine.set_round(self.round)
        self.engine.set_fixed_schedule(self.schedule == "fixed")
        if log:
            self.engine.enable_log(True)
        self._barrier("init")
        self.xfer_fallback = None
        if self.is_cuda:
            self.engine.set_xfer(self.xfer != "copy")
        try:
            self.selftest("kernel" if self.is_cuda and self.xfer != "copy" else "copy")
        except RuntimeError as e:  # collective: every rank sees the same failure
            if not (self.is_cuda and self.xfer == "auto"):
                raise
            self.xfer_fallback = str(e)[:300]
            self.engine.set_xfer(False)
            self.selftest("copy")
        self.xfer_mode = self.engine.xfer_mode()
        self.engine.start()

    def selftest(self, attempt: str = "copy"):
        """Collective start-up check of the peer-memory paths on this node (before any training):
        every worker DMA-writes a known pattern into its inbox on every shard owner, and every
        owner verifies what landed; every worker pulls the version-0 snapshots and compares each
        shard with its owner's published checksum (the ranks' weights need not agree yet: an elastic
        joiner's are replaced by load_canonical_state next). Raises on any mismatch on any rank (so a
        caller can fall back to the collective plane instead of training on a broken path).

        ``attempt`` ("kernel" / "copy": the transport under test) tags every store key of this
        attempt -- checksums, barrier, verdict -- so a retry after a failed kernel-path attempt never
        meets the first attempt's counters (a reused barrier key is already at world size and would
        let an owner check its inbox before the workers' second pushes landed)."""
        dev = self.device
        tag = f"{attempt}"
        ok, why = True, ""
        for k in self.my_shards:  # the snapshot each owner published: bf16/fp32(master)
            v = self.master[k].to(self.param_dtype).double()
            self.store.set(f"{self._key}/ck/{tag}/{k}", f"{float(v.sum())!r} {float(v.abs().sum())!r}")
        if self.is_worker:
            pat = self._selftest_pattern(0, self.total, self.rank)
            # with error feedback the push goes through the feedback kernel, as training's will: the
            # pattern is exact in MX e4m3, so a zero residual stays zero (reset below all the same)
            self.engine.push(0, pat, 0, self.total, self._stream_ptr(), self._resid_on())
            self.reset_push_residual()
            if self.clip:  # the scalar slots travel by the same transport: round-trip a block too
                blk = torch.arange(64, dtype=torch.float32, device=dev) + 0.5 * (self.rank + 1)
                self.engine.push_scalars(0, blk, self._stream_ptr())
            got = torch.empty_like(self.params_flat)
            self.engine.pull(0, got, self._stream_ptr())
            if self.is_cuda:
                torch.cuda.synchronize(dev)
            for k in range(self.P):
                self.store.wait([f"{self._key}/ck/{tag}/{k}"])
                want_s, want_a = (float(x) for x in self.store.get(f"{self._key}/ck/{tag}/{k}").decode().split())
                sl = got.narrow(0, self.shard_off[k], self.shard_len[k]).double()
                if abs(float(sl.sum()) - want_s) > 1e-6 * max(want_a, 1.0) or \
                        abs(float(sl.abs().sum()) - want_a) > 1e-6 * max(want_a, 1.0):
                    ok, why = False, f"rank {self.rank}: pulled shard {k} != its owner's snapshot"
        if fault("selftest_fail_rank") == self.rank:  # fault injection (tests)
            ok, why = False, f"rank {self.rank}: injected self-test failure"
        if attempt == "kernel" and fault("selftest_fail_kernel") == self.rank:  # fails the kernel path only
            ok, why = False, f"rank {self.rank}: injected kernel-transport self-test failure"
        self._barrier(f"selftest-push/{tag}")
        for k in self.my_shards:
            for wi, w in enumerate(self.worker_ranks):
                v = self.engine.inbox_view(k, wi, 0)
                want = self._selftest_pattern(self.shard_off[k], self.shard_off[k] + self.shard_len[k], w)
                if self.push_mx:
                    # the pattern is exact in MX e4m3: payload and scale bytes must be its quantisation,
                    # and dequantise back to it
                    sv = self.engine.inbox_scales_view(k, wi, 0)
                    wq, ws = quantize_mx_ref(want)
                    if not (torch.equal(v.view(torch.uint8), wq.view(torch.uint8)) and torch.equal(sv, ws)
                            and torch.equal(dequantize_mx_ref(v.view(torch.float8_e4m3fn), sv), want.float())):
                        ok, why = False, f"rank {self.rank}: shard {k} MX inbox of worker {w} holds wrong data"
                    sv.zero_()
                elif not torch.equal(v, want):
                    ok, why = False, f"rank {self.rank}: shard {k} inbox of worker {w} holds wrong data"
                v.view(torch.uint8).zero_() if self.push_mx else v.zero_()
                if self.clip:
                    sv = self.engine.scalar_view(k, wi, 0)
                    if not torch.equal(sv, torch.arange(64, dtype=torch.float32, device=dev) + 0.5 * (w + 1)):
                        ok, why = False, f"rank {self.rank}: shard {k} scalar slot of worker {w} holds wrong data"
                    sv.zero_()
        if self.is_cuda:
            torch.cuda.synchronize(dev)
        self._agree("selftest", "" if ok else why, attempt=tag)
        self.selftest_ok = True

    def _selftest_pattern(self, lo: int, hi: int, rank: int) -> torch.Tensor:
        """Elements [lo, hi) of the self-test gradient of worker ``rank``: depends on rank, shard
        (through the position) and position. bf16 push: ``i % 251 + rank + 1``. fp8 push: that pattern
        is not representable in e4m3, so small integers in [-7, 7] (every block holds all 15 of them:
        its amax is 7) times a per-block power of two 2^((block + rank) % 9 - 4), which MX e4m3
        holds exactly."""
        i = torch.arange(lo, hi, device=self.device)
        if not self.push_mx:
            return (i % 251 + (rank + 1)).to(self.param_dtype)
        v = (i * 7 + 3 * rank) % 15 - 7
        e = ((i // 32 + rank) % 9 - 4).float()
        return (v.float() * torch.exp2(e)).to(self.param_dtype)

    def _agree(self, tag: str, err: str, attempt: str = ""):
        """Collective status exchange through the store: every rank raises if any rank failed.
        ``attempt`` keeps the keys of a retried exchange apart from the earlier ones."""
        key = f"{self._key}/{tag}" + (f"/{attempt}" if attempt else "")
        self.store.set(f"{key}/{self.rank}", err or "ok")
        errs = []
        for r in range(self.world):
            self.store.wait([f"{key}/{r}"])
            v = self.store.get(f"{key}/{r}").decode()
            if v != "ok":
                errs.append(v)
        if errs:
            raise RuntimeError(f"AsyncPS {tag} failed: " + "; ".join(errs))

    # ------------------------------------------------------------------ helpers
    @property
    def params_flat(self) -> torch.Tensor:
        """The working weights of the current step (the buffer the model's parameters view)."""
        return self.pwork

    @property
    def push_bytes_per_elem(self) -> float:
        """Bytes one gradient element takes on its way to the owner: the element size, or 33/32
        (e4m3 payload + its share of the block's scale byte) under ``push_dtype="fp8"``."""
        return 33.0 / 32.0 if self.push_mx else float(self.grads[0].element_size())

    def _barrier(self, tag: str):
        if self.world == 1:
            return
        k = f"{self._key}/bar/{tag}"
        self.store.add(k, 1)
        t0 = time.time()
        while int(self.store.add(k, 0)) < self.world:
            if time.time() - t0 > 600:
                raise RuntimeError(f"AsyncPS barrier {tag} timed out")
            time.sleep(0.001)

    def _stream_ptr(self, s=None) -> int:
        if not self.is_cuda:
            return 0
        s = s or torch.cuda.current_stream(self.device)
        return s.cuda_stream

    def _mark(self, stream=None, then=None):
        """An event recorded on ``stream`` (None: the current stream); ``then``, a stream, waits for it."""
        ev = torch.cuda.Event()
        ev.record(stream or torch.cuda.current_stream(self.device))
        if then is not None:
            then.wait_event(ev)
        return ev

    def _all_max(self, vals: list, dtype=torch.float64) -> list:
        """Collective: the element-wise maximum over the ranks of a few host scalars."""
        t = torch.tensor(vals, dtype=dtype)
        if self.world > 1 and dist.is_initialized():
            if dist.get_backend() == "nccl":
                t = t.to(self.device)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return t.tolist()

    def _resid_on(self, stream=None):
        """The residual argument of an ``engine.push`` about to be launched on ``stream`` (None: the
        current stream): ``None`` with feedback off. If the last launch that touched the residual ran
        on another stream, ``stream`` first waits for everything issued there (the bucket-to-stream
        mapping, ``rebucket``, the probes and ``reset_push_residual`` may all change streams)."""
        if self.push_residual is None:
            return None
        if self.is_cuda:
            s = stream or torch.cuda.current_stream(self.device)
            last = self._resid_stream
            if last is not None and last != s:
                ev = torch.cuda.Event()
                ev.record(last)
                s.wait_event(ev)
            self._resid_stream = s
        return self.push_residual

    def reset_push_residual(self):
        """Zero this worker's error-feedback residual (no-op with feedback off), ordered behind every
        push issued so far; later pushes are ordered behind the reset."""
        if self._resid_on() is not None:
            self.push_residual.zero_()

    def _to_work(self):
        """The pulled buffer of this step into the working weights (stream-ordered on the current
        stream: after the previous step's kernels, before this step's)."""
        if self.pwork is not self.pbufs[self.cb]:
            self.pwork.copy_(self.pbufs[self.cb])

    def memory_bytes(self) -> dict:
        eb = lambda t: t.numel() * t.element_size()  # noqa: E731
        work = eb(self.pwork) if all(self.pwork is not b for b in self.pbufs) else 0
        return {"params": sum(eb(b) for b in self.pbufs) + work, "grads": 2 * eb(self.grads[0]),
                "master": sum(eb(t) for t in self.master.values()),
                "state": sum(eb(t) for t in list(self.state1.values()) + list(self.state2.values())),
                "push_residual": eb(self.push_residual) if self.push_residual is not None else 0}

    # ------------------------------------------------------------------ per-step protocol
    def begin_step(self, track: bool = True):
        if not self.is_worker:
            return
        t = self.step_idx
        self.gb = t % 2
        if self.is_cuda and self.push_done[self.gb] is not None:
            # the push copies of step t-2 read this gradient buffer
            torch.cuda.current_stream(self.device).wait_event(self.push_done[self.gb])
        self.flat.begin(self.grads[self.gb])
        self.flat.bind_grads(self.grads[self.gb])  # two buffers alternate: every p.grad is re-pointed
        if self.prefetch:
            self.cb = t % 2
            if self._prefetched is not None and self._prefetched[0] == t:
                self.pulled = self._prefetched[1]
                if self.is_cuda:
                    torch.cuda.current_stream(self.device).wait_event(self.pull_done[self.cb])
                self._to_work()
                return
        self.pulled = self._pull_into(t, self.cb, None)
        self._to_work()

    def _pull_into(self, t: int, nb: int, stream) -> list:
        """Pull of step t into working buffer ``nb`` on ``stream`` (None: the current stream): the
        bf16 snapshots, or with MX the e4m3 + scales and their bf16 dequantisation."""
        sptr = stream.cuda_stream if stream is not None else self._stream_ptr()
        if not self.pull_mx:
            return list(self.engine.pull(t, self.pbufs[nb], sptr))
        # the engine dequantises into the bf16 buffer on the same stream (fused into the gather)
        return list(self.engine.pull_mx(t, self.q8s[nb], self.sc8s[nb], self.pbufs[nb], sptr))

    def _prefetch_pull(self, t: int):
        """Issue the pull of step t (the next one) now: the SSP wait happens on the host here, the
        DMA on the pull stream, after the step that last used that buffer (t-2) is done with it."""
        nb = t % 2
        if self.is_cuda:
            if self.step_done[nb] is not None:
                self.pull_stream.wait_event(self.step_done[nb])
            pulled = self._pull_into(t, nb, self.pull_stream)
            self.pull_done[nb] = self._mark(self.pull_stream)
        else:
            pulled = self.engine.pull(t, self.pbufs[nb], 0)
        self._prefetched = (t, list(pulled))

    def _push(self, b: _Bucket):
        g = self.grads[self.gb]
        if self.is_cuda:
            cs = self.comm_stream
            self._mark(then=cs)
            self.engine.push(self.step_idx, g, b.lo, b.hi, cs.cuda_stream, self._resid_on(cs))
        else:
            self.engine.push(self.step_idx, g, b.lo, b.hi, 0, self._resid_on())

    def finish_step(self, track: bool = True):
        if not self.is_worker:
            return
        self.flat.launch_ready(flush=True)
        if self.clip:
            # the whole gradient is in the buffer now (the buckets above are already on their way):
            # one read-only pass -> this push's scalar, which follows the buckets on the comm stream
            # ahead of the commit, so it lands behind the same release as they do
            blk = self.scal[self.gb]
            grad_clip_coef_(self.grads[self.gb], self.cfg.clip_norm, blk, self.clip_partials)
            if self.is_cuda:
                self._mark(then=self.comm_stream)
            self.engine.push_scalars(self.step_idx, blk, self.comm_stream.cuda_stream if self.is_cuda else 0)
            self._last_scal = blk
        if self.is_cuda:  # the commit posts behind the push copies, on their stream
            self.engine.commit(self.step_idx, self.pulled, self.comm_stream.cuda_stream)
            self.push_done[self.gb] = self._mark(self.comm_stream)
            self.step_done[self.cb] = self._mark()
        else:
            self.engine.commit(self.step_idx, self.pulled, 0)
        self.step_idx += 1
        if self.prefetch:
            self._prefetch_pull(self.step_idx)

    def idle_step(self):
        pass

    def grad_norm(self) -> tuple:
        """``(norm, coef)`` of this worker's last finished step: the L2 norm of its whole gradient
        as pushed and the clipping coefficient the owners applied to it. For logs and tests: reads
        the device, so it synchronises; the step itself never calls it."""
        if not self.clip:
            raise RuntimeError("grad_norm() needs OptimConfig.clip_norm > 0 (the norm pass runs only then)")
        if self._last_scal is None:
            raise RuntimeError("grad_norm() before the first finished step")
        c, n = self._last_scal[:2].tolist()
        return n, c

    # ------------------------------------------------------------------ end of run / reporting
    def drain(self):
        """Block until every worker's pushes so far are applied everywhere (collective: all ranks)."""
        self.engine.wait_all_applied(self._workers_step())
        if self.is_cuda:
            torch.cuda.synchronize(self.device)

    def _workers_step(self) -> int:
        """Collective: the workers' step (the owners that are not workers learn it here)."""
        return self._all_max([self.step_idx if self.is_worker else 0], torch.int64)[0]

    def refresh_weights(self):
        """After ``drain``: the working weights (the model's parameter views) = the latest applied
        snapshot. Workers otherwise hold the weights of their last pull, one round behind."""
        if self.is_worker and self.engine is not None:
            self.pulled = self._pull_into(0, self.cb, None)
            self._to_work()
            if self.is_cuda:
                torch.cuda.synchronize(self.device)

    def _build_buckets(self, bucket_mb: float):
        """Push buckets: consecutive parameter ranges of ~``bucket_mb`` (the tail padding travels
        with the last bucket)."""
        elem = torch.finfo(self.param_dtype).bits // 8
        cap = max(ALIGN, int(bucket_mb * (1 << 20)) // elem)
        self.buckets: list[_Bucket] = []
        cur = _Bucket(0, lo=0)
        for n, p, o, k in self._layout:
            cur.params.append((n, p, o, k))
            cur.hi = o + _round(k, ALIGN)
            if cur.hi - cur.lo >= cap:
                self.buckets.append(cur)
                cur = _Bucket(len(self.buckets), lo=cur.hi)
        if cur.params:
            self.buckets.append(cur)
        self.buckets[-1].hi = self.total
        self.bucket_mb = float(bucket_mb)
        self.flat.set_buckets(self.buckets)

    def rebucket(self, bucket_mb: float):
        """Rebuild the push buckets at another size (between steps; every rank the same size)."""
        self._build_buckets(bucket_mb)

    def probe_push_sizes(self, sizes_mb=(1, 2, 4, 8, 16, 32, 64), reps: int = 3) -> dict:
        """The bandwidth of THIS plane's push transport vs bucket size, measured before training
        (collective, every rank): each worker DMA-copies its whole gradient buffer into its inbox
        slot on every owner in chunks of ``size`` MB -- one engine push per chunk on the push
        stream, exactly what a step's bucket pushes do (no commit: nothing is applied) --
        and the max over ranks of the time gives {MB: GB/s}. The RCCL send/recv probe
        (parallel/bucketing.py probe_p2p) measures the collective plane's transport, not this one."""
        out = {}
        g = self.grads[0]
        cs = self.comm_stream if self.is_cuda else None
        for mb in sizes_mb:
            n = max(ALIGN, int(mb * (1 << 20)) // g.element_size() // ALIGN * ALIGN)  # chunk ends stay 16-B aligned

            def run():
                for lo in range(0, self.total, n):
                    self.engine.push(self.step_idx, g, lo, min(lo + n, self.total),
                                     cs.cuda_stream if cs is not None else 0, self._resid_on(cs))
                if cs is not None:
                    cs.synchronize()

            el = self._time_pushes(run, reps, "push-size probe")
            out[mb] = round(self.total * self.push_bytes_per_elem * self.P / max(el, 1e-9) / 1e9, 1) if el > 0 else None
        return out

    def _time_pushes(self, run, reps: int, what: str) -> float:
        """Collective: the seconds one ``run()`` takes on a worker (once untimed, then ``reps`` timed;
        the push stream is idle before the clock starts and before it stops), maximum over the ranks.
        A failure on any rank raises on every rank instead of stranding the others in the all_reduce."""
        el, err = 0.0, None
        sync = self.comm_stream.synchronize if self.is_cuda else (lambda: None)
        if self.is_worker:
            try:
                run()
                sync()
                t0 = time.perf_counter()
                for _ in range(reps):
                    run()
                sync()
                el = (time.perf_counter() - t0) / reps
            except Exception as e:  # noqa: BLE001 -- reported collectively below
                err = e
            finally:  # the pushes ran the feedback path: leave the residual zero, also after a failure
                self.reset_push_residual()
        el, failed = self._all_max([el, 1.0 if err is not None else 0.0])
        if failed > 0:
            raise RuntimeError(f"{what} failed on a rank{f': {err}' if err is not None else ''}")
        return el

    def probe_xfer_blocks(self, caps=(8, 16, 24, 32, 48, 64, 96), reps: int = 3, keep: float = 0.9) -> dict:
        """The scatter kernel's workgroup budget (collective, every rank; before training): each
        worker pushes its whole gradient buffer into its inbox slot on every owner in one launch per
        cap, timed (max over ranks). Returns {"GBps": {cap: GB/s}, "chosen": cap}: the SMALLEST cap
        within ``keep`` of the best bandwidth -- the fewest CUs the push takes from the backward
        pass running beside it for (nearly) the same link throughput -- and sets it on the engine.
        Only meaningful where the kernel transport runs (a remote owner); otherwise returns {}."""
        remote = self.is_cuda and self.xfer_mode == "kernel" and any(o != self.rank for o in self.owners)
        if self._all_max([1.0 if remote else 0.0])[0] == 0.0 or not self.is_cuda:
            return {}
        g, st = self.grads[0], self.comm_stream
        old = self.engine.xfer_blocks_cap()
        res = {}
        for cap in caps:
            self.engine.set_xfer_blocks(int(cap))
            try:
                el = self._time_pushes(lambda: self.engine.push(self.step_idx, g, 0, self.total, st.cuda_stream,
                                                                self._resid_on(st)), reps, "xfer workgroup probe")
            except RuntimeError:
                self.engine.set_xfer_blocks(old)
                raise
            res[int(cap)] = round(self.total * self.push_bytes_per_elem / max(el, 1e-9) / 1e9, 1) if el > 0 else None
        ok = {c: v for c, v in res.items() if v}
        if not ok:  # no worker timed anything (a pure-owner world): keep the default
            self.engine.set_xfer_blocks(old)
            return {"GBps": res, "chosen": old}
        best = max(ok.values())
        chosen = min(c for c, v in ok.items() if v >= keep * best)
        self.engine.set_xfer_blocks(chosen)
        return {"GBps": res, "chosen": chosen}

    def probe_bandwidth(self, reps: int = 3) -> dict:
        """After ``drain``: time this worker's full push (DMA of the whole gradient into its inbox slot
        on every owner, no commit) and a full pull (latest snapshots into a scratch buffer) -- the
        peer-memory data plane's achieved bandwidth on this node (xGMI links at N > 1)."""
        if not (self.is_worker and self.is_cuda):
            return {}
        g = self.grads[0]
        tmp = torch.empty_like(self.params_flat)
        st = torch.cuda.current_stream(self.device)
        out = {}
        try:
            for name, fn in (("push", lambda: self.engine.push(self.step_idx, g, 0, self.total, st.cuda_stream,
                                                                self._resid_on(st))),
                             # step_idx: the latest admissible snapshot under both schedules (a fixed
                             # schedule keeps only the last S + 1 versions; step 0's is long gone)
                             ("pull", lambda: self.engine.pull(self.step_idx, tmp, st.cuda_stream))):
                fn()
                torch.cuda.synchronize(self.device)
                s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                s.record()
                for _ in range(reps):
                    fn()
                e.record()
                e.synchronize()
                ms = s.elapsed_time(e) / reps
                bpe = self.push_bytes_per_elem if name == "push" else g.element_size()
                out[f"{name}_GBps"] = round(self.total * bpe / (ms * 1e-3) / 1e9, 1)
        finally:  # the timed pushes ran the feedback path: leave the residual zero, also after a failure
            self.reset_push_residual()
        return out

    def abort(self):
        """Non-collective teardown after a failure (a dead peer would never reach close()'s
        barriers): raise the shared error so every peer's waits fail, stop the engine, unmap the
        peers' memory and free this rank's. Pushes not yet applied are lost; recovery restarts from
        a checkpoint (runtime/elastic.py)."""
        if self.closed or self.engine is None:
            return
        try:
            self.engine.inject_error(f"rank {self.rank} aborted")
        except Exception:  # noqa: BLE001
            pass
        self.engine.stop()
        hist, vers, log = self.staleness_histogram(), self.versions(), self.apply_log()
        self._final = (hist, vers, log)
        self.engine.close_peers()
        self.engine.free_local()
        self.engine = None
        self.flat.release()
        self.closed = True

    def close(self):
        """Collective: stop the engine, unmap the peers' memory, free this rank's (all ranks call).
        After a failure (the shared error is set) this is ``abort``: no barriers with dead peers."""
        if self.closed:
            return
        if self.engine.error():
            self.abort()
            return
        self.engine.stop()
        self._barrier("stop")
        self.engine.close_peers()
        self._barrier("unmapped")
        hist, vers, log = self.staleness_histogram(), self.versions(), self.apply_log()
        self._final = (hist, vers, log)
        self.engine.free_local()
        self.engine = None
        self.flat.release()
        self.closed = True

    def staleness_histogram(self):
        if self.engine is None:
            return list(self._final[0])
        return list(self.engine.histogram())

    def staleness_p50(self) -> int:
        h = self.staleness_histogram()
        tot, acc = sum(h), 0
        for i, c in enumerate(h):
            acc += c
            if tot and acc * 2 >= tot:
                return i
        return -1

    def versions(self) -> list[int]:
        if self.engine is None:
            return list(self._final[1])
        return [int(self.engine.version(k)) for k in range(self.P)]

    def apply_log(self):
        if self.engine is None:
            return list(self._final[2])
        return [tuple(x) for x in self.engine.apply_log()]

    def set_lr(self, lr: float):
        """``lr``: the synchronous (per-round) learning rate; each push runs with its async share."""
        for d in self.dyn.values():
            d.set(lr=lr * self.hyper["lr_factor"])

    def num_params(self) -> int:
        return self.flat.num_params()

    def state_dict(self) -> dict:
        """This rank's shard state (call after ``drain``)."""
        return {"master": {k: v.detach().cpu() for k, v in self.master.items()},
                "state1": {k: v.cpu() for k, v in self.state1.items()},
                "state2": {k: v.cpu() for k, v in self.state2.items()},
                "dyn": {k: d.t.cpu() for k, d in self.dyn.items()}, "versions": self.versions(),
                "step_idx": self.step_idx}

    # ------------------------------------------------------------------ checkpoint / resume
    def _shard_tensors(self, k: int) -> list:
        """Shard k's tensors in the order a checkpoint file holds them: fp32 master, step scalars, the
        optimizer states that exist."""
        return [self.master[k], self.dyn[k].t] + [d[k] for d in (self.state1, self.state2) if k in d]

    def _layout_meta(self) -> dict:
        return {"world": self.world, "owners": self.owners, "workers": self.worker_ranks, "P": self.P,
                "shard_off": self.shard_off, "shard_len": self.shard_len, "total": self.total,
                "staleness": self.S, "semantics": self.semantics, "round": self.round, "push_dtype": self.push_dtype,
                "push_error_feedback": self.push_error_feedback,
                "optimizer": self.cfg.to_dict(), "params": self.flat.param_meta()}

    def save(self, prefix: str, blocking: bool = True):
        """Sharded checkpoint (collective: every rank calls at the same step). After a drain, each
        shard owner writes ``{prefix}.rank{r}.psd`` (atomic, CRC-checked: csrc/checkpoint.cpp) with
        its fp32 masters, optimizer state and step scalars, plus the shard versions and every
        worker's SSP clock; rank 0 writes ``{prefix}.manifest.json``. With ``push_error_feedback``
        each worker's file also carries its residual as one extra tensor after the shard tensors
        (``"push_residual": true`` in its per-rank JSON; the manifest records
        ``push_error_feedback``), snapshotted after the drain, when no push is rewriting it. The device state is
        snapshotted (HBM->HBM) before any rank returns, so the engines' next applies cannot race
        the copy; with ``blocking=False`` the device->host copy and the file write run on a host
        thread while training continues. Returns that thread (or None).

        Reference: the periodic checkpoint thread (src/parameter_server_service.cpp:150-169) and
        ParameterServerCore::save_checkpoint (src/parameter_server.cpp:112-144), which kept no
        optimizer state, versions or worker iteration."""
        import json
        import threading

        self.drain()  # masters, optimizer state, versions and clocks now form one consistent cut
        C = native()
        snap = []
        meta = {"step_idx": self.step_idx if self.is_worker else None, "shards": {}}
        for k in self.my_shards:
            ts = self._shard_tensors(k)
            snap.extend(t.detach().clone() for t in ts)
            meta["shards"][str(k)] = {"version": int(self.engine.version(k)), "clocks": list(self.engine.clocks(k)),
                                      "n": len(ts)}
        # error feedback: this worker's residual, one extra tensor after the shard tensors. The drain
        # above left the comm stream idle, so no push is rewriting it.
        meta["push_residual"] = self.push_residual is not None
        if self.push_residual is not None:
            snap.append(self.push_residual.detach().clone())
        meta["step_idx"] = self._workers_step()
        if self.is_cuda:
            torch.cuda.synchronize(self.device)
        self._barrier(f"ckpt-snap-{self._ckpt_seq}")  # every owner's snapshot taken before anyone pushes
        self._ckpt_seq += 1
        man = {"format": "psd-async-v1", **self._layout_meta(), **meta, "rank": self.rank}
        man_s = json.dumps(man)
        path = f"{prefix}.rank{self.rank}.psd"

        def write():
            host = [t.cpu() for t in snap]
            C.save_native_ckpt(path, man_s, host)
            if self.rank == 0:
                m0 = {k: v for k, v in man.items() if k not in ("shards", "rank", "push_residual")}
                with open(f"{prefix}.manifest.json.tmp", "w") as f:
                    f.write(json.dumps(m0))
                os.replace(f"{prefix}.manifest.json.tmp", f"{prefix}.manifest.json")

        if blocking:
            write()
            return None
        th = threading.Thread(target=write, name="psd-async-ckpt", daemon=True)
        th.start()
        return th

    def load(self, prefix: str):
        """Resume from ``save(prefix)`` with the same layout (collective, before the first step):
        every owner restores its shards' masters, optimizer state and step scalars and re-publishes
        them as the saved shard versions with the saved SSP clocks; every worker continues at the
        saved step (its first pull waits on the restored clocks). The error-feedback residual: with
        feedback on and a residual in this rank's file it is restored; with feedback on and none in
        the file (an older checkpoint, or one saved without feedback) it starts at zero; with
        feedback off a residual in the file is ignored."""
        import json

        man, ts = native().load_native_ckpt(f"{prefix}.rank{self.rank}.psd")
        m = json.loads(man)
        mine = self._layout_meta()
        for key in ("world", "owners", "workers", "shard_off", "shard_len", "total", "round"):
            if m[key] != mine[key]:
                raise ValueError(f"checkpoint {prefix}: {key} {m[key]} does not match this run's {mine[key]}")
        if m["optimizer"]["kind"] != self.cfg.kind:
            raise ValueError(f"checkpoint optimizer {m['optimizer']['kind']} != {self.cfg.kind}")
        # the push dtype is recorded with the optimizer settings (a checkpoint from before it existed
        # was a bf16 push). A drained checkpoint holds no in-flight gradient, so resuming with the
        # other push dtype is supported: the masters, state, versions and clocks do not depend on it.
        self.resumed_push_dtype = m.get("push_dtype", "bf16")
        self.engine.stop()
        i = 0
        for k in self.my_shards:
            sh = m["shards"][str(k)]
            for dst, src in zip(self._shard_tensors(k), ts[i:]):
                dst.copy_(src)
            i += sh["n"]
            self.engine.publish_initial(k, sh["version"], sh["clocks"])
        # error feedback: restored when on and the file carries a residual; zero when the file has none
        # (an older checkpoint, or one saved without feedback); ignored when off
        if self.push_residual is not None:
            self.reset_push_residual()
            if m.get("push_residual", False):
                self.push_residual.copy_(ts[i])
        self.step_idx = int(m["step_idx"])
        self._prefetched = None
        self.engine.start()
        if self.is_cuda:
            torch.cuda.synchronize(self.device)
        self._barrier(f"ckpt-load-{self._ckpt_seq}")
        self._ckpt_seq += 1
        if self.is_worker:  # working weights = the restored snapshot (forward hooks, eval before a step);
            # with MX pulls the e4m3 copy the fp8 convolutions read (install_fp8_weights) is pulled too
            self.pulled = self._pull_into(0, self.cb, None)
            self._to_work()
            if self.is_cuda:
                torch.cuda.synchronize(self.device)

    def canonical_keys(self) -> list:
        return ["master", "state1", "state2"][: 1 + self.cfg.num_states]

    def dyn_template(self) -> torch.Tensor:
        """A tensor shaped like the step-scalar block (the receive buffer of a broadcast)."""
        return torch.zeros(8, dtype=torch.int32, device=self.device)

    def canonical_state(self, root: int) -> dict | None:
        """Collective: drain, then gather every shard's fp32 master + optimizer state onto rank
        ``root`` in the layout-independent canonical order (owners hold disjoint ranges: a sum
        reduce is the gather). Returns the tensors on ``root``, None elsewhere."""
        self.drain()
        out = {}
        for key in self.canonical_keys():
            full = torch.zeros(self.total, dtype=torch.float32, device=self.device)
            for k, t in getattr(self, key).items():
                full.narrow(0, self.shard_off[k], self.shard_len[k]).copy_(t)
            if self.world > 1 and dist.is_initialized():
                dist.reduce(full, root)
            if self.rank == root:
                out[key] = self.flat.to_canonical(full)
        # step scalars: every shard advanced in lock-step (one apply per round), take shard 0's
        d = self.dyn[0].t.detach().clone() if 0 in self.dyn else torch.zeros(8, dtype=torch.int32, device=self.device)
        if self.world > 1 and dist.is_initialized():
            if self.owners[0] != root:
                if self.rank == self.owners[0]:
                    dist.send(d, root)
                elif self.rank == root:
                    dist.recv(d, self.owners[0])
        if self.rank != root:
            return None
        out["dyn"] = d
        return out

    def load_canonical_state(self, sd: dict):
        """Inverse of ``canonical_state`` for this (possibly different) world and shard layout:
        every rank passes the full canonical tensors; owners keep their ranges and re-publish them
        (version 0 of this plane), workers take the weights."""
        full = {key: self.flat.from_canonical(sd[key].to(self.device), key)
                for key in ("master", "state1", "state2") if key in sd}
        self.engine.stop()
        for k in self.my_shards:
            for key, dst in (("master", self.master), ("state1", self.state1), ("state2", self.state2)):
                if key in full and k in dst:
                    dst[k].copy_(full[key].narrow(0, self.shard_off[k], self.shard_len[k]))
            if "dyn" in sd:
                self.dyn[k].t.copy_(sd["dyn"].to(self.dyn[k].t.device))
                # lr / grad scale of THIS plane's semantics and worker count
                self.dyn[k].set(lr=self.cfg.lr * self.hyper["lr_factor"], grad_scale=self.hyper["grad_scale"])
            self.engine.publish_initial(k)
        self.engine.start()
        self.params_flat.copy_(full["master"].to(self.param_dtype))
        for b in self.pbufs:
            if b is not self.pwork:
                b.copy_(self.params_flat)
        for q, sc, b in zip(self.q8s, self.sc8s, self.pbufs):
            # MX pulls: the e4m3 weights the fp8 convolutions read, and the working bf16 copy as a
            # pull would leave it (dequantised)
            native().quant_mx_(full["master"], q, sc)
            native().dequant_mx_(q, sc, b)
        self._to_work()
        self.step_idx = 0
        self._prefetched = None
        # the canonical state carries no residual (it belongs to a worker of the old layout): error
        # feedback restarts at zero, at most one step's quantisation error is lost
        self.reset_push_residual()
        if self.is_cuda:
            torch.cuda.synchronize(self.device)
        self._barrier(f"canon-load-{self._ckpt_seq}")
        self._ckpt_seq += 1

    def export_reference(self, path: str, epoch: int, iteration: int = 0):
        """The reference's binary checkpoint layout (src/parameter_server.cpp:112-144: fp32 params by
        name) on rank 0, from the drained fp32 masters (collective)."""
        sd = self.canonical_state(root=0)
        if self.rank != 0:
            return
        names, shapes, vals = [], [], []
        idx, _ = self.flat.canon_index()
        params = [(n, p) for n, p in self.model.named_parameters() if p.requires_grad]
        for (n, p), (_o, c, k) in zip(params, idx):
            names.append(n)
            shapes.append(list(p.shape))
            vals.append(sd["master"].narrow(0, c, k).view(p.shape).cpu())
        native().save_reference_ckpt(path, epoch, iteration, names, shapes, vals)

    def describe(self) -> str:
        return (f"AsyncPS(world={self.world}, shards={self.P} on ranks {self.owners}, workers={self.worker_ranks}, "
                f"SSP bound={self.S}, buckets={len(self.buckets)}, params={self.num_params() / 1e6:.2f}M, "
                f"memory={self.engine.memory_kind()}, xfer={self.xfer_mode}"
                f"{', push=fp8' if self.push_mx else ''}{' + error feedback' if self.push_error_feedback else ''})")
