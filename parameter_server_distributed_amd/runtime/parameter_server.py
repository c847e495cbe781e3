"""Parameter-server role: the five reference RPCs (+ additive ones) over the native ``PSCore``.

Reference parity:
  parameter_server_service_impl (src/parameter_server_service.cpp:15-175) -> ParameterServerService
    ReceiveGradients :32-59, ServeParameters :61-83, CheckSyncStatus :85-95,
    SaveCheckpoint :97-115 (default path ``checkpoint_epoch_<e>.ckpt``), LoadCheckpoint :117-143
  periodic_checkpoint (:150-169: every 5 s, save when iteration / interval advanced) -> ``_ckpt_loop``
  run_server (:177-191) -> ``serve``
The shard table / barrier / optimizer live in C++ (csrc/ps_core.cpp) and, with ``device="cuda"``,
in HBM with the gfx950 fused-apply kernel.

Fixed defects: D3 (the barrier follows live membership when ``coordinator`` is given -- the PS
polls ListWorkers), D4 (bounded iteration window), D7 (no unlocked shared state), D8 (load clears
iteration states), D9 (late pushes are reported), D10 (layout mismatches are rejected loudly),
D11 (LoadCheckpoint returns the iteration so workers resume from it), D12 (bulk payloads).
"""
from __future__ import annotations

import json
import os
import threading

import torch

from .. import native
from ..ops.optim import OptimConfig
from ..rpc import schema, service
from ..utils.log import get_logger

pb = schema.parameter_server
log = get_logger("parameter_server")


def make_config(total_workers: int, optim: OptimConfig, mode: str = "sync", staleness: int = -1,
                reference_compat: bool = False, staleness_lr_scaling: bool = False, window: int = 64):
    C = native()
    cfg = C.PSConfig()
    cfg.total_workers = int(total_workers)
    cfg.async_mode = 1 if mode == "async" else 0
    cfg.staleness_bound = int(staleness)
    cfg.window = int(window)
    cfg.reference_compat = bool(reference_compat)
    if reference_compat:  # p -= g: SGD with lr 1 (src/parameter_server.cpp:87)
        optim = OptimConfig("sgd", lr=1.0, momentum=0.0)
    cfg.opt_kind = optim.code
    cfg.lr = optim.lr
    cfg.momentum, cfg.dampening, cfg.nesterov = optim.momentum, optim.dampening, optim.nesterov
    cfg.weight_decay = optim.weight_decay
    cfg.trust_coef = optim.trust_coef
    cfg.exclude_1d = int(optim.exclude_1d)
    cfg.beta1, cfg.beta2, cfg.eps = optim.beta1, optim.beta2, optim.eps
    cfg.staleness_lr_scaling = bool(staleness_lr_scaling)
    return cfg


class ParameterServerService:
    def __init__(self, total_workers: int = 2, checkpoint_interval: int = 10, device: str = "cpu",
                 optim: OptimConfig | None = None, mode: str = "sync", staleness: int = -1,
                 reference_compat: bool = False, ckpt_dir: str = ".", coordinator: str | None = None,
                 ckpt_poll_s: float = 5.0, membership_poll_s: float = 1.0, staleness_lr_scaling: bool = False):
        C = native()
        self.optim = optim or OptimConfig("sgd", lr=0.1, momentum=0.0)
        self.cfg = make_config(total_workers, self.optim, mode, staleness, reference_compat, staleness_lr_scaling)
        self.core = C.PSCore(self.cfg, device)
        self.mode = mode
        self.interval = int(checkpoint_interval)
        self.ckpt_dir = ckpt_dir
        self._stop = threading.Event()
        self._threads = []
        self._last_epoch = 0
        if self.interval > 0:
            self._spawn(self._ckpt_loop, ckpt_poll_s, name="ps-ckpt")
        self.coordinator = coordinator
        self._known_live: set[int] = set()
        self._formed = False  # barrier follows membership only once the initial cohort has joined
        if coordinator:
            self._coord = service.Stub(coordinator, schema.coordinator, timeout=5.0)
            self._spawn(self._membership_loop, membership_poll_s, name="ps-membership")

    def _spawn(self, fn, *a, name):
        t = threading.Thread(target=fn, args=a, name=name, daemon=True)
        t.start()
        self._threads.append(t)

    # ------------------------------------------------------------------ helpers
    def _split(self, flat: torch.Tensor):
        names, shapes, offs = self.core.names(), self.core.shapes(), self.core.offsets()
        out = []
        for n, s, o in zip(names, shapes, offs):
            k = 1
            for d in s:
                k *= d
            out.append((n, flat.narrow(0, o, k).reshape(s)))
        return out

    @staticmethod
    def _decode(msgs):
        names, tensors = [], []
        for n, t in service.protos_to_tensors(msgs):
            names.append(n)
            tensors.append(t)
        return names, tensors

    # ------------------------------------------------------------------ reference RPCs
    def ReceiveGradients(self, req, ctx):
        names, tensors = self._decode(req.gradients)
        r = self.core.push(req.worker_id, req.iteration, names, tensors, req.pulled_version or -1)
        if not r.success:
            log.warning("push from worker %d iter %d rejected: %s", req.worker_id, req.iteration, r.message)
        return pb.PushResponse(success=r.success, message=r.message, iteration=r.iteration,
                               aggregation_complete=r.aggregation_complete, workers_received=r.workers_received,
                               total_workers=r.total_workers, version=r.version, staleness=r.staleness)

    def ServeParameters(self, req, ctx):
        ready, it, ver, flat = self.core.pull(req.worker_id, req.iteration, max(req.wait_ms, 0) / 1000.0)
        out = pb.ParameterUpdate(iteration=it, ready=ready, version=ver)
        if flat is not None and flat.numel() > 0 and self.core.initialized():
            out.parameters.extend(service.tensors_to_protos(self._split(flat), raw=req.accept_raw))
        return out

    def CheckSyncStatus(self, req, ctx):
        ready, recv, total = self.core.sync_status(req.iteration)
        return pb.SyncStatusResponse(iteration=req.iteration, ready=ready, workers_received=recv, total_workers=total)

    def SaveCheckpoint(self, req, ctx):
        path = req.path or os.path.join(self.ckpt_dir, f"checkpoint_epoch_{req.epoch}.ckpt")
        ok = self.core.save_reference(path, req.epoch)
        if ok:
            self._save_native_sidecar(path)
        return pb.SaveCheckpointResponse(success=ok, message="saved" if ok else "parameters not initialised",
                                         checkpoint_path=path)

    def LoadCheckpoint(self, req, ctx):
        try:
            ok, epoch = self.core.load_reference(req.path)
        except Exception as e:  # noqa: BLE001 - report to the client like the reference's success=false
            return pb.LoadCheckpointResponse(success=False, message=str(e))
        self._load_native_sidecar(req.path)
        out = pb.LoadCheckpointResponse(success=ok, message="loaded", epoch=epoch,
                                        iteration=self.core.current_iteration())
        _, _, _, flat = self.core.pull(-1, 0, 0.0)
        out.parameters.extend(service.tensors_to_protos(self._split(flat), raw=req.accept_raw))
        log.info("loaded %s (epoch %d, iteration %d)", req.path, epoch, self.core.current_iteration())
        return out

    # ------------------------------------------------------------------ additive RPCs
    def InitParameters(self, req, ctx):
        if self.core.initialized():
            return pb.PushResponse(success=False, message="already initialised", version=self.core.version(),
                                   total_workers=self.core.total_workers())
        names, tensors = self._decode(req.gradients)
        shapes = [list(t.shape) for t in tensors]
        self.core.init_params(names, shapes, tensors)
        log.info("initialised %d tensors (%d elements) from worker %d", len(names), self.core.numel(), req.worker_id)
        return pb.PushResponse(success=True, message="initialised", total_workers=self.core.total_workers())

    def GetStats(self, req, ctx):
        return pb.StatsResponse(version=self.core.version(), current_iteration=self.core.current_iteration(),
                                total_workers=self.core.total_workers(),
                                staleness_histogram=list(self.core.staleness_histogram()),
                                counters_json=json.dumps(dict(self.core.counters())))

    def SetTotalWorkers(self, req, ctx):
        self.core.set_total_workers(req.total_workers)
        log.info("total_workers -> %d", req.total_workers)
        return pb.PushResponse(success=True, total_workers=req.total_workers)

    # ------------------------------------------------------------------ threads
    def _ckpt_loop(self, poll_s: float):
        while not self._stop.wait(poll_s):
            it = self.core.current_iteration()
            epoch = it // self.interval
            if epoch > self._last_epoch and it > 0 and self.core.initialized():
                path = os.path.join(self.ckpt_dir, f"checkpoint_epoch_{epoch}.ckpt")
                if self.core.save_reference(path, epoch):
                    self._save_native_sidecar(path)
                    self._last_epoch = epoch
                    log.info("periodic checkpoint %s (iteration %d)", path, it)

    def _membership_loop(self, poll_s: float):
        req = schema.coordinator.ListWorkersRequest()
        while not self._stop.wait(poll_s):
            try:
                r = self._coord.ListWorkers(req, timeout=2.0, wait_for_ready=False)
            except Exception:  # noqa: BLE001 - coordinator briefly unavailable
                continue
            live = {w.worker_id for w in r.workers}
            if not live:
                continue
            for gone in self._known_live - live:
                self.core.forget_worker(gone)
            self._known_live = live
            if not self._formed:
                # startup: keep argv's total_workers until that many have registered, so early
                # workers do not race ahead with a smaller barrier
                if len(live) < self.core.total_workers():
                    continue
                self._formed = True
            if len(live) != self.core.total_workers():
                log.info("membership epoch %d: %d live workers -> barrier size", r.membership_epoch, len(live))
                self.core.set_total_workers(len(live))

    # optimizer state next to the reference-format file (which holds fp32 params only)
    def _save_native_sidecar(self, path: str):
        try:
            st = self.core.state_tensors()
            man = json.dumps({"iteration": self.core.current_iteration(), "version": self.core.version(),
                              "optimizer": self.optim.to_dict(), "names": self.core.names(),
                              "shapes": self.core.shapes(), "offsets": self.core.offsets()})
            native().save_native_ckpt(path + ".state", man, st)
        except Exception as e:  # noqa: BLE001
            log.warning("state sidecar not written: %s", e)

    def _load_native_sidecar(self, path: str):
        side = path + ".state"
        if not os.path.exists(side):
            return
        man, ts = native().load_native_ckpt(side)
        m = json.loads(man)
        if m.get("names") == self.core.names():
            self.core.load_state_tensors(ts, int(m["iteration"]), int(m["version"]))

    def resume_latest(self) -> str | None:
        """Load the newest ``checkpoint_epoch_<N>.ckpt`` (+ its optimizer-state sidecar) found in
        ``ckpt_dir`` -- a supervised restart (scripts/supervise.sh) comes back with its parameters,
        where the reference's restart lost them (scripts/scale_workers.sh:137-144)."""
        import re

        best, path = -1, None
        for f in os.listdir(self.ckpt_dir) if os.path.isdir(self.ckpt_dir) else []:
            m = re.fullmatch(r"checkpoint_epoch_(\d+)\.ckpt", f)
            if m and int(m.group(1)) > best:
                best, path = int(m.group(1)), os.path.join(self.ckpt_dir, f)
        if path is None:
            log.info("resume: no checkpoint in %s, starting fresh", self.ckpt_dir)
            return None
        ok, epoch = self.core.load_reference(path)
        self._load_native_sidecar(path)
        self._last_epoch = epoch
        log.info("resumed from %s (epoch %d, iteration %d)", path, epoch, self.core.current_iteration())
        return path

    def stop(self):
        self._stop.set()


def serve(listen: str, total_workers: int = 2, checkpoint_interval: int = 10, block: bool = True,
          resume_latest: bool = False, **kw):
    svc = ParameterServerService(total_workers, checkpoint_interval, **kw)
    if resume_latest:
        svc.resume_latest()
    server = service.make_server(max_workers=max(32, 4 * total_workers + 8))
    service.add_service(server, pb, svc)
    bound = server.add_insecure_port(listen)
    if bound == 0:
        raise RuntimeError(f"parameter_server: cannot bind {listen}")
    server.start()
    log.info("parameter server listening on %s (port %d): %d workers, %s mode, checkpoint every %d iterations",
             listen, bound, total_workers, svc.mode, checkpoint_interval)
    if block:
        try:
            server.wait_for_termination()
        finally:
            svc.stop()
    return server, svc, bound
