"""LARS / LAMB through the planes that apply updates: the async peer-memory engine (layer table per
shard, shard boundaries on tensor starts) and the gRPC-path PSCore.

Accuracy rule as tests/test_optim_layerwise.py: per tensor, the error against an fp64 replay of the
update on the logged gradients is at most 4x the error of the fp32-eager replay, floor two fp32 ulps
of max |w|.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from test_async_ps import _port
from test_optim_layerwise import CFGS, EPS32, _ref_step

from parameter_server_distributed_amd import models
from parameter_server_distributed_amd.ops.optim import OptimConfig
from parameter_server_distributed_amd.parallel.async_ps import AsyncPS, snap_bounds

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
# the MLP's weights are ~0.03 and its gradients ~1e-3: a trust coefficient / lr that move them visibly
ASYNC_CFGS = {"lars": dict(CFGS["lars"], lr=0.5), "lamb": dict(CFGS["lamb"], lr=2e-3)}


def _replay(cfg, lay, w0, grads, dt):
    """The update of section 2 in ``dt`` on the logged gradient rounds (each a list of K sources)."""
    n = w0.numel()
    w, s1, s2 = w0.to(dt, copy=True), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
    for step, srcs in enumerate(grads, 1):
        _ref_step(cfg, lay, w, srcs, s1, s2, step, dt)
    return w, s1, s2


def _check(lay, w0, got, ref, eag, what):
    bad = []
    for name, o, k, _d, _w in lay:
        sl = slice(o, o + k)
        floor = 2 * EPS32 * float(torch.maximum(ref[sl].abs().max(), w0[sl].double().abs().max()))
        ek = float((got[sl].double() - ref[sl]).abs().max())
        ee = float((eag[sl].double() - ref[sl]).abs().max())
        line = f"{what} {name}: kernel {ek:.3e} eager {ee:.3e} bound {max(4 * ee, floor):.3e}"
        print("LWERR async", line)
        if ek > max(4 * ee, floor):
            bad.append(line)
    assert not bad, "error above 4x the fp32-eager error (and the 2-ulp floor):\n" + "\n".join(bad)


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_async_world1_matches_replay(devname, kind):
    """World 1, SSP bound 0, 5 steps of the MLP: the master and the published weights equal the replay
    of the logged gradients through the per-tensor update."""
    if devname == "cuda" and not torch.cuda.is_available():
        pytest.fail("GPU test selected but no GPU visible")
    dev = torch.device("cuda", 0) if devname == "cuda" else torch.device("cpu")
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    torch.manual_seed(0)
    spec = models.build("mlp", dev, dt, hidden=64)
    cfg = OptimConfig(**ASYNC_CFGS[kind])
    ps = AsyncPS(spec.model, cfg, staleness=0, bucket_mb=0.0005, param_dtype=dt, device=dev, timeout_s=60)
    try:
        lay = [(n, o, k, p.dim(), "") for (n, p, o, k) in ps._layout]
        assert ps.layers[0].num_segments == len(lay)
        w0 = ps.master[0].cpu().clone()
        x, y = spec.make_batch(16, dev, seed=0)
        grads = []
        for _ in range(5):
            ps.begin_step()
            spec.loss(spec.model(x), y).backward()
            ps.finish_step()
            if dev.type == "cuda":
                torch.cuda.synchronize()
            grads.append([ps.grads[(ps.step_idx - 1) % 2].cpu().clone()])
        ps.drain()
        ps.refresh_weights()
        master, published = ps.master[0].cpu(), ps.params_flat.float().cpu()
        assert ps.versions() == [5]
    finally:
        ps.close()
    ref = _replay(cfg, lay, w0, grads, torch.float64)
    eag = _replay(cfg, lay, w0, grads, torch.float32)
    assert not torch.equal(master, w0)
    _check(lay, w0, master, ref[0], eag[0], f"{kind} master")
    _check(lay, w0, published, ref[0], eag[0].to(dt).float(), f"{kind} published")


def _lw_worker(rank, world, port, kind, shards, steps, out_dir, tag, device, mode):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    spec = models.build("mlp", dev, dt, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**ASYNC_CFGS[kind]), num_shards=shards, staleness=0, bucket_mb=0.0005,
                 param_dtype=dt, device=dev, schedule="fixed", timeout_s=60)
    prefix = os.path.join(out_dir, "ck")
    if mode == "resume":
        ps.load(prefix)
        assert ps.step_idx == steps
    else:
        x, y = spec.make_batch(16, dev, seed=rank)
        for _ in range(steps):
            ps.begin_step()
            spec.loss(spec.model(x), y).backward()
            ps.finish_step()
        ps.drain()
        if mode == "save":
            ps.save(prefix)
    torch.save({"master": {k: v.cpu().clone() for k, v in ps.master.items()},
                "state1": {k: v.cpu().clone() for k, v in ps.state1.items()},
                "shard_off": ps.shard_off, "shard_len": ps.shard_len, "total": ps.total,
                "starts": [o for (_n, _p, o, _k) in ps._layout], "mem": ps.engine.memory_kind(),
                "versions": ps.versions()},
               os.path.join(out_dir, f"{tag}{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


def _gather(out_dir, tag, world):
    """The full flat master / state1 assembled from every rank's shards, and rank 0's record."""
    R = [torch.load(os.path.join(out_dir, f"{tag}{r}.pt"), weights_only=False) for r in range(world)]
    full = {key: torch.full((R[0]["total"],), float("nan")) for key in ("master", "state1")}
    for r in R:
        for key in full:
            for k, v in r[key].items():
                full[key][r["shard_off"][k]:r["shard_off"][k] + r["shard_len"][k]] = v
    assert all(torch.isfinite(v).all() for v in full.values())
    return full, R[0]


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_async_world2_shards_on_tensor_starts_and_match_one_shard_bitwise(tmp_path, kind):
    out = str(tmp_path)
    mp.spawn(_lw_worker, args=(2, _port(), kind, 2, 4, out, "p2_", "cpu", "save"), nprocs=2, join=True)
    mp.spawn(_lw_worker, args=(2, _port(), kind, 1, 4, out, "p1_", "cpu", "run"), nprocs=2, join=True)
    two, r2 = _gather(out, "p2_", 2)
    one, r1 = _gather(out, "p1_", 2)
    assert len(r2["shard_off"]) == 2 and all(o in r2["starts"] for o in r2["shard_off"]), r2["shard_off"]
    assert r2["versions"] == [4, 4] and r1["versions"] == [4]
    for key in two:
        assert torch.equal(two[key], one[key]), key
    # a checkpoint written with the snapped boundaries restores ...
    mp.spawn(_lw_worker, args=(2, _port(), kind, 2, 4, out, "res_", "cpu", "resume"), nprocs=2, join=True)
    res, rr = _gather(out, "res_", 2)
    assert rr["versions"] == [4, 4]
    for key in two:
        assert torch.equal(two[key], res[key]), key
    # ... and another shard layout is still rejected
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**ASYNC_CFGS[kind]), staleness=0, bucket_mb=0.0005,
                 param_dtype=torch.float32)
    try:
        with pytest.raises((ValueError, RuntimeError)):
            ps.load(os.path.join(out, "ck"))
    finally:
        ps.close()


@pytest.mark.gpu
@pytest.mark.slow
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_async_gpu_ipc_two_shards_match_one_shard_bitwise(tmp_path, gpu, kind):
    """Two ranks on one MI355X (inbox / publish buffers mapped across processes): norm pass, finalize
    and apply on each owner's engine stream; P = 2 (cut on a tensor start) equals P = 1 bit for bit."""
    out = str(tmp_path)
    mp.spawn(_lw_worker, args=(2, _port(), kind, 2, 4, out, "p2_", "cuda:0", "run"), nprocs=2, join=True)
    mp.spawn(_lw_worker, args=(2, _port(), kind, 1, 4, out, "p1_", "cuda:0", "run"), nprocs=2, join=True)
    two, r2 = _gather(out, "p2_", 2)
    one, _ = _gather(out, "p1_", 2)
    assert r2["mem"] in ("uncached", "finegrained"), r2["mem"]
    assert all(o in r2["starts"] for o in r2["shard_off"])
    for key in two:
        assert torch.equal(two[key], one[key]), key


def test_snap_bounds():
    starts = [0, 64, 704, 768]
    assert snap_bounds(50944, 2, starts) == [0, 768, 50944]
    assert snap_bounds(50944, 4, starts) == [0, 64, 704, 768, 50944]  # strictly increasing, one start per cut
    assert snap_bounds(1024, 3, [0, 64, 512, 576, 960]) == [0, 512, 576, 1024]
    assert snap_bounds(1024, 3, [0, 832, 896, 960]) == [0, 832, 896, 1024]  # a cut leaves starts for the later ones
    with pytest.raises(ValueError, match="tensors"):
        snap_bounds(50944, 5, starts)


def test_pscore_sync_lars_matches_reference(C):
    """PSCore on CPU: two workers in sync mode with lars; after 3 iterations the pulled parameters
    match the fp64 reference under the same rule. Async mode with a layer-wise kind is rejected."""
    from parameter_server_distributed_amd.runtime.parameter_server import make_config

    cfg = OptimConfig(**CFGS["lars"])
    core = C.PSCore(make_config(2, cfg, "sync"), "cpu")
    gen = torch.Generator().manual_seed(7)
    shapes = [[40, 30], [30], [9000], [3, 5, 7]]
    names = [f"t{i}" for i in range(len(shapes))]
    vals = [(torch.rand(s, generator=gen) + 0.5) for s in shapes]
    core.init_params(names, shapes, vals)
    offs, n = core.offsets(), core.numel()
    lay = [(nm, o, v.numel(), v.dim(), "") for nm, o, v in zip(names, offs, vals)]
    w0 = torch.zeros(n)
    for (_nm, o, k, _d, _w), v in zip(lay, vals):
        w0[o:o + k] = v.flatten()
    rounds = []
    for it in range(3):
        srcs = []
        for wid in range(2):
            gs = [torch.randn(s, generator=gen) * 0.05 for s in shapes]
            r = core.push(wid, it, names, gs, -1)
            assert r.success, r.message
            flat = torch.zeros(n)
            for (_nm, o, k, _d, _w), g in zip(lay, gs):
                flat[o:o + k] = g.flatten()
            srcs.append(flat)
        assert r.aggregation_complete
        rounds.append(srcs)
    ready, _it, version, got = core.pull(0, 2, 1.0)
    assert ready and version == 3
    ref = _replay(cfg, lay, w0, rounds, torch.float64)
    eag = _replay(cfg, lay, w0, rounds, torch.float32)
    _check(lay, w0, got, ref[0], eag[0], "pscore lars")
    with pytest.raises(RuntimeError, match="async"):
        C.PSCore(make_config(2, cfg, "async"), "cpu")
