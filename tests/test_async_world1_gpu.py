"""World 1, SSP bound >= 1, on the GPU: the configuration the headline async benchmark runs.

Three paths are on by default there and nowhere else (utils/config.py FEATURES):

  async_cached_local      inbox / publish buffers in plain cached device memory (world > 1: uncached IPC)
  async_direct_pull       every step pulls straight into the working weights on the compute stream
  async_apply_background  the owner's apply on a normal-priority stream, at most 512 workgroups

The model is a handful of raw parameters whose one shard exceeds 512 * 256 * 8 = 1,048,576 elements,
so the 512-workgroup cap really shortens the launch and the kernels stride (the MLP of the other
async tests is three orders of magnitude below that). Each run is one fresh child process (gloo
group of 1, cuda:0); the parent only reads the records.

  (a) free schedule, S = 1, 2: the replay of tests/test_async_ps.py (final master, every pulled
      weight, every staleness, the SSP bound) and the engine's own report of what it uses;
  (b) fixed schedule, S = 1: the run is a deterministic delayed-gradient SGD, so all three features
      on, all off and each singly off are bit-equal in master, state and every step's weights,
      gradient and pulled version -- memory kind, pull route and grid size change no arithmetic;
  (c) the other kernels under the cap, features on: MX e4m3 push, MX e4m3 publish / pull, the scaled
      (clipping) apply and LAMB's per-tensor kernels, each through the replay that models it.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn as nn
from test_async_ps import CFGS, _port, _replay_and_check

from parameter_server_distributed_amd.ops.optim import OptimConfig
from parameter_server_distributed_amd.parallel.async_ps import AsyncPS

CAP_BINDS = 512 * 256 * 8
STEPS = 6
CLIP = 100.0  # the gradient norms of this model are ~1e3 (1.1 M elements of magnitude ~1)
FEATS = ("async_cached_local", "async_direct_pull", "async_apply_background")
ALL_OFF = ",".join(f"{f}=0" for f in FEATS)
SHAPES = [(1049, 1051), (1000,), (77,), (5,)]  # 1,102,499 + odd 1-D sizes; reverse order in the flat buffer


class RawParams(nn.Module):
    """Raw parameters, no GEMM (nothing autotunes): loss_t = sum sin(p * x_t), so the gradient
    x_t * cos(p * x_t) depends on the weights, differs per step and is bounded by |x_t| <= 1.5."""

    def __init__(self, dev, dt):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.ps = nn.ParameterList([nn.Parameter((torch.randn(s, generator=g) * 0.5).to(dt).to(dev)) for s in SHAPES])

    def inputs(self, t, dev, dt):
        g = torch.Generator().manual_seed(1000 + t)
        return [((torch.rand(s, generator=g) + 0.5) * (torch.randint(0, 2, s, generator=g) * 2 - 1)).to(dt).to(dev)
                for s in SHAPES]

    def loss(self, xs):
        return sum((p * x).sin().sum() for p, x in zip(self.ps, xs))


def _lamb_cfg():
    from test_async_layerwise import ASYNC_CFGS

    return ASYNC_CFGS["lamb"]


def _worker(rank, port, out_dir, features, stale, schedule, kind, clip, push, pull, device="cuda:0"):
    if features:
        os.environ["PSD_FEATURES"] = features
    else:
        os.environ.pop("PSD_FEATURES", None)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=1)
    dev, dt = torch.device(device), torch.bfloat16
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    model = RawParams(dev, dt)
    cfg = _lamb_cfg() if kind == "lamb" else CFGS[kind]
    ps = AsyncPS(model, OptimConfig(**cfg, clip_norm=clip), num_shards=1, staleness=stale, bucket_mb=0.001,
                 param_dtype=dt, log=True, device=dev, schedule=schedule, push_dtype=push, pull_dtype=pull,
                 timeout_s=60)
    assert ps.shard_len[0] > CAP_BINDS, ps.shard_len  # else the cap does not bind and the run proves nothing
    init_master = {k: v.cpu().clone() for k, v in ps.master.items()}
    rec = []
    for t in range(STEPS):
        xs = model.inputs(t, dev, dt)
        ps.begin_step()
        clocks = [min(ps.engine.clocks(k)) for k in range(ps.P)]
        model.loss(xs).backward()
        ps.finish_step()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        g = ps.grads[(ps.step_idx - 1) % 2].float().cpu().clone()
        n, c = ps.grad_norm() if clip > 0 else (float("nan"), 1.0)
        rec.append({"step": t, "pulled": list(ps.pulled), "clock_min": clocks, "grad": g, "norm": n, "coef": c,
                    "weights": ps.params_flat.float().cpu().clone()})
    ps.drain()
    out = {"rank": rank, "rec": rec, "log": ps.apply_log(), "init": init_master,
           "master": {k: v.cpu() for k, v in ps.master.items()},
           "state1": {k: v.cpu() for k, v in ps.state1.items()}, "state2": {k: v.cpu() for k, v in ps.state2.items()},
           "mem": ps.engine.memory_kind(), "prefetch": ps.prefetch, "apply_grid_cap": ps.engine.apply_grid_cap(),
           "apply_background": ps.engine.apply_background(), "hist": ps.staleness_histogram(),
           "versions": ps.versions(), "shard_off": ps.shard_off, "shard_len": ps.shard_len,
           "workers": ps.worker_ranks, "owners": ps.owners, "xfer": ps.xfer_mode, "xfer_fallback": ps.xfer_fallback,
           "layout": [(o, k, p.dim()) for (_n, p, o, k) in ps._layout]}
    if schedule == "free":  # the latest snapshot, as a worker sees it (a fixed schedule has dropped version 0's slot)
        ps.refresh_weights()
        out["final_weights"] = ps.params_flat.float().cpu().clone()
    torch.save(out, os.path.join(out_dir, "r0.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


def _run(out_dir, features="", stale=1, schedule="free", kind="momentum", clip=0.0, push="bf16", pull="bf16",
         device="cuda:0"):
    mp.spawn(_worker, args=(_port(), str(out_dir), features, stale, schedule, kind, clip, push, pull, device),
             nprocs=1, join=True)
    return torch.load(os.path.join(str(out_dir), "r0.pt"), weights_only=False)


def _assert_fast_paths(r):
    assert r["mem"] == "device", r["mem"]
    assert r["prefetch"] is False
    assert r["apply_grid_cap"] == 512
    assert r["apply_background"] is True
    assert r["shard_len"][0] > CAP_BINDS
    assert not torch.equal(r["master"][0], r["init"][0]), "the run must move the master"
    assert r["versions"] == [STEPS]


# ------------------------------------------------------------------ (a) free schedule, replay
@pytest.mark.gpu
@pytest.mark.parametrize("stale", [1, 2])
def test_world1_defaults_match_replay(tmp_path, gpu, stale):
    r = _run(tmp_path, stale=stale)
    _assert_fast_paths(r)
    hist = _replay_and_check(str(tmp_path), 1, stale, bf16=True)
    assert sum(hist) == STEPS and hist == r["hist"], (hist, r["hist"])


# ------------------------------------------------------------------ (b) fixed schedule, bitwise
VARIANTS = {"all_on": "", "all_off": ALL_OFF, **{f"{f}_off": f"{f}=0" for f in FEATS}}


@pytest.fixture(scope="module")
def fixed_runs(tmp_path_factory):
    """name -> (record, directory) of the fixed-schedule S = 1 run with that feature set; each runs once."""
    done = {}

    def get(name):
        if name not in done:
            d = tmp_path_factory.mktemp(f"fixed_{name}")
            done[name] = (_run(d, features=VARIANTS[name], stale=1, schedule="fixed"), str(d))
        return done[name]

    return get


@pytest.mark.gpu
def test_world1_fixed_schedule_defaults_match_replay(gpu, fixed_runs):
    r, d = fixed_runs("all_on")
    _assert_fast_paths(r)
    _replay_and_check(d, 1, 1, bf16=True)
    # the stale path really ran: every gradient but the first was computed one version behind
    assert [e["pulled"] for e in r["rec"]] == [[max(t - 1, 0)] for t in range(STEPS)]
    assert r["hist"][:2] == [1, STEPS - 1] and sum(r["hist"]) == STEPS, r["hist"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", [v for v in VARIANTS if v != "all_on"])
def test_world1_fixed_schedule_features_change_no_bit(gpu, fixed_runs, name):
    on, _ = fixed_runs("all_on")
    off, _ = fixed_runs(name)
    if name == "all_off":
        assert off["mem"] in ("uncached", "finegrained"), off["mem"]
        assert off["prefetch"] is True
        assert off["apply_grid_cap"] == 0 and off["apply_background"] is False
    else:  # exactly the one feature is off
        assert (off["mem"] == "device") == (name != "async_cached_local_off"), off["mem"]
        assert off["prefetch"] is (name == "async_direct_pull_off")
        assert off["apply_grid_cap"] == (0 if name == "async_apply_background_off" else 512)
    assert off["shard_len"] == on["shard_len"] and off["shard_len"][0] > CAP_BINDS
    assert off["log"] == on["log"] and off["hist"] == on["hist"]
    assert [e["pulled"] for e in off["rec"]] == [[max(t - 1, 0)] for t in range(STEPS)]
    assert off["hist"][:2] == [1, STEPS - 1] and sum(off["hist"]) == STEPS, off["hist"]
    for key in ("master", "state1", "state2"):
        assert on[key].keys() == off[key].keys()
        for k in on[key]:
            assert torch.equal(on[key][k].view(torch.int32), off[key][k].view(torch.int32)), (name, key)
    assert 0 in on["state1"]  # momentum: there is a state to compare
    for ea, eb in zip(on["rec"], off["rec"]):
        for key in ("weights", "grad"):  # fp32 copies of bf16 buffers: equal values are equal bits, NaN aside
            assert torch.equal(ea[key].view(torch.int32), eb[key].view(torch.int32)), (name, ea["step"], key)


# ------------------------------------------------------------------ (c) the other kernels under the cap
@pytest.mark.gpu
def test_world1_fp8_push_under_the_cap_matches_replay(tmp_path, gpu):
    """The MX-source instantiation of the flat apply under the cap: replayed with every gradient
    replaced by its MX round trip (tests/test_push_fp8.py)."""
    import test_push_fp8 as F

    assert F.CFGS["momentum"] == CFGS["momentum"]
    r = _run(tmp_path, stale=1, schedule="fixed", push="fp8")
    _assert_fast_paths(r)
    F._replay_and_check(str(tmp_path), 1, 1, bf16=True, kind="momentum", push="fp8")
    assert [e["pulled"] for e in r["rec"]] == [[max(t - 1, 0)] for t in range(STEPS)]


@pytest.mark.gpu
def test_world1_fp8_pull_under_the_cap_matches_replay(tmp_path, gpu):
    """quant_publish on the background stream, pull_mx straight into the working weights."""
    r = _run(tmp_path, stale=1, pull="fp8")
    _assert_fast_paths(r)
    _replay_and_check(str(tmp_path), 1, 1, mx=True)


@pytest.mark.gpu
def test_world1_clipped_momentum_under_the_cap_matches_replay(tmp_path, gpu):
    """The scaled instantiation of the flat apply under the cap (tests/test_async_clip.py's replay)."""
    import test_async_clip as A

    assert A.CFGS["momentum"] == CFGS["momentum"]
    r = _run(tmp_path, stale=1, clip=CLIP)
    _assert_fast_paths(r)
    coefs = A._replay_and_check(str(tmp_path), 1, 1, bf16=True, kind="momentum", clip=CLIP)
    assert len(coefs) == STEPS and any(c < 1.0 for c in coefs), coefs
    assert all(e["norm"] > CLIP for e in r["rec"] if e["coef"] < 1.0)


@pytest.mark.gpu
def test_world1_lamb_under_the_cap_matches_fp64_within_4x_fp32_eager(tmp_path, gpu):
    """The per-tensor kernels of optim_lw.hip (norm pass, finalize, apply) under the engine's cap:
    the replay and the rule of tests/test_async_layerwise.py on the logged gradients."""
    from test_async_layerwise import _check, _replay

    r = _run(tmp_path, stale=1, kind="lamb")
    _assert_fast_paths(r)
    # one worker: round i is its step-i push
    assert [(e[2], e[4]) for e in r["log"]] == [(t, t + 1) for t in range(STEPS)], r["log"]
    cfg = OptimConfig(**_lamb_cfg())
    lay = [(f"t{i}", o, k, d, "") for i, (o, k, d) in enumerate(r["layout"])]
    w0 = r["init"][0]
    grads = [[e["grad"]] for e in r["rec"]]
    ref = _replay(cfg, lay, w0, grads, torch.float64)
    eag = _replay(cfg, lay, w0, grads, torch.float32)
    _check(lay, w0, r["master"][0], ref[0], eag[0], "lamb master")
    _check(lay, w0, r["final_weights"], ref[0], eag[0].to(torch.bfloat16).float(), "lamb published")
    for e in r["rec"]:
        assert 0 <= e["step"] - e["pulled"][0] <= 1 and min(e["clock_min"]) >= e["step"] - 1, e["pulled"]
