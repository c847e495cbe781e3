"""Error feedback for the MX fp8 gradient push (``AsyncPS(push_dtype="fp8", push_error_feedback=True)``):
the feedback instantiations of the quantising scatter (csrc/kernels/xfer.hip), ``push_quant_mx_`` with
a residual, and the plane around them (parallel/async_ps.py, csrc/async_ps.cpp).

The reference for everything is ``ops.push_quant_mx_ef_ref``: ``v = fp32(g) + r``, MX e4m3 of ``v``
with the push's non-finite rule, ``r' = v - dq(q)`` (0 where ``v`` is not finite). The residual
update is exact in fp32, so every comparison is bitwise:

  * ``q``, ``scales`` and the residual of chained pushes equal the reference on the CPU and on the
    GPU at every workgroup count (both kernel widths);
  * a world-1 run's masters are the fused apply of the reference feedback stream, and its residual
    the reference's;
  * a multi-process run equals the fp32 replay of its recorded apply order with every push's slice
    replaced by the worker's reference feedback stream -- tolerances of tests/test_push_fp8.py;
  * kernel, copy and host transports give the same bytes; checkpoints carry the residual.

Test data keeps ``|v|`` in [2^-60, 2^60] or exactly zero (fp32 subnormals are not under contract).
"""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from parameter_server_distributed_amd import models, ops
from parameter_server_distributed_amd.ops import dequantize_mx_ref, quantize_mx_ref
from parameter_server_distributed_amd.ops.optim import OptimConfig, OptimDyn, fused_apply_, push_quant_mx_
from parameter_server_distributed_amd.parallel.async_ps import AsyncPS
from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

CLIP = 1.5
CFGS = {"momentum": dict(kind="momentum", lr=0.05, momentum=0.9, weight_decay=1e-3),
        "adamw": dict(kind="adamw", lr=2e-3, weight_decay=0.01, beta1=0.9, beta2=0.999, eps=1e-8)}
C_RTOL = 12 * 2.0 ** -23  # the norm kernel's bound (tests/test_grad_clip.py)
SIZES = [32, 32 * 1025, 16 * (3 * 2048 + 2048 + 582)]
DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _u8(t):
    return t.view(torch.uint8)


def _ef_ref(g, r):
    return ops.push_quant_mx_ef_ref(g, r)


def _quant_data(n, dtype, seed=0):
    """``n`` elements in 32-blocks: magnitudes spread down to 2^-20 of the block's amax (far below
    half a quantum: those are what feedback is for), block scales over 2^-12 .. 2^7; with n >= 64
    block 0 is all zero and block 1 has amax exactly 448 * 2^-3."""
    g = torch.Generator().manual_seed(seed)
    nb = n // 32
    x = (torch.rand(nb, 32, generator=g) + 0.5) * torch.exp2(-torch.randint(0, 21, (nb, 32), generator=g).float())
    x = x * torch.where(torch.rand(nb, 32, generator=g) < 0.5, -1.0, 1.0)
    x[:, 7] = 1.25
    x[:, 9] = 1.25 * 2.0 ** -20
    x = x * torch.exp2(torch.randint(-12, 8, (nb, 1), generator=g).float())
    if n >= 64:
        x[0] = 0.0
        x[1] = x[1] / x[1].abs().max() * 2.0 ** -4
        x[1, 30] = 448.0 * 2.0 ** -3
    return x.reshape(n).to(dtype)


def _chain(n, dtype, steps=3):
    """The inputs and the reference outputs of ``steps`` chained pushes from a zero residual."""
    xs, want, r = [], [], torch.zeros(n)
    for t in range(steps):
        x = _quant_data(n, dtype, seed=40 + t)
        q, s, r = _ef_ref(x, r)
        xs.append(x)
        want.append((_u8(q).clone(), s.clone(), r.clone()))
    assert want[0][2].abs().max() > 0, "the second and third calls see a non-zero residual"
    return xs, want


@pytest.fixture(scope="module", params=[torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def chains(request):
    """Per size: the chained inputs and reference outputs, built once per dtype and never written."""
    return request.param, {n: _chain(n, request.param) for n in SIZES}


def _run_chain(xs, want, device, bps):
    n = xs[0].numel()
    r = torch.zeros(n, device=device)
    for x, (wq, ws, wr) in zip(xs, want):
        q = torch.zeros(n, dtype=torch.uint8, device=device)
        sc = torch.zeros(n // 32, dtype=torch.uint8, device=device)
        push_quant_mx_(x.to(device), q, sc, blocks_per_seg=bps, residual=r)
        assert torch.equal(sc.cpu(), ws), ("scale bytes", n, bps)
        assert torch.equal(q.cpu(), wq), ("payload bytes", n, bps)
        assert torch.equal(r.cpu().view(torch.int32), wr.view(torch.int32)), ("residual", n, bps)


# ------------------------------------------------------------------ 1. chained pushes, bitwise
@pytest.mark.parametrize("n", SIZES)
def test_push_ef_cpu_chained_matches_reference_bitwise(chains, n):
    _dtype, data = chains
    _run_chain(*data[n], "cpu", 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_push_ef_gpu_chained_matches_reference_bitwise(gpu, chains, n):
    """blocks_per_seg 1, 3 and 0 (the default) take the 1024-lane instantiation, 128 the 256-lane
    one; each equals the reference bit for bit, hence one another."""
    _dtype, data = chains
    for bps in (1, 3, 0, 128):
        _run_chain(*data[n], gpu, bps)


# ------------------------------------------------------------------ 2. guards, unaligned scale destination
def _guarded(n, device):
    buf = torch.full((n + 128,), -77.25, device=device)
    return buf, buf[64:64 + n]


def _check_guarded(dtype, device):
    n = 64 * 21
    xs, want = _chain(n, dtype, steps=2)
    buf, r = _guarded(n, device)
    r.zero_()
    scb = torch.full((n // 32 + 8,), 0xEE, dtype=torch.uint8, device=device)
    for x, (wq, ws, wr) in zip(xs, want):
        q = torch.zeros(n, dtype=torch.uint8, device=device)
        push_quant_mx_(x.to(device), q, scb[2:2 + n // 32], residual=r)  # scale bytes 2 off a dword
        assert torch.equal(q.cpu(), wq) and torch.equal(scb[2:2 + n // 32].cpu(), ws)
        assert torch.equal(r.cpu(), wr)
    assert scb[:2].tolist() == [0xEE] * 2 and scb[2 + n // 32:].tolist() == [0xEE] * 6
    assert (buf[:64] == -77.25).all() and (buf[64 + n:] == -77.25).all(), "residual guards"


@DTYPES
def test_push_ef_cpu_guards_untouched(dtype):
    _check_guarded(dtype, "cpu")


@pytest.mark.gpu
@DTYPES
def test_push_ef_gpu_guards_untouched(gpu, dtype):
    _check_guarded(dtype, gpu)


# ------------------------------------------------------------------ 3. non-finite values
def _check_nonfinite(dtype, device):
    n = 32 * 6
    x = _quant_data(n, dtype, seed=3)
    _q, _s, r0 = _ef_ref(_quant_data(n, dtype, seed=4), torch.zeros(n))  # a residual of a real push
    bad, blocks = [32 + 5, 3 * 32 + 31, 4 * 32], [1, 3, 4]
    r0[bad[0]], r0[bad[1]], r0[bad[2]] = 2.0 ** -9, -2.0 ** -7, 2.0 ** -11  # non-zero where v is not finite
    x[bad[0]], x[bad[1]], x[bad[2]] = float("nan"), float("inf"), -float("inf")
    sat = [32 + 6, 4 * 32 + 9]  # finite elements of non-finite blocks, beyond 448 at the block's unit scale
    x[sat[0]], x[sat[1]] = 1000.0, -1000.0
    wq, ws, wr = _ef_ref(x, r0)
    q = torch.zeros(n, dtype=torch.uint8, device=device)
    sc = torch.zeros(n // 32, dtype=torch.uint8, device=device)
    r = r0.clone().to(device)
    push_quant_mx_(x.to(device), q, sc, residual=r)
    q, sc, r = q.cpu(), sc.cpu(), r.cpu()
    assert q[bad].tolist() == [0x7F] * 3
    assert sc[blocks].tolist() == [127] * 3
    assert r[bad].tolist() == [0.0] * 3 and torch.isfinite(r).all()
    assert torch.equal(q, _u8(wq)) and torch.equal(sc, ws)
    assert torch.equal(r.view(torch.int32), wr.view(torch.int32))
    # finite elements of such a block: unit scale, saturation at +-448, r' = v - dq as usual
    v = x.float() + r0
    keep = torch.isfinite(v)
    d = dequantize_mx_ref(q.view(torch.float8_e4m3fn), sc)
    assert torch.equal(r[keep], (v - d)[keep])
    assert q[sat].tolist() == [0x7E, 0xFE] and d[sat].tolist() == [448.0, -448.0]
    assert r[sat].tolist() == [float(v[sat[0]]) - 448.0, float(v[sat[1]]) + 448.0] and abs(r[sat[0]]) > 500


@DTYPES
def test_push_ef_cpu_nonfinite_residual_is_zero(dtype):
    _check_nonfinite(dtype, "cpu")


@pytest.mark.gpu
@DTYPES
def test_push_ef_gpu_nonfinite_residual_is_zero(gpu, dtype):
    _check_nonfinite(dtype, gpu)


# ------------------------------------------------------------------ 4. sub-quantum delivery
def _check_subquantum(dtype, device):
    """Two blocks of one 1.0 and 31 elements of 1e-6 over 256 steps. The block's scale is 2^-8 (1.0
    sits in the top binade of e4m3), so a quantum near zero is 2^-9 * 2^-8 = 2^-17: the bound."""
    steps, n = 256, 64
    g = torch.full((n,), 1e-6)
    g[3], g[32 + 17] = 1.0, -1.0
    g = g.to(dtype).to(device)
    small = torch.ones(n, dtype=torch.bool)
    small[3] = small[32 + 17] = False
    q = torch.zeros(n, dtype=torch.uint8, device=device)
    sc = torch.zeros(n // 32, dtype=torch.uint8, device=device)
    plain = torch.zeros(n, dtype=torch.float64)
    for _ in range(steps):
        push_quant_mx_(g, q, sc)
        plain += dequantize_mx_ref(q.cpu().view(torch.float8_e4m3fn), sc.cpu()).double()
    assert (plain[small] == 0).all(), "without feedback the small elements never arrive"
    r = torch.zeros(n, device=device)
    tot = torch.zeros(n, dtype=torch.float64)
    for _ in range(steps):
        push_quant_mx_(g, q, sc, residual=r)
        tot += dequantize_mx_ref(q.cpu().view(torch.float8_e4m3fn), sc.cpu()).double()
    true = steps * g.float().cpu().double()
    err = (tot - true).abs().max().item()
    print(f"sub-quantum delivery {dtype}: max |sum - 256 g| = {err:.3e} (bound 2^-17 = {2.0 ** -17:.3e})")
    assert err <= 2.0 ** -17
    if dtype == torch.bfloat16:  # telescoping: nothing is lost, only deferred
        assert ((tot + r.cpu().double()) - true == 0).all()


@DTYPES
def test_push_ef_cpu_delivers_subquantum_components(dtype):
    _check_subquantum(dtype, "cpu")


@pytest.mark.gpu
@DTYPES
def test_push_ef_gpu_delivers_subquantum_components(gpu, dtype):
    _check_subquantum(dtype, gpu)


# ------------------------------------------------------------------ 5. argument errors, 6. defaults
def _mlp_ps(**kw):
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    return spec, lambda: AsyncPS(spec.model, OptimConfig(**CFGS["momentum"]), staleness=0, bucket_mb=0.0005,
                                 param_dtype=torch.float32, **kw)


def test_push_ef_argument_errors():
    x, q, sc = torch.zeros(64), torch.empty(64, dtype=torch.uint8), torch.empty(2, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="residual"):
        push_quant_mx_(x, q, sc, residual=torch.zeros(64, dtype=torch.bfloat16))
    with pytest.raises(RuntimeError, match="residual"):
        push_quant_mx_(x, q, sc, residual=torch.zeros(32))
    with pytest.raises(RuntimeError, match="residual"):
        push_quant_mx_(x, q, sc, residual=torch.zeros(128)[::2])
    with pytest.raises(ValueError, match="push_error_feedback.*fp8"):
        _mlp_ps(push_dtype="bf16", push_error_feedback=True)[1]()
    with pytest.raises(ValueError, match="push_error_feedback.*fp8"):
        _mlp_ps(push_error_feedback=True)[1]()
    spec, _ = _mlp_ps()
    with pytest.raises(ValueError, match=r"push_error_feedback.*async plane.*AsyncPS"):
        CollectivePS(spec.model, OptimConfig(**CFGS["momentum"]), param_dtype=torch.float32,
                     grad_dtype=torch.float32, push_error_feedback=True)


@pytest.mark.gpu
def test_push_ef_gpu_argument_errors(gpu):
    x = torch.zeros(64, device=gpu)
    q, sc = torch.empty(64, dtype=torch.uint8, device=gpu), torch.empty(2, dtype=torch.uint8, device=gpu)
    with pytest.raises(RuntimeError, match="residual"):  # wrong device
        push_quant_mx_(x, q, sc, residual=torch.zeros(64))
    with pytest.raises(RuntimeError, match="residual"):  # 4 bytes off a 16-byte boundary
        push_quant_mx_(x, q, sc, residual=torch.zeros(68, device=gpu)[1:65])
    with pytest.raises(RuntimeError, match="residual"):
        push_quant_mx_(x, q, sc, residual=torch.zeros(64, dtype=torch.float16, device=gpu))


@pytest.mark.parametrize("push", [None, "fp8"])
def test_push_ef_is_off_by_default(push):
    ps = _mlp_ps(**({"push_dtype": push} if push else {}))[1]()
    assert ps.push_residual is None and ps.memory_bytes()["push_residual"] == 0
    assert "error feedback" not in ps.describe()
    ps.reset_push_residual()  # a no-op
    ps.close()


# ------------------------------------------------------------------ 7. world 1: exact trajectory
def _world1(device, kind="momentum", feedback=True, push="fp8", **kw):
    """A one-process plane (world 1, SSP bound 0) on the MLP and ``run(k)``: k steps on one fixed
    batch, drained; returns the flat gradient of each step."""
    torch.manual_seed(0)
    dev = torch.device(device)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    spec = models.build("mlp", dev, dt, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS[kind]), staleness=0, bucket_mb=0.0005, param_dtype=dt, device=dev,
                 push_dtype=push, push_error_feedback=feedback, **kw)
    x, y = spec.make_batch(16, dev, seed=0)

    def run(k):
        grads = []
        for _ in range(k):
            ps.begin_step()
            spec.loss(spec.model(x), y).backward()
            ps.finish_step()
            if dev.type == "cuda":
                torch.cuda.synchronize()
            grads.append(ps.grads[(ps.step_idx - 1) % 2].clone())
        ps.drain()
        return grads

    return ps, run


def _check_world1(device, kind):
    ps, run = _world1(device, kind)
    dev = ps.device
    assert ps.selftest_ok and ps.push_residual.dtype == torch.float32 and ps.push_residual.numel() == ps.total
    assert not ps.push_residual.any(), "the self-test leaves the residual zero"
    assert ps.memory_bytes()["push_residual"] == 4 * ps.total and "error feedback" in ps.describe()
    cfg = OptimConfig(**CFGS[kind])
    m = ps.master[0].clone()
    s1, s2 = torch.zeros_like(m), (torch.zeros_like(m) if cfg.num_states >= 2 else None)
    grads = run(4)
    dyn = OptimDyn(dev, lr=cfg.lr)
    r = torch.zeros(ps.total)
    for g in grads:
        q, s, r = _ef_ref(g.cpu(), r)
        dq = dequantize_mx_ref(q, s)
        src = dq.to(g.dtype)
        assert torch.equal(src.float(), dq), "dq is exact in the gradient dtype"
        fused_apply_(cfg, dyn, m, [src.to(dev)], s1, s2)
    assert r.abs().max() > 0
    assert torch.equal(ps.master[0].cpu(), m.cpu()), "masters = fused apply of the reference feedback stream"
    assert torch.equal(ps.push_residual.cpu().view(torch.int32), r.view(torch.int32))
    # the probes push without training: they run the feedback path and leave the residual zero
    assert isinstance(ps.probe_push_sizes(sizes_mb=(0.05, 1), reps=1), dict)
    assert not ps.push_residual.any()
    assert ps.probe_xfer_blocks(caps=(8, 48), reps=1) == {}  # world 1: no remote owner, nothing is pushed
    assert not ps.push_residual.any()  # (with a remote owner: test_async_push_ef_gpu_ipc_matches_replay)
    ps.probe_bandwidth(reps=1)
    assert not ps.push_residual.any()
    ps.push_residual.fill_(0.5)  # reset_push_residual itself
    ps.reset_push_residual()
    assert not ps.push_residual.any()
    ps.close()


@pytest.mark.parametrize("kind", ["momentum", "adamw"])
def test_async_push_ef_world1_cpu_equals_apply_of_feedback_stream(kind):
    _check_world1("cpu", kind)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["momentum", "adamw"])
def test_async_push_ef_world1_gpu_equals_apply_of_feedback_stream(gpu, kind):
    _check_world1("cuda:0", kind)


# ------------------------------------------------------------------ 8. multi-process runs, replay-checked
def _worker(rank, world, port, shards, stale, steps, out_dir, device="cpu", kind="momentum", xfer="auto", clip=0.0,
            probe=False):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    spec = models.build("mlp", dev, dt, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS[kind], clip_norm=clip), num_shards=shards, staleness=stale,
                 bucket_mb=0.0005, param_dtype=dt, log=True, device=dev, xfer=xfer, timeout_s=120, push_dtype="fp8",
                 push_error_feedback=True)
    assert not ps.push_residual.any()
    if probe:
        # the workgroup probe with a real remote owner, before the first step: it pushes a non-zero
        # gradient buffer through the feedback path (a push that left its error behind would show) and
        # must leave the residual all zero; the replay of the steps that follow checks that it did
        assert ps.xfer_mode == "kernel" and any(o != rank for o in ps.owners)
        ps.grads[0].copy_(torch.randn(ps.total, generator=torch.Generator().manual_seed(7 + rank)))
        got = ps.probe_xfer_blocks(caps=(8, 48), reps=2)
        assert got["chosen"] in (8, 48) and all(v for v in got["GBps"].values()), got
        torch.cuda.synchronize()
        assert not ps.push_residual.any(), "probe_xfer_blocks leaves the residual zero"
        ps.grads[0].zero_()
    init_master = {k: v.cpu().clone() for k, v in ps.master.items()}
    x, y = spec.make_batch(16, dev, seed=rank)
    rec = []
    for t in range(steps):
        ps.begin_step()
        clocks = [min(ps.engine.clocks(k)) for k in range(ps.P)]
        spec.loss(spec.model(x), y).backward()
        ps.finish_step()
        if dev.type == "cuda":
            torch.cuda.synchronize()
        g = ps.grads[(ps.step_idx - 1) % 2].float().cpu().clone()
        n, c = ps.grad_norm() if clip > 0 else (float("nan"), 1.0)
        rec.append({"step": t, "pulled": list(ps.pulled), "clock_min": clocks, "grad": g, "norm": n, "coef": c,
                    "weights": ps.params_flat.float().cpu().clone()})
    ps.drain()
    inbox = {(k, wi, sl): (_u8(ps.engine.inbox_view(k, wi, sl)).cpu().clone(),
                           ps.engine.inbox_scales_view(k, wi, sl).cpu().clone())
             for k in ps.my_shards for wi in range(ps.W) for sl in range(stale + 1)}
    buckets = [(b.lo, b.hi) for b in ps.buckets]
    torch.save({"rank": rank, "rec": rec, "log": ps.apply_log(), "init": init_master,
                "master": {k: v.cpu() for k, v in ps.master.items()}, "shard_off": ps.shard_off,
                "shard_len": ps.shard_len, "workers": ps.worker_ranks, "owners": ps.owners, "xfer": ps.xfer_mode,
                "mem": ps.engine.memory_kind(), "residual": ps.push_residual.cpu().clone(), "inbox": inbox,
                "buckets": buckets, "grad_bf16": dt == torch.bfloat16},
               os.path.join(out_dir, f"r{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


def _replay_opt(kind, p, g, st, step):
    """One fp32 step of the apply's math on a shard (tests/test_push_fp8.py _replay_opt)."""
    c = CFGS[kind]
    if kind == "momentum":
        g = g + c["weight_decay"] * p
        st["buf"] = g.clone() if "buf" not in st else c["momentum"] * st["buf"] + g
        return p - c["lr"] * st["buf"]
    p = p * (1.0 - c["lr"] * c["weight_decay"])
    st["m"] = c["beta1"] * st.get("m", torch.zeros_like(p)) + (1 - c["beta1"]) * g
    st["v"] = c["beta2"] * st.get("v", torch.zeros_like(p)) + (1 - c["beta2"]) * g * g
    bc1, bc2 = 1 - c["beta1"] ** step, 1 - c["beta2"] ** step
    return p - c["lr"] * (st["m"] / bc1 / (st["v"].sqrt() / bc2 ** 0.5 + c["eps"]))


def _load(out_dir, world):
    return [torch.load(os.path.join(out_dir, f"r{r}.pt"), weights_only=False) for r in range(world)]


def _replay_and_check(out_dir, world, stale, bf16=False, kind="momentum", clip=0.0):
    """tests/test_push_fp8.py _replay_and_check, its tolerances unchanged, with every push's slice
    replaced by the reference feedback stream of that worker: dq(q(g_t + r_t)), r_0 = 0. The
    recorded clip coefficient must be that of the RAW gradient. Also: each worker's final residual is
    the reference's, bitwise. Returns the recorded coefficients."""
    R = _load(out_dir, world)
    workers, owners = R[0]["workers"], R[0]["owners"]
    off, ln = R[0]["shard_off"], R[0]["shard_len"]
    K = W = len(workers)
    recs = {R[r]["rank"]: {e["step"]: e for e in R[r]["rec"]} for r in range(world)}
    coefs, stream = [], {}
    for w in workers:
        r = torch.zeros_like(recs[w][0]["grad"])
        for t in sorted(recs[w]):
            e = recs[w][t]
            if clip > 0:  # the norm of the raw gradient: before the residual is added, before quantisation
                want = min(1.0, clip / (float(e["grad"].double().norm()) + 1e-6))
                assert abs(e["coef"] - want) <= C_RTOL * want, (w, t, e["coef"], want, e["norm"])
            coefs.append(e["coef"])
            g = e["grad"].to(torch.bfloat16) if R[w]["grad_bf16"] else e["grad"]
            q, s, r = _ef_ref(g, r)
            stream[w, t] = dequantize_mx_ref(q, s)
        assert r.abs().max() > 0
        assert torch.equal(R[w]["residual"].view(torch.int32), r.view(torch.int32)), ("residual of worker", w)
    for k, o in enumerate(owners):
        assert off[k] % 64 == 0 and ln[k] % 64 == 0
        log = [e for e in R[o]["log"] if e[0] == k]
        p = R[o]["init"][k].clone()
        opt_state = {}
        snaps = {0: p.clone()}
        assert len(log) % K == 0
        for i in range(len(log) // K):
            rnd = log[i * K:(i + 1) * K]
            assert all(e[4] == i + 1 for e in rnd), rnd
            g = torch.zeros_like(p)
            for (_k, w, t, st, v) in rnd:
                e = recs[w][t]
                assert st == i - e["pulled"][k], (k, w, t, st, i, e["pulled"][k])
                g = g + torch.tensor(e["coef"], dtype=torch.float32) * stream[w, t].narrow(0, off[k], ln[k])
            p = _replay_opt(kind, p, g * (1.0 / K), opt_state, i + 1)
            snaps[i + 1] = p.clone()
        assert len(log) == W * len(recs[workers[0]]), "every push applied exactly once"
        tol = dict(rtol=1e-5, atol=1e-6) if kind == "momentum" else dict(rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(R[o]["master"][k], p, **tol)
        for w in workers:
            for t, e in recs[w].items():
                want, wtol = snaps[e["pulled"][k]], tol
                if bf16:  # published snapshots are bf16(master): one ulp where the replay sits on a tie
                    want = want.to(torch.bfloat16).float()
                    wtol = dict(rtol=2 ** -7, atol=1e-6)
                torch.testing.assert_close(e["weights"].narrow(0, off[k], ln[k]), want, **wtol)
                assert min(e["clock_min"]) >= t - stale, (w, t, e["clock_min"])
    return coefs


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["momentum", "adamw"])
@pytest.mark.parametrize("world,shards,stale", [(2, 2, 0), (3, 2, 1)])
def test_async_push_ef_matches_replay(tmp_path, world, shards, stale, kind):
    mp.spawn(_worker, args=(world, _port(), shards, stale, 5, str(tmp_path), "cpu", kind), nprocs=world, join=True)
    _replay_and_check(str(tmp_path), world, stale, kind=kind)


@pytest.mark.slow
def test_async_push_ef_clip_norm_is_of_the_raw_gradient(tmp_path):
    mp.spawn(_worker, args=(3, _port(), 2, 1, 5, str(tmp_path), "cpu", "momentum", "auto", CLIP), nprocs=3, join=True)
    coefs = _replay_and_check(str(tmp_path), 3, 1, clip=CLIP)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), sorted(coefs)


@pytest.mark.gpu
def test_async_push_ef_gpu_ipc_matches_replay(tmp_path, gpu):
    """Two ranks sharing cuda:0 through real IPC, SSP bound 1, clipping on. The shard cut falls inside
    a bucket, so that bucket's launch has two segments (one local, one peer). Before the first step
    every rank runs ``probe_xfer_blocks`` against its remote owner on a non-zero gradient buffer: the
    probe must leave the residual zero, or the replay of the steps after it would not match."""
    mp.spawn(_worker, args=(2, _port(), 2, 1, 5, str(tmp_path), "cuda:0", "momentum", "auto", CLIP, True), nprocs=2,
             join=True)
    coefs = _replay_and_check(str(tmp_path), 2, 1, bf16=True, clip=CLIP)
    assert any(c < 1.0 for c in coefs), sorted(coefs)
    R = _load(str(tmp_path), 2)
    assert R[0]["mem"] in ("uncached", "finegrained") and R[0]["xfer"] == "kernel"
    cut = R[0]["shard_off"][1]
    assert any(lo < cut < hi for lo, hi in R[0]["buckets"]), (cut, R[0]["buckets"])


# ------------------------------------------------------------------ 9. GPU: the transports agree
@pytest.mark.gpu
def test_async_push_ef_gpu_kernel_and_copy_transports_agree_bitwise(tmp_path, gpu):
    res = {}
    for xfer in ("kernel", "copy"):
        d = tmp_path / xfer
        d.mkdir()
        mp.spawn(_worker, args=(2, _port(), 2, 0, 4, str(d), "cuda:0", "momentum", xfer), nprocs=2, join=True)
        _replay_and_check(str(d), 2, 0, bf16=True)
        res[xfer] = _load(str(d), 2)
    assert [r["xfer"] for r in res["kernel"]] == ["kernel"] * 2
    assert [r["xfer"] for r in res["copy"]] == ["hipMemcpyAsync"] * 2
    for a, b in zip(res["kernel"], res["copy"]):
        assert a["log"] == b["log"]
        for k in a["master"]:
            assert torch.equal(a["master"][k], b["master"][k]), k
        assert torch.equal(a["residual"].view(torch.int32), b["residual"].view(torch.int32))
        assert a["inbox"].keys() == b["inbox"].keys() and len(a["inbox"]) == 2
        for key in a["inbox"]:
            assert torch.equal(a["inbox"][key][0], b["inbox"][key][0]), ("payload", key)
            assert torch.equal(a["inbox"][key][1], b["inbox"][key][1]), ("scales", key)
        for ea, eb in zip(a["rec"], b["rec"]):
            assert ea["pulled"] == eb["pulled"]
            assert torch.equal(ea["weights"], eb["weights"]) and torch.equal(ea["grad"], eb["grad"])


# ------------------------------------------------------------------ 10. checkpoints
def _ckpt_worker(rank, world, port, mode, prefix, out_dir, steps):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS["momentum"]), num_shards=2, staleness=0, bucket_mb=0.0005,
                 param_dtype=torch.float32, push_dtype="fp8", push_error_feedback=True)
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    tr = Trainer(spec.model, spec.loss, ps, spec.make_batch(16, torch.device("cpu"), seed=rank),
                 checkpoint_prefix=prefix if mode == "save" else None, checkpoint_every=3 if mode == "save" else 0)
    if mode == "resume":
        ps.load(prefix)
        assert ps.step_idx == 3 and ps.push_residual.abs().max() > 0
    for _ in range(steps):
        tr.step()
    tr.wait_checkpoint()
    ps.drain()
    ps.refresh_weights()
    torch.save({"master": {k: v.clone() for k, v in ps.master.items()}, "versions": ps.versions(),
                "params": ps.params_flat.clone(), "step": ps.step_idx, "residual": ps.push_residual.clone()},
               os.path.join(out_dir, f"{mode}{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_async_push_ef_save_resume_exact(tmp_path):
    """A 2-rank feedback run checkpointed at step 3 and resumed in new processes ends bitwise equal to
    the uninterrupted 6-step run, residuals included (SSP bound 0: rounds sum in worker order)."""
    prefix = str(tmp_path / "ck")
    mp.spawn(_ckpt_worker, args=(2, _port(), "full", prefix, str(tmp_path), 6), nprocs=2, join=True)
    mp.spawn(_ckpt_worker, args=(2, _port(), "save", prefix, str(tmp_path), 3), nprocs=2, join=True)
    man = json.load(open(prefix + ".manifest.json"))
    assert man["push_dtype"] == "fp8" and man["push_error_feedback"] is True
    mp.spawn(_ckpt_worker, args=(2, _port(), "resume", prefix, str(tmp_path), 3), nprocs=2, join=True)
    for r in range(2):
        full = torch.load(os.path.join(str(tmp_path), f"full{r}.pt"), weights_only=True)
        res = torch.load(os.path.join(str(tmp_path), f"resume{r}.pt"), weights_only=True)
        assert res["versions"] == full["versions"] == [6, 6] and res["step"] == full["step"] == 6
        for k in full["master"]:
            assert torch.equal(full["master"][k], res["master"][k]), (r, k)
        assert torch.equal(full["params"], res["params"]), r
        assert torch.equal(full["residual"].view(torch.int32), res["residual"].view(torch.int32)), r


def test_async_push_ef_world1_save_resume_and_mixed_checkpoints(tmp_path):
    """World 1: resumed masters and residual are bitwise those of the uninterrupted run; a checkpoint
    saved without feedback resumes with feedback on and a zero residual; one saved with feedback
    resumes with feedback off (the residual in the file is ignored)."""
    full, run = _world1("cpu")
    run(6)
    want_m, want_r = full.master[0].clone(), full.push_residual.clone()
    full.close()

    a, run = _world1("cpu")
    run(3)
    ef_prefix = str(tmp_path / "ef")
    a.save(ef_prefix)
    saved_r = a.push_residual.clone()
    a.close()
    from parameter_server_distributed_amd import native

    man, ts = native().load_native_ckpt(ef_prefix + ".rank0.psd")
    m = json.loads(man)
    assert m["push_error_feedback"] is True and m["push_residual"] is True
    assert len(ts) == m["shards"]["0"]["n"] + 1 and torch.equal(ts[-1], saved_r)
    assert json.load(open(ef_prefix + ".manifest.json"))["push_error_feedback"] is True

    b, run = _world1("cpu")
    b.load(ef_prefix)
    assert b.step_idx == 3 and torch.equal(b.push_residual, saved_r)
    run(3)
    assert torch.equal(b.master[0], want_m)
    assert torch.equal(b.push_residual.view(torch.int32), want_r.view(torch.int32))
    b.close()

    c, run = _world1("cpu", feedback=False)  # saved with feedback, resumed without
    c.load(ef_prefix)
    assert c.push_residual is None and c.step_idx == 3
    run(1)
    assert c.versions() == [4] and torch.isfinite(c.master[0]).all()
    plain_prefix = str(tmp_path / "plain")
    c.save(plain_prefix)
    plain_m = c.master[0].clone()
    c.close()
    m = json.loads(native().load_native_ckpt(plain_prefix + ".rank0.psd")[0])
    assert m["push_error_feedback"] is False and m["push_residual"] is False

    d, run = _world1("cpu")  # saved without feedback, resumed with: the residual starts at zero
    d.push_residual.fill_(0.25)
    d.load(plain_prefix)
    assert d.step_idx == 4 and not d.push_residual.any() and torch.equal(d.master[0], plain_m)
    run(1)
    assert d.push_residual.abs().max() > 0
    # an older checkpoint has neither key
    del m["push_error_feedback"], m["push_residual"]
    ts = native().load_native_ckpt(plain_prefix + ".rank0.psd")[1]
    native().save_native_ckpt(str(tmp_path / "old.rank0.psd"), json.dumps(m), list(ts))
    d.load(str(tmp_path / "old"))
    assert d.step_idx == 4 and not d.push_residual.any()
    d.close()


def test_canonical_state_drops_the_residual():
    ps, run = _world1("cpu")
    run(2)
    assert ps.push_residual.abs().max() > 0
    sd = ps.canonical_state(root=0)
    assert sorted(sd) == ["dyn", "master", "state1"]
    ps.load_canonical_state(sd)
    assert not ps.push_residual.any()
    ps.close()


# ------------------------------------------------------------------ 11. CLI and config
def test_cli_and_config_know_push_error_feedback(tmp_path):
    from parameter_server_distributed_amd.cli.worker import build_parser
    from parameter_server_distributed_amd.utils.config import apply_config, load_config

    assert build_parser().parse_args(["c:1", "0"]).push_error_feedback is False
    assert build_parser().parse_args(["c:1", "0", "--push-error-feedback"]).push_error_feedback is True
    cfg = tmp_path / "run.yaml"
    cfg.write_text("push-dtype: fp8\npush-error-feedback: true\n")
    ap = build_parser()
    argv = ["--config", str(cfg), "c:1", "0"]
    apply_config(ap, argv)
    a = ap.parse_intermixed_args(argv)
    assert a.push_dtype == "fp8" and a.push_error_feedback is True
    shipped = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "configs",
                           "elastic_async_fp8_push_ef.yaml")
    c = load_config(shipped)
    assert c["push_dtype"] == "fp8" and c["push_error_feedback"] is True and c["ps_plane"] == "async"
    ap = build_parser()
    argv = ["--config", shipped, "c:1", "0"]
    apply_config(ap, argv)
    assert ap.parse_intermixed_args(argv).push_error_feedback is True
