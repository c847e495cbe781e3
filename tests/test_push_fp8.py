"""MX fp8 gradient push on the asynchronous plane (``AsyncPS(push_dtype="fp8")``): the quantising
push (csrc/kernels/xfer.hip xfer_quant_kernel, ``push_quant_mx_``), the MX-source instantiations of
the owner's kernels (optim.hip, optim_lw.hip, reduce_pack.hip) and the engine around them
(csrc/async_ps.cpp).

The invariants:

  * the quantiser's payload and scale bytes are those of ``ops.quantize_mx_ref`` bit for bit, except
    that a NaN or +-inf element arrives as NaN;
  * ``dq(q)`` is exactly representable in bf16 (and fp32), so an apply fed MX sources is BITWISE the
    bf16 / fp32-source apply fed ``dq(q)``;
  * a multi-process run equals the fp32 replay of its recorded apply order with every recorded
    gradient slice replaced by ``dequantize_mx_ref(*quantize_mx_ref(slice))`` -- the replay's sources
    are exact, so the tolerances are those of tests/test_async_ps.py (rtol 1e-5 momentum / 1e-4
    adamw on the master);
  * ``push_dtype="bf16"`` (the default) is the plane as it was.
"""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from parameter_server_distributed_amd import models, native
from parameter_server_distributed_amd.ops import dequantize_mx_ref, quantize_mx_ref
from parameter_server_distributed_amd.ops.optim import (LayerTable, OptimConfig, OptimDyn, fused_apply_, multi_reduce_,
                                                        push_quant_mx_)
from parameter_server_distributed_amd.parallel.async_ps import AsyncPS
from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

CLIP = 1.5
CFGS = {"sgd": dict(kind="sgd", lr=0.05, weight_decay=1e-3),
        "momentum": dict(kind="momentum", lr=0.05, momentum=0.9, weight_decay=1e-3),
        "adamw": dict(kind="adamw", lr=2e-3, weight_decay=0.01, beta1=0.9, beta2=0.999, eps=1e-8),
        "lamb": dict(kind="lamb", lr=2e-3, weight_decay=1e-2, beta1=0.9, beta2=0.999, eps=1e-6)}
C_RTOL = 12 * 2.0 ** -23  # the norm kernel's bound (tests/test_grad_clip.py)


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _u8(t):
    return t.view(torch.uint8)


def _mx_roundtrip(x):
    return dequantize_mx_ref(*quantize_mx_ref(x))


# ------------------------------------------------------------------ 1. the quantiser
def _quant_data(n, dtype, pattern="mixed", seed=0):
    """``n`` elements in 32-blocks: magnitudes spread down to 2^-20 of the block's amax, block
    scales over 2^-12 .. 2^7. "mixed" (n >= 64): block 0 all zero, block 1 with amax exactly
    448 * 2^-3. "zero" / "amax448" / "wide": one property for the single-block size."""
    g = torch.Generator().manual_seed(seed)
    nb = n // 32
    x = (torch.rand(nb, 32, generator=g) + 0.5) * torch.exp2(-torch.randint(0, 21, (nb, 32), generator=g).float())
    x = x * torch.where(torch.rand(nb, 32, generator=g) < 0.5, -1.0, 1.0)
    x[:, 7] = 1.25  # every block's amax, 2^-20 of it is still there
    x[:, 9] = 1.25 * 2.0 ** -20
    x = x * torch.exp2(torch.randint(-12, 8, (nb, 1), generator=g).float())
    if pattern == "zero":
        x[0] = 0.0
    elif pattern == "amax448":
        x[0] = x[0] / x[0].abs().max() * 0.5
        x[0, 3] = -448.0 * 2.0 ** 5
    elif pattern == "mixed":
        x[0] = 0.0
        x[1] = x[1] / x[1].abs().max() * 2.0 ** -4
        x[1, 30] = 448.0 * 2.0 ** -3
    return x.reshape(n).to(dtype)


def _check_quant(x, q, sc):
    rq, rs = quantize_mx_ref(x)
    assert torch.equal(sc.cpu(), rs.cpu()), "scale bytes"
    assert torch.equal(_u8(q).cpu(), _u8(rq).cpu()), "payload bytes"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n,pattern", [(32, "zero"), (32, "amax448"), (32, "wide"), (64, "mixed"),
                                       (32 * 1025, "mixed")])
def test_push_quant_cpu_matches_reference_bitwise(n, pattern, dtype):
    x = _quant_data(n, dtype, pattern)
    if pattern == "mixed":
        assert not x[:32].any() and float(x[32:64].abs().max()) == 448.0 * 2.0 ** -3
    q = torch.empty(n, dtype=torch.float8_e4m3fn)
    sc = torch.empty(n // 32, dtype=torch.uint8)
    push_quant_mx_(x, q, sc)
    _check_quant(x, q, sc)
    q8 = torch.empty(n, dtype=torch.uint8)  # uint8 payload tensors are accepted too
    push_quant_mx_(x, q8, sc)
    assert torch.equal(q8, _u8(q))


def _nonfinite_case(dtype, device):
    x = _quant_data(32 * 6, dtype, "wide", seed=3).to(device)
    x[32 + 5] = float("nan")
    x[3 * 32 + 31] = float("inf")
    x[4 * 32] = -float("inf")
    return x, [32 + 5, 3 * 32 + 31, 4 * 32], [1, 3, 4]


def _check_nonfinite(x, q, sc, bad, bad_blocks):
    d = dequantize_mx_ref(q.view(torch.float8_e4m3fn), sc).cpu()
    assert torch.isnan(d[bad]).all(), d[bad]
    assert all(int(_u8(q)[i]) == 0x7F for i in bad)
    keep = torch.ones(x.numel() // 32, dtype=torch.bool)
    keep[bad_blocks] = False
    rq, rs = quantize_mx_ref(x.cpu())
    assert torch.equal(sc.cpu()[keep], rs[keep])
    assert torch.equal(_u8(q).cpu().view(-1, 32)[keep], _u8(rq).view(-1, 32)[keep])
    assert int(torch.isnan(d).sum()) == len(bad), "only the non-finite elements become NaN"
    assert sc.cpu()[bad_blocks].tolist() == [127] * len(bad_blocks)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_push_quant_cpu_nonfinite_arrives_as_nan(dtype):
    x, bad, blocks = _nonfinite_case(dtype, "cpu")
    q = torch.empty(x.numel(), dtype=torch.float8_e4m3fn)
    sc = torch.empty(x.numel() // 32, dtype=torch.uint8)
    push_quant_mx_(x, q, sc)
    _check_nonfinite(x, q, sc, bad, blocks)


def test_push_quant_rejects_partial_blocks():
    with pytest.raises(RuntimeError, match="multiple of 32"):
        push_quant_mx_(torch.zeros(40), torch.empty(40, dtype=torch.uint8), torch.empty(1, dtype=torch.uint8))


# ------------------------------------------------------------------ 2. the apply's bitwise invariant
LW_TENSORS = [(0, 8192 + 64, 2), (8192 + 64, 40, 1), (8192 + 128, 200, 2)]  # (offset, numel, ndim), 64-aligned
LW_N = 8192 + 128 + 256


def _mx_sources(n, K, device, seed=0):
    g = torch.Generator().manual_seed(seed)
    qs, ss, dq = [], [], []
    for _ in range(K):
        x = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 3, (n,), generator=g).float())
        q, s = quantize_mx_ref(x)
        qs.append(q.to(device))
        ss.append(s.to(device))
        dq.append(dequantize_mx_ref(q, s))
    return qs, ss, dq


def _run_apply(kind, n, grads, device, scales=None, mx_scales=None, layers=None, steps=2, grid_cap=0):
    cfg = OptimConfig(**CFGS[kind])
    g = torch.Generator().manual_seed(11)
    master = torch.randn(n, generator=g).to(device)
    s1 = torch.zeros(n, device=device) if cfg.num_states >= 1 else None
    s2 = torch.zeros(n, device=device) if cfg.num_states >= 2 else None
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=device)
    dyn = OptimDyn(device, lr=cfg.lr, grad_scale=1.0 / len(grads))
    tab = LayerTable(LW_TENSORS, n, cfg.exclude_1d, device) if layers else None
    for _ in range(steps):
        fused_apply_(cfg, dyn, master, grads, s1, s2, shadow, layers=tab, scales=scales, mx_scales=mx_scales,
                     grid_cap=grid_cap)
    return [t for t in (master, s1, s2, shadow) if t is not None]


def _coefs(K, device):
    return [torch.tensor([0.37 + 0.21 * k] + [9.0] * 63, device=device) for k in range(K)]


def _assert_same(a, b, what):
    assert len(a) == len(b)
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x.cpu().view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32),
                           y.cpu().view(torch.int16 if y.dtype == torch.bfloat16 else torch.int32)), (what, i)


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("kind", ["sgd", "momentum", "adamw", "lamb"])
def test_apply_cpu_mx_sources_bitwise_equal_dequantised_sources(kind, K, scaled):
    lw = kind == "lamb"
    n = LW_N if lw else 64 * 37
    qs, ss, dq = _mx_sources(n, K, "cpu")
    sc = _coefs(K, "cpu") if scaled else None
    want = _run_apply(kind, n, dq, "cpu", scales=sc, layers=lw)
    got = _run_apply(kind, n, qs, "cpu", scales=sc, mx_scales=ss, layers=lw)
    _assert_same(got, want, (kind, K, scaled))
    got8 = _run_apply(kind, n, [_u8(q) for q in qs], "cpu", scales=sc, mx_scales=ss, layers=lw)
    _assert_same(got8, want, "uint8 payload")


@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, 3])
def test_multi_reduce_cpu_mx_sources_bitwise(K, scaled):
    n = 64 * 9
    qs, ss, dq = _mx_sources(n, K, "cpu", seed=2)
    sc = _coefs(K, "cpu") if scaled else None
    for odt in (torch.float32, torch.bfloat16):
        want, got = torch.empty(n, dtype=odt), torch.empty(n, dtype=odt)
        multi_reduce_(want, dq, 0.5, scales=sc)
        multi_reduce_(got, qs, 0.5, scales=sc, mx_scales=ss)
        _assert_same([got], [want], (K, scaled, odt))


def test_mx_sources_argument_errors():
    n = 64
    qs, ss, dq = _mx_sources(n, 2, "cpu")
    cfg, dyn = OptimConfig(kind="sgd", lr=0.1), OptimDyn("cpu", lr=0.1)
    m = torch.zeros(n)
    with pytest.raises(ValueError, match="mx_scales"):  # a partial list, as for scales
        fused_apply_(cfg, dyn, m, qs, mx_scales=[ss[0]])
    with pytest.raises(ValueError, match="mx_scales"):
        multi_reduce_(m, qs, mx_scales=[ss[0], None])
    with pytest.raises(RuntimeError, match="mx_scales"):  # fp8 payloads without their scales
        fused_apply_(cfg, dyn, m, qs)
    with pytest.raises(RuntimeError, match="float8_e4m3fn or uint8"):
        fused_apply_(cfg, dyn, m, dq, mx_scales=ss)
    with pytest.raises(RuntimeError, match="32-element blocks"):
        fused_apply_(cfg, dyn, torch.zeros(40), [torch.zeros(40, dtype=torch.uint8)],
                     mx_scales=[torch.zeros(1, dtype=torch.uint8)])


# ------------------------------------------------------------------ 3. multi-process runs, replay-checked
def _worker(rank, world, port, shards, stale, steps, out_dir, device="cpu", kind="momentum", xfer="auto", clip=0.0,
            push="fp8", pull="bf16"):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    dev = torch.device(device)
    if dev.type == "cuda":
        torch.cuda.set_device(dev)
    dt = torch.bfloat16 if dev.type == "cuda" else torch.float32
    spec = models.build("mlp", dev, dt, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS[kind], clip_norm=clip), num_shards=shards, staleness=stale,
                 bucket_mb=0.0005, param_dtype=dt, log=True, device=dev, xfer=xfer, timeout_s=120, push_dtype=push,
                 pull_dtype=pull)
    init_master = {k: v.cpu().clone() for k, v in ps.master.items()}
    slot_bytes = [int(ps.engine.inbox_slot_bytes(k)) for k in range(ps.P)]
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
    torch.save({"rank": rank, "rec": rec, "log": ps.apply_log(), "init": init_master,
                "master": {k: v.cpu() for k, v in ps.master.items()}, "shard_off": ps.shard_off,
                "shard_len": ps.shard_len, "workers": ps.worker_ranks, "owners": ps.owners, "xfer": ps.xfer_mode,
                "mem": ps.engine.memory_kind(), "slot_bytes": slot_bytes, "elem": ps.grads[0].element_size(),
                "layout": [(o, k, p.dim()) for (_n, p, o, k) in ps._layout]},
               os.path.join(out_dir, f"r{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


def _replay_opt(kind, p, g, st, step, segs):
    """One fp32 step of the apply's math on a shard (``segs``: its tensors, (start, end, ndim), for lamb)."""
    c = CFGS[kind]
    if kind == "momentum":
        g = g + c["weight_decay"] * p
        st["buf"] = g.clone() if "buf" not in st else c["momentum"] * st["buf"] + g
        return p - c["lr"] * st["buf"]
    if kind == "adamw":
        p = p * (1.0 - c["lr"] * c["weight_decay"])
    st["m"] = c["beta1"] * st.get("m", torch.zeros_like(p)) + (1 - c["beta1"]) * g
    st["v"] = c["beta2"] * st.get("v", torch.zeros_like(p)) + (1 - c["beta2"]) * g * g
    bc1, bc2 = 1 - c["beta1"] ** step, 1 - c["beta2"] ** step
    d = st["m"] / bc1 / (st["v"].sqrt() / bc2 ** 0.5 + c["eps"])
    if kind == "adamw":
        return p - c["lr"] * d
    p = p.clone()
    for a, b, nd in segs:  # lamb: per tensor, no decay and no trust ratio on ndim <= 1
        w = p[a:b]
        u = d[a:b] + (c["weight_decay"] if nd > 1 else 0.0) * w
        wn, un = float(w.double().norm()), float(u.double().norm())
        r = wn / un if (nd > 1 and wn > 0 and un > 0) else 1.0
        p[a:b] = w - c["lr"] * r * u
    return p


def _load(out_dir, world):
    return [torch.load(os.path.join(out_dir, f"r{r}.pt"), weights_only=False) for r in range(world)]


def _replay_and_check(out_dir, world, stale, bf16=False, kind="momentum", clip=0.0, push="fp8", mx_pull=False):
    """The fp32 replay of the logged rounds (tests/test_async_ps.py _replay_and_check, its
    tolerances) with every push's gradient slice replaced by its MX round trip -- what the owner
    dequantises -- times the worker's recorded clip coefficient, which must be that of the RAW
    gradient. Returns the recorded coefficients."""
    R = _load(out_dir, world)
    workers, owners = R[0]["workers"], R[0]["owners"]
    off, ln = R[0]["shard_off"], R[0]["shard_len"]
    K = W = len(workers)
    recs = {R[r]["rank"]: {e["step"]: e for e in R[r]["rec"]} for r in range(world)}
    coefs = []
    for w in workers:
        for t, e in recs[w].items():
            if clip > 0:  # the norm of the gradient before quantisation
                want = min(1.0, clip / (float(e["grad"].double().norm()) + 1e-6))
                assert abs(e["coef"] - want) <= C_RTOL * want, (w, t, e["coef"], want, e["norm"])
            coefs.append(e["coef"])
    for k, o in enumerate(owners):
        assert off[k] % 64 == 0 and ln[k] % 64 == 0  # a block never straddles a shard
        segs = [(a - off[k], a - off[k] + n, nd) for (a, n, nd) in R[0]["layout"] if off[k] <= a < off[k] + ln[k]]
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
                sl = e["grad"].narrow(0, off[k], ln[k])
                if push == "fp8":
                    sl = _mx_roundtrip(sl)
                g = g + torch.tensor(e["coef"], dtype=torch.float32) * sl
            p = _replay_opt(kind, p, g * (1.0 / K), opt_state, i + 1, segs)
            snaps[i + 1] = p.clone()
        assert len(log) == W * len(recs[workers[0]]), "every push applied exactly once"
        tol = dict(rtol=1e-5, atol=1e-6) if kind == "momentum" else dict(rtol=1e-4, atol=1e-5)
        torch.testing.assert_close(R[o]["master"][k], p, **tol)
        for w in workers:
            for t, e in recs[w].items():
                want, wtol = snaps[e["pulled"][k]], tol
                if mx_pull:  # MX e4m3 publish: the worker's weights are dequant(quant_mx(master))
                    want = _mx_roundtrip(want)
                    wtol = dict(rtol=2 ** -3, atol=2 ** -9 * float(want.abs().max()))
                elif bf16:  # published snapshots are bf16(master): one ulp where the replay sits on a tie
                    want = want.to(torch.bfloat16).float()
                    wtol = dict(rtol=2 ** -7, atol=1e-6)
                torch.testing.assert_close(e["weights"].narrow(0, off[k], ln[k]), want, **wtol)
                assert min(e["clock_min"]) >= t - stale, (w, t, e["clock_min"])
    return coefs


def _assert_slot_bytes(R, push):
    """An inbox slot: shard_len * 33 / 32 bytes under fp8 push (the element size per element
    otherwise), rounded up only for alignment (256-byte slots, so every region stays 16-byte aligned)."""
    for k, n in enumerate(R["shard_len"]):
        exact = n * 33 // 32 if push == "fp8" else n * R["elem"]
        sb = R["slot_bytes"][k]
        assert exact <= sb < exact + 256 and sb % 256 == 0, (k, n, sb)


@pytest.mark.slow
@pytest.mark.parametrize("kind", ["momentum", "adamw"])
@pytest.mark.parametrize("world,shards,stale", [(2, 2, 0), (3, 2, 1)])
def test_async_fp8_push_matches_replay(tmp_path, world, shards, stale, kind):
    mp.spawn(_worker, args=(world, _port(), shards, stale, 5, str(tmp_path), "cpu", kind), nprocs=world, join=True)
    _replay_and_check(str(tmp_path), world, stale, kind=kind)
    _assert_slot_bytes(_load(str(tmp_path), world)[0], "fp8")


@pytest.mark.slow
def test_async_fp8_push_replay_sees_the_quantisation(tmp_path):
    """The check has teeth: the same run replayed with the RAW gradients misses the tolerance."""
    mp.spawn(_worker, args=(2, _port(), 2, 0, 5, str(tmp_path), "cpu", "momentum"), nprocs=2, join=True)
    with pytest.raises(AssertionError):
        _replay_and_check(str(tmp_path), 2, 0, push="bf16")


@pytest.mark.slow
def test_async_fp8_push_clip_norm_is_of_the_raw_gradient(tmp_path):
    """Step-0 norms of ranks 0, 1, 2 on this model are 2.21, 1.99, 1.19 against clip_norm 1.5: some
    pushes clip and some do not; the coefficient multiplies the dequantised source."""
    mp.spawn(_worker, args=(3, _port(), 2, 1, 5, str(tmp_path), "cpu", "momentum", "auto", CLIP), nprocs=3, join=True)
    coefs = _replay_and_check(str(tmp_path), 3, 1, clip=CLIP)
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), sorted(coefs)


@pytest.mark.slow
def test_async_fp8_push_w17_group_prereduce(tmp_path):
    world = 17
    mp.spawn(_worker, args=(world, _port(), 2, 0, 3, str(tmp_path), "cpu", "momentum"), nprocs=world, join=True)
    _replay_and_check(str(tmp_path), world, 0)


@pytest.mark.slow
def test_async_fp8_push_lamb_matches_replay(tmp_path):
    mp.spawn(_worker, args=(3, _port(), 2, 1, 5, str(tmp_path), "cpu", "lamb"), nprocs=3, join=True)
    _replay_and_check(str(tmp_path), 3, 1, kind="lamb")


@pytest.mark.slow
def test_async_fp8_push_semantics_push_runs(tmp_path):
    """Apply-on-arrival semantics (K = 1) and the fixed schedule take MX sources too."""
    torch.manual_seed(0)
    for kw in (dict(semantics="push"), dict(schedule="fixed")):
        spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
        ps = AsyncPS(spec.model, OptimConfig(**CFGS["momentum"]), staleness=1, bucket_mb=0.0005,
                     param_dtype=torch.float32, push_dtype="fp8", **kw)
        x, y = spec.make_batch(16, torch.device("cpu"), seed=0)
        before = ps.master[0].clone()
        for _ in range(3):
            ps.begin_step()
            spec.loss(spec.model(x), y).backward()
            ps.finish_step()
        ps.drain()
        assert ps.versions() == [3] and not torch.equal(before, ps.master[0])
        assert torch.isfinite(ps.master[0]).all()
        ps.close()


# ------------------------------------------------------------------ 4. world 1: exact trajectory, errors, slots
def _world1(push, kind="momentum", **kw):
    """A one-process plane (world 1, SSP bound 0) on the MLP and ``run(k)``: k steps on one fixed
    batch, drained; returns the flat gradient of each step."""
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS[kind]), staleness=0, bucket_mb=0.0005, param_dtype=torch.float32,
                 push_dtype=push, **kw)
    x, y = spec.make_batch(16, torch.device("cpu"), seed=0)

    def run(k, poke=None):
        grads = []
        for _ in range(k):
            ps.begin_step()
            spec.loss(spec.model(x), y).backward()
            if poke is not None:
                poke(ps.grads[ps.gb])
            ps.finish_step()
            grads.append(ps.grads[(ps.step_idx - 1) % 2].clone())
        ps.drain()
        return grads

    return ps, run


def test_async_fp8_push_world1_equals_apply_of_dequantised_gradients():
    """World 1, SSP 0: the master after the run is BITWISE the fused apply of dq(q(gradient)) step by
    step, and the inbox slot holds the last gradient's payload and scale bytes."""
    ps, run = _world1("fp8")
    cfg = OptimConfig(**CFGS["momentum"])
    m, s1 = ps.master[0].clone(), torch.zeros_like(ps.master[0])
    grads = run(4)
    dyn = OptimDyn("cpu", lr=cfg.lr)
    for g in grads:
        fused_apply_(cfg, dyn, m, [_mx_roundtrip(g)], s1)
    assert torch.equal(ps.master[0], m)
    n = ps.shard_len[0]
    assert ps.engine.inbox_slot_bytes(0) == -(-(n * 33 // 32) // 256) * 256
    assert ps.engine.inbox_view(0, 0, 0).dtype == torch.float8_e4m3fn
    assert ps.engine.inbox_scales_view(0, 0, 0).shape == (n // 32,)
    rq, rs = quantize_mx_ref(grads[-1])
    assert torch.equal(_u8(ps.engine.inbox_view(0, 0, 0)), _u8(rq))
    assert torch.equal(ps.engine.inbox_scales_view(0, 0, 0), rs)
    ps.close()


def test_async_fp8_push_nonfinite_gradient_reaches_the_master_as_nan():
    """An inf in the gradient buffer (element 5: fc2.bias) is not laundered into 448 * scale."""
    ps, run = _world1("fp8", overlap=False)  # every bucket leaves in finish_step, after the poke

    def poke(g):
        g[5] = float("inf")

    run(1, poke)
    assert torch.isnan(ps.master[0][5]) and int(torch.isnan(ps.master[0]).sum()) == 1
    ps.close()


def test_push_dtype_argument_errors():
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    with pytest.raises(ValueError, match="push_dtype"):
        AsyncPS(spec.model, OptimConfig(**CFGS["momentum"]), param_dtype=torch.float32, push_dtype="fp4")
    with pytest.raises(ValueError, match=r"push_dtype='fp8'.*async plane.*AsyncPS"):
        CollectivePS(spec.model, OptimConfig(**CFGS["momentum"]), param_dtype=torch.float32,
                     grad_dtype=torch.float32, push_dtype="fp8")
    with pytest.raises(ValueError, match="push_dtype"):
        CollectivePS(spec.model, OptimConfig(**CFGS["momentum"]), param_dtype=torch.float32,
                     grad_dtype=torch.float32, push_dtype="e5m2")


def test_default_push_is_bf16_and_slots_are_unchanged():
    ps, run = _world1("bf16")
    run(1)
    assert ps.push_dtype == "bf16" and not ps.push_mx
    n = ps.shard_len[0]
    assert ps.engine.inbox_slot_bytes(0) == -(-(n * 4) // 256) * 256
    assert ps.engine.inbox_view(0, 0, 0).dtype == torch.float32
    with pytest.raises(RuntimeError, match="MX-push engines only"):
        ps.engine.inbox_scales_view(0, 0, 0)
    ps.close()


def test_cli_and_config_know_push_dtype(tmp_path):
    from parameter_server_distributed_amd.cli.worker import build_parser
    from parameter_server_distributed_amd.utils.config import apply_config

    assert build_parser().parse_args(["c:1", "0"]).push_dtype == "bf16"
    assert build_parser().parse_args(["c:1", "0", "--push-dtype", "fp8"]).push_dtype == "fp8"
    cfg = tmp_path / "run.yaml"
    cfg.write_text("push-dtype: fp8\npull-dtype: bf16\n")
    ap = build_parser()
    argv = ["--config", str(cfg), "c:1", "0"]
    apply_config(ap, argv)
    assert ap.parse_intermixed_args(argv).push_dtype == "fp8"


# ------------------------------------------------------------------ 5. checkpoints
def _ckpt_worker(rank, world, port, mode, prefix, out_dir, steps, push):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(0)
    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=64)
    ps = AsyncPS(spec.model, OptimConfig(**CFGS["momentum"]), num_shards=2, staleness=0, bucket_mb=0.0005,
                 param_dtype=torch.float32, push_dtype=push)
    from parameter_server_distributed_amd.runtime.trainer import Trainer

    tr = Trainer(spec.model, spec.loss, ps, spec.make_batch(16, torch.device("cpu"), seed=rank),
                 checkpoint_prefix=prefix if mode == "save" else None, checkpoint_every=3 if mode == "save" else 0)
    if mode == "resume":
        ps.load(prefix)
        assert ps.step_idx == 3 and ps.resumed_push_dtype == "fp8"
    for _ in range(steps):
        tr.step()
    tr.wait_checkpoint()
    ps.drain()
    ps.refresh_weights()
    torch.save({"master": {k: v.clone() for k, v in ps.master.items()}, "versions": ps.versions(),
                "params": ps.params_flat.clone(), "step": ps.step_idx},
               os.path.join(out_dir, f"{mode}{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.slow
def test_async_fp8_push_save_resume_exact(tmp_path):
    """A 2-rank fp8-push run checkpointed at step 3 and resumed in new processes ends bitwise equal to
    the uninterrupted 6-step run (SSP bound 0: rounds sum in worker order)."""
    prefix = str(tmp_path / "ck")
    mp.spawn(_ckpt_worker, args=(2, _port(), "full", prefix, str(tmp_path), 6, "fp8"), nprocs=2, join=True)
    mp.spawn(_ckpt_worker, args=(2, _port(), "save", prefix, str(tmp_path), 3, "fp8"), nprocs=2, join=True)
    assert json.load(open(prefix + ".manifest.json"))["push_dtype"] == "fp8"
    mp.spawn(_ckpt_worker, args=(2, _port(), "resume", prefix, str(tmp_path), 3, "fp8"), nprocs=2, join=True)
    for r in range(2):
        full = torch.load(os.path.join(str(tmp_path), f"full{r}.pt"), weights_only=True)
        res = torch.load(os.path.join(str(tmp_path), f"resume{r}.pt"), weights_only=True)
        assert res["versions"] == full["versions"] == [6, 6] and res["step"] == full["step"] == 6
        for k in full["master"]:
            assert torch.equal(full["master"][k], res["master"][k]), (r, k)
        assert torch.equal(full["params"], res["params"]), r


def test_checkpoint_without_the_key_loads_as_bf16_and_fp8_resumes_with_bf16_push(tmp_path):
    """Older checkpoints have no push_dtype: they were bf16 pushes. A checkpoint saved under fp8 push
    resumed with bf16 push is SUPPORTED: a drained checkpoint holds no in-flight gradient, so the
    masters, state, versions and clocks restore exactly and training continues with raw pushes."""
    ps, run = _world1("fp8")
    run(3)
    prefix = str(tmp_path / "ck")
    ps.save(prefix)
    saved = ps.master[0].clone()
    ps.close()
    C = native()
    man, ts = C.load_native_ckpt(prefix + ".rank0.psd")
    m = json.loads(man)
    assert m["push_dtype"] == "fp8"
    del m["push_dtype"]
    C.save_native_ckpt(str(tmp_path / "old.rank0.psd"), json.dumps(m), list(ts))

    ps2, run2 = _world1("bf16")
    ps2.load(str(tmp_path / "old"))
    assert ps2.resumed_push_dtype == "bf16"
    ps2.load(prefix)
    assert ps2.resumed_push_dtype == "fp8" and ps2.push_dtype == "bf16"
    assert ps2.step_idx == 3 and ps2.versions() == [3] and torch.equal(ps2.master[0], saved)
    run2(1)
    assert ps2.versions() == [4] and torch.isfinite(ps2.master[0]).all()
    ps2.close()


# ------------------------------------------------------------------ 6. convergence smoke
# Mean loss of the last 20 of 200 steps, world 2, S = 0, a learnable task (uniform noise plus 0.2 x a
# fixed random prototype of the class, a fresh batch per step and rank). The margin is 3 x the
# seed-to-seed spread (max - min) of the bf16-push run over 5 seeds, measured in
# profiles/push_fp8.md ("Convergence"): bf16 final losses 0.00763 .. 0.02091.
CONV_SPREAD_BF16 = 0.01327
CONV_STEPS = 200


def _conv_worker(rank, world, port, push, seed, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(seed)
    dev = torch.device("cpu")
    spec = models.build("mlp", dev, torch.float32, hidden=64)
    proto = torch.rand(10, 784, generator=torch.Generator().manual_seed(1234))
    ps = AsyncPS(spec.model, OptimConfig(kind="momentum", lr=0.05, momentum=0.9), num_shards=2, staleness=0,
                 bucket_mb=0.0005, param_dtype=torch.float32, push_dtype=push)
    losses = []
    for t in range(CONV_STEPS):
        g = torch.Generator().manual_seed(100000 * seed + 2 * t + rank)
        y = torch.randint(0, 10, (32,), generator=g)
        x = (0.8 * torch.rand(32, 784, generator=g) + 0.2 * proto[y]).view(32, 1, 28, 28)
        ps.begin_step()
        loss = spec.loss(spec.model(x), y)
        loss.backward()
        ps.finish_step()
        losses.append(float(loss.detach()))
    ps.drain()
    torch.save(losses, os.path.join(out_dir, f"{push}_s{seed}_r{rank}.pt"))
    ps.close()
    dist.barrier()
    dist.destroy_process_group()


def _conv_loss(out_dir, push, seed):
    mp.spawn(_conv_worker, args=(2, _port(), push, seed, out_dir), nprocs=2, join=True)
    per_rank = [torch.load(os.path.join(out_dir, f"{push}_s{seed}_r{r}.pt")) for r in range(2)]
    return sum(sum(l[-20:]) / 20 for l in per_rank) / 2, sum(l[0] for l in per_rank) / 2


@pytest.mark.slow
def test_async_fp8_push_convergence_smoke(tmp_path):
    fp8, first = _conv_loss(str(tmp_path), "fp8", 0)
    bf16, _ = _conv_loss(str(tmp_path), "bf16", 0)
    print(f"fp8 push {fp8:.4f}, bf16 push {bf16:.4f}, first step {first:.4f}, margin {3 * CONV_SPREAD_BF16:.4f}")
    assert bf16 < 0.5 * first, "the task is learnable: the bf16 run itself converges"
    assert abs(fp8 - bf16) <= 3 * CONV_SPREAD_BF16, (fp8, bf16)


# ------------------------------------------------------------------ 7. GPU: the kernels
GRID_WRAP_N = 32 * (2048 * 256 // 4 + 1)  # the flat apply's 2048 x 256-lane grid wraps (8 elements per lane)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n", [32, 32 * 1025, 16 * (3 * 2048 + 2048 + 582)])
def test_push_quant_gpu_matches_reference_bitwise(gpu, n, dtype):
    """The last size is 8774 16-element items. A workgroup (1024 lanes, 2 items per lane) takes 2048
    per pass, so with 3 workgroups per segment the grid-stride loop runs twice and the second pass is
    partial: one workgroup full, one with 582 items (its first unrolled item cut inside a wave, its
    second empty), one idle. 200 workgroups take the 256-lane variant of the kernel (a grid that
    fills the GPU). Every blocks_per_seg value gives the same bytes."""
    x = _quant_data(n, dtype, "mixed" if n >= 64 else "wide", seed=5).to(gpu)
    outs = []
    for bps in ((1, 3, 200) if n > 32 else (1, 2, 200)):
        q = torch.zeros(n, dtype=torch.float8_e4m3fn, device=gpu)
        sc = torch.zeros(n // 32, dtype=torch.uint8, device=gpu)
        push_quant_mx_(x, q, sc, blocks_per_seg=bps)
        _check_quant(x.cpu(), q, sc)
        outs.append((_u8(q).cpu(), sc.cpu()))
    for o in outs[1:]:
        assert torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1])
    q0 = torch.zeros(n, dtype=torch.uint8, device=gpu)  # the default workgroup count, uint8 payload
    sc0 = torch.zeros(n // 32, dtype=torch.uint8, device=gpu)
    push_quant_mx_(x, q0, sc0)
    assert torch.equal(q0.cpu(), outs[0][0]) and torch.equal(sc0.cpu(), outs[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_push_quant_gpu_nonfinite_arrives_as_nan(gpu, dtype):
    x, bad, blocks = _nonfinite_case(dtype, gpu)
    q = torch.zeros(x.numel(), dtype=torch.float8_e4m3fn, device=gpu)
    sc = torch.zeros(x.numel() // 32, dtype=torch.uint8, device=gpu)
    push_quant_mx_(x, q, sc)
    _check_nonfinite(x, q.cpu(), sc.cpu(), bad, blocks)


@pytest.mark.gpu
def test_push_quant_gpu_unaligned_scale_destination(gpu):
    """A segment whose scale bytes start 2 bytes off a dword (a 64-element boundary inside a shard)
    takes the 2-byte stores; neighbours of the written range stay untouched."""
    n = 64 * 21
    x = _quant_data(n, torch.bfloat16, "mixed", seed=9).to(gpu)
    q = torch.zeros(n, dtype=torch.uint8, device=gpu)
    buf = torch.full((n // 32 + 8,), 0xEE, dtype=torch.uint8, device=gpu)
    push_quant_mx_(x, q, buf[2:2 + n // 32])
    rq, rs = quantize_mx_ref(x.cpu())
    assert torch.equal(q.cpu(), _u8(rq)) and torch.equal(buf[2:2 + n // 32].cpu(), rs)
    assert buf[:2].tolist() == [0xEE] * 2 and buf[2 + n // 32:].tolist() == [0xEE] * 6


@pytest.fixture(scope="module")
def gpu_mx_sources(gpu):
    """16 MX sources of the wrapping size, shared by the GPU apply tests (built once, never written)."""
    g = torch.Generator().manual_seed(21)
    n = GRID_WRAP_N
    qs, ss, dq = [], [], []
    base = torch.randn(n, generator=g) * torch.exp2(torch.randint(-6, 3, (n,), generator=g).float())
    for k in range(16):
        q, s = quantize_mx_ref(base.roll(977 * k) * (1.0 + 0.125 * k))
        qs.append(q.to(gpu))
        ss.append(s.to(gpu))
        dq.append(dequantize_mx_ref(q, s).to(torch.bfloat16).to(gpu))  # exact: dq(q) is representable in bf16
    return qs, ss, dq


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("kind", ["momentum", "adamw"])
@pytest.mark.parametrize("n", [64, GRID_WRAP_N])
def test_apply_gpu_mx_sources_bitwise_equal_bf16_sources(gpu, gpu_mx_sources, n, kind, K, scaled):
    qs, ss, dq = gpu_mx_sources
    qs, dq = [q[:n] for q in qs[:K]], [d[:n] for d in dq[:K]]
    ss = [s[:n // 32] for s in ss[:K]]
    sc = _coefs(K, gpu) if scaled else None
    want = _run_apply(kind, n, dq, gpu, scales=sc, steps=1)
    got = _run_apply(kind, n, qs, gpu, scales=sc, mx_scales=ss, steps=1)
    _assert_same(got, want, (kind, K, scaled, n))
    if n == 64:  # dq(q) really is what the bf16 tensors hold
        assert torch.equal(dq[0].float().cpu(), dequantize_mx_ref(qs[0].cpu(), ss[0].cpu()))


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, 4, 16])
def test_apply_lw_gpu_lamb_mx_sources_bitwise(gpu, gpu_mx_sources, K, scaled):
    qs, ss, dq = gpu_mx_sources
    n = LW_N
    qs, dq = [q[:n] for q in qs[:K]], [d[:n] for d in dq[:K]]
    ss = [s[:n // 32] for s in ss[:K]]
    sc = _coefs(K, gpu) if scaled else None
    for cap in (0, 1):  # one workgroup walks every chunk
        want = _run_apply("lamb", n, dq, gpu, scales=sc, layers=True, grid_cap=cap)
        got = _run_apply("lamb", n, qs, gpu, scales=sc, mx_scales=ss, layers=True, grid_cap=cap)
        _assert_same(got, want, ("lamb", K, scaled, cap))


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, 4, 16])
@pytest.mark.parametrize("n", [64, GRID_WRAP_N])
def test_multi_reduce_gpu_mx_sources_bitwise(gpu, gpu_mx_sources, n, K, scaled):
    qs, ss, dq = gpu_mx_sources
    qs, dq = [q[:n] for q in qs[:K]], [d[:n] for d in dq[:K]]
    ss = [s[:n // 32] for s in ss[:K]]
    sc = _coefs(K, gpu) if scaled else None
    for odt in (torch.float32, torch.bfloat16):
        want, got = torch.empty(n, dtype=odt, device=gpu), torch.empty(n, dtype=odt, device=gpu)
        multi_reduce_(want, dq, 0.25, scales=sc)
        multi_reduce_(got, qs, 0.25, scales=sc, mx_scales=ss)
        _assert_same([got], [want], (n, K, scaled, odt))


# ------------------------------------------------------------------ 8. GPU: ranks sharing cuda:0 through IPC
@pytest.mark.gpu
@pytest.mark.parametrize("world,stale", [(2, 1), (3, 0)])
def test_async_fp8_push_gpu_ipc_matches_replay(tmp_path, gpu, world, stale):
    mp.spawn(_worker, args=(world, _port(), 2, stale, 5, str(tmp_path), "cuda:0"), nprocs=world, join=True)
    _replay_and_check(str(tmp_path), world, stale, bf16=True)
    R = _load(str(tmp_path), world)
    assert R[0]["mem"] in ("uncached", "finegrained") and R[0]["xfer"] == "kernel"
    _assert_slot_bytes(R[0], "fp8")


@pytest.mark.gpu
def test_async_fp8_push_gpu_kernel_and_copy_transports_agree_bitwise(tmp_path, gpu):
    res = {}
    for xfer in ("kernel", "copy"):
        d = tmp_path / xfer
        d.mkdir()
        mp.spawn(_worker, args=(3, _port(), 2, 0, 4, str(d), "cuda:0", "momentum", xfer, CLIP), nprocs=3, join=True)
        _replay_and_check(str(d), 3, 0, bf16=True, clip=CLIP)
        res[xfer] = _load(str(d), 3)
    assert [r["xfer"] for r in res["kernel"]] == ["kernel"] * 3
    assert [r["xfer"] for r in res["copy"]] == ["hipMemcpyAsync"] * 3
    for a, b in zip(res["kernel"], res["copy"]):
        assert a["log"] == b["log"]
        for k in a["master"]:
            assert torch.equal(a["master"][k], b["master"][k]), k
        for ea, eb in zip(a["rec"], b["rec"]):
            assert ea["pulled"] == eb["pulled"]
            assert torch.equal(ea["weights"], eb["weights"]) and torch.equal(ea["grad"], eb["grad"])


@pytest.mark.gpu
def test_async_fp8_push_with_fp8_pull_gpu(tmp_path, gpu):
    mp.spawn(_worker, args=(2, _port(), 2, 1, 4, str(tmp_path), "cuda:0", "adamw", "auto", 0.0, "fp8", "fp8"),
             nprocs=2, join=True)
    _replay_and_check(str(tmp_path), 2, 1, kind="adamw", mx_pull=True)


@pytest.mark.gpu
def test_async_default_push_gpu_unchanged(tmp_path, gpu):
    """push_dtype="bf16" is the plane as it was: the default construction and the explicit one give
    bitwise-equal masters, weights and apply logs (SSP bound 0), the same slot bytes (bf16 elements,
    256-byte rounded), memory kind and transport."""
    res = {}
    for name, push in (("default", None), ("explicit", "bf16")):
        d = tmp_path / name
        d.mkdir()
        args = (3, _port(), 2, 0, 4, str(d), "cuda:0", "momentum", "auto", 0.0)
        mp.spawn(_worker if push else _default_worker, args=args + ((push,) if push else ()), nprocs=3, join=True)
        _replay_and_check(str(d), 3, 0, bf16=True, push="bf16")
        res[name] = _load(str(d), 3)
    for a, b in zip(res["default"], res["explicit"]):
        assert a["log"] == b["log"] and a["slot_bytes"] == b["slot_bytes"]
        assert (a["mem"], a["xfer"]) == (b["mem"], b["xfer"])
        assert a["mem"] in ("uncached", "finegrained") or a["rank"] not in a["owners"]  # rank 2 owns no memory
        assert a["xfer"] == "kernel"
        _assert_slot_bytes(a, "bf16")
        for k in a["master"]:
            assert torch.equal(a["master"][k], b["master"][k]), k
        for ea, eb in zip(a["rec"], b["rec"]):
            assert torch.equal(ea["weights"], eb["weights"]) and torch.equal(ea["grad"], eb["grad"])


def _default_worker(rank, world, port, shards, stale, steps, out_dir, device, kind, xfer, clip):
    """``_worker`` through a construction that never names push_dtype (the parent's call)."""
    import functools

    orig = AsyncPS.__init__

    @functools.wraps(orig)
    def init(self, *a, **kw):
        kw.pop("push_dtype")
        orig(self, *a, **kw)

    AsyncPS.__init__ = init
    try:
        _worker(rank, world, port, shards, stale, steps, out_dir, device, kind, xfer, clip)
    finally:
        AsyncPS.__init__ = orig
