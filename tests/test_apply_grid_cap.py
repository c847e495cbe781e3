"""The flat fused apply (csrc/kernels/optim.hip fused_apply_kernel) under a workgroup cap.

The launcher's grid is min(ceil(n / 8 / 256), 2048) workgroups and ``grid_cap`` bounds it from above; the
async engine's background apply runs with a cap of 512, which changes the launch only above
512 * 256 * 8 = 1,048,576 elements. Both sizes here need more than 512 workgroups uncapped (515 with
an odd number of extra vector rounds, and 1221), and both leave an n % 8 tail.

  * grid independence: the update is elementwise, so every element's arithmetic is the same whichever
    workgroup performs it -- master, states and the bf16 shadow after two steps are bit-equal for
    caps 1, 7, 512 and the uncapped launch;
  * the uncapped launch against an fp64 replay of ``opt_update`` under the rule of
    tests/test_grad_clip.py (kernel error <= max(4 x the fp32-eager error, two fp32 ulps of max |w|));
  * 64 guard elements behind master, states and shadow keep their sentinel at every cap.
"""
import functools

import pytest
import torch
from test_grad_clip import CFGS as CLIP_CFGS
from test_grad_clip import EPS32, SCALE_VALUES, _ref_step, _scale_tensors

from parameter_server_distributed_amd.ops import dequantize_mx_ref, quantize_mx_ref
from parameter_server_distributed_amd.ops.optim import OptimConfig, OptimDyn, fused_apply_

CAP_BINDS = 512 * 256 * 8  # elements one capped launch covers without striding
SIZES = [CAP_BINDS + 8 * 256 * 3 + 5, 2_500_003]
N_MAX = max(SIZES)
CAPS = (1, 7, 512)
STEPS = 2  # the `first` branch, then the stateful one
KMAX = 3
GUARD = 64
# eps of the Adam kinds as in tests/test_grad_clip.py (CFGS there: a small eps makes the comparison a
# matter of luck at |g| ~ eps, not of the update's rounding)
CFGS = {
    "sgd": dict(kind="sgd", lr=0.1, weight_decay=1e-2),
    "momentum": CLIP_CFGS["momentum"],
    "adam": dict(kind="adam", lr=1e-2, weight_decay=1e-2, eps=1e-3),
    "adamw": CLIP_CFGS["adamw"],
}
SENTINEL = {torch.float32: 12345.0, torch.bfloat16: -777.0}


@functools.lru_cache(maxsize=None)
def _weights():
    gen = torch.Generator().manual_seed(99)
    return (torch.rand(N_MAX, generator=gen) + 0.5) * (torch.randint(0, 2, (N_MAX,), generator=gen) * 2 - 1)


@functools.lru_cache(maxsize=None)
def _sources(src):
    """STEPS x KMAX gradient sources of the largest size (CPU, shared, never modified); a smaller
    case takes prefixes. "mx": the construction of tests/test_push_fp8.py gpu_mx_sources -- one base,
    rolled and rescaled per source, as (e4m3 payload, E8M0 bytes, dequantised fp32)."""
    gen = torch.Generator().manual_seed(2024 + len(src))
    if src != "mx":
        dt = torch.bfloat16 if src == "bf16" else torch.float32
        return [[(torch.randn(N_MAX, generator=gen) * 0.05).to(dt) for _ in range(KMAX)] for _ in range(STEPS)]
    n = N_MAX // 32 * 32
    base = torch.randn(n, generator=gen) * torch.exp2(torch.randint(-6, 3, (n,), generator=gen).float())
    out = []
    for s in range(STEPS):
        step = []
        for k in range(KMAX):
            q, sc = quantize_mx_ref(base.roll(977 * (KMAX * s + k)) * (1.0 + 0.125 * k))
            step.append((q, sc, dequantize_mx_ref(q, sc)))
        out.append(step)
    return out


def _case_inputs(src, n, K):
    """(payloads per step, mx scale bytes per step or None, the fp32/bf16 values the update sees)."""
    S = _sources(src)
    if src != "mx":
        vals = [[g[:n] for g in step[:K]] for step in S]
        return vals, None, vals
    return ([[q[:n] for (q, _s, _d) in step[:K]] for step in S],
            [[s[:n // 32] for (_q, s, _d) in step[:K]] for step in S],
            [[d[:n] for (_q, _s, d) in step[:K]] for step in S])


def _guarded(n, dtype, dev, fill=None):
    t = torch.full((n + GUARD,), SENTINEL[dtype], dtype=dtype, device=dev)
    if fill is not None:
        t[:n] = fill
    return t


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _run(cfg, dev, n, K, grads, mxs, scales, cap, w0):
    """Two steps at one cap; the guarded buffers (master, state1, state2, shadow; None where unused)
    after each step."""
    bufs = [_guarded(n, torch.float32, dev, w0),
            _guarded(n, torch.float32, dev, 0.0) if cfg.num_states >= 1 else None,
            _guarded(n, torch.float32, dev, 0.0) if cfg.num_states >= 2 else None,
            _guarded(n, torch.bfloat16, dev, 0.0)]
    m, s1, s2, sh = [b[:n] if b is not None else None for b in bufs]
    dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
    per_step = []
    for step in range(STEPS):
        fused_apply_(cfg, dyn, m, grads[step], s1, s2, sh, grid_cap=cap, scales=scales,
                     mx_scales=mxs[step] if mxs is not None else None)
        per_step.append([b.clone() if b is not None else None for b in bufs])
    assert dyn.step == STEPS
    return per_step


@pytest.mark.gpu
@pytest.mark.parametrize("scaled", [False, True], ids=["plain", "scales"])
@pytest.mark.parametrize("K", [1, KMAX])
@pytest.mark.parametrize("src", ["bf16", "fp32", "mx"])
@pytest.mark.parametrize("kind", list(CFGS))
@pytest.mark.parametrize("n", SIZES)
def test_capped_flat_apply_is_grid_independent_and_matches_fp64(gpu, n, kind, src, K, scaled):
    if src == "mx":
        n = n // 32 * 32  # MX sources come in whole 32-element blocks
    assert (n + 8 * 256 - 1) // (8 * 256) > max(CAPS), "every cap must bind"
    cfg = OptimConfig(**CFGS[kind])
    pay, mxs, vals = _case_inputs(src, n, K)
    w0 = _weights()[:n]
    cvals = SCALE_VALUES[1:1 + K] if scaled else [1.0] * K  # 0.25, 0.731, 0.5: none of them 1
    scales = _scale_tensors(cvals, gpu) if scaled else None
    grads = [[g.to(gpu) for g in step] for step in pay]
    mxd = [[s.to(gpu) for s in step] for step in mxs] if mxs is not None else None
    names = ["master", "state1", "state2", "shadow"]

    base = _run(cfg, gpu, n, K, grads, mxd, scales, 0, w0.to(gpu))
    # ---- the uncapped launch against fp64, yardstick fp32 eager (the rule of tests/test_grad_clip.py)
    lay = [("flat", 0, n, 1, "")]
    c32 = torch.tensor(cvals, dtype=torch.float32)
    traj = {}
    for dt in (torch.float64, torch.float32):
        w, a, b = w0.to(dt, copy=True), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
        traj[dt] = []
        for step in range(1, STEPS + 1):
            _ref_step(cfg, lay, w, vals[step - 1], c32, a, b, step, dt)
            traj[dt].append((w.clone(), a.clone(), b.clone()))
    bad, worst = [], (0.0, "")
    for step in range(STEPS):
        prev = traj[torch.float64][step - 1][0] if step else w0.double()
        w64, a64, b64 = traj[torch.float64][step]
        w32, a32, b32 = traj[torch.float32][step]
        ref = {"master": w64, "state1": a64, "state2": b64, "shadow": w64}
        eag = {"master": w32.double(), "state1": a32.double(), "state2": b32.double(),
               "shadow": w32.to(torch.bfloat16).double()}
        floor = 2 * EPS32 * float(torch.maximum(w64.abs().max(), prev.abs().max()))
        for name, buf in zip(names, base[step]):
            if buf is None:
                continue
            got = buf[:n].float().cpu().double()
            assert torch.isfinite(got).all()
            ek = float((got - ref[name]).abs().max())
            ee = float((eag[name] - ref[name]).abs().max())
            bound = max(4 * ee, floor)
            line = f"step {step + 1} {name:7s} kernel {ek:.3e} eager {ee:.3e} bound {bound:.3e}"
            worst = max(worst, (ek / bound, line))
            if ek > bound:
                bad.append(line)
    tag = f"n={n} {kind} {src} K={K} {'scales' if scaled else 'plain'}"
    print(f"CAPERR {tag} worst err/bound {worst[0]:.3f} | {worst[1]}")
    assert not torch.equal(base[-1][0][:n].cpu(), w0), "the apply must move the master"

    # ---- every cap: the bits of the uncapped launch, guards untouched
    for cap in (0,) + CAPS:
        run = base if cap == 0 else _run(cfg, gpu, n, K, grads, mxd, scales, cap, w0.to(gpu))
        for step in range(STEPS):
            for name, got, want in zip(names, run[step], base[step]):
                if got is None:
                    continue
                assert torch.equal(_bits(got[:n]), _bits(want[:n])), (cap, step + 1, name)
                guard = got[n:]
                assert guard.numel() == GUARD and bool((guard == SENTINEL[got.dtype]).all()), \
                    f"cap {cap} step {step + 1}: {name} written past n"
    assert not bad, "kernel error above 4x the fp32-eager error (and the 2-ulp floor):\n" + "\n".join(bad)
