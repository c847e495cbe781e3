"""LARS / LAMB and per-tensor decay exclusion of the fused PS apply (csrc/kernels/optim_lw.hip, and its
host twin in csrc/ops.cpp), on the CPU path (always) and on cuda:0 (``-m gpu``).

Accuracy rule: the reference is an fp64 torch implementation of the update on the same inputs, the
yardstick an fp32 torch-eager implementation of the same formulas. Per tensor, on master, states and
shadow, the kernel's max abs error against fp64 must be at most 4x the fp32-eager error against fp64
(the factor covers the different summation order: both errors grow as sqrt(n) * eps), with a floor
of two fp32 ulps of the tensor's max |w|. Measured values: profiles/optim_layerwise.md.
"""
import functools
import math

import pytest
import torch

from parameter_server_distributed_amd.ops.optim import LayerTable, OptimConfig, OptimDyn, fused_apply_

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
ALIGN = 64
STEPS = 3
EPS32 = 2.0 ** -23


def _dev(name):
    if name == "cuda":
        if not torch.cuda.is_available():
            pytest.fail("GPU test selected but no GPU visible")
        return torch.device("cuda", 0)
    return torch.device("cpu")


# (name, shape, what): the smallest tensors that exercise each edge -- 1-D sizes below / at / above the
# 64-element alignment, a chunk exactly full (8192), a chunk boundary plus a short chunk (8200), many
# chunks (3 * 8192 + 72), an all-zero gradient and all-zero weights
SHAPES = [
    ("b1", (1,), ""), ("w8192", (64, 128), ""), ("b7", (7,), ""), ("w8200", (8, 1025), ""), ("b64", (64,), ""),
    ("w24648", (8, 3081), ""), ("b65", (65,), ""), ("zg", (16, 20), "zero_grad"), ("b200", (200,), ""),
    ("zw", (12, 30), "zero_weight"),
]
SHAPES_2D = [s for s in SHAPES if len(s[1]) == 2]

CFGS = {
    "lars": dict(kind="lars", lr=1.0, momentum=0.9, weight_decay=1e-2, trust_coef=0.02, eps=1e-8),
    "lars_nesterov": dict(kind="lars", lr=1.0, momentum=0.9, nesterov=True, dampening=0.0, weight_decay=1e-2,
                          trust_coef=0.02),
    "lamb": dict(kind="lamb", lr=0.01, weight_decay=1e-2, eps=1e-6),
    "momentum_x1d": dict(kind="momentum", lr=0.1, momentum=0.9, weight_decay=1e-2, exclude_1d=True),
    "adamw_x1d": dict(kind="adamw", lr=1e-2, weight_decay=1e-2, exclude_1d=True),
}


def _layout(shapes):
    lay, off = [], 0
    for name, shape, what in shapes:
        n = math.prod(shape)
        lay.append((name, off, n, len(shape), what))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return lay, off


def _table(lay, n, cfg, dev, lo=0, hi=None):
    hi = n if hi is None else hi
    flat = [(o, k, d) for (_n, o, k, d, _w) in lay]
    return LayerTable.for_range(flat, lo, hi, cfg.exclude_1d, dev, ALIGN)


@functools.lru_cache(maxsize=None)
def _inputs(shapes_key, K, bf16):
    """Weights and STEPS x K gradient sources of one layout (CPU, shared and never modified)."""
    shapes = SHAPES if shapes_key == "all" else SHAPES_2D
    lay, n = _layout(shapes)
    gen = torch.Generator().manual_seed(1234 + K + 100 * int(bf16))
    w = torch.zeros(n)
    srcs = [[torch.zeros(n) for _ in range(K)] for _ in range(STEPS)]
    for name, o, k, _d, what in lay:
        if what != "zero_weight":  # |w| in [0.5, 1.5]: the tolerance floor is in ulps of max |w|
            w[o:o + k] = (torch.rand(k, generator=gen) + 0.5) * (torch.randint(0, 2, (k,), generator=gen) * 2 - 1)
        if what != "zero_grad":
            for s in range(STEPS):
                for q in range(K):
                    srcs[s][q][o:o + k] = torch.randn(k, generator=gen) * 0.05
    dt = torch.bfloat16 if bf16 else torch.float32
    return lay, n, w, [[g.to(dt) for g in step] for step in srcs]


def _ref_step(cfg, lay, w, srcs, s1, s2, step, dt):
    """One step of the update in dtype ``dt`` (fp64: the reference; fp32: the eager yardstick), per
    tensor, exactly as the issue states it. Every hyper-parameter and every scalar derived from one
    (1 - beta, the bias corrections) is held in ``dt`` too: the fp32 yardstick is fp32 throughout, like
    the kernel, whose betas are fp32 (1 - beta2^t cancels, so beta2's fp32 rounding alone moves the
    Adam step by ~1e-5 relative: an error of the number format, not of the summation order).
    Returns the ratios; updates w / s1 / s2 in place."""
    K = len(srcs)
    g = torch.zeros_like(w)
    for s in srcs:
        g = g + s.to(dt)
    g = g * torch.tensor(1.0 / K, dtype=dt)
    S = lambda x: torch.tensor(float(x), dtype=dt)  # noqa: E731
    b1, b2, mom = S(cfg.beta1), S(cfg.beta2), S(cfg.momentum)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    ratios = []
    for _name, o, k, d, _what in lay:
        sl = slice(o, o + k)
        wt, gt = w[sl], g[sl]
        excl = cfg.exclude_1d and d <= 1
        wd = cfg.weight_decay * (0.0 if excl else 1.0)
        r = torch.ones((), dtype=dt)
        if cfg.kind == "lars":
            wn, gn = wt.norm(), gt.norm()
            if not excl and wn > 0 and gn > 0:
                r = cfg.trust_coef * wn / (gn + wd * wn + cfg.eps)
            dd = r * (gt + wd * wt)
            buf = dd.clone() if step == 1 else mom * s1[sl] + (1 - S(cfg.dampening)) * dd
            s1[sl] = buf
            w[sl] = wt - cfg.lr * (dd + mom * buf if cfg.nesterov else buf)
        elif cfg.kind == "lamb":
            m = b1 * s1[sl] + (1 - b1) * gt
            v = b2 * s2[sl] + (1 - b2) * gt * gt
            s1[sl], s2[sl] = m, v
            u = (m / bc1) / (v.sqrt() / bc2.sqrt() + cfg.eps) + wd * wt
            wn, un = wt.norm(), u.norm()
            if not excl and wn > 0 and un > 0:
                r = wn / un
            w[sl] = wt - cfg.lr * r * u
        elif cfg.kind == "momentum":
            gg = gt + wd * wt
            buf = gg.clone() if step == 1 else mom * s1[sl] + (1 - S(cfg.dampening)) * gg
            s1[sl] = buf
            w[sl] = wt - cfg.lr * (gg + mom * buf if cfg.nesterov else buf)
        else:  # adamw
            wt = wt * (1 - S(cfg.lr) * S(wd))
            m = b1 * s1[sl] + (1 - b1) * gt
            v = b2 * s2[sl] + (1 - b2) * gt * gt
            s1[sl], s2[sl] = m, v
            w[sl] = wt - (S(cfg.lr) / bc1) * (m / (v.sqrt() / bc2.sqrt() + cfg.eps))
        ratios.append(float(r))
    return ratios


@functools.lru_cache(maxsize=None)
def _trajectories(cfg_name, K, bf16):
    """fp64 reference and fp32 eager yardstick after each step: [(w, s1, s2)] per dtype (computed once)."""
    cfg = OptimConfig(**CFGS[cfg_name])
    lay, n, w0, srcs = _inputs("all", K, bf16)
    out = {}
    for dt in (torch.float64, torch.float32):
        w, s1, s2 = w0.to(dt, copy=True), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
        traj = []
        for step in range(1, STEPS + 1):
            ratios = _ref_step(cfg, lay, w, srcs[step - 1], s1, s2, step, dt)
            traj.append((w.clone(), s1.clone(), s2.clone(), ratios))
        out[dt] = traj
    return out


def _state(cfg, n, dev):
    s1 = torch.zeros(n, device=dev) if cfg.num_states >= 1 else None
    s2 = torch.zeros(n, device=dev) if cfg.num_states >= 2 else None
    return s1, s2


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("cfg_name", list(CFGS))
def test_layerwise_matches_fp64_within_4x_fp32_eager(devname, cfg_name, K, bf16):
    dev = _dev(devname)
    cfg = OptimConfig(**CFGS[cfg_name])
    lay, n, w0, srcs = _inputs("all", K, bf16)
    traj = _trajectories(cfg_name, K, bf16)
    lt = _table(lay, n, cfg, dev)
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
    pad = torch.ones(n, dtype=torch.bool)
    for _name, o, k, _d, _w in lay:
        pad[o:o + k] = False
    report, bad = [], []
    for step in range(1, STEPS + 1):
        prev = traj[torch.float64][step - 2][0] if step > 1 else w0.double()
        fused_apply_(cfg, dyn, w, [g.to(dev) for g in srcs[step - 1]], s1, s2, shadow, layers=lt)
        w64, a64, b64, r64 = traj[torch.float64][step - 1]
        w32, a32, b32, _ = traj[torch.float32][step - 1]
        got = {"master": w.cpu().double(), "shadow": shadow.float().cpu().double()}
        ref = {"master": w64, "shadow": w64}
        eag = {"master": w32.double(), "shadow": w32.to(torch.bfloat16).double()}
        if s1 is not None:
            got["state1"], ref["state1"], eag["state1"] = s1.cpu().double(), a64, a32.double()
        if s2 is not None:
            got["state2"], ref["state2"], eag["state2"] = s2.cpu().double(), b64, b32.double()
        assert all(torch.isfinite(v).all() for v in got.values())
        assert not got["master"][pad].any() and not got["shadow"][pad].any(), "alignment padding must stay zero"
        if cfg.kind in ("lars", "lamb"):
            ratio = lt.ratio.cpu()
            for ti, (name, _o, _k, d, what) in enumerate(lay):
                assert abs(float(ratio[ti]) - r64[ti]) <= 1e-5 * abs(r64[ti]), (name, float(ratio[ti]), r64[ti])
                if d <= 1 or (what == "zero_weight" and step == 1) or (what == "zero_grad" and cfg.kind == "lars"):
                    assert float(ratio[ti]) == 1.0, (name, step, float(ratio[ti]))
        for name, o, k, _d, _what in lay:
            sl = slice(o, o + k)
            floor = 2 * EPS32 * float(torch.maximum(w64[sl].abs().max(), prev[sl].abs().max()))
            for key in got:
                ek = float((got[key][sl] - ref[key][sl]).abs().max())
                ee = float((eag[key][sl] - ref[key][sl]).abs().max())
                line = f"step {step} {name:7s} {key:7s} kernel {ek:.3e} eager {ee:.3e} bound {max(4 * ee, floor):.3e}"
                report.append(line)
                if ek > max(4 * ee, floor):
                    bad.append(line)
    worst = {}
    for line in report:  # one summary line per quantity: the worst kernel / bound of the run
        f = line.split()
        worst[f[3]] = max(worst.get(f[3], (0.0, "")), (float(f[5]) / (float(f[9]) or 1e-300), line))
    for key, (q, line) in worst.items():
        print(f"LWERR {devname} {cfg_name} K={K} {'bf16' if bf16 else 'fp32'} worst {key}: err/bound {q:.3f} | {line}")
    assert not bad, "kernel error above 4x the fp32-eager error (and the 2-ulp floor):\n" + "\n".join(bad)


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("kind", ["lars", "lamb", "momentum", "adamw"])
def test_excluded_tensor_with_zero_gradient_is_untouched(devname, kind):
    """1-D tensors take no weight decay: with a zero gradient (and, for lamb, zero state: the first
    step) nothing moves them, bit for bit, while a 2-D tensor is decayed."""
    dev = _dev(devname)
    cfg = OptimConfig(kind, lr=0.1, momentum=0.9, weight_decay=0.1, exclude_1d=True)
    lay, n, w0, _ = _inputs("all", 1, False)
    lt = _table(lay, n, cfg, dev)
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0)
    fused_apply_(cfg, dyn, w, torch.zeros(n, device=dev), s1, s2, None, layers=lt)
    got = w.cpu()
    for name, o, k, d, what in lay:
        same = torch.equal(got[o:o + k], w0[o:o + k])
        assert same == (d <= 1 or what == "zero_weight"), (name, same)
    assert torch.isfinite(got).all()


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("kind", ["lars", "lamb"])
def test_zero_norm_tensors_take_ratio_one_and_stay_finite(devname, kind):
    dev = _dev(devname)
    cfg = OptimConfig(kind, lr=0.1, momentum=0.9, weight_decay=0.0)
    lay, n, w0, srcs = _inputs("all", 1, False)
    lt = _table(lay, n, cfg, dev)
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    fused_apply_(cfg, OptimDyn(dev, lr=cfg.lr), w, srcs[0][0].to(dev), s1, s2, None, layers=lt)
    ratio = lt.ratio.cpu()
    for ti, (name, _o, _k, _d, what) in enumerate(lay):
        if what:  # ||g|| = 0 (with wd = 0 also ||u|| = 0 for lamb) or ||w|| = 0
            assert float(ratio[ti]) == 1.0, (name, float(ratio[ti]))
    assert torch.isfinite(ratio).all() and torch.isfinite(w).all()
    for t in (s1, s2):
        assert t is None or torch.isfinite(t).all()


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("kind", ["momentum", "adamw"])
def test_exclude_1d_without_1d_tensors_equals_flat_kernel_bitwise(devname, kind, bf16):
    """The segmented apply runs the flat kernel's update: on a layout with no 1-D tensor (every
    wd_mult 1) it must reproduce ``fused_apply_`` without a table bit for bit."""
    dev = _dev(devname)
    base = dict(kind=kind, lr=0.05, momentum=0.9, nesterov=kind == "momentum", weight_decay=1e-2)
    seg, flat = OptimConfig(**base, exclude_1d=True), OptimConfig(**base)
    K = 3
    lay, n, w0, srcs = _inputs("2d", K, bf16)
    lt = _table(lay, n, seg, dev)
    res = []
    for cfg, layers in ((seg, lt), (flat, None)):
        w = w0.to(dev, copy=True)
        s1, s2 = _state(cfg, n, dev)
        sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
        dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
        for step in range(STEPS):
            fused_apply_(cfg, dyn, w, [g.to(dev) for g in srcs[step]], s1, s2, sh, layers=layers)
        res.append([t.cpu() for t in (w, s1, s2, sh.float()) if t is not None])
    for a, b in zip(*res):
        assert torch.equal(a, b)


def _run(cfg, dev, lay, n, w0, srcs, grid_cap=0, cut=None):
    """STEPS steps on the whole buffer, or (``cut``: a tensor start) on two ranges with a table each."""
    K = len(srcs[0])
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    ranges = [(0, n)] if cut is None else [(0, cut), (cut, n)]
    tabs = [_table(lay, n, cfg, dev, lo, hi) for lo, hi in ranges]
    dyns = [OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K) for _ in ranges]
    for step in range(STEPS):
        gs = [g.to(dev) for g in srcs[step]]
        for (lo, hi), lt, dyn in zip(ranges, tabs, dyns):
            nv = lambda t: None if t is None else t.narrow(0, lo, hi - lo)  # noqa: E731
            fused_apply_(cfg, dyn, nv(w), [nv(g) for g in gs], nv(s1), nv(s2), nv(sh), layers=lt, grid_cap=grid_cap)
    return [t.cpu() for t in (w, s1, s2, sh.float()) if t is not None]


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("cfg_name", ["lars", "lamb", "momentum_x1d"])
def test_result_is_invariant_bitwise(devname, cfg_name):
    """Chunks are numbered from the segment start and every sum has a fixed order: the same call
    twice, grid_cap 0 and 2, and the buffer applied as two ranges cut at a tensor start all agree."""
    dev = _dev(devname)
    cfg = OptimConfig(**CFGS[cfg_name])
    lay, n, w0, srcs = _inputs("all", 3, True)
    base = _run(cfg, dev, lay, n, w0, srcs)
    cut = next(o for (name, o, _k, _d, _w) in lay if name == "w24648")
    for other in (_run(cfg, dev, lay, n, w0, srcs), _run(cfg, dev, lay, n, w0, srcs, grid_cap=2),
                  _run(cfg, dev, lay, n, w0, srcs, cut=cut)):
        for a, b in zip(base, other):
            assert torch.equal(a, b)


# ------------------------------------------------------------------ interface
def test_config_resolves_exclude_1d_and_states():
    assert OptimConfig("lars").exclude_1d is True and OptimConfig("lamb").exclude_1d is True
    assert OptimConfig("momentum").exclude_1d is False and OptimConfig("lars", exclude_1d=False).exclude_1d is False
    assert OptimConfig("lars").num_states == 1 and OptimConfig("lamb").num_states == 2
    assert OptimConfig("lars").code == 4 and OptimConfig("lamb").code == 5
    assert OptimConfig("lars").trust_coef == 0.001


def test_fused_apply_requires_or_rejects_layers():
    n = 128
    w, g, s1, s2 = torch.ones(n), torch.ones(n), torch.zeros(n), torch.zeros(n)
    dyn = OptimDyn(torch.device("cpu"), lr=0.1)
    for cfg in (OptimConfig("lars"), OptimConfig("lamb"), OptimConfig("momentum", exclude_1d=True)):
        with pytest.raises(ValueError, match="layers"):
            fused_apply_(cfg, dyn, w, g, s1, s2)
    lt = LayerTable([(0, 100, 2)], n, False, "cpu")
    with pytest.raises(ValueError, match="no layer table"):
        fused_apply_(OptimConfig("momentum"), dyn, w, g, s1, None, layers=lt)
    with pytest.raises(ValueError):  # a tensor off the 64-element grid
        LayerTable([(0, 10, 1), (32, 10, 1)], n, True, "cpu")
    with pytest.raises(ValueError):  # a table built for another range length
        fused_apply_(OptimConfig("lars", exclude_1d=False), dyn, torch.ones(64), torch.ones(64), torch.zeros(64),
                     layers=lt)


def test_collective_plane_rejects_layerwise_and_names_the_async_plane():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=16)
    for cfg in (OptimConfig("lars"), OptimConfig("lamb"), OptimConfig("momentum", exclude_1d=True)):
        with pytest.raises(ValueError, match="async"):
            CollectivePS(spec.model, cfg)


def test_async_push_semantics_rejects_lamb():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.parallel.async_ps import AsyncPS

    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=16)
    with pytest.raises(ValueError, match="push"):
        AsyncPS(spec.model, OptimConfig("lamb"), semantics="push", param_dtype=torch.float32)


def test_ps_cli_accepts_lamb_and_trust_coef():
    from parameter_server_distributed_amd.cli.parameter_server import build_parser, optim_from_args

    a = build_parser().parse_intermixed_args(["--optimizer", "lamb", "--trust-coef", "0.002"])
    cfg = optim_from_args(a)
    assert (cfg.kind, cfg.trust_coef, cfg.exclude_1d) == ("lamb", 0.002, True)
    a = build_parser().parse_intermixed_args(["--optimizer", "lars", "--no-exclude-1d"])
    assert optim_from_args(a).exclude_1d is False and optim_from_args(a).momentum == 0.9
