"""Global-norm gradient clipping: the norm pass (csrc/kernels/clip.hip), the per-source scales of the
multi-source consumers (optim.hip, optim_lw.hip, reduce_pack.hip) and their host twins in
csrc/ops.cpp, on the CPU path (always) and on cuda:0 (``-m gpu``).

Norm tolerance: an element passes through at most 32 sequential (4 vectors of 8 per lane; the n % 8
tail goes to lane 255, which then holds at most 3 vectors) and 9 tree (6 butterfly levels + 3 wave
sums) fp32 additions of non-negative terms; the products are exact inside the fma and the finalize
adds in fp64. That is at most 41 * 2^-24 relative on the sum, the square root halves it, plus the
roundings of the sqrt and of the fp32 result: (41 / 2 + 2) * 2^-24 < 12 * 2^-23 relative on n.

Scaled-apply accuracy rule (that of tests/test_optim_layerwise.py): the reference is an fp64 torch
implementation with the same fp32 scale values, the yardstick an fp32 torch-eager one; per tensor, on
master, states and shadow, the kernel's max abs error against fp64 is at most 4x the yardstick's,
with a floor of two fp32 ulps of the tensor's max |w|.
"""
import functools
import math

import pytest
import torch

from parameter_server_distributed_amd import native
from parameter_server_distributed_amd.ops.optim import (LayerTable, OptimConfig, OptimDyn, clip_chunks, fused_apply_,
                                                        grad_clip_coef_, multi_reduce_)

DEVICES = [pytest.param("cpu", id="cpu"), pytest.param("cuda", id="gpu", marks=pytest.mark.gpu)]
ALIGN = 64
STEPS = 3
EPS32 = 2.0 ** -23
NORM_RTOL = 12 * 2.0 ** -23


def _dev(name):
    if name == "cuda":
        if not torch.cuda.is_available():
            pytest.fail("GPU test selected but no GPU visible")
        return torch.device("cuda", 0)
    return torch.device("cpu")


# ------------------------------------------------------------------ 1. the norm kernel
NORM_SIZES = [1, 7, 8, 64, 8191, 8192, 8193, 8200, 3 * 8192 + 72]
WRAP_N = 2048 * 8192 + 100  # 2049 chunks: the grid-stride loop of the 2048-workgroup grid wraps


@functools.lru_cache(maxsize=None)
def _norm_input(n, bf16, what=""):
    """(stored values on the CPU, fp64 norm of exactly those values); shared, never modified."""
    gen = torch.Generator().manual_seed(77 + n % 1000 + int(bf16))
    g = torch.zeros(n) if what == "zero" else torch.randn(n, generator=gen) * 0.05
    g = g.to(torch.bfloat16 if bf16 else torch.float32)
    return g, float(g.double().square().sum().sqrt())


def _clip(g, clip_norm, grid_cap=0):
    out = torch.full((64,), -7.0, dtype=torch.float32, device=g.device)
    part = torch.full((clip_chunks(g.numel()),), float("nan"), dtype=torch.float32, device=g.device)  # never zeroed
    grad_clip_coef_(g, clip_norm, out, part, grid_cap)
    return out.cpu()


def _coef32(clip_norm, n_kernel):
    """min(1, clip_norm / (n + 1e-6)) in fp32 from the kernel's own n."""
    q = torch.tensor(clip_norm, dtype=torch.float32) / (torch.tensor(n_kernel, dtype=torch.float32) +
                                                        torch.tensor(1e-6, dtype=torch.float32))
    return float(torch.clamp(q, max=1.0))


def _check_norm(out, ref, clip_norm):
    c, n = float(out[0]), float(out[1])
    print(f"CLIPNORM n {n!r} ref {ref!r} rel {abs(n - ref) / max(ref, 1e-300):.3e} bound {NORM_RTOL:.3e} c {c!r}")
    assert abs(n - ref) <= NORM_RTOL * ref
    want = _coef32(clip_norm, n)
    assert abs(c - want) <= EPS32 * want, (c, want)
    assert not out[2:].ne(-7.0).any(), "the pass writes out[0] and out[1] only"
    return c, n


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("n", NORM_SIZES)
def test_norm_matches_fp64_and_coef_follows_it(devname, n, bf16):
    dev = _dev(devname)
    g, ref = _norm_input(n, bf16)
    gd = g.to(dev)
    # clip_norm below the norm (the push is clipped) and above it (c = 1 exactly)
    c_lo, _ = _check_norm(_clip(gd, 0.5 * ref), ref, 0.5 * ref)
    assert 0.49 < c_lo < 0.51
    c_hi, _ = _check_norm(_clip(gd, 2.0 * ref), ref, 2.0 * ref)
    assert c_hi == 1.0
    outs = [_clip(gd, 0.5 * ref, cap) for cap in (1, 3, 0)]
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2]), "bits must not depend on grid_cap"


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_norm_of_zero_buffer_gives_coef_one(devname, bf16):
    dev = _dev(devname)
    g, _ = _norm_input(8200, bf16, "zero")
    out = _clip(g.to(dev), 1.0)
    assert float(out[1]) == 0.0 and float(out[0]) == 1.0


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_norm_grid_stride_wraps_at_2049_chunks(devname, bf16):
    dev = _dev(devname)
    g, ref = _norm_input(WRAP_N, bf16)
    gd = g.to(dev)
    base = _clip(gd, 1.0)
    _check_norm(base, ref, 1.0)
    for cap in (1, 3):
        assert torch.equal(base, _clip(gd, 1.0, cap))


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_nan_in_the_buffer_gives_nan_norm(devname, bf16):
    dev = _dev(devname)
    g = _norm_input(8200, bf16)[0].clone()
    g[8195] = float("nan")  # in the short last chunk
    out = _clip(g.to(dev), 1.0)
    assert math.isnan(float(out[1])) and math.isnan(float(out[0]))
    g = _norm_input(8193, bf16)[0].clone()
    g[8192] = float("inf")  # the n % 8 tail; torch: an infinite norm gives coefficient 0
    out = _clip(g.to(dev), 1.0)
    assert math.isinf(float(out[1])) and float(out[0]) == 0.0


def test_cpu_and_gpu_norm_paths_share_one_summation_order():
    """The host twin adds in the device order; here: its chunk partials are those of a plain fp32
    re-implementation of that order (lanes, butterfly, waves)."""
    g, _ = _norm_input(8200, False)
    part = torch.zeros(clip_chunks(8200))
    grad_clip_coef_(g, 1.0, torch.zeros(64), part)
    x = g[:8192].view(4, 256, 8).permute(1, 0, 2).reshape(256, 32)  # lane l: vectors l, l + 256, ...
    acc = torch.zeros(256)
    for j in range(32):  # fmaf(x, x, acc): the product is exact in fp64, one rounding to fp32
        acc = (acc.double() + x[:, j].double() ** 2).float()
    w = acc.view(4, 64)
    for m in (32, 16, 8, 4, 2, 1):
        w = w + w[:, torch.arange(64) ^ m]
    want = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
    assert float(part[0]) == float(want)


@pytest.mark.gpu
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
def test_gpu_norm_equals_the_host_twin_bitwise(bf16):
    dev = _dev("cuda")
    for n in (8191, 3 * 8192 + 72):
        g, ref = _norm_input(n, bf16)
        assert torch.equal(_clip(g, 0.5 * ref), _clip(g.to(dev), 0.5 * ref))


# ------------------------------------------------------------------ 2. / 3. the scaled apply
# the layout list of tests/test_optim_layerwise.py
SHAPES = [
    ("b1", (1,), ""), ("w8192", (64, 128), ""), ("b7", (7,), ""), ("w8200", (8, 1025), ""), ("b64", (64,), ""),
    ("w24648", (8, 3081), ""), ("b65", (65,), ""), ("zg", (16, 20), "zero_grad"), ("b200", (200,), ""),
    ("zw", (12, 30), "zero_weight"),
]

# eps of the Adam-type kinds: the kernel adds the sources with one fma each, the eager yardstick with
# a multiply and an add, so the two round the K-source sum g differently (by ~K * 2^-24 * sum |c g|,
# ~1e-9 here). The Adam direction g / (|g| + eps) has slope up to 1 / eps in g: at |g| < eps = 1e-6 an
# element turns that 1e-9 into 1e-3 of the step, and which of the two implementations is unluckier
# at the one or two such elements of a tensor decides a max-error comparison (the rule was made for
# a kernel and a yardstick that add in the same order). eps = 1e-3 bounds the slope, so the rule
# compares rounding of the whole update again and not the luck at |g| ~ eps.
CFGS = {
    "momentum": dict(kind="momentum", lr=0.1, momentum=0.9, weight_decay=1e-2),
    "adamw": dict(kind="adamw", lr=1e-2, weight_decay=1e-2, eps=1e-3),
    "lars": dict(kind="lars", lr=1.0, momentum=0.9, weight_decay=1e-2, trust_coef=0.02, eps=1e-8),
    "lamb": dict(kind="lamb", lr=0.01, weight_decay=1e-2, eps=1e-3),
    "adamw_x1d": dict(kind="adamw", lr=1e-2, weight_decay=1e-2, eps=1e-3, exclude_1d=True),
}
SCALE_VALUES = [1.0, 0.25, 0.731, 0.5, 0.9990234375, 0.0625, 0.333, 1.0, 0.87, 0.125, 0.6, 0.05, 0.999, 0.42, 0.75, 0.2]


def _layout(shapes):
    lay, off = [], 0
    for name, shape, what in shapes:
        n = math.prod(shape)
        lay.append((name, off, n, len(shape), what))
        off += (n + ALIGN - 1) // ALIGN * ALIGN
    return lay, off


@functools.lru_cache(maxsize=None)
def _inputs(K, bf16):
    """Weights, STEPS x K gradient sources and K fp32 scales (CPU, shared and never modified)."""
    lay, n = _layout(SHAPES)
    gen = torch.Generator().manual_seed(4321 + K + 100 * int(bf16))
    w = torch.zeros(n)
    srcs = [[torch.zeros(n) for _ in range(K)] for _ in range(STEPS)]
    for name, o, k, _d, what in lay:
        if what != "zero_weight":
            w[o:o + k] = (torch.rand(k, generator=gen) + 0.5) * (torch.randint(0, 2, (k,), generator=gen) * 2 - 1)
        if what != "zero_grad":
            for s in range(STEPS):
                for q in range(K):
                    srcs[s][q][o:o + k] = torch.randn(k, generator=gen) * 0.05
    dt = torch.bfloat16 if bf16 else torch.float32
    scales = torch.tensor(SCALE_VALUES[:K], dtype=torch.float32)
    return lay, n, w, [[g.to(dt) for g in step] for step in srcs], scales


def _ref_step(cfg, lay, w, srcs, scales, s1, s2, step, dt):
    """One step in dtype ``dt`` (fp64: the reference; fp32: the eager yardstick) on the clipped sum
    ``(1 / K) sum_k c_k g_k``; every scalar is held in ``dt``. Updates w / s1 / s2 in place."""
    K = len(srcs)
    g = torch.zeros_like(w)
    for c, s in zip(scales, srcs):
        g = g + c.to(dt) * s.to(dt)
    g = g * torch.tensor(1.0 / K, dtype=dt)
    S = lambda x: torch.tensor(float(x), dtype=dt)  # noqa: E731
    b1, b2, mom = S(cfg.beta1), S(cfg.beta2), S(cfg.momentum)
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
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
            w[sl] = wt - cfg.lr * buf
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
            w[sl] = wt - cfg.lr * buf
        elif cfg.kind == "sgd":
            w[sl] = wt - cfg.lr * (gt + wd * wt)
        else:  # adam (decay in the gradient) / adamw (decoupled decay)
            if cfg.kind == "adam":
                gt = gt + wd * wt
            else:
                wt = wt * (1 - S(cfg.lr) * S(wd))
            m = b1 * s1[sl] + (1 - b1) * gt
            v = b2 * s2[sl] + (1 - b2) * gt * gt
            s1[sl], s2[sl] = m, v
            w[sl] = wt - (S(cfg.lr) / bc1) * (m / (v.sqrt() / bc2.sqrt() + cfg.eps))


@functools.lru_cache(maxsize=None)
def _trajectories(cfg_name, K, bf16):
    """fp64 reference and fp32 eager yardstick after each step (computed once, never modified)."""
    cfg = OptimConfig(**CFGS[cfg_name])
    lay, n, w0, srcs, scales = _inputs(K, bf16)
    out = {}
    for dt in (torch.float64, torch.float32):
        w, s1, s2 = w0.to(dt, copy=True), torch.zeros(n, dtype=dt), torch.zeros(n, dtype=dt)
        traj = []
        for step in range(1, STEPS + 1):
            _ref_step(cfg, lay, w, srcs[step - 1], scales, s1, s2, step, dt)
            traj.append((w.clone(), s1.clone(), s2.clone()))
        out[dt] = traj
    return out


def _table(lay, n, cfg, dev):
    if not cfg.needs_layers:
        return None
    return LayerTable.for_range([(o, k, d) for (_n, o, k, d, _w) in lay], 0, n, cfg.exclude_1d, dev, ALIGN)


def _state(cfg, n, dev):
    s1 = torch.zeros(n, device=dev) if cfg.num_states >= 1 else None
    s2 = torch.zeros(n, device=dev) if cfg.num_states >= 2 else None
    return s1, s2


def _scale_tensors(values, dev):
    return [torch.tensor([float(v)], dtype=torch.float32, device=dev) for v in values]


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("cfg_name", list(CFGS))
def test_scaled_apply_matches_fp64_within_4x_fp32_eager(devname, cfg_name, K, bf16):
    dev = _dev(devname)
    cfg = OptimConfig(**CFGS[cfg_name])
    lay, n, w0, srcs, scales = _inputs(K, bf16)
    traj = _trajectories(cfg_name, K, bf16)
    lt = _table(lay, n, cfg, dev)
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    shadow = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
    sc = _scale_tensors(scales.tolist(), dev)
    pad = torch.ones(n, dtype=torch.bool)
    for _name, o, k, _d, _w in lay:
        pad[o:o + k] = False
    bad, worst = [], (0.0, "")
    for step in range(1, STEPS + 1):
        prev = traj[torch.float64][step - 2][0] if step > 1 else w0.double()
        fused_apply_(cfg, dyn, w, [g.to(dev) for g in srcs[step - 1]], s1, s2, shadow, layers=lt, scales=sc)
        w64, a64, b64 = traj[torch.float64][step - 1]
        w32, a32, b32 = traj[torch.float32][step - 1]
        got = {"master": w.cpu().double(), "shadow": shadow.float().cpu().double()}
        ref = {"master": w64, "shadow": w64}
        eag = {"master": w32.double(), "shadow": w32.to(torch.bfloat16).double()}
        if s1 is not None:
            got["state1"], ref["state1"], eag["state1"] = s1.cpu().double(), a64, a32.double()
        if s2 is not None:
            got["state2"], ref["state2"], eag["state2"] = s2.cpu().double(), b64, b32.double()
        assert all(torch.isfinite(v).all() for v in got.values())
        assert not got["master"][pad].any() and not got["shadow"][pad].any(), "alignment padding must stay zero"
        for name, o, k, _d, _what in lay:
            sl = slice(o, o + k)
            floor = 2 * EPS32 * float(torch.maximum(w64[sl].abs().max(), prev[sl].abs().max()))
            for key in got:
                ek = float((got[key][sl] - ref[key][sl]).abs().max())
                ee = float((eag[key][sl] - ref[key][sl]).abs().max())
                bound = max(4 * ee, floor)
                line = f"step {step} {name:7s} {key:7s} kernel {ek:.3e} eager {ee:.3e} bound {bound:.3e}"
                worst = max(worst, (ek / bound, line))
                if ek > bound:
                    bad.append(line)
    print(f"CLIPERR {devname} {cfg_name} K={K} {'bf16' if bf16 else 'fp32'} worst err/bound {worst[0]:.3f} | {worst[1]}")
    assert not bad, "kernel error above 4x the fp32-eager error (and the 2-ulp floor):\n" + "\n".join(bad)


def _run(cfg, dev, K, bf16, scales):
    lay, n, w0, srcs, _ = _inputs(K, bf16)
    lt = _table(lay, n, cfg, dev)
    w = w0.to(dev, copy=True)
    s1, s2 = _state(cfg, n, dev)
    sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
    dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
    for step in range(STEPS):
        fused_apply_(cfg, dyn, w, [g.to(dev) for g in srcs[step]], s1, s2, sh, layers=lt, scales=scales)
    return [t.cpu() for t in (w, s1, s2, sh.float()) if t is not None]


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 3, 16])
@pytest.mark.parametrize("cfg_name", list(CFGS))
def test_scales_of_exactly_one_reproduce_the_unscaled_bits(devname, cfg_name, K, bf16):
    """fmaf(1, g, acc) == acc + g: the scaled instantiations with every scale 1.0 give the bits of
    the unscaled kernels (and a scale that is not 1 does move the result)."""
    dev = _dev(devname)
    cfg = OptimConfig(**CFGS[cfg_name])
    base = _run(cfg, dev, K, bf16, None)
    ones = _run(cfg, dev, K, bf16, _scale_tensors([1.0] * K, dev))
    for a, b in zip(base, ones):
        assert torch.equal(a, b)
    half = _run(cfg, dev, K, bf16, _scale_tensors([0.5] * K, dev))
    assert not torch.equal(base[0], half[0])


@pytest.mark.parametrize("devname", DEVICES)
@pytest.mark.parametrize("out_bf16", [True, False], ids=["out_bf16", "out_fp32"])
@pytest.mark.parametrize("bf16", [True, False], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", [1, 3, 16])
def test_multi_reduce_with_scales_matches_fp64(devname, K, bf16, out_bf16):
    """out = scale * sum_k c_k g_k by K sequential fmas and one multiply: at most K + 1 fp32
    roundings, each of at most 2^-24 of sum_k |c_k g_k| -- plus, for a bf16 output, its rounding
    (bf16 keeps 8 significant bits: half an ulp is at most 2^-8 relative). Scales of 1.0 give the unscaled bits."""
    dev = _dev(devname)
    _lay, n, _w, srcs, scales = _inputs(K, bf16)
    n -= 3  # not a multiple of 8: the scalar tail runs too
    gs = [g[:n].to(dev) for g in srcs[0]]
    out = torch.zeros(n, dtype=torch.bfloat16 if out_bf16 else torch.float32, device=dev)
    multi_reduce_(out, gs, 0.5, scales=_scale_tensors(scales.tolist(), dev))
    ref = torch.zeros(n, dtype=torch.float64)
    mag = torch.zeros(n, dtype=torch.float64)
    for c, g in zip(scales, srcs[0]):
        ref += c.double() * g[:n].double()
        mag += (c.double() * g[:n].double()).abs()
    ref, mag = 0.5 * ref, 0.5 * mag
    bound = (K + 1) * 2.0 ** -24 * mag + (2.0 ** -8 * (ref.abs() + (K + 1) * 2.0 ** -24 * mag) if out_bf16 else 0.0) + 1e-45
    err = (out.cpu().double() - ref).abs()
    print(f"MRED K={K} worst err/bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    plain, ones = torch.zeros_like(out), torch.zeros_like(out)
    multi_reduce_(plain, gs, 0.5)
    multi_reduce_(ones, gs, 0.5, scales=_scale_tensors([1.0] * K, dev))
    assert torch.equal(plain, ones)


# ------------------------------------------------------------------ 4. config and rejections
def test_config_validates_clip_norm():
    assert OptimConfig("adamw").clip_norm == 0.0
    assert OptimConfig("adamw", clip_norm=1).clip_norm == 1.0
    assert OptimConfig("lamb", clip_norm=1.0).to_dict()["clip_norm"] == 1.0
    for bad in (-1, float("nan"), float("inf"), -0.5):
        with pytest.raises(ValueError, match="clip_norm"):
            OptimConfig("momentum", clip_norm=bad)


def test_collective_plane_rejects_clip_norm_and_names_the_async_plane():
    from parameter_server_distributed_amd import models
    from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

    spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=16)
    with pytest.raises(ValueError, match="async plane"):
        CollectivePS(spec.model, OptimConfig("momentum", clip_norm=1.0))
    CollectivePS(spec.model, OptimConfig("momentum", clip_norm=0.0))  # off: accepted as before


def test_worker_cli_parses_clip_grad_norm():
    from parameter_server_distributed_amd.cli.worker import build_parser

    assert build_parser().parse_intermixed_args(["--clip-grad-norm", "1.0"]).clip_grad_norm == 1.0
    assert build_parser().parse_intermixed_args([]).clip_grad_norm == 0.0


def test_grpc_worker_clips_with_the_same_formula():
    from parameter_server_distributed_amd.runtime.worker import Worker

    w = Worker.__new__(Worker)  # compute_gradients needs the model, the batch and clip_norm only
    from parameter_server_distributed_amd import models

    torch.manual_seed(0)
    w.spec = models.build("mlp", torch.device("cpu"), torch.float32, hidden=16)
    w.model, w.batch = w.spec.model, w.spec.make_batch(8, torch.device("cpu"), seed=1)
    w.clip_norm = 0.0
    _, raw = w.compute_gradients()
    norm = math.sqrt(sum(float(g.double().square().sum()) for _n, g in raw))
    w.clip_norm = 0.5 * norm
    _, clipped = w.compute_gradients()
    c = min(1.0, w.clip_norm / (norm + 1e-6))
    for (_n, a), (_m, b) in zip(raw, clipped):
        torch.testing.assert_close(b, a * c, rtol=1e-5, atol=1e-8)


def test_mix_of_null_and_set_scales_is_refused():
    n = 128
    w, s1 = torch.ones(n), torch.zeros(n)
    gs = [torch.ones(n) for _ in range(3)]
    dyn = OptimDyn(torch.device("cpu"), lr=0.1)
    one = torch.ones(1)
    cfg = OptimConfig("momentum")
    for scales in ([one, None, one], [one, one], [None, None, None, one]):
        with pytest.raises(ValueError, match="scales"):
            fused_apply_(cfg, dyn, w, gs, s1, None, scales=scales)
        with pytest.raises(ValueError, match="scales"):
            multi_reduce_(torch.zeros(n), gs, 1.0, scales=scales)
    C = native()
    with pytest.raises(RuntimeError, match="every gradient source or for none"):
        C.fused_apply_(w, gs, s1, None, None, dyn.t, cfg.code, scales=[one, None, one])
    with pytest.raises(RuntimeError, match="every gradient source or for none"):
        C.multi_reduce_(torch.zeros(n), gs, 1.0, [one, None, None])
    lt = LayerTable([(0, n, 2)], n, True, "cpu")
    with pytest.raises(RuntimeError, match="every gradient source or for none"):
        C.fused_apply_lw_(w, gs, s1, torch.zeros(n), None, dyn.t, OptimConfig("lamb").code, layers=lt.t,
                          scales=[None, one, one])
    assert torch.equal(w, torch.ones(n)), "a refused call must not touch the master"
    with pytest.raises(RuntimeError, match="fp32"):
        C.fused_apply_(w, gs, s1, None, None, dyn.t, cfg.code, scales=[one.double()] * 3)
