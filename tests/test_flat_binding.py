"""The flat-buffer model binding both PS data planes share (parallel/flat.py): a sink parameter that
gets no gradient, release, the canonical hand-over between the planes, and the layouts that resumed
checkpoints depend on. CPU, world 1, fp32 parameters, no process group."""
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from parameter_server_distributed_amd.ops.optim import OptimConfig
from parameter_server_distributed_amd.parallel.async_ps import AsyncPS
from parameter_server_distributed_amd.parallel.collective_ps import CollectivePS

F32 = dict(param_dtype=torch.float32)
SGD = dict(kind="sgd", lr=0.1, weight_decay=0.0)
ADAM = dict(kind="adam", lr=1e-2, weight_decay=0.0)


class SinkLinear(nn.Linear):
    def psd_direct_grad_params(self):
        return [self.weight, self.bias]


class Toy(nn.Module):
    """Two sink layers added together (the second can be switched out of the forward), plain head."""

    def __init__(self):
        super().__init__()
        self.a, self.b, self.head = SinkLinear(64, 64), SinkLinear(64, 64), nn.Linear(64, 8)
        self.use_b = True

    def forward(self, x):
        h = self.a(x)
        if self.use_b:
            h = h + self.b(x)
        return self.head(h)


def _toy():
    torch.manual_seed(0)
    return Toy()


def _mlp2():
    torch.manual_seed(0)
    return nn.Sequential(nn.Linear(40, 72), nn.ReLU(), nn.Linear(72, 8))


def _plane(kind, model, cfg=SGD, **kw):
    kw = {"bucket_mb": 0.001, **kw}
    if kind == "collective":
        return CollectivePS(model, OptimConfig(**cfg), grad_dtype=torch.float32, **F32, **kw)
    return AsyncPS(model, OptimConfig(**cfg), staleness=0, **F32, **kw)


def _batch(model, n=4, seed=1):
    g = torch.Generator().manual_seed(seed)
    first = next(m for m in model.modules() if isinstance(m, nn.Linear))
    return torch.randn(n, first.in_features, generator=g), torch.randint(0, 8, (n,), generator=g)


def _step(ps, model, x, y):
    ps.begin_step()
    F.cross_entropy(model(x), y).backward()
    ps.finish_step()
    if hasattr(ps, "refresh_weights"):  # async: the workers' weights are one pull behind until refreshed
        ps.drain()
        ps.refresh_weights()


def _params(model):
    return {n: p.detach().clone() for n, p in model.named_parameters()}


@pytest.mark.parametrize("kind", ["collective", "async"])
def test_missing_sink_gradient_is_zeroed(kind):
    """A sink parameter that gets no gradient in a step must not move: its view still holds an older
    step's gradient (on the async plane the one of step t-2: two buffers alternate, hence two skipped
    steps after two used ones) and is zeroed when its bucket is flushed."""
    model = _toy()
    ps = _plane(kind, model)
    try:
        assert ps._zero_plan == [(0, 8), (64, 512)]  # not None: else the whole buffer is zeroed anyway
        assert len(ps.buckets) == 3
        x, y = _batch(model)
        for t, use in enumerate([True, True, False, False]):
            model.use_b = use
            before = _params(model)
            _step(ps, model, x, y)
            after = _params(model)
            for n in ("b.weight", "b.bias"):
                assert torch.equal(before[n], after[n]) != use, f"step {t}: {n} {'unchanged' if use else 'moved'}"
            assert not torch.equal(before["a.weight"], after["a.weight"]), f"step {t}"
            assert not torch.equal(before["head.weight"], after["head.weight"]), f"step {t}"
    finally:
        ps.close()


def _hooked(model):
    return [n for n, p in model.named_parameters() if getattr(p, "_post_accumulate_grad_hooks", None)]


@pytest.mark.parametrize("kind", ["collective", "async"])
def test_close_releases_the_model(kind):
    model = _toy()
    x, y = _batch(model)
    ps = _plane(kind, model)
    _step(ps, model, x, y)
    assert len(_hooked(model)) == 6 and hasattr(model.a, "_psd_grad_sink")
    ps.close()
    assert not any(hasattr(m, "_psd_grad_sink") for m in model.modules())
    assert not _hooked(model)
    grads = [g.clone() for g in ([ps.grads_flat] if kind == "collective" else ps.grads)]
    model.zero_grad()
    F.cross_entropy(model(x), y).backward()  # does not call into the closed plane
    assert all(torch.equal(a, b) for a, b in zip(grads, [ps.grads_flat] if kind == "collective" else ps.grads))
    # a second plane over the same model trains
    ps2 = _plane("async" if kind == "collective" else "collective", model)
    try:
        before = _params(model)
        _step(ps2, model, x, y)
        assert all(not torch.equal(before[n], p) for n, p in model.named_parameters())
    finally:
        ps2.close()


def test_closing_an_older_plane_keeps_the_newer_planes_sinks():
    """The elastic runtime builds the next plane over the same model; releasing the previous one
    afterwards must remove its own sinks only."""
    model = _toy()
    x, y = _batch(model)
    old = _plane("async", model)
    new = _plane("async", model)
    try:
        old.close()
        for m in (model.a, model.b):
            v = m._psd_grad_sink(m.weight)
            g = new.grads[new.gb]
            assert g.data_ptr() <= v.data_ptr() < g.data_ptr() + g.numel() * g.element_size()
        assert len(_hooked(model)) == 6
        before = _params(model)
        _step(new, model, x, y)
        assert all(not torch.equal(before[n], p) for n, p in model.named_parameters())
    finally:
        new.close()
        old.close()


def test_canonical_handover_across_planes():
    """The one layout-independent format both planes share: collective -> async -> collective (another
    bucket size), bit for bit."""
    m1 = _mlp2()
    x, y = _batch(m1)
    c1 = _plane("collective", m1, ADAM)
    for _ in range(3):
        _step(c1, m1, x, y)
    sd = c1.canonical_state(root=0)
    want = _params(m1)
    assert set(sd) == {"master", "state1", "state2", "dyn"} and sd["master"].numel() == c1.num_params()

    m2 = _mlp2()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)
    a = _plane("async", m2, ADAM)
    try:
        a.load_canonical_state(sd)
        for n, p in m2.named_parameters():
            assert torch.equal(p, want[n]), n
        sd2 = a.canonical_state(root=0)
        for k in ("master", "state1", "state2"):
            assert torch.equal(sd2[k], sd[k]), k
    finally:
        a.close()

    m3 = _mlp2()
    with torch.no_grad():
        for p in m3.parameters():
            p.sub_(1.0)
    c3 = _plane("collective", m3, ADAM, bucket_mb=16.0)
    assert len(c3.buckets) != len(c1.buckets)
    c3.load_canonical_state(sd2)
    for n, p in m3.named_parameters():
        assert torch.equal(p, want[n]), n
    sd3 = c3.canonical_state(root=0)
    for k in ("master", "state1", "state2"):
        assert torch.equal(sd3[k], sd[k]), k
    c1.close()
    c3.close()


# name -> offset in the flat buffers (reverse registration order, 64-element aligned)
TOY_OFFSETS = {"head.bias": 0, "head.weight": 64, "b.bias": 576, "b.weight": 640, "a.bias": 4736, "a.weight": 4800}
MLP2_OFFSETS = {"2.bias": 0, "2.weight": 64, "0.bias": 640, "0.weight": 768}
LAYOUTS = [
    # model, offsets, collective buckets (offset, numel, slice_numel), collective total,
    # async P = 1 (total, shard_off, shard_len), async P = 2 (the total is padded to P * 64)
    (_toy, TOY_OFFSETS, [(0, 576, 576), (576, 4160, 4160), (4736, 4160, 4160)], 8896,
     (8896, [0], [8896]), (8960, [0, 4480], [4480, 4480])),
    (_mlp2, MLP2_OFFSETS, [(0, 640, 640), (640, 3008, 3008)], 3648,
     (3648, [0], [3648]), (3712, [0, 1856], [1856, 1856])),
]


@pytest.mark.parametrize("make,offsets,cbuckets,total,a1,a2", LAYOUTS, ids=["toy", "mlp2"])
def test_layouts_are_pinned(make, offsets, cbuckets, total, a1, a2):
    """A resumed checkpoint depends on these numbers. The literal values were printed by a run of the
    commit before the binding was shared (the planes then still computed everything themselves), not
    by this code."""
    c = _plane("collective", make())
    assert [(b.offset, b.numel, b.slice_numel) for b in c.buckets] == cbuckets
    assert {n: o for b in c.buckets for (n, _p, o, _k) in b.params} == offsets
    assert c.total == total
    c.close()
    for kw, want in (({}, a1), ({"ps_ranks": [0, 0]}, a2)):
        a = _plane("async", make(), **kw)
        try:
            assert {n: o for (n, _p, o, _k) in a._layout} == offsets
            assert (a.total, a.shard_off, a.shard_len) == want
        finally:
            a.close()
