"""The conv / BN hand-over records and helpers (ops/handover.py) and the single copies of the routing
pieces in ops/conv.py (_dgrad_route, _write_dw), on the CPU with fake candidates and pinned autotune
decisions: nothing is timed and no kernel runs. One GPU test: a stale record is ignored, not used."""
import copy
import types

import pytest
import torch

from parameter_server_distributed_amd.ops import autotune, handover as ho
from parameter_server_distributed_amd.ops import conv as convmod

CL = torch.channels_last


# ---------------------------------------------------------------------------------------------
# records


def test_records_index_and_unpack_like_the_tuples_they_replace():
    f = ho.BnFwd("y", "x", "mean", "ss", "mbits", "xd", "mean_d")
    y, x, mean, ss, mbits, xd, mean_d = f
    assert (y, x, mean, ss, mbits, xd, mean_d) == ("y", "x", "mean", "ss", "mbits", "xd", "mean_d")
    assert f[0] == "y" and f[6] == "mean_d" and len(f) == 7
    pre = ho.BwdPre("g", "part", 3)
    assert pre.part_d is None and pre[:3] == ("g", "part", 3) and pre[2] == 3
    assert ho.BwdPre("g", "part", 3, "pd").part_d == "pd"
    fold = ho.FoldPending("g", "coef", "y")
    assert fold.P is None and fold[:3] == ("g", "coef", "y")
    assert ho.FoldPending("g", "coef", "y", "P")[3] == "P"
    y, part, rows = ho.StatsPending("y", "part", 2)
    assert (y, part, rows) == ("y", "part", 2)
    t, q, sc = ho.Q8Pending("t", "q", "scales")
    assert (t, q, sc) == ("t", "q", "scales") and ho.Q8Pending("t", "q", "s")[1] == "q"


def _pairs():
    a = torch.zeros(2, 8, 4, 4)
    thin = torch.zeros(2, 8, 1, 1)
    thin_cl = thin.as_strided(thin.shape, (8, 1, 8, 8))  # the channels_last strides of the same memory
    cl = torch.zeros(2, 8, 4, 4).contiguous(memory_format=CL)
    return {  # name: (a, b, same without strides, same with strides)
        "itself": (a, a, True, True),
        "other tensor, equal shape": (a, torch.zeros(2, 8, 4, 4), False, False),
        "same data_ptr, other shape": (a, a.view(2, 8, 16), False, False),
        "equal memory, other strides": (thin, thin_cl, True, False),
        "channels_last vs its contiguous copy": (cl, cl.contiguous(), False, False),
    }


@pytest.mark.parametrize("name", list(_pairs()))
def test_same_in_both_modes(name):
    a, b, loose, strict = _pairs()[name]
    if name == "equal memory, other strides":
        assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() != b.stride()
    assert ho.same(a, b, strides=False) is loose
    assert ho.same(a, b, strides=True) is strict


@pytest.mark.parametrize("strides", [False, True])
def test_take_clears_on_hit_and_on_miss(strides):
    t = torch.zeros(2, 8, 4, 4)
    mod = types.SimpleNamespace()
    assert ho.take(mod, "_psd_bwd_pre", t, strides) is None  # absent
    assert ho.take(None, "_psd_bwd_pre", t, strides) is None
    rec = ho.BwdPre(t, "part", 1)
    mod._psd_bwd_pre = rec
    assert ho.take(mod, "_psd_bwd_pre", t, strides) is rec
    assert mod._psd_bwd_pre is None
    mod._psd_bwd_pre = ho.BwdPre(torch.zeros(2, 8, 4, 4), "part", 1)
    assert ho.take(mod, "_psd_bwd_pre", t, strides) is None
    assert mod._psd_bwd_pre is None
    mod._psd_bwd_pre = ho.BwdPre(torch.zeros(2, 8, 4, 4), "part", 1)
    with pytest.raises(RuntimeError, match="not the one"):
        ho.take(mod, "_psd_bwd_pre", t, strides, mismatch="not the one")
    assert mod._psd_bwd_pre is None  # cleared before the check


def test_take_keeps_each_mode():
    thin = torch.zeros(2, 8, 1, 1)
    thin_cl = thin.as_strided(thin.shape, (8, 1, 8, 8))
    mod = types.SimpleNamespace(_psd_q8_pending=ho.Q8Pending(thin, "q", "s"))
    assert ho.take(mod, "_psd_q8_pending", thin_cl, strides=True) is None
    mod._psd_q8_pending = ho.Q8Pending(thin, "q", "s")
    assert ho.take(mod, "_psd_q8_pending", thin_cl, strides=False).q == "q"


def test_pop_dr():
    t = torch.ones(1, 2, 2, 2)
    assert ho.pop_dr(types.SimpleNamespace()) is None
    assert ho.pop_dr(types.SimpleNamespace(_psd_pending_dr=[])) is None
    mod = types.SimpleNamespace(_psd_pending_dr=[torch.zeros(1), t])
    assert ho.pop_dr(mod) is t and len(mod._psd_pending_dr) == 1
    t4 = torch.arange(8.).view(1, 2, 2, 2)
    mod._psd_pending_dr.append(ho.StridedDr(t4, 4, 4))
    full = ho.pop_dr(mod)
    assert full.shape == (1, 2, 4, 4) and torch.equal(full[:, :, ::2, ::2], t4) and float(full.sum()) == float(t4.sum())


def test_route_res_grad_both_ways():
    g = torch.ones(2)
    assert ho.route_res_grad(None, g) is g
    to = types.SimpleNamespace(_psd_pending_dr=[])
    assert ho.route_res_grad(to, g) is None and to._psd_pending_dr == [g]


def test_sinks_and_momentum():
    mod = types.SimpleNamespace(weight="w", bias="b", momentum=None)
    assert ho.sinks(mod) == (None, None) and ho.bn_momentum(mod) == 0.1
    mod._psd_grad_sink, mod.momentum = (lambda p: p + "_view"), 0.25
    assert ho.sinks(mod) == ("w_view", "b_view") and ho.bn_momentum(mod) == 0.25


def test_bn_reexports_the_moved_names():
    from parameter_server_distributed_amd.ops import bn

    assert bn.StridedDr is ho.StridedDr and bn.take_dr is ho.take_dr


# ---------------------------------------------------------------------------------------------
# _dgrad_route with fake candidates


KEY = ("conv", "dgrad", "test_handover")
SENTINEL = ("a timed candidate's hand-over",)


class _Route:
    """Fake bwd-data candidates over a fake BN; every autotune.choose call is recorded and answered from
    pinned decisions only (a key that is not pinned fails the test instead of timing)."""

    def __init__(self, monkeypatch, names, bx="bx"):
        self.bn = types.SimpleNamespace(_psd_bwd_pre=SENTINEL, _psd_pending_dr=[])
        self.dr = torch.full((2,), 7.0)
        self.fu = dict(mode=2, bn=self.bn, bx=bx, mean="mean", mbits="mbits", dr=self.dr)
        self.ran, self.outs, self.asked = [], {n: torch.full((2,), float(i)) for i, n in enumerate(names)}, []
        self.cands = {n: self._cand(n) for n in names}
        real = autotune.choose

        def choose(key, candidates, default, probe=None, group=None):
            self.asked.append((key, list(candidates), default))
            assert autotune.decisions().get(key) in candidates, f"{key} is not pinned to one of {list(candidates)}"
            return real(key, candidates, default, probe, group)

        monkeypatch.setattr(autotune, "choose", choose)
        self.pinned = []

    def _cand(self, name):
        def fn():
            self.ran.append(name)
            if name.startswith("psdnb"):  # a fused epilogue hands its partials over
                self.bn._psd_bwd_pre = ("pre of", name)
            return self.outs[name]
        return fn

    def pin(self, key, name):
        autotune.set_decision(key, name)
        self.pinned.append(key)

    def unpin(self):
        for k in self.pinned:
            autotune.set_decision(k, None)


@pytest.fixture
def route(monkeypatch):
    made = []

    def make(names, bx="bx"):
        made.append(_Route(monkeypatch, names, bx))
        return made[-1]
    yield make
    for r in made:
        r.unpin()


def test_route_without_bn_input_keeps_only_fused_candidates(route):
    r = route(["miopen", "psdn0", "psdnb0", "psdnb1"], bx=None)
    r.pin(KEY + ("bnbwd",), "miopen")  # the key of a BN with its input: must not be the one asked
    r.pin(KEY + ("nobx", "bnbwd"), "psdnb1")
    out = convmod._dgrad_route(KEY, r.cands, "miopen", r.fu, None)
    assert out is r.outs["psdnb1"] and r.ran == ["psdnb1"]
    assert r.asked == [(KEY + ("nobx", "bnbwd"), ["psdnb0", "psdnb1"], "psdnb0")]


def test_route_without_bn_input_and_no_fused_candidate_raises(route):
    r = route(["miopen", "psdn0"], bx=None)
    with pytest.raises(RuntimeError, match="without its stored input"):
        convmod._dgrad_route(KEY, r.cands, "miopen", r.fu, None)
    assert r.ran == [] and r.asked == []


def test_route_unfused_winner_clears_the_handover_and_requeues_dr(route):
    r = route(["miopen", "psdn0", "psdnb0"])
    r.pin(KEY + ("bnbwd",), "psdn0")
    out = convmod._dgrad_route(KEY, r.cands, "miopen", r.fu, None)
    assert out is r.outs["psdn0"] and r.ran == ["psdn0"]
    assert r.bn._psd_bwd_pre is None
    assert len(r.bn._psd_pending_dr) == 1 and r.bn._psd_pending_dr[0] is r.dr
    assert r.asked == [(KEY + ("bnbwd",), ["miopen", "psdn0", "psdnb0"], "miopen")]


def test_route_fused_winner_keeps_its_handover_and_the_dr(route):
    r = route(["miopen", "psdn0", "psdnb0"])
    r.pin(KEY + ("bnbwd",), "psdnb0")
    out = convmod._dgrad_route(KEY, r.cands, "miopen", r.fu, None)
    assert out is r.outs["psdnb0"] and r.ran == ["psdnb0"]
    assert r.bn._psd_bwd_pre == ("pre of", "psdnb0") and r.bn._psd_pending_dr == []


def test_route_without_fusion_asks_the_plain_key(route):
    r = route(["miopen", "psdn0"])
    r.pin(KEY, "psdn0")
    assert convmod._dgrad_route(KEY, r.cands, "miopen", None, None) is r.outs["psdn0"]
    assert r.asked == [(KEY, ["miopen", "psdn0"], "miopen")]


# the same rules when the call comes from the BN-backward fold (_fold_backward): its candidates are
# "unfold" / "psdnf<v>" / "psdnb<v>", timed as dgrad + wgrad pairs (``timed``), and "unfold" winning
# means the caller runs the ordinary backward: nothing runs here, None comes back, dr is re-queued

FKEY = ("conv1x1", "dgrad_fold", "test_handover")


def _fold_call(r, default="unfold"):
    timed = {n: (lambda n=n: r.ran.append("timed " + n)) for n in r.cands}
    return convmod._dgrad_route(FKEY, r.cands, default, r.fu, None, timed=timed, defer="unfold")


def test_fold_route_without_bn_input_keeps_only_fused_candidates(route):
    r = route(["unfold", "psdnf0", "psdnb0", "psdnb1"], bx=None)
    r.pin(FKEY + ("bnbwd",), "unfold")
    r.pin(FKEY + ("nobx", "bnbwd"), "psdnb1")
    assert _fold_call(r) is r.outs["psdnb1"] and r.ran == ["psdnb1"]
    assert r.asked == [(FKEY + ("nobx", "bnbwd"), ["psdnb0", "psdnb1"], "psdnb0")]
    assert r.bn._psd_bwd_pre == ("pre of", "psdnb1") and r.bn._psd_pending_dr == []


def test_fold_route_without_bn_input_and_no_fused_candidate_raises(route):
    r = route(["unfold", "psdnf0"], bx=None)
    with pytest.raises(RuntimeError, match="without its stored input"):
        _fold_call(r)
    assert r.ran == []


def test_fold_route_unfused_winner_clears_the_handover_and_requeues_dr(route):
    r = route(["unfold", "psdnf0", "psdnb0"])
    r.pin(FKEY + ("bnbwd",), "psdnf0")
    assert _fold_call(r) is r.outs["psdnf0"] and r.ran == ["psdnf0"]
    assert r.bn._psd_bwd_pre is None and r.bn._psd_pending_dr == [r.dr]


def test_fold_route_fused_winner_keeps_its_handover_and_the_dr(route):
    r = route(["unfold", "psdnf0", "psdnb0"])
    r.pin(FKEY + ("bnbwd",), "psdnb0")
    assert _fold_call(r) is r.outs["psdnb0"] and r.ran == ["psdnb0"]
    assert r.bn._psd_bwd_pre == ("pre of", "psdnb0") and r.bn._psd_pending_dr == []


def test_fold_route_unfold_returns_to_the_caller_with_dr_requeued(route):
    r = route(["unfold", "psdnf0", "psdnb0"])
    r.pin(FKEY + ("bnbwd",), "unfold")
    assert _fold_call(r) is None and r.ran == []  # the caller runs the unfolded path
    assert r.bn._psd_bwd_pre is None and r.bn._psd_pending_dr == [r.dr]
    assert r.asked == [(FKEY + ("bnbwd",), ["unfold", "psdnf0", "psdnb0"], "unfold")]


def test_fold_route_unfold_without_fusion(route):
    r = route(["unfold", "psdnf0"])
    r.fu = None
    r.pin(FKEY, "unfold")
    assert _fold_call(r) is None and r.ran == []
    assert r.bn._psd_bwd_pre is SENTINEL and r.bn._psd_pending_dr == []


# ---------------------------------------------------------------------------------------------
# _write_dw with a fake weight-gradient candidate


def _fake_wgrad(cout, k, cin, calls):
    """A candidate of the narrow wgrad kernel's shape: writes OHWI rows into ``into`` or a fresh tensor and
    returns the [Cout, Cin, k, k] channels_last view."""
    def fn(into=None):
        calls.append(into)
        o = into if into is not None else torch.empty(cout, k * k * cin)
        o.copy_(torch.arange(float(o.numel())).view(o.shape))
        return o.view(cout, k, k, cin).permute(0, 3, 1, 2)
    return fn


@pytest.mark.parametrize("layout,k", [("ohwi", 3), ("oi", 1)])
def test_write_dw_contiguous_sink_is_written_by_the_kernel(layout, k):
    calls = []
    sv = torch.zeros(4, 8, k, k).contiguous(memory_format=CL if layout == "ohwi" else torch.contiguous_format)
    dw = convmod._write_dw(sv, _fake_wgrad(4, k, 8, calls), layout)
    assert dw is sv and len(calls) == 1
    assert calls[0].data_ptr() == sv.data_ptr() and calls[0].shape == (4, k * k * 8)
    want = torch.arange(float(sv.numel())).view(4, k, k, 8).permute(0, 3, 1, 2)
    assert torch.equal(sv, want)


def test_write_dw_other_sink_layout_goes_through_copy():
    calls = []
    sv = torch.zeros(4, 8, 3, 3)  # NCHW-contiguous: not the kernel's OHWI layout
    dw = convmod._write_dw(sv, _fake_wgrad(4, 3, 8, calls), "ohwi")
    assert dw is sv and calls == [None]
    assert torch.equal(sv, torch.arange(float(sv.numel())).view(4, 3, 3, 8).permute(0, 3, 1, 2))


def test_write_dw_without_a_sink_returns_the_fresh_tensor():
    calls = []
    dw = convmod._write_dw(None, _fake_wgrad(4, 3, 8, calls), "ohwi")
    assert calls == [None] and dw.shape == (4, 8, 3, 3)
    assert torch.equal(dw, torch.arange(float(dw.numel())).view(4, 3, 3, 8).permute(0, 3, 1, 2))


def test_write_dw_copy_only_layout_never_hands_the_sink_to_the_candidate():
    sv, fresh = torch.zeros(4, 8, 1, 1), torch.ones(4, 8, 1, 1)
    assert convmod._write_dw(sv, lambda: fresh, None) is sv and torch.equal(sv, fresh)
    assert convmod._write_dw(None, lambda: fresh, None) is fresh
    assert convmod._write_dw(sv, lambda: None, None) is None


def test_write_dw_passes_a_decline_through():
    sv = torch.zeros(4, 8, 3, 3).contiguous(memory_format=CL)
    assert convmod._write_dw(sv, lambda into=None: None, "ohwi") is None
    assert convmod._write_dw(sv.contiguous(), lambda into=None: None, "ohwi") is None


def test_out_hw():
    assert convmod._out_hw(56, 56, 3, 1, 1) == (56, 56)
    assert convmod._out_hw(56, 57, 3, 2, 1) == (28, 29)
    assert convmod._out_hw(224, 224, 7, 2, 3) == (112, 112)
    assert convmod._out_hw(14, 14, 1, 2, 0) == (7, 7)


# ---------------------------------------------------------------------------------------------
# GPU: a stale record is ignored, not used


@pytest.mark.gpu
def test_stale_records_are_ignored_not_used(gpu, monkeypatch):
    """Conv1x1(64, 256) on the narrow kernel (the psdn0 route and shape of tests/test_convn.py
    test_conv_bn_module_psdn_route_matches_fp32) into a training FusedBatchNorm2d(256). A
    ``_psd_stats_pending`` made for another tensor of the same shape (garbage partials) and a
    ``_psd_bwd_pre`` made for another gradient must be cleared and ignored: output, running statistics
    and every gradient bit-equal to a run with nothing planted."""
    from parameter_server_distributed_amd.ops.bn import FusedBatchNorm2d
    from parameter_server_distributed_amd.ops.conv import Conv1x1

    monkeypatch.setenv("PSD_AUTOTUNE_FORCE", "psdn0")
    key = ("conv1x1", "fwd", 8 * 16 * 16, 64, 256)
    autotune.set_decision(key, None)
    torch.manual_seed(3)
    conv = Conv1x1(64, 256).to(gpu, torch.bfloat16).to(memory_format=CL)
    bn0 = FusedBatchNorm2d(256).to(gpu)
    bn0.weight.data = torch.randn(256, device=gpu).to(torch.bfloat16)
    bn0.bias.data = torch.randn(256, device=gpu).to(torch.bfloat16)
    x = torch.randn(8, 64, 16, 16, device=gpu).to(torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    y = conv(x).detach()
    assert autotune.decisions()[key] == "psdn0"
    autotune.set_decision(key, None)
    dy = torch.randn_like(y)
    runs = []
    for plant in (False, True):
        bn = copy.deepcopy(bn0)
        yin = y.clone(memory_format=torch.preserve_format).requires_grad_(True)
        if plant:
            other = torch.empty_like(yin)
            garbage = torch.full((4, 2, 256), 1e30, device=gpu, dtype=torch.float32)
            bn._psd_stats_pending = ho.StatsPending(other, garbage, 4)
        out = bn(yin)
        assert bn._psd_stats_pending is None
        if plant:
            bn._psd_bwd_pre = ho.BwdPre(torch.empty_like(dy), torch.full((4, 2, 256), 1e30, device=gpu), 4)
        out.backward(dy)
        assert bn._psd_bwd_pre is None
        runs.append((out.detach(), bn.running_mean, bn.running_var, yin.grad, bn.weight.grad, bn.bias.grad))
    for a, b in zip(*runs):
        assert torch.equal(a, b)
