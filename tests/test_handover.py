"""The conv / BN and the transformer hand-over records and helpers (ops/handover.py) and the single copies of the
routing pieces in ops/conv.py (_dgrad_route, _write_dw), on the CPU with fake candidates and pinned autotune
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
    t, q, sc = ho.Q8Pending("t", "q", "scales")[:3]  # (a fourth field follows: the Linear's forward token)
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
# the transformer side: the Linear's tag, tokens and takes


def test_transformer_records_index_and_unpack_like_the_tuples_they_replace():
    lin, tok = ho.LinearSrc("lin", 3)
    assert (lin, tok) == ("lin", 3) and ho.LinearSrc("lin", 3)[1] == 3
    tok, ptr, db = ho.BiasHand(3, 4096, "db")
    assert (tok, ptr, db) == (3, 4096, "db") and ho.BiasHand(3, 4096, "db")[2] == "db"
    tok, g = ho.PendingDx(3, "g")
    assert (tok, g) == (3, "g") and ho.PendingDx(3, "g")[0] == 3
    assert ho.Q8Pending("t", "q", "s").tok is None and len(ho.Q8Pending("t", "q", "s")) == 4
    assert ho.Q8Pending("t", "q", "s", 7).tok == 7 and ho.Q8Pending("t", "q", "s", 7)[3] == 7


def _lin(tok=5, bias="b", act=None, ran_mx=True):
    return types.SimpleNamespace(_psd_tok=tok, bias=bias, act=act, _psd_ran_mx=ran_mx)


def test_linear_src_is_the_latest_forward_of_the_named_linear():
    lin, other, out = _lin(), _lin(), torch.zeros(2)
    assert ho.linear_src(out) is None and ho.linear_src(out, lin) is None  # no tag
    ho.tag_output(lin, out, 5)
    assert ho.linear_src(out) == (lin, 5) and ho.linear_src(out, lin).lin is lin
    assert ho.linear_src(out, other) is None  # the tag names another module
    lin._psd_tok = 6  # the Linear ran again: the tag's token is old
    assert ho.linear_src(out) is None and ho.linear_src(out, lin) is None
    ho.drop_tag(out)
    assert not hasattr(out, "_psd_src")
    ho.drop_tag(out)  # nothing to drop
    assert ho.forward_token(lin) == 6 and ho.forward_token(None) is None
    assert ho.forward_token(types.SimpleNamespace()) is None


@pytest.mark.parametrize("name,lin,tag_tok,want", [
    ("bias absent", _lin(bias=None), 5, False),
    ("act gelu", _lin(act="gelu"), 5, False),
    ("stale token", _lin(), 4, False),
    ("fresh", _lin(), 5, True),
    ("fresh, act 'none'", _lin(act="none"), 5, True),
])
def test_bias_src_truth_table(name, lin, tag_tok, want):
    out = torch.zeros(2)
    assert ho.bias_src(out) is None
    ho.tag_output(lin, out, tag_tok)
    src = ho.bias_src(out)
    assert (src is not None) is want
    if want:
        assert src.lin is lin and src.tok == 5


@pytest.mark.parametrize("name,declared_is_tagged,ran_mx,tag_tok,want", [
    ("another Linear", False, True, 5, None),
    ("did not run MX", True, False, 5, None),
    ("stale token", True, True, 4, None),
    ("fresh", True, True, 5, 5),
])
def test_mx_grad_token_truth_table(name, declared_is_tagged, ran_mx, tag_tok, want):
    lin, out = _lin(ran_mx=ran_mx), torch.zeros(2)
    ho.tag_output(lin if declared_is_tagged else _lin(), out, tag_tok)
    assert ho.mx_grad_token(lin, out) == want
    assert ho.mx_grad_token(None, out) is None and ho.mx_grad_token(lin, None) is None
    assert ho.mx_grad_token(lin, torch.zeros(2)) is None  # no tag


def test_take_dq8_four_cases():
    dy = torch.zeros(4, 8)
    cases = {"wrong token": (6, dy, False), "other data_ptr": (5, torch.zeros(4, 8), False),
             "same data_ptr, other shape": (5, dy.view(8, 4), False), "match": (5, dy, True)}
    for name, (tok, t, hit) in cases.items():
        mod = types.SimpleNamespace()
        ho.leave_dq8(mod, tok, t, "q", "s")
        rec = mod._psd_dq8_pending
        assert isinstance(rec, ho.Q8Pending) and rec.tok == tok and rec.q == "q"
        got = ho.take_dq8(mod, 5, dy)
        assert (got is rec) if hit else (got is None), name
        assert mod._psd_dq8_pending is None, name
    # the record is keyed by the [tokens, out] view the Linear's backward compares
    mod, dy3 = types.SimpleNamespace(), torch.zeros(2, 2, 8)
    ho.leave_dq8(mod, 5, dy3, "q", "s")
    assert ho.take_dq8(mod, 5, dy3.view(4, 8)).scales == "s"
    assert ho.take_dq8(mod, 5, dy) is None  # nothing left


def test_take_bias_four_cases():
    dy = torch.zeros(4, 8)
    cases = {"wrong token": (6, dy, False), "other data_ptr": (5, torch.zeros(4, 8), False), "match": (5, dy, True),
             "match by data_ptr alone": (5, dy.view(8, 4), True)}
    for name, (tok, t, hit) in cases.items():
        lin = _lin()
        ho.hand_bias(ho.LinearSrc(lin, tok), t, "db")
        rec = lin._psd_bias_hand
        assert isinstance(rec, ho.BiasHand) and rec == (tok, t.data_ptr(), "db")
        got = ho.take_bias(lin, 5, dy)
        assert (got is rec and got.db == "db") if hit else (got is None), name
        assert lin._psd_bias_hand is None, name
    assert ho.take_bias(types.SimpleNamespace(), 5, dy) is None  # absent


def test_take_dx_takes_its_own_token_and_empties_the_queue():
    mod = types.SimpleNamespace(_psd_pending_dx=[])
    for tok, g in ((4, "old"), (5, "mine"), (6, "newer-stale")):
        ho.queue_dx(mod, tok, g)
    assert all(isinstance(e, ho.PendingDx) for e in mod._psd_pending_dx)
    assert ho.take_dx(mod, 5) == "mine" and mod._psd_pending_dx == []
    mod._psd_pending_dx += [(5, "first"), (5, "newest")]  # raw tuples, as a test plants them
    assert ho.take_dx(mod, 5) == "newest" and mod._psd_pending_dx == []
    mod._psd_pending_dx += [ho.PendingDx(4, "old"), ho.PendingDx(6, "newer")]
    assert ho.take_dx(mod, 5) is None and mod._psd_pending_dx == []
    assert ho.take_dx(mod, 5) is None


def test_grad_out():
    param, view = torch.zeros(3, 2, dtype=torch.bfloat16), torch.zeros(3, 2)
    mod = types.SimpleNamespace(_psd_grad_sink=lambda p: view if p is param else None)
    assert ho.grad_out(mod, param) is view and ho.grad_out(mod, param, like=param) is view
    other = torch.zeros(5, dtype=torch.float64)
    assert ho.grad_out(mod, other) is None  # the sink has no view of it
    fresh = ho.grad_out(mod, other, like=other)
    assert fresh is not other and (fresh.shape, fresh.dtype, fresh.device) == (other.shape, other.dtype, other.device)
    bare = types.SimpleNamespace()
    assert ho.grad_out(bare, param) is None
    fresh = ho.grad_out(bare, param, like=param)
    assert fresh is not param and fresh.shape == param.shape and fresh.dtype == torch.bfloat16


def test_leave_q8_and_mx_pair():
    cons, t = types.SimpleNamespace(), torch.zeros(2, 3, 64)
    q, sc = ho.mx_pair(t.shape, t.device)
    assert q.shape == t.shape and q.dtype == torch.float8_e4m3fn and sc.shape == (12,) and sc.dtype == torch.uint8
    q5, sc5 = ho.mx_pair((4, 96), t.device, e5m2=True)
    assert q5.shape == (4, 96) and q5.dtype == torch.float8_e5m2 and sc5.shape == (12,) and sc5.dtype == torch.uint8
    ho.leave_q8(cons, t, q, sc)
    rec = cons._psd_q8_pending
    assert isinstance(rec, ho.Q8Pending) and rec.t is t and rec.q is q and rec.scales is sc and rec.tok is None
    assert ho.take(cons, "_psd_q8_pending", t, strides=True) is rec and cons._psd_q8_pending is None


@pytest.mark.parametrize("tok", [None, 5])
@pytest.mark.parametrize("handover", [0, 1])
@pytest.mark.parametrize("dgrad", [0, 1])
@pytest.mark.parametrize("wgrad", [0, 1])
def test_mx_grad_gate(monkeypatch, tok, handover, dgrad, wgrad):
    monkeypatch.setenv("PSD_FEATURES", f"fp8_llama_handover={handover},fp8_dgrad={dgrad},fp8_wgrad={wgrad}")
    want = tok is not None and handover == 1 and dgrad == 1 and wgrad == 0
    assert ho.mx_grad_gate(tok) is want


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
