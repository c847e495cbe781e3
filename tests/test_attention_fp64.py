"""The attention kernels (kernels/attention.hip, S <= 128; kernels/attention_long.hip, S = 192 .. 4096)
against references they cannot pass by being nearly right: the exact set of keys every row sums, and
fp64 bounds per element that scale with the element's own terms.

Part A -- exact probes. The Q third of qkv is exact zeros, so every score is exactly 0 and the kernels'
arithmetic is exact: p = exp2(0) = 1, l = n (an integer sum), m = 0, lse = logf(n), with n(b, q) the number
of keys the row sees under the mask of ops/attention.py's docstring. n and the visible set come from
index comparisons alone (_visible), never from a softmax. K is random bf16 (it must not matter). V names
the key in small integers -- V[k, 0] = k & 63, V[k, 1] = k >> 6, V[k, 2 + k % 62] = 1 -- and dO is zeros
and ones, dO[q, d] = 1 where (q + d) % 5 == 0: every partial sum is an integer below 2^24, exact in fp32.
  lse  |lse - log n| <= 4 * 2^-23 * max(1, log n)  (logf is good to a few ulps and nothing before it
       rounds). Neighbouring counts differ by >= 1/4096 in log n: this pins n for every row.
  O    |O - (sum of the visible V) / n| <= (2^-8 + 2^-20) |ref| on the streaming kernels: one bf16
       rounding of an fp32 value (they round p = 1 to bf16, exactly, and divide by l at the end). The
       whole-head kernels (S <= 128) round the normalised probability bf16(1 / n) before P V, one more
       relative 2^-8 on every term of the row: (2^-7 + 2^-13) |ref| there, the derivation of dV's bound
       below. (The emulation of their documented numerics, _emulate, misses the tighter bound at every n
       that is no power of two: test_whole_head_emulation_needs_the_second_rounding.)
  dK   exactly 0 everywhere (Q = 0).
  dV   |dV - sum_{q sees k} dO[q, d] / n(q)| <= (2^-7 + 2^-13) |ref|: terms of one sign; P rounded to bf16
       gives 2^-8 per term, the output rounding 2^-8, 2^-13 covers exp2(-lse log2 e) against 1 / n.
  padded rows, and keys no query sees: exact zeros. Dropout p = 0.1: lse bitwise the p = 0 lse.
The mirrored probe (K zero, Q random) checks lse, O, dV the same way and dQ exactly 0.

Part B -- random inputs (randn * 1.5 for qkv, randn for dO, rounded to bf16), per element in fp64, staged as
in tests/test_row_kernels_fp64.py: the forward from qkv; the backward from exactly the tensors it is
given, the kernel's own o and lse (both kernel families form D = rowsum(dO . o) and p = exp(s - lse) from
them, and so does the reference). u = 2^-8 is bf16's unit roundoff (the kernels round to nearest even),
e = 2^-13 the slack for the fp32 scores and exp2; P, dP = dO V^T, D, dS = P (dP - D), T = P (|dP| + |D|)
in fp64, scale = 1/8:
  O    (u + e) (P |V|) + u |ref|                     lse  max(1e-5 + 1e-5 |ref|, 4 E32)
  dV   (u + e) (P^T |dO|) + u |ref|
  dQ   scale ((u |dS| + e T) |K|) + u |ref|          dK   scale ((u |dS| + e T)^T |Q|) + u |ref|
Each product's bf16 operand (P or dS) is off by <= u per term and the stored result by one more u; 1e-5
is the cross-entropy lse rule of test_row_kernels_fp64.py, and E32 (fp32 eager logsumexp against fp64 on
the case) only speaks where eager itself is past 1e-5. None of this is measured from a kernel. Padded
rows and masked-out contributions are exact zeros. Each case prints one ATTNERR line: per output the
worst err / bound with its position (b, h, row, column), the largest error and the rms of err / bound
(recorded in profiles/attn_fp64.md, not asserted: a biased rounding shows there first).

Part C -- CPU. _emulate is an fp32 torch composite with the kernels' documented numerics (P and dS
rounded to bf16 before the second products, outputs rounded to bf16, the backward staged from its own
o / lse; 64-key chunks with an online softmax from S = 192, the whole head at once below). It must pass
both checkers at S = 32, 128, 192 under every mask, and the checkers must report each mutant of it:
an off-by-one in each mask edge, a skipped 32 x 32 block, a missing accumulator rescale, a D that is
not the staged one."""
import math

import pytest
import torch

EPS32 = 2.0 ** -23
U = 2.0 ** -8   # bf16 unit roundoff
E = 2.0 ** -13  # fp32 score / exp2 slack
LOG2E = 1.4426950408889634
H = 2
WINDOWS = (1, 32, 33, 65, 200)
# S: 32, 96, 128 the whole-head instantiations that differ; 192, 320 a 64-row last tile with an even / odd
# chunk count; 512, 576 the last "long" and the first "xlong" size; 1024 many chunks; 4096 the ballot limit
SIZES = (32, 96, 128, 192, 320, 512, 576, 1024, 4096)
MASKS = ("full", "lens", "causal", "causal+lens", "causal+docs", "causal+docs+lens")
WMASKS = ("window", "window+docs", "window+docs+lens")


# ------------------------------------------------------------------------------------------ layout
def _heads(t, heads):
    """[B, S, heads * 64] -> [B, heads, S, 64]"""
    B, S, _ = t.shape
    return t.view(B, S, heads, 64).permute(0, 2, 1, 3)


def _split(qkv, heads):
    """packed [B, S, 3 * heads * 64] -> q, k, v, each [B, heads, S, 64]"""
    B, S, _ = qkv.shape
    return qkv.view(B, S, 3, heads, 64).permute(2, 0, 3, 1, 4).unbind(0)


def _visible(B, S, lens, causal, doc, window, dev, mut=None):
    """[B, q, key] bool, from the module docstring of ops/attention.py by index comparisons: q < L, key < L,
    causal: key <= q, documents: key >= doc[q] (clamped to [0, q]), window: key >= q - W + 1. A padded row
    sees nothing. mut: one edge moved by one (the mutants of Part C)."""
    idx = torch.arange(S, device=dev)
    L = torch.full((B,), S, device=dev) if lens is None else lens.to(dev).long().clamp(0, S)
    qi, ki = idx[None, :, None], idx[None, None, :]
    Lk = L + 1 if mut == "len" else L  # key <= L
    vis = (qi < L[:, None, None]) & (ki < Lk[:, None, None])
    if causal:
        vis = vis & ((ki < qi) if mut == "causal" else (ki <= qi))
    if doc is not None:
        d = torch.minimum(doc.to(dev).long().clamp(min=0), idx[None, :])
        if mut == "doc":  # the first token of a document starts one early
            d = d - ((d == idx[None, :]) & (idx[None, :] > 0)).long()
        vis = vis & (ki >= d[:, :, None])
    if window:
        vis = vis & (ki >= qi - int(window) + (0 if mut == "window" else 1))
    return vis


# ------------------------------------------------------------------------------------------ report
class _Err:
    """One case's checks: prints its ATTNERR line; .bad maps an output's name to its report where an
    element is above its bound (or not finite)."""

    def __init__(self, case):
        self.case, self.cells, self.bad, self.worst = case, [], {}, {}

    def add(self, name, got, ref, bound):
        assert tuple(got.shape) == tuple(ref.shape) == tuple(bound.shape), (name, got.shape, ref.shape, bound.shape)
        got = got.double()
        if not bool(torch.isfinite(got).all()):
            self.cells.append(f"{name}: non-finite")
            self.bad[name] = f"{name}: non-finite values"
            self.worst[name] = math.inf
            return
        err = (got - ref).abs()
        ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)  # above a zero bound: inf
        i = int(ratio.argmax())
        pos = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ratio.shape))
        on = bound > 0
        rms = float(ratio[on].clamp(max=1e6).square().mean().sqrt()) if bool(on.any()) else 0.0
        w = float(ratio.flatten()[i])
        cell = (f"{name}: err/bound {w:.3f} at {pos} (err {float(err.flatten()[i]):.3e}, ref "
                f"{float(ref.flatten()[i]):.3e}) maxerr {float(err.max()):.3e} rms {rms:.3f}")
        self.cells.append(cell)
        self.worst[name] = w
        if w > 1.0:
            self.bad[name] = cell

    def zero(self, name, got):
        z = torch.zeros(got.shape, dtype=torch.float64, device=got.device)
        self.add(name, got, z, z)

    def line(self):
        return f"ATTNERR {self.case} | " + " | ".join(self.cells)

    def finish(self):
        print(self.line())
        assert not self.bad, f"{self.case}: above the bound:\n" + "\n".join(self.bad.values())


# ------------------------------------------------------------------------------------------ Part A
def _probe_inputs(B, S, zero, seed):
    """(qkv, dO) of the exact probe, on the CPU. zero: "q" or "k", the third that is exact zeros."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    x = (torch.randn(B, S, 3, H, 64, generator=g) * 1.5).to(torch.bfloat16)
    x[:, :, 0 if zero == "q" else 1] = 0
    k = torch.arange(S)
    v = torch.zeros(S, 64)
    v[:, 0] = (k & 63).float()
    v[:, 1] = (k >> 6).float()
    v[k, 2 + k % 62] = 1.0
    x[:, :, 2] = v.to(torch.bfloat16)[None, :, None, :]
    d = torch.arange(64)
    do = ((k[:, None] + d[None, :]) % 5 == 0).to(torch.bfloat16)  # [S, 64], every head the same
    return x.view(B, S, 3 * H * 64), do.repeat(1, H)[None].repeat(B, 1, 1).contiguous()


def check_probe(qkv, do, heads, lens, causal, doc, window, o, lse, dqkv, zero="q", case="probe"):
    """Part A's assertions for one call (module docstring); lse None: not returned (the module path)."""
    B, S, _ = qkv.shape
    dev = qkv.device
    rep = _Err(case)
    vis = _visible(B, S, lens, causal, doc, window, dev)
    n = vis.sum(-1)  # [B, S]
    live = n > 0
    nd = n.clamp(min=1).double()
    logn = torch.where(live, nd.log(), torch.zeros_like(nd))
    inv = torch.where(live, 1.0 / nd, torch.zeros_like(nd))
    visd = vis.double()
    if lse is not None:
        bound = torch.where(live, 4 * EPS32 * logn.clamp(min=1.0), torch.zeros_like(nd))
        rep.add("lse", lse, logn[:, None, :].expand(B, heads, S), bound[:, None, :].expand(B, heads, S))
    v = _split(qkv, heads)[2].double()
    dod = _heads(do, heads).double()
    o_ref = torch.stack([(visd @ v[:, h]) * inv[..., None] for h in range(heads)], 1)
    # the whole-head kernels round the normalised probability to bf16, the streaming ones p = 1 (docstring)
    rel_o = 2.0 ** -7 + 2.0 ** -13 if S <= 128 else 2.0 ** -8 + 2.0 ** -20
    rep.add("o", _heads(o, heads), o_ref, rel_o * o_ref.abs())
    dq, dk, dv = _split(dqkv, heads)
    if zero == "q":
        rep.zero("dk", dk)
    else:
        rep.zero("dq", dq)
    dv_ref = torch.stack([visd.transpose(1, 2) @ (dod[:, h] * inv[..., None]) for h in range(heads)], 1)
    rep.add("dv", dv, dv_ref, (2.0 ** -7 + 2.0 ** -13) * dv_ref.abs())
    pad = ~live  # a padded row: nothing of dQKV
    if bool(pad.any()):
        rep.zero("dqkv-pad", dqkv[pad])
    return rep


# ------------------------------------------------------------------------------------------ Part B
def _qkv(B, S, seed, scale=1.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(B, S, 3 * H * 64, generator=g) * scale).to(torch.bfloat16)


def _dout(B, S, seed):
    g = torch.Generator(device="cpu").manual_seed(1000 + seed)
    return torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16)


def check_random(qkv, do, heads, lens, causal, doc, window, o, lse, dqkv, case="random"):
    """Part B's bounds for one call (module docstring)."""
    B, S, _ = qkv.shape
    dev = qkv.device
    scale = 1.0 / 8.0
    rep = _Err(case)
    vis = _visible(B, S, lens, causal, doc, window, dev)[:, None]  # [B, 1, q, key]
    live = vis.any(-1)  # [B, 1, S]
    q, k, v = (t.double() for t in _split(qkv, heads))
    neg = float("-inf")
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, neg)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    lse_ref = torch.where(live, torch.logsumexp(torch.where(live[..., None], s, zero), -1), zero)
    # forward, from qkv
    P = torch.where(vis, (s - lse_ref[..., None]).exp(), zero)
    o_ref = P @ v
    rep.add("o", _heads(o, heads), o_ref, (U + E) * (P @ v.abs()) + U * o_ref.abs())
    qf, kf, _ = (t.float() for t in _split(qkv, heads))
    s32 = (qf @ kf.transpose(-1, -2) * scale).masked_fill(~vis, neg)
    lse32 = torch.logsumexp(torch.where(live[..., None], s32, torch.zeros((), device=dev)), -1)
    e32 = float(torch.where(live, (lse32.double() - lse_ref).abs(), zero).max())
    lb = torch.maximum(1e-5 + 1e-5 * lse_ref.abs(), torch.full_like(lse_ref, 4 * e32))
    rep.add("lse", lse, lse_ref, torch.where(live.expand_as(lse_ref), lb, zero))
    # backward, from the o and lse it is given
    Pb = torch.where(vis, (s - lse.double()[..., None]).exp(), zero)
    dod = _heads(do, heads).double()
    D = (dod * _heads(o, heads).double()).sum(-1)
    dP = dod @ v.transpose(-1, -2)
    dS = Pb * (dP - D[..., None])
    W = U * dS.abs() + E * (Pb * (dP.abs() + D.abs()[..., None]))
    dq, dk, dv = _split(dqkv, heads)
    dv_ref = Pb.transpose(-1, -2) @ dod
    rep.add("dv", dv, dv_ref, (U + E) * (Pb.transpose(-1, -2) @ dod.abs()) + U * dv_ref.abs())
    dq_ref = scale * (dS @ k)
    rep.add("dq", dq, dq_ref, scale * (W @ k.abs()) + U * dq_ref.abs())
    dk_ref = scale * (dS.transpose(-1, -2) @ q)
    rep.add("dk", dk, dk_ref, scale * (W.transpose(-1, -2) @ q.abs()) + U * dk_ref.abs())
    pad = ~live[:, 0]
    if bool(pad.any()):
        rep.zero("o-pad", o[pad])
        rep.zero("dqkv-pad", dqkv[pad])
    rep.e32 = e32
    return rep


# ------------------------------------------------------------------------------------------ cases
def _lengths(S):
    """S, S - 31, a multiple of 64, a multiple of 32 plus 1, 1, 0 (in range; duplicates at S = 32 dropped)."""
    m64 = 64 * max(S // 128, 1) if S > 64 else S
    m33 = 32 * max(S // 64, 1) + 1 if S > 33 else 1
    out = []
    for n in (S, S - 31, m64, m33, 1, 0):
        if n not in out:
            out.append(n)
    return out


# document boundaries at, just before and just after 32-row and 64-row edges
_EDGES = (1, 31, 64, 97, 127, 160, 193, 255, 320, 385, 511, 513, 576, 703, 1023, 2048, 2049, 3071, 4000)


def _layouts(S):
    """Two rows of document lengths: boundaries around the block edges; all one-token documents."""
    cuts = [0] + [e for e in _EDGES if e < S] + [S]
    return [[b - a for a, b in zip(cuts, cuts[1:])], [1] * S]


def _cases(S, mask, first_layout_only=False):
    """Sub-cases of one (S, mask): (tag, lens, causal, doc, B), lens / doc as CPU tensors or None. Each
    length meets each document layout in a batch row; S = 4096 takes one row per sub-case (and S - 31 for
    the lengths)."""
    from parameter_server_distributed_amd.ops.attention import doc_starts

    causal = mask != "full" and mask != "lens"
    ls = (_lengths(S) if S < 4096 else [S - 31]) if "lens" in mask else [None]
    lay = (_layouts(S)[:1] if first_layout_only else _layouts(S)) if "docs" in mask else [None]
    rows = [(n, d) for d in lay for n in ls]
    if len(rows) == 1 and S < 4096:
        rows = rows * 2
    groups = [[r] for r in rows] if S == 4096 else [rows]
    for gi, grp in enumerate(groups):
        lens = torch.tensor([n for n, _ in grp], dtype=torch.int32) if "lens" in mask else None
        doc = doc_starts([d for _, d in grp], S) if "docs" in mask else None
        yield f"S={S} {mask}" + (f" #{gi}" if len(groups) > 1 else ""), lens, causal, doc, len(grp)


def _masks(S):
    return MASKS + (WMASKS if S >= 192 else ())


def _dev(t, dev):
    return None if t is None else t.to(dev)


# ------------------------------------------------------------------------------------------ Part C: emulation
def _bf(t):
    return t.to(torch.bfloat16).float()


def _emulate(qkv, do, heads, lens, causal, doc, window, mut=None):
    """fp32 composite with the kernels' documented numerics -> (o, lse, dqkv) in the kernels' layouts and
    dtypes. S <= 128: the whole head at once, the normalised probabilities rounded to bf16; above: 64-key
    chunks, running max m and sum l, the accumulator rescaled at every chunk, the un-normalised
    probabilities rounded to bf16 and one 1 / l at the end. Backward: p = exp2(s sl - lse log2 e) and
    D = rowsum(dO . o) from its own o / lse, P and dS rounded to bf16 before the second products.
    mut: a mask edge of _visible; "skip": the keys 32 .. 63 never multiplied for the queries 128 .. 159 in
    forward and dQ, "skip_t": in dK/dV only; "norescale": the O accumulators keep their scale when the max
    rises; "D": D = rowsum(P . dP) of the exact P instead of the given o."""
    B, S, _ = qkv.shape
    dev = qkv.device
    scale = 0.125
    sl = scale * LOG2E
    vis = _visible(B, S, lens, causal, doc, window, dev, mut)[:, None]
    vis_f, vis_t = vis, vis
    if mut in ("skip", "skip_t"):
        cut = vis.clone()
        cut[:, :, 128:160, 32:64] = False
        vis_f, vis_t = (cut, vis) if mut == "skip" else (vis, cut)
    q, k, v = (t.float() for t in _split(qkv, heads))
    dof = _heads(do, heads).float()
    neg = float("-inf")
    s = q @ k.transpose(-1, -2)  # raw scores; the kernels fold the scale into the exp2 argument
    sm = s.masked_fill(~vis_f, neg)
    live = vis_f.any(-1)
    one, zero = torch.ones(()), torch.zeros(())
    if S <= 128:
        m = sm.max(-1).values
        p = torch.exp2((sm - m[..., None]) * sl)
        l = p.sum(-1)
        acc = _bf(p * (1.0 / l)[..., None]) @ v
    else:
        m = torch.full(sm.shape[:-1], neg)
        l = torch.zeros_like(m)
        acc = torch.zeros_like(q)
        for c in range(0, S, 64):
            sc = sm[..., c:c + 64]
            mn = torch.maximum(m, sc.max(-1).values)
            dead = mn == neg  # no key yet: alpha = 1 and p = 0 by select
            alpha = torch.where(dead, one, torch.exp2((m - mn) * sl))
            p = torch.where(dead[..., None], zero, torch.exp2((sc - mn[..., None]) * sl))
            l = l * alpha + p.sum(-1)
            acc = acc * (one if mut == "norescale" else alpha[..., None]) + _bf(p) @ v[..., c:c + 64, :]
            m = mn
        acc = acc * (1.0 / l)[..., None]
    lse = torch.where(live, m * scale + l.log(), zero).expand(B, heads, S).contiguous()
    o4 = torch.where(live[..., None], acc, zero).to(torch.bfloat16)  # [B, heads, S, 64]
    o = o4.permute(0, 2, 1, 3).reshape(B, S, heads * 64)

    p = torch.exp2(s * sl - (lse * LOG2E)[..., None])
    dP = dof @ v.transpose(-1, -2)
    D = (dof * o4.float()).sum(-1)
    if mut == "D":
        P64 = torch.softmax((s.double() * scale).masked_fill(~vis, neg), -1)
        D = torch.where(live, (P64 * dP.double()).sum(-1), zero.double()).float()
    dS = p * (dP - D[..., None])
    dSq = _bf(torch.where(vis_f, dS, zero))
    dSt = _bf(torch.where(vis_t, dS, zero))
    Pt = _bf(torch.where(vis_t, p, zero))
    dq = (dSq @ k) * scale
    dk = (dSt.transpose(-1, -2) @ q) * scale
    dv = Pt.transpose(-1, -2) @ dof
    dqkv = torch.stack([dq, dk, dv], 0).to(torch.bfloat16).permute(1, 3, 0, 2, 4).reshape(B, S, 3 * heads * 64)
    return o, lse, dqkv


def _emulated_reports(S, mask, window, mut=None, first_layout_only=False):
    """(probe zero-q, probe zero-k, random) reports of the emulation for every sub-case of (S, mask)."""
    out = []
    for tag, lens, causal, doc, B in _cases(S, mask, first_layout_only):
        tag = f"emu {tag}" + (f" W={window}" if window else "") + (f" mutant={mut}" if mut else "")
        reps = []
        for zero in ("q", "k"):
            qkv, do = _probe_inputs(B, S, zero, 3)
            got = _emulate(qkv, do, H, lens, causal, doc, window, mut)
            reps.append(check_probe(qkv, do, H, lens, causal, doc, window, *got, zero=zero, case=f"{tag} zero-{zero}"))
        qkv, do = _qkv(B, S, 1), _dout(B, S, 1)
        got = _emulate(qkv, do, H, lens, causal, doc, window, mut)
        reps.append(check_random(qkv, do, H, lens, causal, doc, window, *got, case=f"{tag} random"))
        out.append(reps)
    return out


@pytest.mark.parametrize("S", [32, 128, 192])
def test_emulation_is_within_the_bounds(S):
    """The documented numerics alone fit Part A's and Part B's bounds, under every mask."""
    for mask in _masks(S):
        for W in (WINDOWS if "window" in mask else (None,)):
            for reps in _emulated_reports(S, mask, W):
                for rep in reps:
                    rep.finish()


def test_whole_head_emulation_needs_the_second_rounding():
    """Why Part A's O bound is 2^-7 at S <= 128: the whole-head numerics round bf16(1 / n) and then the
    output, and at an n that is no power of two that alone is past (2^-8 + 2^-20) |ref|; it never passes
    2^-7 + 2^-13. The streaming numerics stay within one rounding."""
    for S, lo in ((128, 2.0 ** -8 + 2.0 ** -20), (192, 0.0)):
        qkv, do = _probe_inputs(2, S, "q", 3)
        o, _, _ = _emulate(qkv, do, H, None, True, None, None)
        vis = _visible(2, S, None, True, None, None, qkv.device).double()
        v = _split(qkv, H)[2].double()
        ref = torch.stack([vis @ v[:, h] for h in range(H)], 1) / vis.sum(-1)[:, None, :, None]
        rel = ((_heads(o, H).double() - ref).abs() / ref.abs().clamp(min=1e-300)).max()
        hi = 2.0 ** -7 + 2.0 ** -13 if S <= 128 else 2.0 ** -8 + 2.0 ** -20
        assert lo < float(rel) <= hi, (S, float(rel))


# (mutant, S, mask, window, which report: 0 probe zero-q / 2 random, the output that must report it)
MUTANTS = [
    ("causal", 128, "causal", None, 0, "lse"),
    ("causal", 192, "causal+docs+lens", None, 0, "lse"),
    ("window", 192, "window", 33, 0, "lse"),
    ("window", 192, "window+docs+lens", 1, 0, "lse"),
    ("len", 128, "lens", None, 0, "lse"),
    ("len", 192, "lens", None, 0, "lse"),
    ("doc", 128, "causal+docs", None, 0, "lse"),
    ("doc", 192, "window+docs", 65, 0, "lse"),
    ("skip", 192, "causal", None, 0, "lse"),
    ("skip", 192, "full", None, 0, "lse"),
    ("skip_t", 192, "causal", None, 0, "dv"),
    ("norescale", 192, "full", None, 2, "o"),
    ("norescale", 192, "causal", None, 2, "o"),
    # the staging: D = dO . bf16(O) differs from the exact rowsum(P . dP) by dO . (O - bf16(O)), which enters
    # every dS of the row with one sign; small elements of dQ show it (err / bound 11 at S = 192, full)
    ("D", 192, "full", None, 2, "dq"),
]


@pytest.mark.parametrize("mut,S,mask,W,which,out", MUTANTS)
def test_checkers_report_the_mutant(mut, S, mask, W, which, out):
    clean = _emulated_reports(S, mask, W)
    bad = _emulated_reports(S, mask, W, mut)
    assert not any(r.bad for reps in clean for r in reps)
    hit = [reps[which] for reps in bad if out in reps[which].bad]
    print("\n".join(reps[which].line() for reps in bad))
    assert hit, f"mutant {mut} not reported in {out}"
    if mut == "skip_t":  # the transposed walk alone: the forward's count is untouched
        assert all("lse" not in reps[0].bad and "o" not in reps[0].bad for reps in bad)


# ------------------------------------------------------------------------------------------ GPU
def _run(C, qkv, do, lens, causal, doc, window, p=0.0, step=None):
    win = () if not window else (int(window),)
    o, lse = C.attn_fwd(qkv, H, p, 11, step, lens, 0, causal, doc, *win)
    dqkv = C.attn_bwd(do, qkv, o, lse, H, p, 11, step, None, lens, 0, causal, doc, *win)
    return o, lse, dqkv


# (S, mask) of the GPU tests; S = 4096: B = 1 and the causal masks only
_SM = [(S, m) for S in SIZES for m in _masks(S) if S < 4096 or m not in ("full", "lens")]


@pytest.mark.gpu
@pytest.mark.parametrize("S,mask", _SM)
def test_zero_score_probes_pin_the_visible_keys(gpu, C, S, mask):
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    for tag, lens, causal, doc, B in _cases(S, mask):
        lens, doc = _dev(lens, gpu), _dev(doc, gpu)
        for zero in ("q", "k"):
            qkv, do = (t.to(gpu) for t in _probe_inputs(B, S, zero, 3))
            for W in (WINDOWS if "window" in mask else (None,)):
                o, lse, dqkv = _run(C, qkv, do, lens, causal, doc, W)
                case = tag + (f" W={W}" if W else "") + f" zero-{zero}"
                check_probe(qkv, do, H, lens, causal, doc, W, o, lse, dqkv, zero=zero, case=case).finish()
                if zero == "q":  # dropout acts on the probabilities, after the row sum
                    lse_p = _run(C, qkv, do, lens, causal, doc, W, 0.1, step)[1]
                    assert torch.equal(lse_p.view(torch.int32), lse.view(torch.int32)), f"{case}: lse with dropout"


@pytest.mark.gpu
@pytest.mark.parametrize("S", SIZES)
def test_probe_through_the_module(gpu, S, monkeypatch):
    """The same probe through FusedSelfAttention, on the kernels and not on SDPA."""
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    def no_sdpa(*a, **k):
        raise AssertionError("the probe took SDPA")

    monkeypatch.setattr(FusedSelfAttention, "_sdpa", no_sdpa)
    W = 65 if S >= 192 else None
    tag, lens, causal, doc, B = next(_cases(S, "window+docs+lens" if W else "causal+docs+lens"))
    lens, doc = _dev(lens, gpu), _dev(doc, gpu)
    qkv, do = (t.to(gpu) for t in _probe_inputs(B, S, "q", 3))
    m = FusedSelfAttention(H, p=0.0, causal=True, window=W).to(gpu)
    assert m._kernel_ok(qkv) if S <= 128 else m._long_kernel_ok(qkv)
    x = qkv.clone().requires_grad_(True)
    o = m(x, lens, doc)
    o.backward(do)
    check_probe(qkv, do, H, lens, causal, doc, W, o.detach(), None, x.grad, case=f"module {tag} W={W}").finish()


@pytest.mark.gpu
@pytest.mark.parametrize("S,mask", [sm for sm in _SM if sm[0] < 4096])
def test_random_inputs_per_element_fp64(gpu, C, S, mask):
    W = 100 if "window" in mask else None
    for tag, lens, causal, doc, B in _cases(S, mask, first_layout_only=True):
        lens, doc = _dev(lens, gpu), _dev(doc, gpu)
        qkv, do = _qkv(B, S, 1).to(gpu), _dout(B, S, 1).to(gpu)
        o, lse, dqkv = _run(C, qkv, do, lens, causal, doc, W)
        case = tag + (f" W={W}" if W else "") + " random"
        check_random(qkv, do, H, lens, causal, doc, W, o, lse, dqkv, case=case).finish()
