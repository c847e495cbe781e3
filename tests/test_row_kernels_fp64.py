"""The three row kernels of every BERT / GPT step -- LayerNorm(x + dropout(h)) and the fused embedding
block (kernels/layernorm.hip), softmax cross-entropy (kernels/xent.hip) -- against fp64 references,
element by element and row by row, at the row counts where their grids wrap, their block partials
change path and their chunk loops take a second round.

Accuracy rule (tests/test_optim_layerwise.py's, adapted to bf16 outputs). Reference: the same formulas
in fp64 torch on the same bf16 inputs. Yardstick: the same formulas in fp32 torch eager; E32 is its
largest absolute error against fp64 for one output tensor of one case.
  bf16 outputs, per element:   |got - ref64| <= 2^-8 |ref64| + 4 E32 + floor
  fp32 mean / rstd, per row:   |got - ref64| <= max(4 E32, floor)
  floor = two fp32 ulps of the tensor's max |ref64|.
2^-8 |ref| is at least half a bf16 ulp (the output rounding); 4x covers the other summation order.
Cross-entropy's lse and loss_row keep rtol = atol = 1e-5 of test_kernels.py, per row instead of on the
mean (the kernel's __expf / __logf are not what fp32 eager runs, so 4x eager is no yardstick there).

The forwards are checked in stages so that errors do not compound: the bf16 sum s first (bitwise
without dropout; with it, one bf16 ulp plus the fp32 product rounding where x and h / (1 - p) cancel,
see _ln_forward), then mean / rstd / y from the kernel's own s, then the backward from exactly the
tensors it is given. Each case prints one ROWERR line: per output the error and bound at the element
with the worst error / bound, the largest error, and E32 (recorded in profiles/row_kernels_fp64.md).
Every id, type, label and position here is in range."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

EPS32 = 2.0 ** -23
EPS = 1e-12
SEED = 7
INF = float("inf")


# ------------------------------------------------------------------------------------------ helpers
def _raw(t):
    return t.contiguous().view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[t.element_size()])


def _same(a, b):
    """Bitwise equal (dtype, shape and every bit)."""
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(_raw(a), _raw(b))


class _Err:
    """Collects one case's checks, prints its ROWERR line, fails on any element above its bound."""

    def __init__(self, case):
        self.case, self.cells, self.bad = case, [], []

    def _add(self, name, got, ref, bound, e32):
        if not bool(torch.isfinite(got).all()):
            self.cells.append(f"{name}: non-finite")
            self.bad.append(f"{name}: non-finite values")
            return
        err = (got.double() - ref).abs().flatten()
        bound = bound.expand_as(ref).flatten()
        q = torch.where(err == 0, torch.zeros_like(err), err / bound)
        i = int(q.argmax())
        cell = (f"{name}: err {float(err[i]):.3e} bound {float(bound[i]):.3e} err/bound {float(q[i]):.3f} "
                f"maxerr {float(err.max()):.3e} eager {e32:.3e}")
        self.cells.append(cell)
        if float(q[i]) > 1.0:
            self.bad.append(cell)

    def bf16(self, name, got, ref, eager):
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
        ref = ref.double()
        e32 = float((eager.double() - ref).abs().max())
        floor = 2 * EPS32 * float(ref.abs().max())
        self._add(name, got, ref, ref.abs() * 2.0 ** -8 + (4 * e32 + floor), e32)

    def fp32(self, name, got, ref, eager):
        assert got.dtype == torch.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
        ref = ref.double()
        e32 = float((eager.double() - ref).abs().max())
        floor = 2 * EPS32 * float(ref.abs().max())
        self._add(name, got, ref, torch.full_like(ref, max(4 * e32, floor)), e32)

    def tol(self, name, got, ref, eager, rtol=1e-5, atol=1e-5):
        assert got.dtype == torch.float32 and got.shape == ref.shape, (name, got.dtype, got.shape, ref.shape)
        ref = ref.double()
        self._add(name, got, ref, atol + rtol * ref.abs(), float((eager.double() - ref).abs().max()))

    def finish(self):
        print(f"ROWERR {self.case} | " + " | ".join(self.cells))
        assert not self.bad, f"{self.case}: above the bound:\n" + "\n".join(self.bad)


def _gen(gpu, *key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator(device=gpu).manual_seed(seed)


def _affine(g, H, gpu):
    gamma = (torch.rand(H, device=gpu, generator=g) + 0.5).to(torch.bfloat16)
    beta = (torch.rand(H, device=gpu, generator=g) - 0.5).to(torch.bfloat16)
    return gamma, beta


def _keep_mask(C, rows, H, p, step, gpu):
    from test_layernorm import _mask

    if p == 0:
        return torch.ones(rows, H, device=gpu, dtype=torch.float64)
    return _mask(C, (rows, H), p, SEED, step, gpu).double()


def _count_dy(rows, H, gpu):
    """dy of zeros and ones whose column sums are small integers: exact in bf16 and in any fp32 order."""
    r = torch.arange(rows, device=gpu)[:, None]
    c = torch.arange(H, device=gpu)[None, :]
    hit = (r + c) % 65 == 0
    count = hit.sum(0)
    assert int(count.max()) <= 256 and int(count.max()) - int(count.min()) <= 1
    return hit.to(torch.bfloat16), count


def _ln_stats(sv, eps):
    mean = sv.mean(-1)
    d = sv - mean[:, None]
    rstd = ((d * d).mean(-1) + eps).rsqrt()
    return mean, rstd, d * rstd[:, None]


def _ln_bwd_ref(dy, xsum, mean, rstd, gamma, mask, p, dt, types=None, NT=0):
    """LayerNorm backward from exactly what the kernel is given (xsum: the LN input), in dtype dt."""
    dy, xsum, gamma, mask = dy.to(dt), xsum.to(dt), gamma.to(dt), mask.to(dt)
    mean, rstd = mean.to(dt)[:, None], rstd.to(dt)[:, None]
    xh = (xsum - mean) * rstd
    dxh = dy * gamma
    a = dxh.mean(-1, keepdim=True)
    b = (dxh * xh).mean(-1, keepdim=True)
    dx = rstd * (dxh - a - xh * b)
    out = {"dx": dx, "dgamma": (dy * xh).sum(0), "dbeta": dy.sum(0)}
    out["dh"] = dx * mask / (1 - p)
    out["dhsum"] = out["dh"].sum(0)
    if NT:
        out["dT"] = torch.stack([(dx * (types == k)[:, None]).sum(0) for k in range(NT)])
    return out


# ------------------------------------------------------------------------------------------ LayerNorm
# rows: 1, 3, 5 a partial block with idle waves; 33 two backward blocks; 800 / 1000 / 1057 the gamma/beta
# finalize at 25 / 32 / 34 block partials (first entry of its unrolled loop, exactly one unrolled round,
# unrolled + tail); 8197 the forward wraps its 2048-block grid (5 waves take a second row); 16421 the
# backward is at its 512-block cap (waves visit 8 or 9 rows)
LN_CASES = [(1, 0.0), (3, 0.0), (5, 0.0), (5, 0.1), (33, 0.0), (800, 0.0), (1000, 0.0), (1057, 0.0), (1057, 0.1),
            (8197, 0.0), (8197, 0.1), (16421, 0.0), (16421, 0.1)]


def _ln_inputs(kind, rows, H, gpu):
    g = _gen(gpu, rows, H, len(kind))
    if kind == "randn":
        x = torch.randn(rows, H, device=gpu, generator=g)
        h = torch.randn(rows, H, device=gpu, generator=g)
    elif kind == "offset":  # mean 50, deviation 0.7: a one-pass E[x^2] - mean^2 variance loses every digit
        x = torch.randn(rows, H, device=gpu, generator=g) * 0.5 + 50
        h = torch.randn(rows, H, device=gpu, generator=g) * 0.5
    else:  # "const": every element of a row equal
        x = (torch.randn(rows, 1, device=gpu, generator=g) * 3).expand(rows, H)
        h = torch.randn(rows, 1, device=gpu, generator=g).expand(rows, H)
    gamma, beta = _affine(g, H, gpu)
    dy = (torch.randn(rows, H, device=gpu, generator=g) + 1).to(torch.bfloat16)
    return x.to(torch.bfloat16).contiguous(), h.to(torch.bfloat16).contiguous(), gamma, beta, dy


def _ln_forward(C, gpu, rep, x, h, gamma, beta, p):
    """Runs ln_fwd and checks s, then mean / rstd / y from the kernel's own s. Returns its outputs,
    the keep-mask and the step tensor."""
    rows, H = x.shape
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    y, s, mean, rstd = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)
    mask = _keep_mask(C, rows, H, p, step, gpu)
    if p == 0:
        assert _same(s, (x.float() + h.float()).to(torch.bfloat16)), "s != bf16(x + h)"
    else:
        # within one bf16 ulp of the rounded fp64 sum (hv * scale + xv may or may not be contracted into
        # an fma). Where x and h / (1 - p) cancel, the fp32 roundings of 1 / (1 - p) and of the product
        # (2^-24 of |h| / (1 - p) each) can exceed an ulp of the tiny sum -- among 10^6 randn elements a
        # few sums fall below 2^-16 |x| -- so that much is allowed on top; it is far below an ulp elsewhere
        want = (x.double() + h.double() * mask / (1 - p)).to(torch.bfloat16)
        ulp = torch.where(want == 0, 0.0, torch.exp2(torch.frexp(want.float())[1].double() - 8))
        over = (s.double() - want.double()).abs() - (ulp + 2.0 ** -23 * h.double().abs() / (1 - p))
        i = int(over.argmax())
        assert float(over.flatten()[i]) <= 0, (
            f"s = {float(s.flatten()[i])} is more than one bf16 ulp from bf16(x + h * mask / (1 - p)) = "
            f"{float(want.flatten()[i])} at element {i}")
    m64, r64, xh64 = _ln_stats(s.double(), EPS)
    m32, r32, xh32 = _ln_stats(s.float(), EPS)
    rep.fp32("mean", mean, m64, m32)
    rep.fp32("rstd", rstd, r64, r32)
    rep.bf16("y", y, xh64 * gamma.double() + beta.double(), xh32 * gamma.float() + beta.float())
    return (y, s, mean, rstd), mask, step


def _ln_backward(C, rep, dy, s, mean, rstd, gamma, mask, p, step, dhsum=False):
    H = s.shape[-1]
    hs = torch.empty(H, device=s.device, dtype=torch.bfloat16) if dhsum else None
    dx, dh, dg, db = C.ln_bwd(dy, s, mean, rstd, gamma, p, SEED, step, None, None, hs)
    r64 = _ln_bwd_ref(dy, s, mean, rstd, gamma, mask, p, torch.float64)
    r32 = _ln_bwd_ref(dy, s, mean, rstd, gamma, mask, p, torch.float32)
    got = {"dx": dx, "dh": dh, "dgamma": dg, "dbeta": db}
    if dhsum:
        got["dhsum"] = hs
    for k, v in got.items():
        rep.bf16(k, v, r64[k], r32[k])
    return got


@pytest.mark.parametrize("kind", ["randn", "offset"])
@pytest.mark.parametrize("rows,p", LN_CASES)
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_rows_match_fp64(gpu, C, H, rows, p, kind):
    x, h, gamma, beta, dy = _ln_inputs(kind, rows, H, gpu)
    rep = _Err(f"ln H={H} rows={rows} p={p} {kind}")
    (y, s, mean, rstd), mask, step = _ln_forward(C, gpu, rep, x, h, gamma, beta, p)
    _ln_backward(C, rep, dy, s, mean, rstd, gamma, mask, p, step)
    rep.finish()


@pytest.mark.parametrize("rows", [37, 8197])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_constant_rows(gpu, C, H, rows):
    """Every element of a row equal and eps = 1e-12: the variance is exactly 0 (so is the fp64
    reference's), y must be beta bit for bit, rstd finite, and the backward finite."""
    x, h, gamma, beta, dy = _ln_inputs("const", rows, H, gpu)
    rep = _Err(f"ln-const H={H} rows={rows}")
    (y, s, mean, rstd), mask, step = _ln_forward(C, gpu, rep, x, h, gamma, beta, 0.0)
    rep.finish()
    assert bool((s == s[:, :1]).all())
    assert _same(y, beta[None, :].expand(rows, H).contiguous())
    assert bool(torch.isfinite(rstd).all()) and bool(torch.isfinite(mean).all())
    for t in C.ln_bwd(dy, s, mean, rstd, gamma, 0.0, SEED, step):
        assert bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("rows", [1057, 16421])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_counts_every_row_once(gpu, C, H, rows):
    """dy of zeros and ones with integer column sums <= 256: dbeta must be that count bit for bit -- a
    lost or doubled block partial of the gamma/beta finalize cannot pass. dgamma under the rule."""
    x, h, gamma, beta, _ = _ln_inputs("randn", rows, H, gpu)
    dy, count = _count_dy(rows, H, gpu)
    rep = _Err(f"ln-count H={H} rows={rows}")
    (y, s, mean, rstd), mask, step = _ln_forward(C, gpu, rep, x, h, gamma, beta, 0.0)
    got = _ln_backward(C, rep, dy, s, mean, rstd, gamma, mask, 0.0, step)
    rep.finish()
    assert _same(got["dbeta"], count.to(torch.bfloat16))


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1057, 16421])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_dhsum_variant(gpu, C, H, rows, p):
    """With dhsum_out the backward also sums dh's columns; everything else keeps its bits."""
    x, h, gamma, beta, dy = _ln_inputs("randn", rows, H, gpu)
    rep = _Err(f"ln-dhsum H={H} rows={rows} p={p}")
    (y, s, mean, rstd), mask, step = _ln_forward(C, gpu, rep, x, h, gamma, beta, p)
    got = _ln_backward(C, rep, dy, s, mean, rstd, gamma, mask, p, step, dhsum=True)
    rep.finish()
    plain = C.ln_bwd(dy, s, mean, rstd, gamma, p, SEED, step)
    for k, t in zip(("dx", "dh", "dgamma", "dbeta"), plain):
        assert _same(got[k], t), k


@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_backward_is_deterministic(gpu, C, H):
    rows, p = 16421, 0.1
    x, h, gamma, beta, dy = _ln_inputs("randn", rows, H, gpu)
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    y, s, mean, rstd = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)
    runs = []
    for _ in range(2):
        hs = torch.empty(H, device=gpu, dtype=torch.bfloat16)
        runs.append(list(C.ln_bwd(dy, s, mean, rstd, gamma, p, SEED, step, None, None, hs)) + [hs])
    for a, b in zip(*runs):
        assert _same(a, b)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [5, 8197])
@pytest.mark.parametrize("H", [768, 1024])
def test_layernorm_mx_operand_is_quant_mx_of_y(gpu, C, H, rows, p):
    """The MX e4m3 copy ln_fwd writes for the consumer Linear: bitwise quant_mx_ of the returned y, at
    both hidden sizes (H = 1024 is the two-lanes-per-block map) and past the forward's grid wrap; the
    other outputs keep the bits of the call without it."""
    g = _gen(gpu, rows, H, 99)
    # columns of very different magnitude: the block scales differ along the row
    spread = torch.exp2(torch.randint(-4, 5, (1, H), device=gpu, generator=g).float())
    x = (torch.randn(rows, H, device=gpu, generator=g) * spread).to(torch.bfloat16)
    h = torch.randn(rows, H, device=gpu, generator=g).to(torch.bfloat16)
    gamma, beta = _affine(g, H, gpu)
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    plain = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)
    q8 = torch.empty(rows, H, device=gpu, dtype=torch.float8_e4m3fn)
    sc8 = torch.empty(rows * H // 32, device=gpu, dtype=torch.uint8)
    both = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step, q8, sc8)
    for name, a, b in zip(("y", "s", "mean", "rstd"), plain, both):
        assert _same(a, b), name
    q = torch.empty(rows, H, device=gpu, dtype=torch.float8_e4m3fn)
    sc = torch.empty(rows * H // 32, device=gpu, dtype=torch.uint8)
    C.quant_mx_(both[0], q, sc)
    assert _same(sc8, sc)
    assert _same(q8, q)
    assert len(torch.unique(sc)) > 1


# ------------------------------------------------------------------------------------------ embedding + LN
EMB_V, EMB_H, EMB_MAXPOS = 1000, 768, 64
# (B, S, NT, p, kind, pos_ids): rows = B * S. 5 and 148 a partial / a few blocks; 16392 the backward's
# 512-block cap; 32776 the forward wraps its 8192-block grid
EMB_CASES = [
    (1, 5, 2, 0.0, "randn", False), (1, 5, 1, 0.0, "offset", False),
    (4, 37, 1, 0.0, "randn", False), (4, 37, 1, 0.1, "offset", False),
    (4, 37, 2, 0.0, "offset", True), (4, 37, 2, 0.1, "randn", False),
    (4, 37, 3, 0.1, "randn", False), (4, 37, 3, 0.0, "offset", False),
    (2049, 8, 2, 0.0, "randn", True), (2049, 8, 1, 0.0, "offset", False),
    (4097, 8, 2, 0.0, "offset", False), (4097, 8, 2, 0.1, "randn", False),
    (4097, 8, 1, 0.1, "offset", False), (4097, 8, 1, 0.0, "randn", False),
]


def _emb_inputs(B, S, NT, kind, pos_ids, gpu):
    rows = B * S
    g = _gen(gpu, rows, NT, len(kind), int(pos_ids))

    def table(n, add=0.0):
        return (torch.randn(n, EMB_H, device=gpu, generator=g) * 0.5 + add).to(torch.bfloat16)

    W, P, T = table(EMB_V), table(EMB_MAXPOS, 50.0 if kind == "offset" else 0.0), table(NT)
    gamma, beta = _affine(g, EMB_H, gpu)
    ids = torch.randint(0, EMB_V, (rows,), device=gpu, generator=g)
    ids[: min(10, rows - 1)] = 3  # a run of repeated ids
    types = torch.randint(0, NT, (rows,), device=gpu, generator=g)
    # positions that restart every 7 tokens (packed documents), or the column index r % S
    pos = torch.arange(rows, device=gpu) % 7 if pos_ids else None
    dy = (torch.randn(rows, EMB_H, device=gpu, generator=g) + 1).to(torch.bfloat16)
    assert 0 <= int(ids.min()) and int(ids.max()) < EMB_V and 0 <= int(types.min()) and int(types.max()) < NT
    assert S <= EMB_MAXPOS and (pos is None or (0 <= int(pos.min()) and int(pos.max()) < EMB_MAXPOS))
    return W, P, T, gamma, beta, ids, types, pos, dy


def _emb_case(C, gpu, rep, B, S, NT, p, kind, pos_ids, dy=None):
    rows, H = B * S, EMB_H
    W, P, T, gamma, beta, ids, types, pos, dy_r = _emb_inputs(B, S, NT, kind, pos_ids, gpu)
    dy = dy_r if dy is None else dy
    step = torch.tensor([5], device=gpu, dtype=torch.int64)
    y, mean, rstd = C.emb_ln_fwd(ids, types, W, P, T, gamma, beta, S, EPS, p, SEED, step, pos)
    mask = _keep_mask(C, rows, H, p, step, gpu)
    prow = pos if pos is not None else torch.arange(rows, device=gpu) % S
    x64 = (W[ids].double() + P[prow].double()) + T[types].double()
    x32 = (W[ids].float() + P[prow].float()) + T[types].float()
    m64, r64, xh64 = _ln_stats(x64, EPS)
    m32, r32, xh32 = _ln_stats(x32, EPS)
    rep.fp32("mean", mean, m64, m32)
    rep.fp32("rstd", rstd, r64, r32)
    rep.bf16("y", y, (xh64 * gamma.double() + beta.double()) * mask / (1 - p),
             (xh32 * gamma.float() + beta.float()) * mask.float() / (1 - p))
    dx, dg, db, dT = C.emb_ln_bwd(dy, ids, types, W, P, T, gamma, mean, rstd, S, p, SEED, step, None, None, None, pos)
    # the dropout sits on the LayerNorm's output: the gradient entering the LN backward is dy * mask / (1 - p)
    nt = NT if NT <= 2 else 0
    one = torch.ones_like(mask)
    b64 = _ln_bwd_ref(dy.double() * mask / (1 - p), x64, mean, rstd, gamma, one, 0.0, torch.float64, types, nt)
    b32 = _ln_bwd_ref(dy.float() * mask.float() / (1 - p), x32, mean, rstd, gamma, one, 0.0, torch.float32, types, nt)
    got = {"dx": dx, "dgamma": dg, "dbeta": db}
    if nt:
        assert dT is not None and tuple(dT.shape) == (NT, H)
        got["dT"] = dT
    else:
        assert dT is None  # more than two types: the caller sums the type rows
    for k, v in got.items():
        rep.bf16(k, v, b64[k], b32[k])
    return got


@pytest.mark.parametrize("B,S,NT,p,kind,pos_ids", EMB_CASES)
def test_embedding_layernorm_rows_match_fp64(gpu, C, B, S, NT, p, kind, pos_ids):
    rep = _Err(f"emb rows={B * S} S={S} NT={NT} p={p} {kind}{' pos_ids' if pos_ids else ''}")
    _emb_case(C, gpu, rep, B, S, NT, p, kind, pos_ids)
    rep.finish()


def test_embedding_layernorm_counts_every_row_once(gpu, C):
    """As the LayerNorm's: dbeta of a 0/1 dy is the integer count bit for bit, at the backward's block cap."""
    B, S = 2049, 8
    dy, count = _count_dy(B * S, EMB_H, gpu)
    rep = _Err(f"emb-count rows={B * S} S={S} NT=2")
    got = _emb_case(C, gpu, rep, B, S, 2, 0.0, "randn", False, dy=dy)
    rep.finish()
    assert _same(got["dbeta"], count.to(torch.bfloat16))


# ------------------------------------------------------------------------------------------ cross-entropy
# V: 8 one chunk and 255 empty threads; 264; 2048 exactly one 16-byte chunk per thread; 2056; 4096 two each
XENT_V = [8, 264, 2048, 2056, 4096]
XENT_KINDS = {"randn3": (3.0, 0.0), "randn3+80": (3.0, 80.0), "randn30": (30.0, 0.0)}  # +80: exp overflows fp32 unshifted


def _xent_inputs(rows, V, kind, gpu, hi=None):
    """Logits and labels; labels include 0, V - 1, one in the last chunk and ignored (-100) rows."""
    g = _gen(gpu, rows, V, len(kind))
    mul, add = XENT_KINDS[kind]
    x = (torch.randn(rows, V, device=gpu, generator=g) * mul + add).to(torch.bfloat16)
    hi = V if hi is None else hi  # labels below hi
    y = torch.randint(0, hi, (rows,), device=gpu, generator=g)
    if rows == 1:
        y[0] = hi - 1
    else:
        y[0], y[1], y[2] = 0, hi - 1, max(hi - 3, 0)
        y[3::7] = -100
    return x, y


def _xent_ref(x, y, up, dt):
    xd = x.to(dt)
    V = x.shape[1]
    valid = y >= 0
    ys = y.clamp_min(0)
    lse = torch.logsumexp(xd, -1)
    loss_row = torch.where(valid, lse - xd.gather(1, ys[:, None])[:, 0], torch.zeros_like(lse))
    count = max(int(valid.sum()), 1)
    dx = (torch.softmax(xd, -1) - F.one_hot(ys, V).to(dt)) * valid[:, None].to(dt) * (up / count)
    return lse, loss_row, loss_row.sum() / count, dx


def _xent_check(C, rep, x, y, up):
    """Forward per row and through the wrapper, gradient under the accuracy rule. Returns
    (loss_row, lse, lse_lo, loss, dx) of the kernels."""
    from parameter_server_distributed_amd.ops.loss import cross_entropy

    lse64, row64, loss64, dx64 = _xent_ref(x, y, up, torch.float64)
    lse32, row32, loss32, dx32 = _xent_ref(x, y, up, torch.float32)
    loss_row, lse, lse_lo = C.xent_fwd(x, y)
    rep.tol("lse", lse, lse64, lse32)
    # lse_lo is what one fp32 addition rounded away: at most half an ulp of lse
    assert lse_lo.dtype == torch.float32 and bool((lse_lo.abs() <= 2.0 ** -24 * lse.abs()).all())
    rep.tol("loss_row", loss_row, row64, row32)
    xk = x.detach().requires_grad_(True)
    loss = cross_entropy(xk, y)
    loss.backward(torch.tensor(up, device=x.device))
    rep.tol("loss", loss.detach(), loss64, loss32)
    assert xk.grad.dtype == torch.bfloat16 and xk.grad.is_contiguous() and xk.grad.shape == x.shape
    rep.bf16("dx", xk.grad, dx64, dx32)
    return loss_row, lse, lse_lo, loss.detach(), xk.grad


@pytest.mark.parametrize("up", [1.0, 0.37])
@pytest.mark.parametrize("kind", list(XENT_KINDS))
@pytest.mark.parametrize("V", XENT_V)
@pytest.mark.parametrize("rows", [1, 37])
def test_cross_entropy_rows_match_fp64(gpu, C, rows, V, kind, up):
    x, y = _xent_inputs(rows, V, kind, gpu)
    rep = _Err(f"xent rows={rows} V={V} {kind} up={up}")
    loss_row, lse, lse_lo, loss, dx = _xent_check(C, rep, x, y, up)
    rep.finish()
    assert bool((loss_row[y < 0] == 0).all()) and bool((dx[y < 0] == 0).all())
    # a row stride other than V: the same bits, and a contiguous [rows, V] gradient
    buf = torch.zeros(rows, V + 64, device=gpu, dtype=torch.bfloat16)
    buf[:, :V] = x
    xs = buf[:, :V]
    assert xs.stride(0) == V + 64 and (rows == 1 or not xs.is_contiguous())
    for a, b in zip(C.xent_fwd(xs, y), (loss_row, lse, lse_lo)):
        assert _same(a, b)
    scale = torch.tensor([up / max(int((y >= 0).sum()), 1)], device=gpu, dtype=torch.float32)
    ds = C.xent_bwd(xs, y, lse, scale, lse_lo)
    assert ds.is_contiguous() and ds.shape == x.shape
    assert _same(ds, C.xent_bwd(x, y, lse, scale, lse_lo))  # also: backward twice gives the same bits
    from parameter_server_distributed_amd.ops.loss import cross_entropy

    xk = xs.detach().requires_grad_(True)
    ls = cross_entropy(xk, y)
    ls.backward(torch.tensor(up, device=gpu))
    assert _same(ls.detach(), loss) and xk.grad.is_contiguous() and _same(xk.grad, dx)


@pytest.mark.parametrize("kind", ["randn3", "randn3+80"])
def test_cross_entropy_all_rows_ignored(gpu, C, kind):
    """Every label -100: the wrapper's count is clamped to 1, so the loss is exactly 0 and the
    gradient exactly zero (F.cross_entropy gives NaN here: no reference)."""
    from parameter_server_distributed_amd.ops.loss import cross_entropy

    x, _ = _xent_inputs(37, 264, kind, gpu)
    y = torch.full((37,), -100, device=gpu, dtype=torch.int64)
    xk = x.detach().requires_grad_(True)
    loss = cross_entropy(xk, y)
    loss.backward(torch.tensor(0.37, device=gpu))
    assert float(loss) == 0.0
    assert bool((xk.grad == 0).all())
    loss_row, lse, _ = C.xent_fwd(x, y)
    assert bool((loss_row == 0).all()) and bool(torch.isfinite(lse).all())


@pytest.mark.parametrize("V,lo", [(4096, 4000), (264, 259)])
@pytest.mark.parametrize("rows", [1, 37])
def test_cross_entropy_masked_vocabulary(gpu, C, rows, V, lo):
    """Columns [lo, V) at -inf (a padded vocabulary's tail). V = 4096: twelve whole 16-byte chunks, each
    the second chunk of its thread, whose running max is finite by then; V = 264: part of one chunk.
    lse, loss and gradient match fp64 (finite there); the masked columns' gradient is exactly 0."""
    x, y = _xent_inputs(rows, V, "randn3", gpu, hi=lo)
    x[:, lo:] = -INF
    assert int(y.max()) < lo
    ref = F.cross_entropy(x.double(), y, reduction="none")  # -100 rows: 0
    assert bool(torch.isfinite(ref).all())
    rep = _Err(f"xent-masked rows={rows} V={V} -inf from {lo}")
    loss_row, lse, lse_lo, loss, dx = _xent_check(C, rep, x, y, 0.37)
    rep.tol("loss_row_vs_F", loss_row, ref, F.cross_entropy(x.float(), y, reduction="none"))
    rep.finish()
    assert bool((dx[:, lo:] == 0).all())
    scale = torch.tensor([0.37], device=gpu, dtype=torch.float32)
    assert _same(C.xent_bwd(x, y, lse, scale, lse_lo), C.xent_bwd(x, y, lse, scale, lse_lo))


def test_cross_entropy_backward_refuses_unaligned_rows(gpu, C):
    """xent_bwd writes 16-byte vectors at dx + r * V: a class count that is no multiple of 8 is refused
    before any launch, even when the logits' own row stride is fine."""
    x = torch.zeros(4, 16, device=gpu, dtype=torch.bfloat16)[:, :12]
    y = torch.zeros(4, device=gpu, dtype=torch.int64)
    lse = torch.zeros(4, device=gpu, dtype=torch.float32)
    scale = torch.ones(1, device=gpu, dtype=torch.float32)
    with pytest.raises(RuntimeError, match="multiple of 8"):
        C.xent_bwd(x, y, lse, scale)
