"""The fused residual add + dropout + RMSNorm kernels (kernels/rmsnorm.hip) against fp64 references, element
by element and row by row, with the helpers and the accuracy rule of tests/test_row_kernels_fp64.py:
reference = the formulas below in fp64 on the same bf16 inputs and on the kernel's own r_new and rstd,
yardstick = the same formulas in fp32 eager; bf16 outputs by ``rep.bf16``, the fp32 rstd by ``rep.fp32``.

    r_new = bf16(r + h * keep / (1 - p))          rstd = rsqrt(mean(r_new^2) + eps)
    y     = bf16(r_new * rstd * gamma)
    xh = r_new * rstd,  g = dy * gamma,  b = mean(g * xh)
    dr = bf16(dr_new + rstd * (g - xh * b))       dh = bf16(dr_fp32 * keep / (1 - p))
    dgamma[c] = sum over rows of dy * xh

The forward is checked in stages, as the LayerNorm's: r_new first (bitwise at p = 0; the one-ulp rule of
``_ln_forward`` with dropout, against the keep-mask of the LayerNorm kernel for the same seed and step --
the two must draw the same mask), then rstd and y from the kernel's own r_new, then the backward from
exactly the tensors it is given. Each case prints ROWERR lines (recorded in profiles/llama_block.md)."""
import pytest
import torch

from test_row_kernels_fp64 import SEED, _count_dy, _Err, _gen, _keep_mask, _ln_inputs, _same

pytestmark = pytest.mark.gpu

EPS = 1e-6
# Row counts, from the kernels' own constants (rmsnorm.hip): 256-lane workgroups = 4 waves, one row per wave
# per round. rms_fwd_blocks = min(ceil(rows / 4), 2048); rms_bwd_blocks = min(ceil(rows / 32), 512), one
# dgamma partial row per block; the finalize (ln_param_grad_kernel) gives each output 8 lanes, lane l walking
# partials l, l + 8, .., four at a time (an unrolled round of 32 partials) and the rest one by one.
#   1, 3, 5   a partial block with idle waves;  33  two backward blocks
#   800 / 1000 / 1057   25 / 32 / 34 partial rows: below one unrolled round (only lane 0 enters it), exactly
#                       one round for every lane, one round plus the tail
#   8197    one past the forward's wrap: 2048 blocks * 4 waves = 8192 rows, so 5 waves take a second row
#   16421   the backward sits at its 512-block cap (513 wanted): 2048 waves visit 8 or 9 rows each
ROWS = [1, 3, 5, 33, 800, 1000, 1057, 8197, 16421]
BWD_CAP_ROWS = 16421


def _step(gpu):
    return torch.tensor([3], device=gpu, dtype=torch.int64)


def _fwd_ref(rn, gamma, dt):
    x = rn.to(dt)
    rstd = ((x * x).mean(-1) + EPS).rsqrt()
    return rstd, x * rstd[:, None] * gamma.to(dt)


def _bwd_ref(dy, drn, rn, rstd, gamma, mask, p, dt):
    dy, rn, gamma, mask = dy.to(dt), rn.to(dt), gamma.to(dt), mask.to(dt)
    rstd = rstd.to(dt)[:, None]
    xh = rn * rstd
    g = dy * gamma
    b = (g * xh).mean(-1, keepdim=True)
    dr = rstd * (g - xh * b)
    if drn is not None:
        dr = drn.to(dt) + dr
    return {"dr": dr, "dh": dr * mask / (1 - p), "dgamma": (dy * xh).sum(0)}


def _check_r_new(r, h, r_new, mask, p):
    if p == 0:
        assert _same(r_new, (r.float() + h.float()).to(torch.bfloat16)), "r_new != bf16(r + h)"
        return
    # the rule of test_row_kernels_fp64._ln_forward for s: within one bf16 ulp of the rounded fp64 sum, plus
    # the fp32 roundings of 1 / (1 - p) and of the product where r and h / (1 - p) cancel
    want = (r.double() + h.double() * mask / (1 - p)).to(torch.bfloat16)
    ulp = torch.where(want == 0, 0.0, torch.exp2(torch.frexp(want.float())[1].double() - 8))
    over = (r_new.double() - want.double()).abs() - (ulp + 2.0 ** -23 * h.double().abs() / (1 - p))
    i = int(over.argmax())
    assert float(over.flatten()[i]) <= 0, (
        f"r_new = {float(r_new.flatten()[i])} is more than one bf16 ulp from bf16(r + h * mask / (1 - p)) = "
        f"{float(want.flatten()[i])} at element {i}")


def _check_fwd(rep, tag, r_new, y, rstd, gamma):
    r64, y64 = _fwd_ref(r_new, gamma, torch.float64)
    r32, y32 = _fwd_ref(r_new, gamma, torch.float32)
    rep.fp32(f"{tag}rstd", rstd, r64, r32)
    rep.bf16(f"{tag}y", y, y64, y32)


def _check_bwd(C, rep, tag, dy, drn, r_new, rstd, gamma, mask, p, step, had_h):
    dr, dh, dg = C.rms_bwd(dy, drn, r_new, rstd, gamma, p, SEED, step, had_h)
    r64 = _bwd_ref(dy, drn, r_new, rstd, gamma, mask, p, torch.float64)
    r32 = _bwd_ref(dy, drn, r_new, rstd, gamma, mask, p, torch.float32)
    rep.bf16(f"{tag}dr", dr, r64["dr"], r32["dr"])
    rep.bf16(f"{tag}dgamma", dg, r64["dgamma"], r32["dgamma"])
    if not had_h:
        assert dh is None
    elif p == 0:
        assert dh is dr, "at p = 0 dh must be the tensor dr itself"
    else:
        assert dh is not dr and dh.data_ptr() != dr.data_ptr()
        rep.bf16(f"{tag}dh", dh, r64["dh"], r32["dh"])
    return dr, dh, dg


@pytest.mark.parametrize("kind", ["randn", "offset"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_rows_match_fp64(gpu, C, H, rows, p, kind):
    r, h, gamma, _, dy = _ln_inputs(kind, rows, H, gpu)
    drn = torch.randn(rows, H, device=gpu, generator=_gen(gpu, rows, H, 5)).to(torch.bfloat16)
    step = _step(gpu)
    rep = _Err(f"rms H={H} rows={rows} p={p} {kind}")
    # with the branch h
    r_new, y, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)
    assert r_new is not r and rstd.shape == (rows,) and rstd.dtype == torch.float32
    mask = _keep_mask(C, rows, H, p, step, gpu)
    _check_r_new(r, h, r_new, mask, p)
    _check_fwd(rep, "", r_new, y, rstd, gamma)
    _check_bwd(C, rep, "", dy, drn, r_new, rstd, gamma, mask, p, step, True)
    _check_bwd(C, rep, "nodrn.", dy, None, r_new, rstd, gamma, mask, p, step, True)
    # without it: r_new is r itself, nothing is written, p / seed / step are ignored
    keep = r.clone()
    r2, y2, rstd2 = C.rms_fwd(r, None, gamma, EPS, p, SEED, step)
    assert r2 is r and _same(r, keep)
    _check_fwd(rep, "noh.", r, y2, rstd2, gamma)
    ones = torch.ones_like(mask)
    _check_bwd(C, rep, "noh.", dy, drn, r, rstd2, gamma, ones, 0.0, step, False)
    _check_bwd(C, rep, "noh.nodrn.", dy, None, r, rstd2, gamma, ones, 0.0, step, False)
    rep.finish()


@pytest.mark.parametrize("rows", [5, 8197])
@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_zero_rows(gpu, C, H, rows):
    """Rows of zeros: y is zero, rstd = rsqrt(eps) is finite, and the backward is finite."""
    z = torch.zeros(rows, H, device=gpu, dtype=torch.bfloat16)
    _, _, gamma, _, dy = _ln_inputs("randn", rows, H, gpu)
    for h in (z, None):
        r_new, y, rstd = C.rms_fwd(z, h, gamma, EPS, 0.1, SEED, _step(gpu))
        assert bool((r_new == 0).all()) and bool((y == 0).all())
        assert bool(torch.isfinite(rstd).all())
        torch.testing.assert_close(rstd, torch.full_like(rstd, EPS ** -0.5), rtol=1e-6, atol=0)
        for t in C.rms_bwd(dy, None, r_new, rstd, gamma, 0.1, SEED, _step(gpu), h is not None):
            assert t is None or bool(torch.isfinite(t.float()).all())


@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_counts_every_row_once(gpu, C, H):
    """r_new, rstd and gamma all ones and a dy of zeros and ones with integer column sums <= 256: dgamma must
    be that count bit for bit, at the backward's block cap -- a lost or doubled row or block partial cannot
    pass."""
    rows = BWD_CAP_ROWS
    one = torch.ones(rows, H, device=gpu, dtype=torch.bfloat16)
    rstd = torch.ones(rows, device=gpu, dtype=torch.float32)
    gamma = torch.ones(H, device=gpu, dtype=torch.bfloat16)
    dy, count = _count_dy(rows, H, gpu)
    for had_h, p in ((True, 0.0), (True, 0.1), (False, 0.0)):
        dg = C.rms_bwd(dy, None, one, rstd, gamma, p, SEED, _step(gpu), had_h)[2]
        assert _same(dg, count.to(torch.bfloat16)), (had_h, p)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("rows", [1057, BWD_CAP_ROWS])
@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_dgamma_out_keeps_every_bit(gpu, C, H, rows, p):
    """dgamma_out given (the PS grad sink) against not given: the given tensor is written and returned, and
    every output keeps its bits."""
    r, h, gamma, _, dy = _ln_inputs("randn", rows, H, gpu)
    step = _step(gpu)
    r_new, y, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)
    plain = C.rms_bwd(dy, r, r_new, rstd, gamma, p, SEED, step, True)
    buf = torch.full((H + 16,), -7.0, device=gpu, dtype=torch.bfloat16)
    out = buf[8:8 + H]
    into = C.rms_bwd(dy, r, r_new, rstd, gamma, p, SEED, step, True, out)
    assert into[2].data_ptr() == out.data_ptr()
    for name, a, b in zip(("dr", "dh", "dgamma"), plain, into):
        assert _same(a, b), name
    assert bool((buf[:8] == -7).all()) and bool((buf[8 + H:] == -7).all())


@pytest.mark.parametrize("H", [768, 1024])
def test_rmsnorm_is_deterministic(gpu, C, H):
    rows, p = BWD_CAP_ROWS, 0.1
    r, h, gamma, _, dy = _ln_inputs("randn", rows, H, gpu)
    step = _step(gpu)
    runs = []
    for _ in range(2):
        r_new, y, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)
        runs.append([r_new, y, rstd] + list(C.rms_bwd(dy, r, r_new, rstd, gamma, p, SEED, step, True)))
    for a, b in zip(*runs):
        assert _same(a, b)


def test_rmsnorm_mask_follows_the_device_step(gpu, C):
    """The step is read on the device: another value draws another mask, the same value the same one."""
    r, h, gamma, _, _ = _ln_inputs("randn", 33, 768, gpu)
    step = _step(gpu)
    a = C.rms_fwd(r, h, gamma, EPS, 0.1, SEED, step)[0]
    step.add_(1)
    b = C.rms_fwd(r, h, gamma, EPS, 0.1, SEED, step)[0]
    step.sub_(1)
    c = C.rms_fwd(r, h, gamma, EPS, 0.1, SEED, step)[0]
    assert not _same(a, b) and _same(a, c)


def test_rmsnorm_misuse_raises(gpu, C):
    """One misuse per argument: a RuntimeError that names it (the checks run before any allocation or launch)."""
    rows, H = 5, 768
    r, h, gamma, _, dy = _ln_inputs("randn", rows, H, gpu)
    step = _step(gpu)
    wide = torch.zeros(rows, 2 * H, device=gpu, dtype=torch.bfloat16)
    fwd = [
        ("r", lambda: C.rms_fwd(r.float(), h, gamma, EPS, 0.0, SEED, step)),  # another dtype
        ("r", lambda: C.rms_fwd(wide[:, :512].contiguous(), None, gamma[:512], EPS, 0.0, SEED, step)),  # H = 512
        ("r", lambda: C.rms_fwd(wide[:, :H], h, gamma, EPS, 0.0, SEED, step)),  # non-contiguous
        ("h", lambda: C.rms_fwd(r, h[:3].contiguous(), gamma, EPS, 0.0, SEED, step)),  # shape mismatch
        ("gamma", lambda: C.rms_fwd(r, h, gamma.cpu(), EPS, 0.0, SEED, step)),  # wrong device
        ("p", lambda: C.rms_fwd(r, h, gamma, EPS, 1.0, SEED, step)),
        ("step", lambda: C.rms_fwd(r, h, gamma, EPS, 0.1, SEED, step.int())),  # wrong dtype
    ]
    r_new, y, rstd = C.rms_fwd(r, h, gamma, EPS, 0.1, SEED, step)
    bwd = [
        ("dy", lambda: C.rms_bwd(dy.float(), None, r_new, rstd, gamma, 0.1, SEED, step, True)),
        ("dr_new", lambda: C.rms_bwd(dy, r[:3].contiguous(), r_new, rstd, gamma, 0.1, SEED, step, True)),
        ("r_new", lambda: C.rms_bwd(dy, None, wide[:, :H], rstd, gamma, 0.1, SEED, step, True)),
        ("rstd", lambda: C.rms_bwd(dy, None, r_new, rstd.double(), gamma, 0.1, SEED, step, True)),
        ("gamma", lambda: C.rms_bwd(dy, None, r_new, rstd, gamma[:512].contiguous(), 0.1, SEED, step, True)),
        ("p", lambda: C.rms_bwd(dy, None, r_new, rstd, gamma, -0.5, SEED, step, True)),
        ("step", lambda: C.rms_bwd(dy, None, r_new, rstd, gamma, 0.1, SEED, step.cpu(), True)),
        ("dgamma_out", lambda: C.rms_bwd(dy, None, r_new, rstd, gamma, 0.1, SEED, step, True, gamma.float())),
    ]
    for name, call in fwd + bwd:
        with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
            call()
