"""The wide fused add + RMSNorm kernels (kernels/rmsnorm_wide.hip, H = 512 n from 1536 to 8192) with the checks,
references and accuracy rule of tests/test_rmsnorm.py; the MX side outputs as tests/test_llama_fp8.py checks the
narrow kernels'. Each rows case prints its ROWERR line (recorded in profiles/rmsnorm_wide.md)."""
import pytest
import torch

from test_llama_fp8 import _mx_out, _rms_inputs, _same_as_ref
from test_rmsnorm import EPS, _check_bwd, _check_fwd, _check_r_new, _step
from test_row_kernels_fp64 import SEED, _count_dy, _Err, _gen, _keep_mask, _ln_inputs, _same

pytestmark = pytest.mark.gpu

# Row counts, from the launchers' constants (rmsnorm_wide.hip): one 256-lane workgroup per row per round.
# rms_wide_fwd_blocks = min(rows, 2048); rms_wide_bwd_blocks = min(ceil(rows / 8), 1024), one dgamma partial row each.
#   2049   one past the forward's cap: workgroup 0 takes a second row (and the LDS slot alternates)
#   8193   the backward sits at its 1024-block cap (1025 wanted): workgroups visit 8 or 9 rows
FWD_WRAP_ROWS, BWD_CAP_ROWS = 2049, 8193
# H: 1536 a partly filled slab (one idle wave), 2048 exactly one slab, 2560 a slab and a quarter, 8192 four slabs
ROW_CASES = [(H, rows) for H in (1536, 2048, 2560, 8192) for rows in (1, 3)] + [(1536, FWD_WRAP_ROWS), (1536, BWD_CAP_ROWS)]


def _mask(C, rows, H, p, step, gpu):
    """The LayerNorm kernel's keep-mask of the same flat elements (it runs at H = 768 / 1024 only)."""
    if p == 0:
        return torch.ones(rows, H, device=gpu, dtype=torch.float64)
    W = 768 if rows * H % 1024 else 1024
    assert rows * H % W == 0
    return _keep_mask(C, rows * H // W, W, p, step, gpu).view(rows, H)


@pytest.mark.parametrize("kind", ["randn", "offset"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H,rows", ROW_CASES)
def test_rmsnorm_wide_rows_match_fp64(gpu, C, H, rows, p, kind):
    if p and rows * H % 1024 and rows * H % 768:
        rows += 1  # H = 2560, one row: 2560 elements are no whole LayerNorm rows, two rows are
    r, h, gamma, _, dy = _ln_inputs(kind, rows, H, gpu)
    drn = torch.randn(rows, H, device=gpu, generator=_gen(gpu, rows, H, 5)).to(torch.bfloat16)
    step = _step(gpu)
    rep = _Err(f"rms H={H} rows={rows} p={p} {kind}")
    r_new, y, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)
    assert r_new is not r and rstd.shape == (rows,) and rstd.dtype == torch.float32
    mask = _mask(C, rows, H, p, step, gpu)
    _check_r_new(r, h, r_new, mask, p)
    _check_fwd(rep, "", r_new, y, rstd, gamma)
    _check_bwd(C, rep, "", dy, drn, r_new, rstd, gamma, mask, p, step, True)
    _check_bwd(C, rep, "nodrn.", dy, None, r_new, rstd, gamma, mask, p, step, True)
    # without h: r_new is r itself, nothing is written
    keep = r.clone()
    r2, y2, rstd2 = C.rms_fwd(r, None, gamma, EPS, p, SEED, step)
    assert r2 is r and _same(r, keep)
    _check_fwd(rep, "noh.", r, y2, rstd2, gamma)
    ones = torch.ones_like(mask)
    _check_bwd(C, rep, "noh.", dy, drn, r, rstd2, gamma, ones, 0.0, step, False)
    _check_bwd(C, rep, "noh.nodrn.", dy, None, r, rstd2, gamma, ones, 0.0, step, False)
    rep.finish()


@pytest.mark.parametrize("H", [1536, 8192])
def test_rmsnorm_wide_counts_every_row_once(gpu, C, H):
    """As test_rmsnorm_counts_every_row_once: dgamma of a 0 / 1 dy is the integer count bit for bit at the block cap."""
    rows = BWD_CAP_ROWS
    one = torch.ones(rows, H, device=gpu, dtype=torch.bfloat16)
    rstd = torch.ones(rows, device=gpu, dtype=torch.float32)
    gamma = torch.ones(H, device=gpu, dtype=torch.bfloat16)
    dy, count = _count_dy(rows, H, gpu)
    for had_h, p in ((True, 0.0), (True, 0.1), (False, 0.0)):
        dg = C.rms_bwd(dy, None, one, rstd, gamma, p, SEED, _step(gpu), had_h)[2]
        assert _same(dg, count.to(torch.bfloat16)), (had_h, p)


@pytest.mark.parametrize("with_h", [True, False])
@pytest.mark.parametrize("rows", [5, FWD_WRAP_ROWS])
@pytest.mark.parametrize("H", [1536, 2560])
def test_rmsnorm_wide_forward_writes_the_mx_copy_of_y(gpu, C, H, rows, with_h):
    r, h, _, _, gamma = _rms_inputs(rows, H, gpu)
    h = h if with_h else None
    plain = C.rms_fwd(r, h, gamma, EPS, 0.1, 11, None)
    q8, sc8 = _mx_out(r, False)
    both = C.rms_fwd(r, h, gamma, EPS, 0.1, 11, None, q8, sc8)
    for a, b in zip(plain, both):  # r_new, y, rstd
        assert _same(a, b)
    _same_as_ref(both[1], q8, sc8, False)


@pytest.mark.parametrize("with_drn", [True, False])
@pytest.mark.parametrize("p", [0.0, 0.1])  # dh is dr itself / a tensor of its own
@pytest.mark.parametrize("rows", [5, 70])  # one workgroup takes all five rows; nine take 7 or 8 each
@pytest.mark.parametrize("H", [1536, 2560])
def test_rmsnorm_wide_backward_writes_the_e5m2_copy_of_dh(gpu, C, H, rows, p, with_drn):
    r, h, dy, drn, gamma = _rms_inputs(rows, H, gpu)
    drn = drn if with_drn else None
    r_new, _, rstd = C.rms_fwd(r, h, gamma, EPS, p, 11, None)
    plain = C.rms_bwd(dy, drn, r_new, rstd, gamma, p, 11, None, True, None)
    q8, sc8 = _mx_out(r, True)
    dr, dh, dg = C.rms_bwd(dy, drn, r_new, rstd, gamma, p, 11, None, True, None, q8, sc8)
    assert (dh.data_ptr() == dr.data_ptr()) == (p == 0.0)
    for a, b in zip(plain, (dr, dh, dg)):
        assert _same(a, b)
    _same_as_ref(dh, q8, sc8, True)


def test_rmsnorm_wide_module_routes_and_differentiates(gpu, monkeypatch):
    """FusedAddRMSNorm(2048) runs the kernels and agrees with add_rmsnorm_ref in fp32 within 1e-2 of each tensor's
    largest entry (the stack comparison's bound, profiles/llama_block.md); feature rmsnorm_wide off: the composite."""
    from parameter_server_distributed_amd.ops import rmsnorm

    H, g = 2048, _gen(gpu, 2048, 4)
    mod = rmsnorm.FusedAddRMSNorm(H, p=0.0).to(gpu).to(torch.bfloat16)
    with torch.no_grad():
        mod.weight.copy_(torch.rand(H, device=gpu, generator=g) + 0.5)
    r, h, dr, dy = (torch.randn(3, 37, H, device=gpu, generator=g).to(torch.bfloat16) for _ in range(4))
    calls, orig = [], rmsnorm._AddRMSFn.apply
    monkeypatch.setattr(rmsnorm._AddRMSFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])

    def run(fn, r, h, w):
        a, b = (t.detach().clone().requires_grad_(True) for t in (r, h))
        out = fn(a, b)
        grads = torch.autograd.grad(out, (a, b, w), (dr.to(r.dtype), dy.to(r.dtype)))
        return [t.detach() for t in out] + list(grads)

    w32 = mod.weight.detach().float().requires_grad_(True)
    want = run(lambda a, b: rmsnorm.add_rmsnorm_ref(a, b, w32, mod.eps), r.float(), h.float(), w32)
    for feats, n in (("", 1), ("rmsnorm_wide=0", 0)):
        monkeypatch.setenv("PSD_FEATURES", feats)
        del calls[:]
        got = run(mod, r, h, mod.weight)
        assert len(calls) == n, feats
        for name, a, b in zip(("r_new", "y", "dr", "dh", "dweight"), got, want):
            assert a.dtype == torch.bfloat16 and float((a.float() - b).abs().max()) <= 1e-2 * float(b.abs().max()), name


def test_rmsnorm_wide_misuse_raises(gpu, C):
    """An H off the rule, an H past 8192 and an r that is only 8-byte aligned: a RuntimeError naming r before any launch."""
    buf = torch.zeros(5 * 2048 + 4, device=gpu, dtype=torch.bfloat16)
    for r in (buf[:5 * 1280].view(5, 1280), torch.zeros(5, 8704, device=gpu, dtype=torch.bfloat16), buf[4:].view(5, 2048)):
        assert r.is_contiguous() and r.data_ptr() % 8 == 0
        gamma = torch.ones(r.shape[1], device=gpu, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match=r"\br\b"):
            C.rms_fwd(r, None, gamma, EPS, 0.0, SEED, _step(gpu))
