"""The wide fused add + LayerNorm kernels (kernels/layernorm_wide.hip, H = 256 n from 1280 to 8192) with the checks,
references and accuracy rule of tests/test_row_kernels_fp64.py, unchanged. Each rows case prints its ROWERR line
(recorded in profiles/layernorm_wide.md)."""
import pytest
import torch
import torch.nn.functional as F

from test_row_kernels_fp64 import (EPS, SEED, _affine, _count_dy, _Err, _gen, _keep_mask, _ln_backward, _ln_forward,
                                   _ln_inputs, _same)

pytestmark = pytest.mark.gpu

# Row counts, from the launchers' constants (launchers_ln.h): one 256-lane workgroup per row per round.
# Forward min(rows, LN_WIDE_FWD_CAP = 2048) workgroups; backward min(ceil(rows / LN_WIDE_BWD_ROWS = 16), cap), cap =
# LN_WIDE_BWD_CAP = 1024 up to H = 4096 and 512 above, one set of partial rows each.
#   2049          one past the forward's cap: workgroup 0 takes a second row
#   16 cap + 1    the backward sits at its cap (cap + 1 wanted): workgroups visit 16 or 17 rows
FWD_WRAP_ROWS, BWD_CAP_ROWS = 2049, {1280: 16 * 1024 + 1, 8192: 16 * 512 + 1}
# H: 1280 a partly filled slab (idle half-waves), 2048 exactly one slab, 2304 a slab and an eighth, 8192 four slabs
ROW_CASES = ([(H, rows) for H in (1280, 2048, 2304, 8192) for rows in (1, 3)]
             + [(1280, FWD_WRAP_ROWS), (1280, BWD_CAP_ROWS[1280])])


@pytest.mark.parametrize("kind", ["randn", "offset"])
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H,rows", ROW_CASES)
def test_layernorm_wide_rows_match_fp64(gpu, C, H, rows, p, kind):
    x, h, gamma, beta, dy = _ln_inputs(kind, rows, H, gpu)
    rep = _Err(f"lnw H={H} rows={rows} p={p} {kind}")
    (y, s, mean, rstd), mask, step = _ln_forward(C, gpu, rep, x, h, gamma, beta, p)
    if p:  # the narrow kernel's mask of the same flat elements (as rows of 1024), bit for bit
        n = rows * H
        assert torch.equal(mask.flatten(), _keep_mask(C, -(-n // 1024), 1024, p, step, gpu).flatten()[:n])
    _ln_backward(C, rep, dy, s, mean, rstd, gamma, mask, p, step, dhsum=True)
    rep.finish()


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [1280, 8192])
def test_layernorm_wide_counts_every_row_once(gpu, C, H, p):
    """As test_layernorm_counts_every_row_once, at the block cap: dbeta of a 0 / 1 dy is the integer count bit for bit,
    with and without the dhsum partial row, and dhsum leaves the other outputs' bits alone."""
    rows = BWD_CAP_ROWS[H]
    s = torch.ones(rows, H, device=gpu, dtype=torch.bfloat16)
    mean = torch.zeros(rows, device=gpu, dtype=torch.float32)
    rstd, gamma = torch.ones_like(mean), torch.ones(H, device=gpu, dtype=torch.bfloat16)
    dy, count = _count_dy(rows, H, gpu)
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    plain = C.ln_bwd(dy, s, mean, rstd, gamma, p, SEED, step)
    both = C.ln_bwd(dy, s, mean, rstd, gamma, p, SEED, step, None, None, torch.empty_like(gamma))
    assert _same(plain[3], count.to(torch.bfloat16))
    for a, b in zip(plain, both):
        assert _same(a, b)


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("H", [1280, 8192])
def test_layernorm_wide_mx_operand_is_quant_mx_of_y(gpu, C, H, p):
    """As test_layernorm_mx_operand_is_quant_mx_of_y: q8_out / sc8_out are bitwise quant_mx_ of the returned y, and
    y, s, mean, rstd keep the bits of the call without them."""
    rows, g = 3, _gen(gpu, H, 99)
    spread = torch.exp2(torch.randint(-4, 5, (1, H), device=gpu, generator=g).float())  # block scales differ
    x = (torch.randn(rows, H, device=gpu, generator=g) * spread).to(torch.bfloat16)
    h = torch.randn(rows, H, device=gpu, generator=g).to(torch.bfloat16)
    gamma, beta = _affine(g, H, gpu)
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    plain = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)
    q8, q = (torch.empty(rows, H, device=gpu, dtype=torch.float8_e4m3fn) for _ in range(2))
    sc8, sc = (torch.empty(rows * H // 32, device=gpu, dtype=torch.uint8) for _ in range(2))
    both = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step, q8, sc8)
    for name, a, b in zip(("y", "s", "mean", "rstd"), plain, both):
        assert _same(a, b), name
    C.quant_mx_(both[0], q, sc)
    assert _same(sc8, sc) and _same(q8, q) and len(torch.unique(sc)) > 1


def test_layernorm_wide_module_routes_differentiates_and_hands_over(gpu):
    """FusedAddLayerNorm(1280) against the fp32 composite within test_fused_add_layernorm_matches_fp32's bound, and
    its MX copy of y taken by the fp8 Linear wired with psd_mx_output_to."""
    from parameter_server_distributed_amd.ops.layernorm import FusedAddLayerNorm
    from parameter_server_distributed_amd.ops.linear import MfmaLinear

    H, g = 1280, _gen(gpu, 1280, 4)
    ln = FusedAddLayerNorm(H, p=0.0).to(gpu).to(torch.bfloat16)
    with torch.no_grad():
        ln.weight.copy_(torch.rand(H, device=gpu, generator=g) + 0.5)
        ln.bias.copy_(torch.rand(H, device=gpu, generator=g) - 0.5)
    lin = MfmaLinear(H, H, fp8="mx").to(gpu).to(torch.bfloat16)
    ln.psd_mx_output_to(lin)
    x, h, dy = (torch.randn(4, 37, H, device=gpu, generator=g).to(torch.bfloat16) for _ in range(3))

    def run(fn, dt, params=None):
        ins = [t.detach().to(dt).requires_grad_(True) for t in (x, h)]
        ins += params or [t.detach().to(dt).requires_grad_(True) for t in (ln.weight, ln.bias)]
        y = fn(*ins)
        return [y.detach()] + list(torch.autograd.grad(y, ins, dy.to(dt))), y

    got, y = run(lambda a, b, w, c: ln(a, b), torch.bfloat16, [ln.weight, ln.bias])
    want, _ = run(lambda a, b, w, c: F.layer_norm(a + b, (H,), w, c, ln.eps), torch.float32)
    for name, a, b in zip(("y", "dx", "dh", "dweight", "dbias"), got, want):
        assert a.dtype == torch.bfloat16 and float((a.float() - b).norm() / b.norm()) < 2e-2, name
    before = lin.psd_mx_handovers
    lin(y)
    assert lin.psd_mx_handovers == before + 1


def test_layernorm_wide_misuse_raises(gpu, C):
    """A hidden size off the rule names H, an x that is only 8-byte aligned names x: RuntimeErrors before any launch."""
    step = torch.tensor([3], device=gpu, dtype=torch.int64)
    for H in (512, 1152, 1600, 8448):
        x = torch.zeros(3, H, device=gpu, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match=r"\bH\b"):
            C.ln_fwd(x, x, x[0], x[0], EPS, 0.0, SEED, step)
    x = torch.zeros(3 * 2048 + 4, device=gpu, dtype=torch.bfloat16)[4:].view(3, 2048)
    ok = torch.zeros(3, 2048, device=gpu, dtype=torch.bfloat16)
    assert x.is_contiguous() and x.data_ptr() % 16 == 8
    with pytest.raises(RuntimeError, match=r"\bx\b"):
        C.ln_fwd(x, ok, ok[0], ok[0], EPS, 0.0, SEED, step)
