"""The dual MX quantiser (kernels/fp8_t.hip quant_mx_dual_kernel, ``ops.quantize_mx_dual``): one read of
x [R, C] bf16 -> the MX copy of x (blocks of 32 along C) and the MX copy of x^T (blocks of 32 along R),
each in its own fp8 format. Both must be bitwise what the two existing kernels (``quantize_mx``,
``quantize_mx_t``) and the PyTorch reference ``quantize_mx_ref`` give for the same tensor."""
import pytest
import torch

# smallest legal; no multiples of the 128 x 64 tile in either direction (R: 160, C: 96 and 320); BERT-like
SHAPES = [(32, 32), (160, 96), (128, 320), (384, 768)]
FORMATS = [(False, False), (False, True), (True, False), (True, True)]  # (e5m2_row, e5m2_t)


def _input(R: int, C: int, seed: int = 0, e5r: bool = False, e5t: bool = False) -> torch.Tensor:
    """Gaussian bf16 [R, C] with per-column magnitudes 2^-6 .. 2^6 (as tests/test_quant_mx_t.py::_input) and
    the edge blocks planted twice, once in a column block (rows 0-31 of a column: a block of x^T) and once in
    a row block (columns 0-31 of a row: a block of x): all zeros; an amax of exactly 56 = 448 * 2^-3 =
    57344 * 2^-10, the frexp boundary of the reference for e4m3 and e5m2 alike; values around the bf16
    minimum normal 2^-126 (the column block with one zero, where the all-zero row crosses it); an amax of
    448 * 32 with tiny companions. Then an inf element inside ordinary blocks (kernels and reference give
    its blocks the unit scale and saturate their finite elements) and a NaN element. The kernels form a block's maximum with
    fmaxf, which passes over a NaN, where the reference's amax propagates it and falls back to the unit
    scale; the two agree where the block's other elements give the unit scale themselves, so the NaN's
    row block and column block get a maximum of 400 (e4m3: in (224, 448]) or 40,000 (e5m2: in (28,672,
    57,344]) for the format each is quantised to (``e5r`` / ``e5t``). A NaN in ordinary blocks is
    compared between the kernels only (_with_stray_nan)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(R, C, generator=g) * torch.exp2(torch.randint(-6, 7, (1, C), generator=g).float())
    lin = torch.linspace(-40.0, 40.0, 32)
    tiny = 2.0 ** -126 * torch.tensor([1.0, -1.5, 1.25, -1.0] * 8)
    small = 1e-3 * torch.randn(32, generator=g)
    # column blocks (rows 0-31 of columns 0-3)
    x[:32, 0] = 0.0
    x[:32, 1] = lin
    x[5, 1] = -56.0
    x[:32, 2] = tiny
    x[:32, 3] = small
    x[31, 3] = 448.0 * 32
    # row blocks (columns 0-31 of rows 8-11; they cross the planted columns, which keep their amax)
    x[8, :32] = 0.0
    x[9, :32] = lin
    x[9, 7] = -56.0
    x[10, :32] = tiny
    x[11, :32] = small
    x[11, 30] = 448.0 * 32
    # the crossings: column 0 stays all zeros, column 2 tiny (row 8 of it zero); columns 1 and 3 keep their amax
    x[8:12, 0] = 0.0
    x[9, 2] = tiny[9]
    x[11, 2] = tiny[11]
    x[R - 9, C - 2] = float("inf")
    nr, nc = R - 3, C - 5  # the NaN, in row block (nr, nc0 ..) and column block (nr0 .., nc)
    nc0, nr0 = nc // 32 * 32, nr // 32 * 32
    x[nr, nc0:nc0 + 32] = x[nr, nc0:nc0 + 32].clamp(-200.0, 200.0)
    x[nr0:nr0 + 32, nc] = x[nr0:nr0 + 32, nc].clamp(-200.0, 200.0)
    x[nr, nc - 1] = 40000.0 if e5r else 400.0
    x[nr - 1, nc] = 40000.0 if e5t else 400.0
    x[nr, nc] = float("nan")
    return x.to(torch.bfloat16)


def _with_stray_nan(x: torch.Tensor) -> torch.Tensor:
    x = x.clone()
    x[x.shape[0] - 2, x.shape[1] - 9] = float("nan")  # blocks of ordinary magnitude
    return x


def _same(q, s, wq, ws):
    return torch.equal(q.view(torch.uint8).cpu(), wq.view(torch.uint8).cpu()) and torch.equal(s.flatten().cpu(),
                                                                                               ws.flatten().cpu())


def _same_as_ref(x, q, s, wq, ws):
    """Every scale byte, and every payload byte of a finite element of ``x`` (the tensor quantised, laid out
    as ``q``), bitwise the host reference's. The NaN and the inf element themselves are held to the existing
    kernels' bytes only (_same): the kernels' converter turns an inf into the format's NaN / inf byte where the
    reference clamps it to the largest finite value, and the sign of the NaN the host arithmetic produces is
    not the converter's."""
    fin = torch.isfinite(x.float().cpu())
    qb, wb = q.view(torch.uint8).cpu(), wq.view(torch.uint8).cpu()
    bad = ((qb != wb) & fin).nonzero()
    assert bad.numel() == 0, (bad[:8].tolist(), qb[fin & (qb != wb)][:8].tolist(), wb[fin & (qb != wb)][:8].tolist())
    assert int((~fin).sum()) == 2
    return torch.equal(s.flatten().cpu(), ws.flatten().cpu())


def test_quantize_mx_dual_on_the_host_is_the_two_references():
    from parameter_server_distributed_amd.ops import quantize_mx_dual, quantize_mx_ref

    x = _input(160, 96)
    for e5r, e5t in FORMATS:
        qr, sr, qt, st = quantize_mx_dual(x, e5m2_row=e5r, e5m2_t=e5t)
        assert qr.shape == (160, 96) and sr.shape == (160 * 3,) and qt.shape == (96, 160) and st.shape == (96, 5)
        assert qr.dtype == (torch.float8_e5m2 if e5r else torch.float8_e4m3fn)
        assert qt.dtype == (torch.float8_e5m2 if e5t else torch.float8_e4m3fn)
        assert sr.dtype == torch.uint8 and st.dtype == torch.uint8
        assert _same(qr, sr, *quantize_mx_ref(x, e5r))
        assert _same(qt, st, *quantize_mx_ref(x.t().contiguous(), e5t))
        assert int(st[0, 0]) == 127 and int(sr[8 * 3]) == 127  # the all-zero blocks: unit scale
    for bad in (torch.zeros(48, 32), torch.zeros(32, 40), torch.zeros(32)):
        with pytest.raises(ValueError):
            quantize_mx_dual(bad.to(torch.bfloat16))


@pytest.mark.gpu
@pytest.mark.parametrize("fmt", FORMATS, ids=lambda f: ("e5m2" if f[0] else "e4m3") + "_" + ("e5m2" if f[1] else "e4m3"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_quant_mx_dual_is_bitwise_both_existing_quantisers(gpu, shape, fmt):
    from parameter_server_distributed_amd.ops import quantize_mx, quantize_mx_dual, quantize_mx_ref, quantize_mx_t

    R, C = shape
    e5r, e5t = fmt
    xc = _input(R, C, seed=R + C, e5r=e5r, e5t=e5t)
    x = xc.to(gpu)
    qr, sr, qt, st = quantize_mx_dual(x, e5m2_row=e5r, e5m2_t=e5t)
    assert qr.shape == (R, C) and sr.shape == (R * C // 32,) and qt.shape == (C, R) and st.shape == (C, R // 32)
    assert all(t.is_contiguous() for t in (qr, sr, qt, st))
    # the two existing kernels on the same tensor
    assert _same(qr, sr, *quantize_mx(x, e5m2=e5r))
    assert _same(qt, st, *quantize_mx_t(x, e5m2=e5t))
    # the PyTorch reference on the host
    assert _same_as_ref(xc, qr, sr, *quantize_mx_ref(xc, e5r))
    assert _same_as_ref(xc.t(), qt, st, *quantize_mx_ref(xc.t().contiguous(), e5t))
    # the all-zero blocks
    assert int(st[0, 0]) == 127 and not qt[0, :32].view(torch.uint8).any()
    assert int(sr[8 * (C // 32)]) == 127 and not qr[8, :32].view(torch.uint8).any()
    # no atomics, nothing grid-dependent: a second run gives the same bytes
    again = quantize_mx_dual(x, e5m2_row=e5r, e5m2_t=e5t)
    for a, b in zip((qr, sr, qt, st), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    # a NaN among ordinary values: as the two existing kernels treat it
    xn = _with_stray_nan(x)
    qr, sr, qt, st = quantize_mx_dual(xn, e5m2_row=e5r, e5m2_t=e5t)
    assert _same(qr, sr, *quantize_mx(xn, e5m2=e5r))
    assert _same(qt, st, *quantize_mx_t(xn, e5m2=e5t))


@pytest.mark.gpu
def test_quant_mx_dual_rejects_what_the_kernel_cannot_take(gpu, C):
    from parameter_server_distributed_amd.ops import quantize_mx_dual

    def outs(R, Cc):
        return (torch.empty(R, Cc, device=gpu, dtype=torch.float8_e5m2),
                torch.empty(R * Cc // 32, device=gpu, dtype=torch.uint8),
                torch.empty(Cc, R, device=gpu, dtype=torch.float8_e4m3fn),
                torch.empty(Cc, R // 32, device=gpu, dtype=torch.uint8))

    x = torch.zeros(64, 96, device=gpu, dtype=torch.bfloat16)
    qr, sr, qt, st = outs(64, 96)
    C.quant_mx_dual_(x, qr, sr, qt, st)
    with pytest.raises(RuntimeError):
        C.quant_mx_dual_(x[:48], qr[:48], sr[:48 * 3], qt[:, :48].contiguous(), st)  # R % 32
    with pytest.raises(RuntimeError):
        C.quant_mx_dual_(x[:, :40].contiguous(), *outs(64, 40))  # C % 32
    with pytest.raises(RuntimeError):
        C.quant_mx_dual_(x.float(), qr, sr, qt, st)  # bf16 only
    with pytest.raises(RuntimeError):
        C.quant_mx_dual_(x, qt.view(torch.float8_e5m2), sr, qr.view(torch.float8_e4m3fn), st)  # swapped output shapes
    with pytest.raises(ValueError):
        quantize_mx_dual(x.float())
    with pytest.raises(ValueError):
        quantize_mx_dual(x[:48])
