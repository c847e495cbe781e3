"""The gated SiLU kernels (kernels/swiglu.hip) on the packed gate/up tensor against fp64, element by element.

Rule, per element:  |got - ref64| <= 2^-8 |ref64| + K * 2^-24 * M  with the magnitude M of the terms
    a  = silu(g) u                       M = |silu(g) u|
    dg = da u sig (1 + g (1 - sig))      M = |da u sig| (1 + |g|)
    du = da g sig                        M = |da g sig|
2^-8 |ref| is at least half a bf16 ulp (the one output rounding); K 2^-24 M covers the fp32 evaluation, where
dg's last factor cancels near g = -1.28. K is taken from the yardstick, ``swiglu_ref`` in fp32 on the GPU at
these shapes and scales: its worst |ref32 - ref64| / (2^-24 M) measured 3.19 for a, 4.03 for dg and 3.19 for
du on an MI355X (profiles/llama_block.md), so K = 4 * 4.03 = 16.1 rounded up to a power of two = 32 (4x for
another operation order, as the row-kernel rule; at least rope's 8). Each case prints the yardstick's ratios
again and the kernel's worst error / bound.

Shapes (T, F): (1, 8) one item; (5, 2048); (1057, 2048) several workgroups; (33, 2736) F % 64 != 0, so rows
straddle waves. Each runs with ``blocks`` = 0, 1 and 3 -- the grid-stride loop wraps -- and must give the same
bits."""
import pytest
import torch

from test_row_kernels_fp64 import _gen, _same

pytestmark = pytest.mark.gpu

K = 32.0
U24 = 2.0 ** -24
SHAPES = [(1, 8), (5, 2048), (1057, 2048), (33, 2736)]


def _inputs(T, F, scale, gpu):
    g = _gen(gpu, T, F, int(scale))
    gu = (torch.randn(T, 2 * F, device=gpu, generator=g) * scale).to(torch.bfloat16)
    da = (torch.randn(T, F, device=gpu, generator=g) + 1).to(torch.bfloat16)
    return gu, da


def _ref64(gu, da):
    F = gu.shape[-1] // 2
    g, u, d = gu[:, :F].double(), gu[:, F:].double(), da.double()
    sig = torch.sigmoid(g)
    ref = {"a": g * sig * u, "dg": d * u * sig * (1 + g * (1 - sig)), "du": d * g * sig}
    mag = {"a": (g * sig * u).abs(), "dg": (d * u * sig).abs() * (1 + g.abs()), "du": (d * g * sig).abs()}
    return ref, mag


def _eager32(gu, da):
    """swiglu_ref and its autograd backward in fp32 on the device (no rounding to bf16)."""
    from parameter_server_distributed_amd.ops.swiglu import swiglu_ref

    F = gu.shape[-1] // 2
    x = gu.float().requires_grad_(True)
    a = swiglu_ref(x)
    (dgu,) = torch.autograd.grad(a, x, da.float())
    return {"a": a.detach(), "dg": dgu[:, :F], "du": dgu[:, F:]}


def _ratio(err, mag):
    return float(torch.where(err == 0, torch.zeros_like(err), err / (U24 * mag)).max())


@pytest.mark.parametrize("scale", [1.0, 3.0])
@pytest.mark.parametrize("T,F", SHAPES)
def test_swiglu_matches_fp64(gpu, C, T, F, scale):
    gu, da = _inputs(T, F, scale, gpu)
    ref, mag = _ref64(gu, da)
    e32 = _eager32(gu, da)
    a = C.swiglu_fwd(gu)
    dgu = C.swiglu_bwd(da, gu)
    assert a.shape == (T, F) and a.dtype == torch.bfloat16 and dgu.shape == (T, 2 * F) and dgu.dtype == torch.bfloat16
    got = {"a": a, "dg": dgu[:, :F], "du": dgu[:, F:]}
    cells, bad = [], []
    for k in ("a", "dg", "du"):
        assert bool(torch.isfinite(got[k].float()).all()), k
        yard = _ratio((e32[k].double() - ref[k]).abs(), mag[k])
        err = (got[k].double() - ref[k]).abs()
        bound = ref[k].abs() * 2.0 ** -8 + K * U24 * mag[k]
        q = torch.where(err == 0, torch.zeros_like(err), err / bound).flatten()
        i = int(q.argmax())
        cells.append(f"{k}: err {float(err.flatten()[i]):.3e} bound {float(bound.flatten()[i]):.3e} "
                     f"err/bound {float(q[i]):.3f} eager32/(2^-24 M) {yard:.2f}")
        if float(q[i]) > 1.0:
            bad.append(cells[-1])
    print(f"ROWERR swiglu T={T} F={F} scale={scale} | " + " | ".join(cells))
    assert not bad, "above the bound:\n" + "\n".join(bad)
    # the grid does not change a bit: one and three workgroups walk the items in a wrapping loop
    for blocks in (1, 3):
        assert _same(C.swiglu_fwd(gu, blocks), a), blocks
        assert _same(C.swiglu_bwd(da, gu, blocks), dgu), blocks
    assert _same(C.swiglu_fwd(gu), a) and _same(C.swiglu_bwd(da, gu), dgu)  # two runs are equal


def test_swiglu_leading_dimensions_and_limits(gpu, C):
    """[B, S, 2F] is T = B * S rows; huge gates take the limits (sig = 0 or 1) without a NaN."""
    gu, da = _inputs(6, 16, 1.0, gpu)
    assert _same(C.swiglu_fwd(gu.view(2, 3, 32)).view(6, 16), C.swiglu_fwd(gu))
    assert _same(C.swiglu_bwd(da.view(2, 3, 16), gu.view(2, 3, 32)).view(6, 32), C.swiglu_bwd(da, gu))
    big = torch.tensor([[-1e30, -200.0, -90.0, 90.0, 200.0, 1e30, 0.0, -0.0] + [2.0] * 8], device=gpu).to(torch.bfloat16)
    a = C.swiglu_fwd(big).float()
    want = torch.tensor([[0.0, 0.0, 0.0, 180.0, 400.0, 2e30, 0.0, 0.0]], device=gpu).to(torch.bfloat16).float()
    torch.testing.assert_close(a, want, rtol=2.0 ** -8, atol=1e-30)
    assert bool(torch.isfinite(C.swiglu_bwd(torch.ones(1, 8, device=gpu, dtype=torch.bfloat16), big).float()).all())


def test_swiglu_module_autograd_and_feature_switch(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops import swiglu as sw

    gu, da = _inputs(33, 64, 1.0, gpu)
    calls = []
    orig = sw._SwigluFn.apply
    monkeypatch.setattr(sw._SwigluFn, "apply", lambda *a: (calls.append(1), orig(*a))[1])
    x = gu.clone().requires_grad_(True)
    y = sw.SwiGLU()(x)
    y.backward(da)
    assert calls == [1]
    monkeypatch.setenv("PSD_FEATURES", "swiglu=0")
    x2 = gu.clone().requires_grad_(True)
    y2 = sw.SwiGLU()(x2)
    y2.backward(da)
    monkeypatch.setenv("PSD_FEATURES", "")
    assert calls == [1]  # the composite
    torch.testing.assert_close(y.float(), y2.float(), rtol=2.0 ** -7, atol=1e-6)  # one bf16 ulp
    torch.testing.assert_close(x.grad.float(), x2.grad.float(), rtol=2.0 ** -7, atol=2.0 ** -7)
    # an fp32 or odd-width tensor takes the composite, not an error
    assert sw.swiglu(torch.randn(4, 24, device=gpu)).shape == (4, 12)
    assert calls == [1]


def test_swiglu_misuse_raises(gpu, C):
    gu, da = _inputs(5, 16, 1.0, gpu)
    wide = torch.zeros(5, 64, device=gpu, dtype=torch.bfloat16)
    cases = [
        ("gu", lambda: C.swiglu_fwd(wide[:, :32])),  # non-contiguous
        ("gu", lambda: C.swiglu_fwd(torch.zeros(5, 24, device=gpu, dtype=torch.bfloat16))),  # F = 12: F % 8 != 0
        ("gu", lambda: C.swiglu_fwd(gu.float())),  # wrong dtype
        ("gu", lambda: C.swiglu_fwd(gu.cpu())),  # wrong device
        ("blocks", lambda: C.swiglu_fwd(gu, -1)),
        ("gu", lambda: C.swiglu_bwd(da, wide[:, :32])),
        ("da", lambda: C.swiglu_bwd(da.float(), gu)),
        ("da", lambda: C.swiglu_bwd(da[:3].contiguous(), gu)),  # shape mismatch
        ("da", lambda: C.swiglu_bwd(wide[:, :16], gu)),
    ]
    for name, call in cases:
        with pytest.raises(RuntimeError, match=rf"\b{name}\b"):
            call()
