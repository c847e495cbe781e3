"""Fused LM head + cross-entropy (csrc/kernels/lmhead_xent.hip, ops/loss.linear_cross_entropy) against an
fp64 reference on the same bf16 inputs. Every element must pass; the tolerances are derived, not tuned:

  bound = K * 2^-23 * max(|X| |W|^T + |b|)     worst-case fp32 accumulation error of one logit
  |lse - ref|      <= bound + 2^-22 (1 + |ref|)
  |loss_row - ref| <= 2 bound + 2^-22 (1 + |lse_ref|)
  |g - g_ref|      <= 2^-8 |g_ref| + 2^-8 A      the output's own bf16 rounding, and the bf16 rounding of dZ
                                                 (with the exp / accumulation error) propagated in worst case:
                                                 A = |dZ_ref| |W| (dX), |dZ_ref|^T |X| (dW), sum |dZ_ref| (db)
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

# (M, K, V, bias, chunk_rows, slices, big): K 64 one K-tile / 192 the ring wraps across tiles / 768 the model's;
# V 128 one tile / 136 an 8-column ragged tail / 1352 ten full tiles and a ragged one; M 1 (its only row
# ignored), 130 (two row blocks), 300 with 128-row chunks (three, the last ragged); slices 0 = the launcher's
# choice. big: |logits| up to 60 with every row's maximum in another tile and slice (online rescale, combine).
CASES = [
    (1, 64, 128, True, None, 0, False),
    (130, 192, 136, False, None, 0, False),
    (300, 768, 1352, True, 128, 3, False),
    (130, 64, 1352, True, None, 4, True),
    (130, 192, 128, True, 64, 1, False),
]


@functools.lru_cache(maxsize=None)
def _case(M, K, V, bias, big):
    g = torch.Generator().manual_seed(M * 7 + K + V)
    w = (torch.randn(V, K, generator=g) * 0.5).bfloat16()
    x = torch.randn(M, K, generator=g).bfloat16()
    if big:  # row i points at column c_i: z[i, c_i] = 60, the rest 60 cos(w_j, w_ci) |w_j| / |w_ci|
        c = (torch.arange(M) * 131) % V
        wc = w.float()[c]
        x = (60.0 * wc / (wc * wc).sum(1, keepdim=True)).bfloat16()
    b = (torch.randn(V, generator=g) * 0.5).bfloat16() if bias else None
    y = torch.randint(0, V, (M,), generator=g)
    y[::7] = -100
    if M > 4:
        y[1], y[2], y[3] = 0, V - 1, V - 3  # the first column, the last, and one inside a ragged tail
    else:
        y[:] = -100
    xd, wd = x.double(), w.double()
    z = xd @ wd.T + (b.double() if bias else 0)
    lse = torch.logsumexp(z, 1)
    ok = y >= 0
    onehot = torch.zeros_like(z)
    onehot[ok, y[ok]] = 1
    loss_row = torch.where(ok, lse - (z * onehot).sum(1), torch.zeros_like(lse))
    count = max(int(ok.sum()), 1)
    dz = (torch.softmax(z, 1) - onehot) * ok[:, None] / count
    absz = xd.abs() @ wd.abs().T + (b.double().abs() if bias else 0)
    ref = dict(lse=lse, loss_row=loss_row, loss=loss_row.sum() / count, bound=K * 2.0 ** -23 * absz.max().item(),
               dx=dz @ wd, dw=dz.T @ xd, db=dz.sum(0), Ax=dz.abs() @ wd.abs(), Aw=dz.abs().T @ xd.abs(),
               Ab=dz.abs().sum(0), zmax=z.abs().max().item())
    return x, w, b, y, ref


def _run(gpu, M, K, V, bias, chunk_rows, slices, big):
    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.loss import linear_cross_entropy

    x, w, b, y, ref = _case(M, K, V, bias, big)
    xg, wg = x.to(gpu).requires_grad_(True), w.to(gpu).requires_grad_(True)
    bg = b.to(gpu).requires_grad_(True) if bias else None
    yg = y.to(gpu)
    loss_row, lse = native().lmhead_xent_fwd(xg.detach(), wg.detach(), None if bg is None else bg.detach(), yg, slices)
    loss = linear_cross_entropy(xg, wg, bg, yg, chunk_rows=chunk_rows, slices=slices)
    assert loss.grad_fn is not None and "LinearXent" in type(loss.grad_fn).__name__  # the kernels, not the composite
    loss.backward()
    out = dict(lse=lse, loss_row=loss_row, loss=loss.detach(), dx=xg.grad, dw=wg.grad)
    if bias:
        out["db"] = bg.grad
    return {k: v.cpu() for k, v in out.items()}, ref


@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_forward_backward_match_fp64(gpu, case):
    out, ref = _run(gpu, *case)
    bound = ref["bound"]
    if case[-1]:
        assert ref["zmax"] > 55
    err = (out["lse"].double() - ref["lse"]).abs()
    assert (err <= bound + 2.0 ** -22 * (1 + ref["lse"].abs())).all(), err.max()
    err = (out["loss_row"].double() - ref["loss_row"]).abs()
    assert (err <= 2 * bound + 2.0 ** -22 * (1 + ref["lse"].abs())).all(), err.max()
    assert (out["loss_row"][_case(*case[:4], case[-1])[3] < 0] == 0).all()
    lim = 2 * bound + 2.0 ** -22 * (1 + ref["lse"].abs().max())
    assert abs(out["loss"].double() - ref["loss"]) <= lim + 2.0 ** -22 * abs(ref["loss"])
    for g, A in (("dx", "Ax"), ("dw", "Aw"), ("db", "Ab")):
        if g in out:
            assert out[g].dtype == torch.bfloat16
            err = (out[g].double() - ref[g]).abs()
            tol = 2.0 ** -8 * ref[g].abs() + 2.0 ** -8 * ref[A]
            assert (err <= tol).all(), (g, (err - tol).max())


def test_two_runs_are_bitwise_equal(gpu):
    a, _ = _run(gpu, *CASES[2])
    b, _ = _run(gpu, *CASES[2])
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)


def test_slice_count_only_reassociates(gpu):
    from parameter_server_distributed_amd import native

    x, w, b, y, ref = _case(300, 768, 1352, True, False)
    args = (x.to(gpu), w.to(gpu), b.to(gpu), y.to(gpu))
    (r1, l1), (r3, l3) = native().lmhead_xent_fwd(*args, 1), native().lmhead_xent_fwd(*args, 3)
    lim = (ref["bound"] + 2.0 ** -22 * (1 + ref["lse"].abs())).to(gpu)
    assert ((l1.double() - l3.double()).abs() <= lim).all() and ((r1.double() - r3.double()).abs() <= 2 * lim).all()
    assert native().lmhead_xent_slices(4096, 40512) >= 2


def test_peak_memory_below_one_logits_tensor(gpu, monkeypatch):
    """Forward + backward at M = 1024, K = 256, V = 4096 in 256-row chunks stay below M * V * 2 bytes, one
    logits tensor (the composite holds two): 2 MB of logit gradient, 4 MB of fp32 weight-gradient scratch,
    1 MB of split-K slab, 0.5 MB of dX. A bias-free head (the Llama one): the column-sum kernel of the bias
    gradient takes a 2048 x V fp32 workspace whatever the chunk, more than the logits at this toy V. The
    bwd-data GEMM is pinned to the MFMA route, whose candidates allocate nothing."""
    from parameter_server_distributed_amd.ops.loss import linear_cross_entropy

    monkeypatch.setenv("PSD_FEATURES", "linear_tune=0")
    M, K, V = 1024, 256, 4096
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).bfloat16().to(gpu).requires_grad_(True)
    w = (torch.randn(V, K, generator=g) * 0.1).bfloat16().to(gpu).requires_grad_(True)
    y = torch.randint(0, V, (M,), generator=g).to(gpu)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(gpu)
    base = torch.cuda.memory_allocated(gpu)
    linear_cross_entropy(x, w, None, y, chunk_rows=256).backward()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(gpu) - base
    print(f"peak {peak} bytes against {M * V * 2}")
    assert peak < M * V * 2
    assert x.grad is not None and w.grad is not None and torch.isfinite(w.grad.float()).all()
