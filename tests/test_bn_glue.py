"""The BatchNorm tensor glue (csrc/bn_ops.cpp, pool_ops.cpp) refuses bad arguments before it launches.

Every entry runs the same checks on the arguments it shares with the others: a host tensor, a
parameter of the wrong dtype, a statistics vector of the wrong length, a strided gradient sink, an
activation of another shape or dtype and a bit-mask of the wrong length all raise ``RuntimeError``
with the entry's prefix. Each bad argument is at least as large as the good one and on the same
device, so a missing check shows as a failed ``pytest.raises``, never as an out-of-range access.
The numerics of these entries are pinned in test_bn.py, test_bnfold.py, test_tail.py and
test_handover.py; the positive cases here only pin the returned counts and shapes.
"""
import copy
from types import SimpleNamespace

import pytest
import torch

BF16, F32, U8 = torch.bfloat16, torch.float32, torch.uint8
SHAPE = (2, 16, 4, 4)  # one-shot elementwise path, 8-channel vectors, a two-row reduce
POOL_SHAPE = (2, 16, 8, 8)  # the pool-fused entries: x before the 3x3/s2 max-pool


def _good(dev, shape=SHAPE):
    """All-good arguments of every entry on ``dev`` (statistics of the identity BN, an all-ones mask)."""
    n, c, h, w = shape
    gen = torch.Generator().manual_seed(0)

    def act(s=shape, dtype=BF16):
        return torch.randn(s, generator=gen).to(dtype).to(dev).contiguous(memory_format=torch.channels_last)

    def vec(k, fill, dtype=F32):
        return torch.full((k,), fill, dtype=dtype, device=dev)

    m = n * h * w
    pooled = (POOL_SHAPE[0], POOL_SHAPE[1], POOL_SHAPE[2] // 2, POOL_SHAPE[3] // 2)
    return SimpleNamespace(
        C=c, M=m, x=act(), dy=act(), dy2=act(), xd=act(), y=act(), act=act, vec=vec,
        gamma=vec(c, 1.0, BF16), beta=vec(c, 0.0, BF16), gamma_d=vec(c, 1.0, BF16),
        mean=vec(c, 0.0), invstd=vec(c, 1.0), mean_d=vec(c, 0.0), invstd_d=vec(c, 1.0),
        rm=vec(c, 0.0), rv=vec(c, 1.0), ss=torch.cat([vec(c, 1.0), vec(c, 0.0)]), coef=vec(3 * c, 0.5),
        mbits=torch.full((m * c // 8,), 255, dtype=U8, device=dev),
        part=torch.zeros(2, 2, c, device=dev), part_d=torch.zeros(2, 2, c, device=dev), rows=2,
        # bn_bwd's mask source (default: x with the forward scale/shift) and sinks
        y_in=None, mbits_in=None, need_dr=False, dgamma_out=None,
        # the pool-fused entries
        xp=act(POOL_SHAPE), gpool=act(pooled), arg=torch.zeros(pooled, dtype=U8, device=dev).contiguous(
            memory_format=torch.channels_last), pool_gamma=vec(POOL_SHAPE[1], 1.0, BF16),
        pool_mean=vec(POOL_SHAPE[1], 0.0),
    )


# entry -> (message prefix, call with the arguments in `a`)
ENTRIES = {
    "bn_bwd": ("psd bn bwd:", lambda C, a: C.bn_bwd(
        a.dy, a.x, a.y_in, a.gamma, a.mean, a.invstd, True, a.need_dr, a.dgamma_out, None, None, a.ss, a.mbits_in)),
    "bn_bwd_reduce_": ("psd bn_bwd_reduce:", lambda C, a: C.bn_bwd_reduce_(a.dy, a.x, a.mean, ss=a.ss)),
    "bn_bwd_pre": ("psd bn_bwd_pre:", lambda C, a: C.bn_bwd_pre(
        a.dy, a.x, a.gamma, a.mean, a.invstd, a.part, a.rows, a.dgamma_out, None)),
    "bn_bwd_dual": ("psd bn bwd_dual:", lambda C, a: C.bn_bwd_dual(
        a.dy, a.x, a.gamma, a.mean, a.invstd, a.mbits, a.dy2, a.xd, a.gamma_d, a.mean_d, a.invstd_d)),
    "bn_bwd_coef": ("psd bn_bwd_coef:", lambda C, a: C.bn_bwd_coef(
        a.dy, a.x, a.gamma, a.mean, a.invstd, mbits=a.mbits, dy2=a.dy2)),
    "bn_pool_bwd": ("psd bn_pool bwd:", lambda C, a: C.bn_pool_bwd(
        a.gpool, None, a.arg, a.xp, a.pool_gamma, a.pool_mean, a.invstd, a.ss)),
    "bn_finalize": ("psd bn_finalize:", lambda C, a: C.bn_finalize(
        a.part, a.rows, a.M, a.gamma, a.beta, a.rm.clone(), a.rv.clone(), 0.1, 1e-5)),
    "bn_elemt_coef": ("psd bn_elemt_coef:", lambda C, a: C.bn_elemt_coef(a.dy, a.x, a.coef)),
    "bn_bwd_dual_pre": ("psd bn_bwd_dual_pre:", lambda C, a: C.bn_bwd_dual_pre(
        a.dy, a.x, a.gamma, a.mean, a.invstd, a.part, a.part_d, a.rows, a.xd, a.gamma_d, a.mean_d, a.invstd_d)),
    "maxpool3s2_bwd": ("psd maxpool bwd:", lambda C, a: C.maxpool3s2_bwd(a.gpool, a.arg, POOL_SHAPE[2], POOL_SHAPE[3])),
}


def _f32(t):
    return t.float()


def _twice(t):
    return torch.cat([t, t])


def _strided(a):
    return torch.zeros(2 * a.C, dtype=BF16, device=a.x.device)[::2]


# (entry, argument, what replaces it): each bad value is at least as large as the good one
BAD = [
    ("bn_bwd", "gamma", lambda a: _f32(a.gamma)),
    ("bn_bwd_pre", "gamma", lambda a: _f32(a.gamma)),
    ("bn_bwd_coef", "gamma", lambda a: _f32(a.gamma)),
    ("bn_bwd_dual", "gamma", lambda a: _f32(a.gamma)),
    ("bn_bwd_dual", "gamma_d", lambda a: _f32(a.gamma_d)),
    ("bn_bwd_dual_pre", "gamma", lambda a: _f32(a.gamma)),
    ("bn_bwd_dual_pre", "gamma_d", lambda a: _f32(a.gamma_d)),
    ("bn_pool_bwd", "pool_gamma", lambda a: _f32(a.pool_gamma)),
    ("bn_bwd", "mean", lambda a: _twice(a.mean)),
    ("bn_bwd_pre", "mean", lambda a: _twice(a.mean)),
    ("bn_pool_bwd", "pool_mean", lambda a: _twice(a.pool_mean)),
    ("bn_bwd_pre", "dgamma_out", _strided),
    ("bn_bwd", "dgamma_out", _strided),  # the control: refused before this refactor too
    ("bn_bwd", "x", lambda a: _f32(a.x)),
    ("bn_bwd", "y_in", lambda a: a.act((2, 16, 4, 8))),
    ("bn_bwd", "mbits_in", lambda a: _twice(a.mbits)),
    ("bn_bwd_dual", "mbits", lambda a: _twice(a.mbits)),
    ("bn_bwd_coef", "mbits", lambda a: _twice(a.mbits)),
]


@pytest.fixture(scope="module")
def good(gpu):
    return _good(gpu)


@pytest.mark.gpu
@pytest.mark.parametrize("entry,field,bad", BAD, ids=[f"{e}-{f}" for e, f, _ in BAD])
def test_bad_argument_is_refused(C, good, entry, field, bad):
    a = copy.copy(good)
    setattr(a, field, bad(good))
    if field == "mbits_in":
        a.need_dr = True  # the bit-mask path is the residual BNs'
    prefix, call = ENTRIES[entry]
    with pytest.raises(RuntimeError, match=prefix):
        call(C, a)


def _shapes(out):
    return [None if t is None else tuple(t.shape) for t in out]


@pytest.mark.gpu
def test_good_arguments_return_the_documented_tensors(C, good):
    a, c = good, good.C
    rows = C.bn_reduce_(a.x, a.rm).shape[0]
    x, v, v2, v3 = SHAPE, (c,), (2 * c,), (3 * c,)
    assert _shapes(C.bn_fwd(a.x, a.gamma, a.beta, a.rm.clone(), a.rv.clone(), a.dy, True, True, 0.1, 1e-5, None, None,
                            mask_out=True)) == [x, v, v, v2, (a.M * c // 8,)]
    assert tuple(C.bn_reduce_(a.x, a.rm).shape) == (rows, 2, c)
    assert _shapes(ENTRIES["bn_finalize"][1](C, a)) == [v, v, v2]
    assert _shapes(ENTRIES["bn_bwd"][1](C, a)) == [x, None, v, v]
    assert tuple(ENTRIES["bn_bwd_reduce_"][1](C, a).shape) == (rows, 2, c)
    assert _shapes(ENTRIES["bn_bwd_pre"][1](C, a)) == [x, v, v]
    assert _shapes(ENTRIES["bn_bwd_dual"][1](C, a)) == [x, x, v, v, v, v]
    assert _shapes(C.bn_bwd_dual(a.dy, a.x, a.gamma, a.mean, a.invstd, a.mbits, a.dy2, a.xd, a.gamma_d, a.mean_d,
                                 a.invstd_d, fold=True)) == [None, x, v, v, v, v, v3, x]
    assert _shapes(ENTRIES["bn_bwd_coef"][1](C, a)) == [x, v3, v, v]
    assert _shapes(C.bn_bwd_coef(a.dy, a.x, a.gamma, a.mean, a.invstd, part=a.part, rows=a.rows)) == [x, v3, v, v]
    assert _shapes(ENTRIES["bn_bwd_dual_pre"][1](C, a)) == [x, x, v, v, v, v, v3, v3]
    assert _shapes(C.bn_bwd_dual_pre(a.dy, a.x, a.gamma, a.mean, a.invstd, a.part, a.part_d[:1], a.rows, a.xd,
                                     a.gamma_d, a.mean_d, a.invstd_d, fold=True, fold_d=True,
                                     derive_d=True)) == [None, None, v, v, v, v, v3, v3]
    assert tuple(ENTRIES["bn_elemt_coef"][1](C, a).shape) == x
    # a 2-D [pixels, C] view of the same activation keeps working
    x2, dy2 = a.x.permute(0, 2, 3, 1).reshape(a.M, c), a.dy.permute(0, 2, 3, 1).reshape(a.M, c)
    assert _shapes(C.bn_bwd_pre(dy2, x2, a.gamma, a.mean, a.invstd, a.part, a.rows)) == [(a.M, c), v, v]
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_good_pool_arguments_return_the_documented_tensors(C, good):
    a, c = good, POOL_SHAPE[1]
    pooled, v = tuple(a.gpool.shape), (c,)
    out = C.bn_pool_fwd(a.xp, a.pool_gamma, a.beta, a.rm.clone(), a.rv.clone(), 0.1, 1e-5)
    assert _shapes(out) == [pooled, pooled, v, v, (2 * c,)] and out[1].dtype == U8
    y, arg, mean, invstd, ss = out
    assert _shapes(C.bn_pool_bwd(a.gpool, None, arg, a.xp, a.pool_gamma, mean, invstd, ss)) == [POOL_SHAPE, v, v]
    _, arg = C.maxpool3s2_fwd(a.xp)
    assert tuple(C.maxpool3s2_bwd(a.gpool, arg, POOL_SHAPE[2], POOL_SHAPE[3]).shape) == POOL_SHAPE
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_good_mx_side_output_is_accepted(C, gpu):
    a = _good(gpu, (2, 32, 4, 4))  # E8M0 scales per 32 channels
    dq = torch.empty_like(a.x, dtype=torch.float8_e5m2)
    dqmx = torch.empty(a.x.numel() // 32, dtype=U8, device=gpu)
    assert _shapes(C.bn_bwd_pre(a.dy, a.x, a.gamma, a.mean, a.invstd, a.part, a.rows, dq=dq, dqmx=dqmx)) == [
        (2, 32, 4, 4), (32,), (32,)]
    assert _shapes(C.bn_bwd(a.dy, a.x, None, a.gamma, a.mean, a.invstd, True, False, None, None, None, a.ss, dq=dq,
                            dqmx=dqmx)) == [(2, 32, 4, 4), None, (32,), (32,)]
    torch.cuda.synchronize()


# Without a device only: where one is present, a regression here would launch a kernel on host
# pointers, and no test may be able to do that.
@pytest.mark.skipif(torch.cuda.is_available(), reason="host tensors must never reach a launch on a GPU machine")
@pytest.mark.parametrize("entry", sorted(ENTRIES))
def test_host_tensors_are_refused(C, entry):
    prefix, call = ENTRIES[entry]
    with pytest.raises(RuntimeError, match=prefix):
        call(C, _good(torch.device("cpu")))
