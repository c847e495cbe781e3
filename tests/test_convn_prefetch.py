"""One-tile-ahead epilogue operand prefetch of the persistent 1x1 kernels (feature
``convp_epi_prefetch``; kernels/convn.hip convp_kernel / convpr_kernel with PF).

The arithmetic does not change, so every case runs the same launch with ``epi_prefetch`` off and on
and compares output, mask bytes, ``part`` and ``part_d`` BITWISE, and checks the plain (off) launch
against an fp32 torch composite at the tolerance ``tests/test_convn.py`` / ``tests/test_tail.py`` use
for the same mode (operands are small integers: outputs exact, partial sums to 1e-6).

Shapes: M = 2 * CUs * 128 + 72 rows (every workgroup runs at least two tiles, so the hand-over of
the operand registers between tiles runs; the last tile is ragged) and one M below CUs * 128 (one
tile per workgroup: only the first-tile prologue); K = 64 / 128 (resident weights, one and two
K-tiles), K = 256 (streamed ring, four K-tiles) and K = 256 + 64 through the K-concatenated second
operand; N = 256 / 512 (one and two column tiles); modes 2 (with and without the BN input), 3, 5
and 8; both persistent variants (one and two workgroups per CU: ring depths 1 .. 5 ahead); the
gathered variant, which ignores the flag; and an output that aliases ``dr``.

Mode 3 and the gathered kernel run the plain epilogue whatever the flag says (mode 3's operand set
does not fit the registers, profiles/convp_epi_prefetch.md): their cases pin that the flag is inert."""
import functools

import pytest
import torch

from parameter_server_distributed_amd import native

pytestmark = pytest.mark.gpu

H, W = 2, 4  # image (even: mode 5's quarter grid is 1 x 2); M = Nb * 8


def _cus(gpu):
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def _rows(gpu, size):
    cus = _cus(gpu)
    m = 2 * cus * 128 + 72 if size == "big" else (cus * 128) // 2 + 72
    assert m % (H * W) == 0
    return m


def _variant(N, kind):
    C = native()
    vs = [v for v in range(C.convn_variants(N)) if C.convn_variant_kind(N, v) == kind]
    assert vs and C.convn_variant_ok(N, vs[0], 1, 1, 1, 0, W, False)
    return vs[0]


def _ints(shape, lo, hi, g, gpu):
    return torch.randint(lo, hi + 1, shape, generator=g, device=gpu).float()


def _nhwc(t2d, Nb):  # [M, C] rows -> channels_last [Nb, C, H, W] bf16 (the same memory)
    return t2d.to(torch.bfloat16).view(Nb, H, W, -1).permute(0, 3, 1, 2)


def _pack(bits):
    w = (1 << torch.arange(8, device=bits.device, dtype=torch.int32))
    return (bits.view(-1, 8).to(torch.int32) * w).sum(1).to(torch.uint8)


@functools.lru_cache(maxsize=None)
def _operands(M, K, K2, N, dev_index):
    """Shared per shape, never modified: A = [dy | x2] rows, W, and the fp32 product."""
    gpu = torch.device("cuda", dev_index)
    g = torch.Generator(device=gpu).manual_seed(1000 * K + N + K2)
    a = _ints((M, K), -1, 1, g, gpu)
    a2 = _ints((M, K2), -1, 1, g, gpu) if K2 else None
    w = _ints((N, K + K2), -1, 1, g, gpu)
    acat = a if a2 is None else torch.cat([a, a2], 1)
    y = acat @ w.t()  # fp32, exact: |y| <= K + K2 < 2^24
    return a, a2, w, y


def _gen(gpu, seed):
    return torch.Generator(device=gpu).manual_seed(seed)


BWD_CASES = [  # mode, K, K2, N, has_bx, size, kind, bias
    (2, 64, 0, 256, True, "big", 3, False),
    (2, 64, 0, 256, False, "big", 3, False),
    (2, 128, 0, 512, False, "big", 3, False),
    (2, 256, 0, 256, True, "big", 3, False),
    (2, 256, 64, 256, True, "big", 3, True),    # the BN-backward fold's operands: [g | x] and a bias
    (2, 64, 0, 256, True, "small", 3, False),
    (2, 256, 0, 512, False, "small", 3, False),
    (2, 64, 0, 256, True, "big", 4, False),     # two workgroups per CU: a two-slot ring (one K-tile ahead)
    (2, 128, 0, 256, False, "big", 4, False),   # ... the same grid on the five-slot ring
    (2, 256, 0, 256, False, "big", 4, False),   # ... and on the streamed ring
    (5, 128, 0, 256, True, "big", 3, False),
    (5, 64, 0, 512, False, "big", 3, False),
    (5, 256, 0, 512, False, "big", 3, False),
    (5, 256, 0, 256, True, "small", 3, False),
    (3, 64, 0, 256, True, "big", 3, False),     # plain path either way
    (3, 256, 0, 512, True, "big", 3, False),
    (2, 128, 0, 256, True, "big", 0, False),    # gathered kernel: the flag is inert
]


def _id(c):
    return "-".join(str(x) for x in c)


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_bwd_prefetch_bitwise_and_reference(gpu, case):
    mode, K, K2, N, has_bx, size, kind, with_bias = case
    C = native()
    M = _rows(gpu, size)
    Nb = M // (H * W)
    v = _variant(N, kind)
    a, a2, w, y = _operands(M, K, K2, N, gpu.index or 0)
    g = _gen(gpu, 17 * mode + K + N)
    bias = _ints((N,), -2, 2, g, gpu) if with_bias else None
    yb = y + bias if with_bias else y
    bx = _ints((M, N), -3, 3, g, gpu)
    mean = _ints((N,), -2, 2, g, gpu)
    bits = torch.randint(0, 2, (M, N), generator=g, device=gpu).bool()
    if mode == 5:
        dr4 = _ints((Nb, H // 2, W // 2, N), -2, 2, g, gpu)
        full = torch.zeros(Nb, H, W, N, device=gpu)
        full[:, ::2, ::2] = dr4
        add = full.view(M, N)
        bdr = dr4.to(torch.bfloat16).permute(0, 3, 1, 2)  # channels_last [Nb, N, H/2, W/2]
    else:
        add = _ints((M, N), -2, 2, g, gpu)
        bdr = add.to(torch.bfloat16)
    args = dict(bdr=bdr, bmbits=_pack(bits))
    if K2:
        args["x2"] = _nhwc(a2, Nb)
    if with_bias:
        args["bias"] = bias
    xd = mean_d = None
    if mode == 3:
        xd = _ints((M, N), -3, 3, g, gpu)
        mean_d = _ints((N,), -2, 2, g, gpu)
        args.update(bxd=xd.to(torch.bfloat16), bmean_d=mean_d)
    dyd = _nhwc(a, Nb)
    wd = w.to(torch.bfloat16)
    bxd16 = bx.to(torch.bfloat16) if has_bx else None
    rows_alloc = max(C.convn_stats_rows(M), C.convn_part_rows(M, N, v, H, W, 1))
    res = {}
    for pf in (False, True):
        out = torch.full((M, N), 7.0, device=gpu, dtype=torch.bfloat16)
        part = torch.full((rows_alloc, 2, N), float("nan"), device=gpu)
        part_d = torch.full((rows_alloc, 2, N), float("nan"), device=gpu) if mode == 3 else None
        if part_d is not None:
            args["part_d"] = part_d
        rows = C.convn_bwd_(dyd, wd, out, 1, 1, 1, 0, part, v, mode, bxd16, mean, epi_prefetch=pf, **args)
        assert rows == C.convn_part_rows(M, N, v, H, W, 1) > 0
        res[pf] = (out, part[:rows], None if part_d is None else part_d[:rows])
    for off, on, what in zip(res[False], res[True], ("out", "part", "part_d")):
        if off is not None:
            assert torch.equal(off.view(torch.int16 if off.dtype == torch.bfloat16 else torch.int32),
                               on.view(torch.int16 if on.dtype == torch.bfloat16 else torch.int32)), what
    # the plain launch against the fp32 composite
    gref = torch.where(bits, yb + add, torch.zeros_like(yb))
    out, part, part_d = res[False]
    torch.testing.assert_close(out.float(), gref, rtol=0, atol=0)
    xm = (bx if has_bx else torch.zeros_like(bx)).double() - mean.double()
    got = part.double().sum(0)
    torch.testing.assert_close(got[0], gref.double().sum(0), rtol=0, atol=1e-6)
    torch.testing.assert_close(got[1], (gref.double() * xm).sum(0), rtol=0, atol=1e-6)
    if mode == 3:
        gd = part_d.double().sum(0)
        torch.testing.assert_close(gd[0], gref.double().sum(0), rtol=0, atol=1e-6)
        torch.testing.assert_close(gd[1], (gref.double() * (xd.double() - mean_d.double())).sum(0), rtol=0, atol=1e-6)


def test_bwd_prefetch_output_aliasing_dr(gpu):
    """``out`` and ``dr`` the same tensor (each tile's dr rows are read before those rows are stored; the
    prefetched rows belong to the next tile): the result of the separate-tensor launch, flag off and on."""
    C = native()
    K, N = 64, 256
    M = _rows(gpu, "big")
    Nb = M // (H * W)
    v = _variant(N, 3)
    a, _, w, y = _operands(M, K, 0, N, gpu.index or 0)
    g = _gen(gpu, 5)
    mean = _ints((N,), -2, 2, g, gpu)
    bits = torch.randint(0, 2, (M, N), generator=g, device=gpu).bool()
    dr = _ints((M, N), -2, 2, g, gpu)
    gref = torch.where(bits, y + dr, torch.zeros_like(y))
    rows_alloc = max(C.convn_stats_rows(M), C.convn_part_rows(M, N, v, H, W, 1))
    for pf in (False, True):
        buf = dr.to(torch.bfloat16)
        part = torch.full((rows_alloc, 2, N), float("nan"), device=gpu)
        rows = C.convn_bwd_(_nhwc(a, Nb), w.to(torch.bfloat16), buf, 1, 1, 1, 0, part, v, 2, None, mean, bdr=buf,
                            bmbits=_pack(bits), epi_prefetch=pf)
        assert rows > 0
        torch.testing.assert_close(buf.float(), gref, rtol=0, atol=0)
        torch.testing.assert_close(part[:rows].double().sum(0)[0], gref.double().sum(0), rtol=0, atol=1e-6)


APPLY_CASES = [  # K, K2, N, residual, size, kind
    (64, 0, 256, True, "big", 3),
    (128, 0, 512, True, "big", 3),
    (256, 0, 256, True, "big", 3),
    (256, 64, 256, False, "big", 3),   # the dual tail: K-concatenated second operand, no residual
    (64, 0, 512, True, "small", 3),
    (256, 0, 256, True, "small", 3),
    (64, 0, 256, True, "big", 4),
    (256, 0, 512, True, "big", 4),
    (128, 0, 256, True, "big", 0),     # gathered kernel: the flag is inert
]


@pytest.mark.parametrize("case", APPLY_CASES, ids=_id)
def test_apply_prefetch_bitwise_and_reference(gpu, case):
    """Mode 8: y = relu(bf16(conv * scale + shift) + residual) and its ReLU bit-mask."""
    K, K2, N, with_res, size, kind = case
    C = native()
    M = _rows(gpu, size)
    Nb = M // (H * W)
    v = _variant(N, kind)
    a, a2, w, y = _operands(M, K, K2, N, gpu.index or 0)
    g = _gen(gpu, 8 + K + N)
    sc = _ints((N,), 1, 1 if K + K2 > 128 else 2, g, gpu)  # keeps |y * sc + sh| < 128: exact in bf16
    sh = _ints((N,), -3, 3, g, gpu) + 0.5  # never exactly zero
    res = _ints((M, N), -4, 4, g, gpu) if with_res else None
    pre = (y * sc + sh).bfloat16().float()
    assert torch.equal(pre, y * sc + sh)
    o = torch.relu(pre + (res if with_res else 0.0))
    want_bits = _pack(o > 0)
    kw = dict(apply_ss=torch.cat([sc, sh]))
    if with_res:
        kw["apply_res"] = res.to(torch.bfloat16)
    if K2:
        kw["x2"] = _nhwc(a2, Nb)
    got = {}
    for pf in (False, True):
        out = torch.full((M, N), 7.0, device=gpu, dtype=torch.bfloat16)
        mb = torch.full((M * N // 8,), 0xA5, device=gpu, dtype=torch.uint8)
        assert C.convn_(_nhwc(a, Nb), w.to(torch.bfloat16), out, 1, 1, 1, 0, variant=v, apply_mask=mb, epi_prefetch=pf,
                        **kw) == 1
        got[pf] = (out, mb)
    assert torch.equal(got[False][0].view(torch.int16), got[True][0].view(torch.int16))
    assert torch.equal(got[False][1], got[True][1])
    torch.testing.assert_close(got[False][0].float(), o.bfloat16().float(), rtol=0, atol=0)
    assert torch.equal(got[False][1], want_bits)
