"""Identity-bottleneck tail ``relu(bn3(conv3(a2)) + x)`` without storing the BN input.

The unfused tail writes y3 = conv3(a2) (the 4x-wide activation), reads it back for the BN statistics'
consumer pass (bn_apply: read y3 and the residual, write the output and its ReLU bit-mask), and
keeps y3 alive until backward, whose BN reduction reads it once more. Per identity block at ResNet-50
b1024 layer1 that is ~5 activation passes of 1.6 GB over a tensor that is a cheap 1x1 GEMM of a
4x-narrower input (K = 64..512).

Here y3 is recomputed instead of stored (kernels/convn.hip):
  forward   1. conv3 statistics pass: the narrow GEMM with the BN statistics epilogue and no store
            2. BN finalize from those partials (mean, invstd, scale/shift, running statistics)
            3. conv3 apply pass: the same GEMM whose epilogue writes relu(bf16(y3) * scale + shift + x)
               and the ReLU bit-mask (bwd mode 8) -- y3 never reaches HBM
  backward  the consumer convolution's bwd-data epilogue (the next block's conv1, modes 2 / 5) reduces
            g = mask (dX + dr) with the BN input taken as 0: sum g and -mean sum g. The missing
            sum g y3 is sum_i W[c][i] (g^T a2)[c][i] -- the fold wgrad's g^T a2, which conv3's
            BN-backward fold computes anyway (kernels/bnfold.hip rowdot) -- so the finalize runs
            after that wgrad, then the folded dgrad / wgrad combination (ops/conv.py _fold_backward).
  Without that fused consumer (e.g. the network's last block, whose output feeds the pooling), the
  backward recomputes y3 once and runs the ordinary BN backward + fold.

Numerics: the statistics (Gram moments or the statistics-only pass) and the apply pass all use the
fp32 product y3 -- the apply normalises it before its one rounding to bf16 -- so the moments are
exactly those of the normalised tensor (within 1e-5 of fp64 per layer,
tests/test_tail.py::test_tail_statistics_match_fp64). The unfused tail normalises the bf16-rounded
stored y3 instead: a rounding-level difference (normalising bf16(y3) with the Gram moments of the
fp32 y3 moved the b8 ResNet-50 test loss by 0.55 %, tools/probes/tail_stats_probe.py). The
backward's sum g y3 also uses the fp32 product.

Reference: the reference's worker has no model at all (its "gradient" is a constant,
/root/reference/src/worker.cpp:316-329); this is the MI355X data-movement design of the
bottleneck tail ResNet-50 training needs.
"""
from __future__ import annotations

import types

import torch

from ..utils.config import feature as _feat
from . import autotune as _at
from .conv import (Conv1x1, ConvNHWC, _fold_backward, _fold_v, _from_2d, _fwd_records, _native, _part_rows, _sink_view,
                   _write_dw, fold_ok)
from .bn import FusedBatchNorm2d
from .handover import (BnFwd, FoldPending, StridedDr, bn_momentum, dual_from_fold, pop_dr, route_res_grad, sinks,
                       take)

__all__ = ["tail_ok", "conv_bn_tail", "dual_tail_ok", "conv_bn_dual_tail", "TAIL_CALLS"]

TAIL_CALLS = {"fwd": 0, "bwd_fused": 0, "bwd_recompute": 0, "dual_fwd": 0, "dual_bwd_fused": 0,
              "dual_bwd_recompute": 0}


def tail_ok(conv, bn, a2: torch.Tensor, idt: torch.Tensor) -> bool:
    """The recomputing tail applies: a Conv1x1 into a training ReLU FusedBatchNorm2d with an identity
    residual, channels_last operands, a shape the narrow kernel and the fold take. An fp8 Conv1x1
    takes it only where the model wired its bn3 fold for it (feature ``tail_fp8``, models/resnet.py:
    the block's conv3 then runs in bf16 inside the tail, its BN passes gone); the tail's output then
    carries no e4m3 copy, so a next fp8 conv1 quantises it itself."""
    if not (_feat("tail_recompute") and _feat("convn")) or not isinstance(conv, Conv1x1):
        return False
    tail8 = conv.fp8 and _feat("tail_fp8") and getattr(bn, "_psd_fold_conv", None) is conv
    if conv.fp8 and not tail8:
        return False
    if not isinstance(bn, FusedBatchNorm2d) or not bn.relu or not bn.training or bn.weight is None:
        return False
    if not (a2.is_cuda and a2.dtype == torch.bfloat16 and idt.dtype == torch.bfloat16 and torch.is_grad_enabled()):
        return False
    if conv.weight.dtype != torch.bfloat16 or (getattr(bn, "_psd_q8_consumer", None) is not None and not tail8):
        return False
    cin, cout = conv.in_channels, conv.out_channels
    if idt.shape != (a2.shape[0], cout, a2.shape[2], a2.shape[3]):
        return False
    if not (a2.is_contiguous(memory_format=torch.channels_last) and idt.is_contiguous(memory_format=torch.channels_last)):
        return False
    C = _native()
    return fold_ok(cin, cout) and C.convn_variants(cout) > 0 and (a2.shape[0] * a2.shape[2] * a2.shape[3]) % 8 == 0


def _kind_ok(kind: int) -> bool:
    """The narrow-kernel variant kinds the tail's 1x1 passes run on: gathered (0), persistent 1x1 (3)
    and its two-workgroups-per-CU form (4, feature convn_p2)."""
    return kind in (0, 3) or (kind == 4 and _feat("convn_p2"))


def _variant(a2, w2, M: int, cin: int, cout: int, h: int, w: int, shift) -> int:
    """Narrow-kernel tile variant of the tail's apply pass (timed on scratch buffers with placeholder
    coefficients). Only the apply pass is timed: the statistics route is chosen on its own
    (_stats_route), and with the Gram route -- the usual winner -- no statistics pass of this
    variant runs at all (timing both passes together picked a slower apply variant)."""
    C = _native()
    dev = a2.device
    # a residual operand of its own (reading the buffer being written, as an earlier version did,
    # timed the pass with its residual reads hitting the cache and picked a slower variant);
    # allocated on the first timed call only -- once decided, every forward lands here and an
    # eager [M, Cout] zero-fill per tail cost ~1 ms/step at batch 1024
    scratch = []

    def make(v):
        def fn():
            if not scratch:
                scratch.extend((torch.zeros(M, cout, device=dev, dtype=torch.bfloat16),
                                torch.zeros(2 * cout, device=dev, dtype=torch.float32)))
            res, ss = scratch
            out = torch.empty(M, cout, device=dev, dtype=torch.bfloat16)
            mb = torch.empty(M * cout // 8, device=dev, dtype=torch.uint8)
            if C.convn_(a2, w2, out, 1, 1, 1, 0, variant=v, apply_ss=ss, apply_res=res, apply_mask=mb,
                        epi_prefetch=_feat("convp_epi_prefetch")) == 0:
                raise _at.Declined("convn apply pass")
            return out
        return fn

    cands = {f"psdn{v}": make(v) for v in range(C.convn_variants(cout))
             if _kind_ok(C.convn_variant_kind(cout, v)) and C.convn_variant_ok(cout, v, 1, 1, 1, 0, w)}
    how = _at.choose(("tail", "apply", M, cin, cout), cands, next(iter(cands)))
    return int(how[4:])


def _stats_route(a2, w2, M: int, cin: int, cout: int, v: int, h: int, w: int, shift) -> str:
    """The tail's statistics: "gram" (one pass over a2 for its Gram matrix and column sums, then
    W^T G W per channel: kernels/bnfold.hip gram stats) or "pass" (the narrow kernel's
    statistics-only pass recomputing the GEMM), timed per shape. The Gram statistics are those of the
    fp32 product, the pass's those of the bf16-rounded one (what the apply pass normalises)."""
    C = _native()
    if not _feat("tail_gram") or C.convw_gram_rows(cin) <= 0 or cout % 4:
        return "pass"
    dev = a2.device

    def gram():
        P = torch.empty(C.convw_gram_rows(cin), cin, device=dev, dtype=torch.float32)
        if not C.convw_gram_(a2, P, variant=_fold_v()):
            raise _at.Declined("convw Gram launch")
        row = torch.empty(2, cout, device=dev, dtype=torch.float32)
        C.bnfold_gram_stats(P, w2, shift, M, row)
        return row

    def pas():
        part = torch.empty(_part_rows(M, cout, v, h, w, 1), 2, cout, device=dev, dtype=torch.float32)
        rows = C.convn_(a2, w2, part, 1, 1, 1, 0, part=part, shift=shift, variant=v, no_store=True)
        if rows == 0:
            raise _at.Declined("convn statistics-only pass")
        return part[:rows].sum(0)  # comparable with the Gram row (same shifted sums)

    return _at.choose(("tail", "stats", M, cin, cout), {"gram": gram, "pass": pas}, "pass")


def _conv1x1_bwd(dy, x, weight, need_x: bool, need_w: bool):
    """The library backward of a stride-1 1x1 convolution: (dx, dw, None)."""
    return torch.ops.aten.convolution_backward(dy, x, weight, None, [1, 1], [0, 0], [1, 1], False, [0, 0], 1,
                                               [need_x, need_w, False])


class _TailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a2, weight, gamma, beta, idt, conv, bn, resid_to):
        C = _native()
        n, cin, h, w = a2.shape
        cout = weight.shape[0]
        M = n * h * w
        w2 = weight.reshape(cout, cin)
        if not w2.is_contiguous():
            w2 = w2.contiguous()
        v = _variant(a2, w2, M, cin, cout, h, w, bn.running_mean)
        if _stats_route(a2, w2, M, cin, cout, v, h, w, bn.running_mean) == "gram":
            # sum y = W s, sum y^2 = W^T G W from one read of a2 (G = a2^T a2, s = 1^T a2: the Gram
            # launch of the weight-gradient kernel) -- the GEMM is not recomputed for the statistics
            P = torch.empty(C.convw_gram_rows(cin), cin, device=a2.device, dtype=torch.float32)
            if not C.convw_gram_(a2, P, variant=_fold_v()):
                raise RuntimeError("psd tail: convw declined the Gram launch")
            part = torch.empty(1, 2, cout, device=a2.device, dtype=torch.float32)
            C.bnfold_gram_stats(P, w2, bn.running_mean, M, part[0])
            rows = 1
        else:
            part = torch.empty(_part_rows(M, cout, v, h, w, 1), 2, cout, device=a2.device, dtype=torch.float32)
            rows = C.convn_(a2, w2, part, 1, 1, 1, 0, part=part, shift=bn.running_mean, variant=v, no_store=True)
            if rows == 0:
                raise RuntimeError("psd tail: convn declined the statistics-only pass")
        mean, invstd, ss = C.bn_finalize(part, rows, M, gamma, beta, bn.running_mean, bn.running_var,
                                         bn_momentum(bn), bn.eps, bn.num_batches_tracked)
        out = torch.empty(M, cout, device=a2.device, dtype=torch.bfloat16)
        mbits = torch.empty(M * cout // 8, device=a2.device, dtype=torch.uint8)
        if C.convn_(a2, w2, out, 1, 1, 1, 0, variant=v, apply_ss=ss, apply_res=idt, apply_mask=mbits,
                    epi_prefetch=_feat("convp_epi_prefetch")) == 0:
            raise RuntimeError("psd tail: convn declined the apply pass")
        y = _from_2d(out, n, h, w)
        # the consumer convolution's bwd-data epilogue runs this BN's backward reduction without its
        # input (bx None: ops/conv.py _bn_bwd_fusion / _dgrad_route)
        bn._psd_fwd = BnFwd(y, None, mean, ss, mbits)
        ctx.mod = conv
        _fwd_records(ctx, conv)
        ctx.bn, ctx.resid_to, ctx.v = bn, resid_to, v
        ctx.save_for_backward(a2, weight, gamma, mean, invstd, mbits)
        TAIL_CALLS["fwd"] += 1
        return y

    @staticmethod
    def backward(ctx, dy):
        a2, weight, gamma, mean, invstd, mbits = ctx.saved_tensors
        C = _native()
        bn = ctx.bn
        bn._psd_fwd = None
        n, cin, h, w = a2.shape
        cout = weight.shape[0]
        M = n * h * w
        dgo, dbo = sinks(bn)
        pre = take(bn, "_psd_bwd_pre", dy, strides=False)
        need_x, need_w = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        if pre is not None and pre.part_d is None:
            # g = mask (dX + dr) and its partials (sum g, -mean sum g) from the consumer's epilogue
            g, part, rows = pre[:3]
            if part.shape[0] <= rows:
                raise RuntimeError("psd tail: the partials buffer has no row for sum g y")
            P = torch.empty(C.convw_fold_rows(cout, cin), cin, device=dy.device, dtype=torch.float32)
            if not C.convw_(g, a2, P, 1, 1, 1, 0, variant=_fold_v(), fold=True):
                raise RuntimeError("psd tail: convw_ declined the fold wgrad")
            C.bnfold_rowdot(P, weight, part[rows])
            g, coef, dg, db = C.bn_bwd_coef(g, g, gamma, mean, invstd, part=part, rows=rows + 1, dgamma_out=dgo,
                                            dbeta_out=dbo)
            y = None
            TAIL_CALLS["bwd_fused"] += 1
        else:
            # no fused consumer: recompute y3 once and run the ordinary BN backward (+ fold)
            P = None
            w2 = weight.reshape(cout, cin).contiguous()
            out = torch.empty(M, cout, device=dy.device, dtype=torch.bfloat16)
            if C.convn_(a2, w2, out, 1, 1, 1, 0, variant=ctx.v) == 0:
                raise RuntimeError("psd tail: convn declined the recompute")
            y = _from_2d(out, n, h, w)
            g, coef, dg, db = C.bn_bwd_coef(dy, y, gamma, mean, invstd, mbits=mbits, dy2=pop_dr(bn), dgamma_out=dgo,
                                            dbeta_out=dbo)
            TAIL_CALLS["bwd_recompute"] += 1
        res_grad = route_res_grad(ctx.resid_to, g)
        dx, dw, dyu = _fold_backward(ctx, FoldPending(g, coef, y, P), a2, weight, need_x, need_w)
        if dyu is not None:  # (y present and the unfolded path won): the ordinary conv backward on dy
            dx, dw, _ = _conv1x1_bwd(dyu, a2, weight, need_x, need_w)
            dw = _write_dw(_sink_view(ctx.mod, weight), lambda: dw, None)
        return dx, dw, dg, db, res_grad, None, None, None


def conv_bn_tail(conv, bn, a2: torch.Tensor, idt: torch.Tensor, resid_to=None) -> torch.Tensor:
    """``relu(bn(conv(a2)) + idt)`` with conv's output never stored (see module docstring).
    ``resid_to``: the fused BN that produced ``idt`` (the residual gradient is handed to it)."""
    return _TailFn.apply(a2, conv.weight, bn.weight, bn.bias, idt, conv, bn, resid_to)


# ---------------------------------------------------------------------------------------------
# Downsample blocks: relu(bn3(conv3(a2)) + bnd(convd(x))) with NEITHER convolution output stored.
#
# The unfused dual tail writes y3 = conv3(a2) and yd = convd(x) (two 4x-wide activations: 1.6 GB
# each at ResNet-50 b1024 layer 1), then one apply pass reads both and writes the block output. Here
# (1x1 downsample convolutions of stride 1 -- layer 1 -- or 2 -- layer 2, on the quarter grid of its
# input; the Gram statistics take inputs of up to 256 channels):
#   forward   1. the two BNs' statistics from the Gram matrices of a2 and x (sum y = W s,
#              sum y^2 = W^T G W: one read of each 64-wide input, the GEMMs are not recomputed)
#             2. both BN finalizes
#             3. ONE apply GEMM on the narrow kernel with the K-concatenated operand [a2 | x] and the
#                weights [r3 o W3 | rd o Wd] (per channel the branch with the larger BN scale keeps
#                its weights, the other is scaled by the ratio of the scales): out = relu(s_big . +
#                t3 + td) and its ReLU bit-mask -- y3 and yd never reach HBM
#   backward  as the folded dual tail (ops/bn.py _BNAddBNReluFn "pair" path): the consumer's
#             bwd-data epilogue reduces sum g; sum g y3 / sum g yd come from the fold wgrads' g^T a2 /
#             g^T x (rowdot); both BNs' input gradients are folded into their convolutions' backward.
#             Without that fused consumer, y3 and yd are recomputed once for the ordinary dual BN
#             backward.
# The ratio-scaled weights are rounded once to bf16 (a K-concatenated GEMM has one accumulator, so
# the per-channel scales of the two BNs cannot both be applied in the epilogue).


def dual_tail_ok(conv3, bn3, a2: torch.Tensor, convd, bnd, xin: torch.Tensor) -> bool:
    """The recomputing dual tail applies: bf16 Conv1x1 conv3 and a stride-1 Conv1x1 downsample into
    training FusedBatchNorm2d bn3 (ReLU) / bnd (no ReLU), channels_last inputs of one spatial shape,
    shapes the fold, the Gram statistics and the K-concatenated narrow kernel take."""
    if not (_feat("tail_recompute") and _feat("dual_recompute") and _feat("convn") and _feat("bn_fold")):
        return False
    if not isinstance(conv3, Conv1x1) or conv3.fp8 or getattr(convd, "fp8", False):
        return False
    strided = _ds_stride(convd)
    if strided is None:
        return False
    if not (isinstance(bn3, FusedBatchNorm2d) and isinstance(bnd, FusedBatchNorm2d) and bn3.relu and not bnd.relu
            and bn3.training and bnd.training and bn3.weight is not None and bnd.weight is not None):
        return False
    if getattr(bn3, "_psd_q8_consumer", None) is not None or not torch.is_grad_enabled():
        return False
    for t in (a2, xin):
        if not (t.is_cuda and t.dtype == torch.bfloat16 and t.dim() == 4
                and t.is_contiguous(memory_format=torch.channels_last)):
            return False
    if a2.shape[0] != xin.shape[0] or a2.shape[2] * strided != xin.shape[2] or a2.shape[3] * strided != xin.shape[3]:
        return False
    if conv3.weight.dtype != torch.bfloat16 or convd.weight.dtype != torch.bfloat16:
        return False
    c3, cd, cout = conv3.in_channels, convd.in_channels, conv3.out_channels
    if convd.out_channels != cout or a2.shape[1] != c3 or xin.shape[1] != cd or cout % 4:
        return False
    C = _native()
    if not (fold_ok(c3, cout) and fold_ok(cd, cout) and C.convw_gram_rows(c3) > 0 and C.convw_gram_rows(cd) > 0):
        return False
    n, _, h, w = a2.shape
    return (n * h * w) % 8 == 0 and any(_dual_variants(cout, w))


def _ds_stride(convd):
    """1 for a Conv1x1 downsample, 2 for a stride-2 1x1 ConvNHWC one (its input is subsampled to the
    quarter grid first, the gradient handed back on the quarter grid), None otherwise."""
    if isinstance(convd, Conv1x1):
        return 1
    if isinstance(convd, ConvNHWC) and convd.kernel_size == (1, 1) and convd.stride == (2, 2) \
            and convd.padding == (0, 0) and convd.groups == 1:
        return 2
    return None


def _dual_variants(cout: int, w: int) -> list:
    C = _native()
    return [v for v in range(C.convn_variants(cout))
            if _kind_ok(C.convn_variant_kind(cout, v)) and C.convn_variant_ok(cout, v, 1, 1, 1, 0, w, True)]


def _gram_moments(x, w2, shift, M: int) -> torch.Tensor:
    """[1, 2, Cout] shifted moments of y = x w2^T from x's Gram matrix (kernels/bnfold.hip)."""
    C = _native()
    cin = x.shape[1]
    P = torch.empty(C.convw_gram_rows(cin), cin, device=x.device, dtype=torch.float32)
    if not C.convw_gram_(x, P, variant=_fold_v()):
        raise RuntimeError("psd dual tail: convw declined the Gram launch")
    part = torch.empty(1, 2, w2.shape[0], device=x.device, dtype=torch.float32)
    C.bnfold_gram_stats(P, w2, shift, M, part[0])
    return part


def _finalize(bn, part, M: int):
    return _native().bn_finalize(part, 1, M, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn_momentum(bn),
                                 bn.eps, bn.num_batches_tracked)


def dual_weights_reference(w3_2, wd_2, ss3, ss_d):
    """torch-op form of C.bnfold_dual_weights (the numerics tests' reference): {wcat, ss}."""
    cout = w3_2.shape[0]
    s3, sd = ss3[:cout], ss_d[:cout]
    big3 = s3.abs() >= sd.abs()
    sbig = torch.where(big3, s3, sd)
    safe = torch.where(sbig == 0, torch.ones_like(sbig), sbig)
    r3 = torch.where(big3, torch.ones_like(s3), s3 / safe)
    rd = torch.where(big3, sd / safe, torch.ones_like(sd))
    r3 = torch.where(sbig == 0, torch.zeros_like(r3), r3)
    rd = torch.where(sbig == 0, torch.zeros_like(rd), rd)
    wcat = torch.cat([w3_2.float() * r3[:, None], wd_2.float() * rd[:, None]], 1).to(torch.bfloat16)
    return wcat, torch.cat([sbig, ss3[cout:] + ss_d[cout:]])


class _DualTailFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a2, w3, g3, b3, xfull, wd, gd, bd, conv3, bn3, convd, bnd):
        C = _native()
        ctx.full_hw = tuple(xfull.shape[2:])
        ctx.stride = _ds_stride(convd)
        # a stride-2 1x1 downsample is a stride-1 one on the quarter grid of its input
        xin = xfull if ctx.stride == 1 else C.subsample2(xfull)
        n, c3, h, w = a2.shape
        cd, cout = xin.shape[1], w3.shape[0]
        M = n * h * w
        w3_2, wd_2 = w3.reshape(cout, c3).contiguous(), wd.reshape(cout, cd).contiguous()
        mean3, invstd3, ss3 = _finalize(bn3, _gram_moments(a2, w3_2, bn3.running_mean, M), M)
        mean_d, invstd_d, ss_d = _finalize(bnd, _gram_moments(xin, wd_2, bnd.running_mean, M), M)
        # per output channel the branch with the larger BN scale keeps its bf16 weights exactly and
        # the other one's are scaled by the ratio (|ratio| <= 1, fp32 product, one rounding); the
        # epilogue applies the larger scale and the summed shift t3 + td:
        #   out = s_big (a2 W3'^T + x Wd'^T) + t3 + td   (s3 = 0, e.g. zero-init gamma: W3' = 0)
        # (one launch, kernels/bnfold.hip; dual_weights_reference above is the same in torch ops)
        wcat, ssc = C.bnfold_dual_weights(w3_2, wd_2, ss3, ss_d)
        out = torch.empty(M, cout, device=a2.device, dtype=torch.bfloat16)
        mbits = torch.empty(M * cout // 8, device=a2.device, dtype=torch.uint8)

        def make(v):
            def fn():
                o = torch.empty(M, cout, device=a2.device, dtype=torch.bfloat16)
                mb = torch.empty(M * cout // 8, device=a2.device, dtype=torch.uint8)
                if C.convn_(a2, wcat, o, 1, 1, 1, 0, variant=v, x2=xin, apply_ss=ssc, apply_mask=mb,
                            epi_prefetch=_feat("convp_epi_prefetch")) == 0:
                    raise _at.Declined("convn dual apply pass")
                return o
            return fn

        cands = {f"psdn{v}": make(v) for v in _dual_variants(cout, w)}
        v = int(_at.choose(("tail", "dual_apply", M, c3, cd, cout), cands, next(iter(cands)))[4:])
        if C.convn_(a2, wcat, out, 1, 1, 1, 0, variant=v, x2=xin, apply_ss=ssc, apply_mask=mbits,
                    epi_prefetch=_feat("convp_epi_prefetch")) == 0:
            raise RuntimeError("psd dual tail: convn declined the apply pass")
        y = _from_2d(out, n, h, w)
        # the consumer convolution's bwd-data epilogue reduces bn3's backward without its input
        # (mode 2, bx None: sum g and -mean3 sum g); backward completes both BNs from the fold products
        bn3._psd_fwd = BnFwd(y, None, mean3, None, mbits)
        ctx.r3, ctx.rd = types.SimpleNamespace(mod=conv3), types.SimpleNamespace(mod=convd)
        _fwd_records(ctx.r3, conv3)
        _fwd_records(ctx.rd, convd)
        ctx.bn3, ctx.bnd, ctx.v = bn3, bnd, v
        ctx.save_for_backward(a2, w3, g3, mean3, invstd3, xin, wd, gd, mean_d, invstd_d, mbits)
        TAIL_CALLS["dual_fwd"] += 1
        return y

    @staticmethod
    def backward(ctx, dy):
        a2, w3, g3, mean3, invstd3, xin, wd, gd, mean_d, invstd_d, mbits = ctx.saved_tensors
        C = _native()
        bn3, bnd = ctx.bn3, ctx.bnd
        bn3._psd_fwd = None
        (dg3o, db3o), (dgdo, dbdo) = sinks(bn3), sinks(bnd)
        n, c3, h, w = a2.shape
        cd, cout = xin.shape[1], w3.shape[0]
        M = n * h * w
        pre = take(bn3, "_psd_bwd_pre", dy, strides=False)
        need = ctx.needs_input_grad
        if pre is not None and pre.part_d is None:
            g = pre.g  # (neither BN input was stored: g stands in for both)
            Ps, dg3, db3, dgd, dbd, coef, coef_d = dual_from_fold(
                pre, w3, a2, wd, xin, g, g3, mean3, invstd3, g, gd, mean_d, invstd_d, (dg3o, db3o), (dgdo, dbdo))
            dxa, dw3, _ = _fold_backward(ctx.r3, FoldPending(g, coef, None, Ps[0]), a2, w3, need[0], need[1])
            dxi, dwd, _ = _fold_backward(ctx.rd, FoldPending(g, coef_d, None, Ps[1]), xin, wd, need[4], need[5])
            TAIL_CALLS["dual_bwd_fused"] += 1
            return dxa, dw3, dg3, db3, _DualTailFn._input_grad(ctx, dxi), dwd, dgd, dbd, None, None, None, None
        # no fused consumer: recompute y3 and yd once, the ordinary dual BN backward (one reduce and
        # one elementwise pass) and the two convolutions' backward
        ys = []
        for inp, wt, cin in ((a2, w3, c3), (xin, wd, cd)):
            o = torch.empty(M, cout, device=dy.device, dtype=torch.bfloat16)
            if C.convn_(inp, wt.reshape(cout, cin).contiguous(), o, 1, 1, 1, 0, variant=0) == 0:
                raise RuntimeError("psd dual tail: convn declined the recompute")
            ys.append(_from_2d(o, n, h, w))
        dx3, dxd, dg3, db3, dgd, dbd = C.bn_bwd_dual(dy, ys[0], g3, mean3, invstd3, mbits, pop_dr(bn3), ys[1], gd,
                                                     mean_d, invstd_d, dg3o, db3o, dgdo, dbdo)
        dxa, dw3, _ = _conv1x1_bwd(dx3, a2, w3, need[0], need[1])
        dxi, dwd, _ = _conv1x1_bwd(dxd, xin, wd, need[4], need[5])
        dw3 = _write_dw(_sink_view(ctx.r3.mod, w3), lambda: dw3, None)
        dwd = _write_dw(_sink_view(ctx.rd.mod, wd), lambda: dwd, None)
        TAIL_CALLS["dual_bwd_recompute"] += 1
        return dxa, dw3, dg3, db3, _DualTailFn._input_grad(ctx, dxi), dwd, dgd, dbd, None, None, None, None

    @staticmethod
    def _input_grad(ctx, dxi):
        """The downsample branch's input gradient: as is for a stride-1 downsample; for a stride-2
        one it lives on the quarter grid -- queued on the BN that produced the block input (the
        consumer conv1's bwd-data epilogue adds it at even (h, w), kernels/convn.hip mode 5) with a
        zero-stride marker returned to the block's _Fork, or materialised when nobody takes it."""
        if dxi is None or ctx.stride == 1:
            return dxi
        H, W = ctx.full_hw
        dr = StridedDr(dxi if dxi.is_contiguous(memory_format=torch.channels_last)
                       else dxi.contiguous(memory_format=torch.channels_last), H, W)
        to = ctx.rd.strided_to
        if isinstance(to, FusedBatchNorm2d):
            to._psd_pending_dr.append(dr)
            n, c = dxi.shape[:2]
            return torch.zeros((), device=dxi.device, dtype=dxi.dtype).expand(n, c, H, W)
        return dr.full()


def conv_bn_dual_tail(conv3, bn3, a2: torch.Tensor, convd, bnd, xin: torch.Tensor) -> torch.Tensor:
    """``relu(bn3(conv3(a2)) + bnd(convd(xin)))`` with neither convolution output stored (see above)."""
    return _DualTailFn.apply(a2, conv3.weight, bn3.weight, bn3.bias, xin, convd.weight, bnd.weight, bnd.bias,
                             conv3, bn3, convd, bnd)
