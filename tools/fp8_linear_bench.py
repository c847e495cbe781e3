#!/usr/bin/env python3
"""Time the MX fp8 Linear recipe (ops/linear.py fp8="mx") against bf16 per BERT-base Linear shape
(M = 32768 tokens = batch 256 x seq 128; K / N of qkv, proj, ffn1, ffn2), each part on its own:

  bf16 fwd / dgrad     the module's forward / bwd-data as routed today (ops/autotune.py picks per shape)
  fp8 fwd GEMM         gemm_fp8_ on MX e4m3 x, W (bias + activation in the epilogue)
  fp8 dgrad GEMM       gemm_fp8_ on MX e5m2 dy, MX e4m3 W^T
  q(x), q(W), q(dy)    the stand-alone quantize_mx passes the recipe runs when no hand-over / published
                       copy arrives; q_t(W) = quant_mx_t_ against a transpose copy + quant_mx_
  LayerNorm forward    with and without the MX side output (the hand-over that replaces q(x))
  weight gradient      (feature fp8_wgrad) the bf16 weight gradient as routed today; gemm_fp8_splitk_ on MX
                       e4m3 dy^T, x^T alone; quantize_mx_dual(dy) against the quantize_mx(e5m2) + quantize_mx_t
                       passes it replaces; quantize_mx_t(x); and the sums of the two arms: bf16 = wgrad +
                       q_e5m2(dy) (what bwd-data needs anyway), fp8 = GEMM + q_dual(dy) + q_t(x)

Variants are interleaved over rounds in one process; the table gives the median and the minimum (us).
Random operands (zero-filled ones read high on this chip).

  python tools/fp8_linear_bench.py [--rounds 7] [--iters 20] [--tokens 32768]
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402
from parameter_server_distributed_amd.ops import quantize_mx, quantize_mx_dual, quantize_mx_t  # noqa: E402
from parameter_server_distributed_amd.ops.linear import MfmaLinear, _dgrad_route, _route  # noqa: E402

SHAPES = [("qkv", 768, 2304, None), ("proj", 768, 768, None), ("ffn1", 768, 3072, "gelu"), ("ffn2", 3072, 768, None)]


def t_us(fn, it):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / it * 1e3


def interleaved(variants: dict, rounds: int, it: int) -> dict:
    for fn in variants.values():  # warm every shape (code objects, autotune decisions)
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            times[k].append(t_us(fn, it))
    return {k: (statistics.median(v), min(v)) for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--tokens", type=int, default=32768)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fp8_linear_bench: needs the GPU")
    C = native()
    dev = torch.device("cuda")
    M = a.tokens
    torch.manual_seed(0)
    print(f"M = {M} tokens, {a.rounds} interleaved rounds x {a.iters} calls, us per call: median (min)\n")
    print("| layer | K | N | bf16 fwd | fp8 fwd GEMM | q(x) | q(W) | bf16 dgrad | fp8 dgrad GEMM | q_e5m2(dy) | q_t(W) | "
          "transpose + q(W^T) |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for name, K, N, act in SHAPES:
        lin = MfmaLinear(K, N, act=act).to(dev, torch.bfloat16)
        with torch.no_grad():
            lin.weight.copy_(torch.randn(N, K) * 0.02)
            lin.bias.copy_(torch.randn(N) * 0.1)
        w, b = lin.weight.detach(), lin.bias.detach()
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        dy = torch.randn(M, N, device=dev).to(torch.bfloat16)
        y = torch.empty(M, N, device=dev, dtype=torch.bfloat16)
        aux = torch.empty_like(y) if act == "gelu" else None
        dx = torch.empty(M, K, device=dev, dtype=torch.bfloat16)
        xq, sx = quantize_mx(x)
        wq, sw = quantize_mx(w)
        dq, sd = quantize_mx(dy, e5m2=True)
        tq, st = quantize_mx_t(w)
        acode = 2 if act == "gelu" else 0
        dxb = torch.empty_like(dx)

        def bf16_fwd():
            with torch.no_grad():
                lin(x)

        def bf16_dgrad():  # the route the module's backward takes for this shape (ops/autotune.py)
            _dgrad_route(("dgrad", M, K, N), dy, w, dxb)()

        res = interleaved({
            "bf16_fwd": bf16_fwd,
            "fp8_fwd": lambda: C.gemm_fp8_(xq, wq, sx, sw, y, b, acode, aux),
            "qx": lambda: quantize_mx(x),
            "qw": lambda: quantize_mx(w),
            "bf16_dgrad": bf16_dgrad,
            "fp8_dgrad": lambda: C.gemm_fp8_(dq, tq, sd, st, dx),
            "qdy": lambda: quantize_mx(dy, e5m2=True),
            "qtw": lambda: quantize_mx_t(w),
            "t_qw": lambda: quantize_mx(w.t().contiguous()),
        }, a.rounds, a.iters)
        cells = " | ".join(f"{res[k][0]:.1f} ({res[k][1]:.1f})" for k in
                           ("bf16_fwd", "fp8_fwd", "qx", "qw", "bf16_dgrad", "fp8_dgrad", "qdy", "qtw", "t_qw"))
        print(f"| {name} | {K} | {N} | {cells} |", flush=True)
    # the weight gradient (feature fp8_wgrad): dW [N, K] = dy^T x over M tokens
    print("\n| layer | K | N | bf16 wgrad | fp8 wgrad GEMM | q_dual(dy) | q_e5m2(dy) + q_t(dy) | q_t(x) | "
          "bf16 arm: wgrad + q_e5m2(dy) | fp8 arm: GEMM + q_dual(dy) + q_t(x) | splits |")
    print("|---|---:|---:|---:|---:|---:|---:|---:|---:|---:|---:|")
    for name, K, N, _act in SHAPES:
        x = torch.randn(M, K, device=dev).to(torch.bfloat16)
        dy = torch.randn(M, N, device=dev).to(torch.bfloat16)
        dwb = torch.empty(N, K, device=dev, dtype=torch.bfloat16)
        dw8 = torch.empty_like(dwb)
        gq, sg = quantize_mx_t(dy)
        xq, sx = quantize_mx_t(x)

        def bf16_wgrad():  # the route the module's backward takes for this shape (ops/autotune.py)
            _route(("wgrad", M, K, N), lambda: C.gemm_splitk_(dy, x, False, False, dwb, False, 1.0, 0),
                   lambda: torch.mm(dy.t(), x, out=dwb), dwb)()

        def two_passes():  # what the dual kernel replaces
            quantize_mx(dy, e5m2=True)
            quantize_mx_t(dy)

        res = interleaved({
            "bf16_wgrad": bf16_wgrad,
            "fp8_wgrad": lambda: C.gemm_fp8_splitk_(gq, xq, sg, sx, dw8, False, 1.0, 0),
            "qdual": lambda: quantize_mx_dual(dy, e5m2_row=True, e5m2_t=False),
            "q2": two_passes,
            "qtx": lambda: quantize_mx_t(x),
            "qdy": lambda: quantize_mx(dy, e5m2=True),
        }, a.rounds, a.iters)
        arm_b = tuple(res["bf16_wgrad"][i] + res["qdy"][i] for i in (0, 1))
        arm_8 = tuple(res["fp8_wgrad"][i] + res["qdual"][i] + res["qtx"][i] for i in (0, 1))
        cells = " | ".join(f"{res[k][0]:.1f} ({res[k][1]:.1f})" for k in ("bf16_wgrad", "fp8_wgrad", "qdual", "q2", "qtx"))
        print(f"| {name} | {K} | {N} | {cells} | {arm_b[0]:.1f} ({arm_b[1]:.1f}) | {arm_8[0]:.1f} ({arm_8[1]:.1f}) | "
              f"{C.gemm_fp8_splits(N, K, M)} |", flush=True)
    # the LayerNorm forward with and without the MX side output (H = 768)
    H = 768
    xs = torch.randn(M, H, device=dev).to(torch.bfloat16)
    hs = torch.randn_like(xs)
    g = torch.ones(H, device=dev, dtype=torch.bfloat16)
    be = torch.zeros(H, device=dev, dtype=torch.bfloat16)
    step = torch.tensor([3], device=dev, dtype=torch.int64)
    q8 = torch.empty(M, H, device=dev, dtype=torch.float8_e4m3fn)
    s8 = torch.empty(M * H // 32, device=dev, dtype=torch.uint8)
    res = interleaved({
        "ln": lambda: C.ln_fwd(xs, hs, g, be, 1e-12, 0.1, 5, step),
        "ln_mx": lambda: C.ln_fwd(xs, hs, g, be, 1e-12, 0.1, 5, step, q8, s8),
        "q": lambda: quantize_mx(xs),
    }, a.rounds, a.iters)
    print(f"\nLayerNorm forward [{M}, {H}], p = 0.1: plain {res['ln'][0]:.1f} ({res['ln'][1]:.1f}) us, with the MX output "
          f"{res['ln_mx'][0]:.1f} ({res['ln_mx'][1]:.1f}) us; the quantize_mx pass it replaces {res['q'][0]:.1f} "
          f"({res['q'][1]:.1f}) us")


if __name__ == "__main__":
    main()
