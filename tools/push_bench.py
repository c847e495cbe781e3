#!/usr/bin/env python3
"""Time what the MX fp8 gradient push costs and saves on ONE GPU (csrc/kernels/xfer.hip
xfer_quant_kernel and the MX-source instantiations of the fused apply):

  * the plain scatter (``xfer_``: the bf16 gradient copied with non-temporal stores) against the
    quantising scatter (``push_quant_mx_``: bf16 in, e4m3 payload + E8M0 scale bytes out) for a
    ResNet-50-size and a BERT-base-size gradient into device memory, at the engine's default
    workgroup budget (48 per segment) and at 256;
  * the quantising scatter with error feedback (``push_quant_mx_`` with a residual: the fp32
    residual read, added, and rewritten in the same pass) against the plain quantising scatter, for
    bf16 and fp32 gradients of both sizes at both budgets;
  * the flat fused apply (momentum, adamw) fed K = 1, 4, 8, 16 bf16 sources against K MX sources of
    the ResNet-50 size, alternating the two so that drift hits both alike.

Each figure is the median of ``--reps`` windows of ``--iters`` calls (device events) with the
min-max spread of the windows beside it. On a build without the fp8 push (``--tree`` pointing at a
checkout of the parent commit) only the bf16 scatter and apply are timed: the same tool gives the
baseline that the bf16 path must still match.

What this cannot show: the destination here is this GPU's own (cached) memory. The push's saving on
an xGMI link, and the owner's saving when its inbox is uncached memory written by peers, need
N > 1 GPUs.

  python tools/push_bench.py [--json out.json] [--md out.md] [--tree /path/to/other/checkout] [--bf16-only]
"""
import argparse
import json
import os
import statistics
import sys

SIZES = {"resnet50": 25_557_032, "bert_base": 110_104_890}  # parameters of the two shipped recipes


def _round(n, a=64):
    return (n + a - 1) // a * a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    ap.add_argument("--md", default="", help="also write the tables to this file")
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose built package is timed (default: this one)")
    ap.add_argument("--bf16-only", action="store_true",
                    help="time the bf16 scatter and apply alone, with the allocations of a build without the fp8 "
                         "push (the like-for-like run against --tree <parent>)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch

    from parameter_server_distributed_amd import native
    from parameter_server_distributed_amd.ops.optim import OptimConfig, OptimDyn

    if not torch.cuda.is_available():
        raise SystemExit("push_bench needs the GPU: a CPU timing says nothing about these kernels")
    C = native()
    dev = torch.device("cuda", 0)
    has_mx = hasattr(C, "push_quant_mx_") and not a.bf16_only
    has_ef = has_mx and "residual" in (C.push_quant_mx_.__doc__ or "")
    lines = []

    def out(s=""):
        print(s, flush=True)
        lines.append(s)

    def window_us(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(a.iters):
            fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) / a.iters * 1e3

    def timed(fns):
        """{name: (median us, min, max)}; the candidates alternate window by window."""
        for fn in fns.values():  # warm-up: code objects, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t[k].append(window_us(fn))
        return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}

    def cell(r, nbytes):
        m, lo, hi = r
        return f"{m:.1f} ({lo:.1f}-{hi:.1f}) | {nbytes / m / 1e6:.2f}"

    res = {"device": torch.cuda.get_device_name(0), "tree": os.path.abspath(a.tree), "has_fp8_push": has_mx,
           "has_error_feedback": has_ef, "iters": a.iters, "reps": a.reps, "scatter": [], "feedback": [], "apply": []}
    out(f"device: {res['device']}; fp8 push in this build: {has_mx}; median of {a.reps} windows of {a.iters} calls")
    out()
    out("| gradient | workgroups | bf16 scatter us (min-max) | TB/s read+written | bytes written | "
        "quantising scatter us (min-max) | TB/s read+written | bytes written | time ratio |")
    out("|---|---:|---:|---:|---:|---:|---:|---:|---:|")
    for name, n in SIZES.items():
        n = _round(n)
        g = (torch.randn(n, device=dev) * 0.05).to(torch.bfloat16)
        dst = torch.empty_like(g)
        q = torch.empty(n, dtype=torch.uint8, device=dev) if has_mx else None
        sc = torch.empty(n // 32, dtype=torch.uint8, device=dev) if has_mx else None
        for bps in (48, 256):
            fns = {"bf16": lambda: C.xfer_([g], [dst], bps, True)}
            if has_mx:
                fns["fp8"] = lambda: C.push_quant_mx_(g, q, sc, bps)
            r = timed(fns)
            assert torch.equal(dst, g)
            row = f"| {name} | {bps} | {cell(r['bf16'], 4 * n)} | {2 * n} | "
            if has_mx:
                row += f"{cell(r['fp8'], 2 * n + n + n // 32)} | {n + n // 32} | {r['fp8'][0] / r['bf16'][0]:.3f} |"
            else:
                row += "- | - | - | - |"
            out(row)
            res["scatter"].append({"gradient": name, "n": n, "blocks_per_seg": bps, "bf16_us": r["bf16"],
                                   "fp8_us": r.get("fp8"), "bf16_bytes_written": 2 * n,
                                   "fp8_bytes_written": n + n // 32})
        del g, dst, q, sc

    if has_ef:
        # bytes through local HBM per element: source read (2 / 4) + payload and scales written (33/32),
        # with feedback 8 more (the fp32 residual read and rewritten)
        out()
        out("| gradient | source | workgroups | quantising scatter us (min-max) | TB/s read+written | "
            "with error feedback us (min-max) | TB/s read+written | time ratio |")
        out("|---|---|---:|---:|---:|---:|---:|---:|")
        for name, n in SIZES.items():
            n = _round(n)
            q = torch.empty(n, dtype=torch.uint8, device=dev)
            sc = torch.empty(n // 32, dtype=torch.uint8, device=dev)
            resid = torch.zeros(n, device=dev)
            for dt in (torch.bfloat16, torch.float32):
                g = (torch.randn(n, device=dev) * 0.05).to(dt)
                esz = g.element_size()
                for bps in (48, 256):
                    r = timed({"fp8": lambda: C.push_quant_mx_(g, q, sc, bps),
                               "ef": lambda: C.push_quant_mx_(g, q, sc, bps, resid)})
                    plain_b = esz * n + n + n // 32
                    src = "bf16" if dt == torch.bfloat16 else "fp32"
                    out(f"| {name} | {src} | {bps} | {cell(r['fp8'], plain_b)} | {cell(r['ef'], plain_b + 8 * n)} | "
                        f"{r['ef'][0] / r['fp8'][0]:.3f} |")
                    res["feedback"].append({"gradient": name, "n": n, "source": src, "blocks_per_seg": bps,
                                            "fp8_us": r["fp8"], "ef_us": r["ef"], "fp8_bytes": plain_b,
                                            "ef_bytes": plain_b + 8 * n})
                del g
            del q, sc, resid

    n = _round(SIZES["resnet50"])
    out()
    out("| kind | K | bf16 sources us (min-max) | TB/s | source bytes | MX sources us (min-max) | TB/s | "
        "source bytes | time ratio |")
    out("|---|---:|---:|---:|---:|---:|---:|---:|---:|")
    for kind in ("momentum", "adamw"):
        cfg = OptimConfig(kind, lr=1e-3, momentum=0.9, weight_decay=1e-2)
        for K in (1, 4, 8, 16):
            w = torch.randn(n, device=dev)
            s1 = torch.zeros(n, device=dev)
            s2 = torch.zeros(n, device=dev) if cfg.num_states >= 2 else None
            sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            gs = [(torch.randn(n, device=dev) * 0.01).to(torch.bfloat16) for _ in range(K)]
            dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
            C.optim_advance_(dyn.t, cfg.beta1, cfg.beta2)
            args = (w, gs, s1, s2, sh, dyn.t, cfg.code, cfg.momentum, cfg.dampening, cfg.nesterov, cfg.weight_decay,
                    cfg.beta1, cfg.beta2, cfg.eps, cfg.maximize, 0)
            fns = {"bf16": lambda: C.fused_apply_(*args)}
            if has_mx:
                qs = [torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(K)]
                ss = [torch.empty(n // 32, dtype=torch.uint8, device=dev) for _ in range(K)]
                for g, q, s in zip(gs, qs, ss):
                    C.push_quant_mx_(g, q, s, 0)
                margs = (w, qs) + args[2:]
                fns["fp8"] = lambda: C.fused_apply_(*margs, [], ss)
            r = timed(fns)
            rest = n * (8 + 8 * cfg.num_states + 2)  # master r/w, states r/w, bf16 shadow
            sb, sm = 2 * n * K, (n + n // 32) * K
            row = f"| {kind} | {K} | {cell(r['bf16'], sb + rest)} | {sb} | "
            if has_mx:
                row += f"{cell(r['fp8'], sm + rest)} | {sm} | {r['fp8'][0] / r['bf16'][0]:.3f} |"
            else:
                row += "- | - | - | - |"
            out(row)
            res["apply"].append({"kind": kind, "K": K, "n": n, "bf16_us": r["bf16"], "fp8_us": r.get("fp8"),
                                 "bf16_source_bytes": sb, "fp8_source_bytes": sm, "other_bytes": rest})
            del w, s1, s2, sh, gs
    for path, text in ((a.json, json.dumps(res, indent=1)), (a.md, "\n".join(lines) + "\n")):
        if path:
            os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
            with open(path, "w") as f:
                f.write(text)


if __name__ == "__main__":
    main()
