#!/usr/bin/env python3
"""Time what global-norm gradient clipping costs on the GPU (csrc/kernels/clip.hip and the scaled
instantiations of the fused apply):

  * the norm pass -- both launches of ``grad_clip_coef_`` -- over a ResNet-50-size and a
    BERT-base-size flat gradient, bf16 and fp32, next to ``torch.linalg.vector_norm`` on the same
    buffer (us per call, and TB/s over the bytes of one read of the buffer);
  * the flat fused apply (momentum, adamw) with and without per-source scales at K = 1, 4, 16 bf16
    sources of the ResNet-50 size, alternating the two so that drift hits both alike.

Each figure is the median of ``--reps`` windows of ``--iters`` calls (device events); the min-max
spread of the windows is printed beside it. On a build without the clipping kernels (the parent
commit) only the unscaled apply is timed, so the same tool gives the baseline.

  python tools/clip_bench.py [--json out.json]
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402
from parameter_server_distributed_amd.ops.optim import OptimConfig, OptimDyn  # noqa: E402

SIZES = {"resnet50": 25_557_032, "bert_base": 110_104_890}  # parameters of the two shipped recipes


def _round(n, a=64):
    return (n + a - 1) // a * a


def window_us(fn, iters):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(iters):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters * 1e3


def timed(fns: dict, iters: int, reps: int) -> dict:
    """{name: (median us, min, max)}; the candidates alternate window by window."""
    for fn in fns.values():  # warm-up: code objects, allocator
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            t[k].append(window_us(fn, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("clip_bench needs the GPU: a CPU timing says nothing about these kernels")
    C = native()
    dev = torch.device("cuda", 0)
    has_clip = hasattr(C, "grad_clip_coef_")
    res = {"device": torch.cuda.get_device_name(0), "has_clip": has_clip, "iters": a.iters, "reps": a.reps,
           "norm": [], "apply": []}

    if has_clip:
        from parameter_server_distributed_amd.ops.optim import clip_chunks, grad_clip_coef_

        print("| buffer | dtype | MB | grad_clip_coef_ us (min-max) | TB/s | vector_norm us (min-max) | TB/s | ratio |")
        print("|---|---|---:|---:|---:|---:|---:|---:|")
        for name, n in SIZES.items():
            n = _round(n)
            for dt in (torch.bfloat16, torch.float32):
                g = (torch.randn(n, device=dev) * 0.05).to(dt)
                out = torch.zeros(64, device=dev)
                part = torch.zeros(clip_chunks(n), device=dev)
                r = timed({"ours": lambda: grad_clip_coef_(g, 1.0, out, part),
                           "torch": lambda: torch.linalg.vector_norm(g, dtype=torch.float32)}, a.iters, a.reps)
                got, want = float(out[1]), float(torch.linalg.vector_norm(g.double()))
                assert abs(got - want) <= 12 * 2.0 ** -23 * want, (got, want)
                nb = n * g.element_size()
                (mo, lo, ho), (mt, lt, ht) = r["ours"], r["torch"]
                print(f"| {name} | {str(dt).split('.')[-1]} | {nb / 2 ** 20:.0f} | {mo:.1f} ({lo:.1f}-{ho:.1f}) | "
                      f"{nb / mo / 1e6:.2f} | {mt:.1f} ({lt:.1f}-{ht:.1f}) | {nb / mt / 1e6:.2f} | {mo / mt:.2f} |",
                      flush=True)
                res["norm"].append({"buffer": name, "dtype": str(dt), "bytes": nb, "ours_us": r["ours"],
                                    "vector_norm_us": r["torch"]})
                del g
    else:
        print("(this build has no grad_clip_coef_: the unscaled apply only)")

    n = _round(SIZES["resnet50"])
    print()
    print("| kind | K | unscaled us (min-max) | TB/s | scaled us (min-max) | TB/s | scaled / unscaled |")
    print("|---|---:|---:|---:|---:|---:|---:|")
    for kind in ("momentum", "adamw"):
        cfg = OptimConfig(kind, lr=1e-3, momentum=0.9, weight_decay=1e-2)
        for K in (1, 4, 16):
            w = torch.randn(n, device=dev)
            s1 = torch.zeros(n, device=dev)
            s2 = torch.zeros(n, device=dev) if cfg.num_states >= 2 else None
            sh = torch.zeros(n, dtype=torch.bfloat16, device=dev)
            gs = [(torch.randn(n, device=dev) * 0.01).to(torch.bfloat16) for _ in range(K)]
            dyn = OptimDyn(dev, lr=cfg.lr, grad_scale=1.0 / K)
            C.optim_advance_(dyn.t, cfg.beta1, cfg.beta2)
            args = (w, gs, s1, s2, sh, dyn.t, cfg.code, cfg.momentum, cfg.dampening, cfg.nesterov, cfg.weight_decay,
                    cfg.beta1, cfg.beta2, cfg.eps, cfg.maximize, 0)
            fns = {"unscaled": lambda: C.fused_apply_(*args)}
            if has_clip:
                sc = [torch.full((1,), 0.5 + 0.03 * k, device=dev) for k in range(K)]
                fns["scaled"] = lambda: C.fused_apply_(*args, sc)
            r = timed(fns, a.iters, a.reps)
            # bytes of one pass: K bf16 sources, master r/w, states r/w, bf16 shadow
            nb = n * (2 * K + 8 + 8 * cfg.num_states + 2)
            mu, lu, hu = r["unscaled"]
            row = f"| {kind} | {K} | {mu:.1f} ({lu:.1f}-{hu:.1f}) | {nb / mu / 1e6:.2f} | "
            if has_clip:
                ms, ls, hs = r["scaled"]
                row += f"{ms:.1f} ({ls:.1f}-{hs:.1f}) | {nb / ms / 1e6:.2f} | {ms / mu:.3f} |"
            else:
                row += "- | - | - |"
            print(row, flush=True)
            res["apply"].append({"kind": kind, "K": K, "bytes": nb, "unscaled_us": r["unscaled"],
                                 "scaled_us": r.get("scaled")})
            del w, s1, s2, sh, gs
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
