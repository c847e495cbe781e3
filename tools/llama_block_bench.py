#!/usr/bin/env python3
"""Time the four kernels of the Llama-style block (csrc/kernels/rmsnorm.hip, swiglu.hip): the fused residual
add + dropout + RMSNorm forward and backward at p = 0 and 0.1, and the gated SiLU forward and backward, at
T = 16,384 tokens, H = 768, F = 2048. us per call, bytes moved and achieved GB/s.

  python tools/llama_block_bench.py            # the four kernels
  python tools/llama_block_bench.py --ref      # also the torch composites add_rmsnorm_ref / swiglu_ref

The bytes counted are what each pass has to move (bf16 tensors read or written once; the fp32 rstd, gamma and
the dgamma partials are not counted):
  rms_fwd      r, h read; r_new, y written                          4 T H * 2
  rms_bwd      dy, dr_new, r_new read; dr written (p = 0: dh is dr)  4 T H * 2, with dropout + dh: 5 T H * 2
  swiglu_fwd   gu [T, 2F] read; a [T, F] written                    3 T F * 2
  swiglu_bwd   da, gu read; dgu [T, 2F] written                     5 T F * 2
The composites' columns are charged the same bytes, so their GB/s is the rate at which they do the same job
(they move more: every intermediate goes through memory). A composite backward is the autograd backward of
its forward, whose graph is built once outside the timed window.

Every figure comes from --repeats timed windows of --iters calls between two device events; with --ref the
two paths alternate inside a window. Printed: median (min - max) us and the rate at the median."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402
from parameter_server_distributed_amd.ops.rmsnorm import add_rmsnorm_ref  # noqa: E402
from parameter_server_distributed_amd.ops.swiglu import swiglu_ref  # noqa: E402

TOKENS, H, F = 16384, 768, 2048
EPS, SEED = 1e-6, 7


def t_us(fn, it):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / it * 1e3


def _fmt(ts):
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} - {max(ts):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=TOKENS, help="rows T")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per window")
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per figure")
    ap.add_argument("--ref", action="store_true", help="also time the torch composites on the same buffers")
    args = ap.parse_args()
    if args.tokens < 1:
        ap.error("--tokens must be >= 1")
    if not torch.cuda.is_available():
        sys.exit("llama_block_bench: no GPU visible; timings are taken on the device only")
    C = native()
    dev = torch.device("cuda")
    T = args.tokens
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)

    r, h, dy, drn = rnd(T, H), rnd(T, H), rnd(T, H), rnd(T, H)
    gamma = (torch.rand(H, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    gu, da = rnd(T, 2 * F), rnd(T, F)
    step = torch.tensor([3], device=dev, dtype=torch.int64)
    cases = []  # (name, bytes, kernel call, composite call or None)
    for p in (0.0, 0.1):
        r_new, _, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)
        ref_f = ref_b = None
        if args.ref:
            rl, hl, gl = (t.clone().requires_grad_(True) for t in (r, h, gamma))
            torch.manual_seed(0)
            out = add_rmsnorm_ref(rl, hl, gl, EPS, p, True)
            ref_f = (lambda p=p: add_rmsnorm_ref(r, h, gamma, EPS, p, True))
            ref_b = (lambda out=out, ins=(rl, hl, gl): torch.autograd.grad(out, ins, (drn, dy), retain_graph=True))
        cases.append((f"rms_fwd p={p}", 4 * T * H * 2,
                      (lambda p=p: C.rms_fwd(r, h, gamma, EPS, p, SEED, step)), ref_f))
        cases.append((f"rms_bwd p={p}", (5 if p > 0 else 4) * T * H * 2,
                      (lambda p=p, rn=r_new, rs=rstd: C.rms_bwd(dy, drn, rn, rs, gamma, p, SEED, step, True)), ref_b))
    ref_f = ref_b = None
    if args.ref:
        gl = gu.clone().requires_grad_(True)
        out = swiglu_ref(gl)
        ref_f = (lambda: swiglu_ref(gu))
        ref_b = (lambda: torch.autograd.grad(out, gl, da, retain_graph=True))
    cases.append(("swiglu_fwd", 3 * T * F * 2, (lambda: C.swiglu_fwd(gu, 0)), ref_f))
    cases.append(("swiglu_bwd", 5 * T * F * 2, (lambda: C.swiglu_bwd(da, gu, 0)), ref_b))

    head = "| kernel | MB moved | kernel us | kernel GB/s |"
    if args.ref:
        head += " composite us | composite GB/s | composite / kernel |"
    print(f"T {T} tokens, H {H}, F {F}; {args.repeats} windows of {args.iters} calls: median (min - max)")
    print(head)
    print("|" + "---:|" * (head.count("|") - 1))
    for name, nbytes, kern, ref in cases:
        tk, tr = [], []
        for _ in range(args.repeats):  # the paths alternate inside a window
            tk.append(t_us(kern, args.iters))
            if ref is not None:
                tr.append(t_us(ref, max(1, args.iters // 10)))
        mk = statistics.median(tk)
        row = f"| {name} | {nbytes / 1e6:.1f} | {_fmt(tk)} | {nbytes / mk / 1e3:.0f} |"
        if ref is not None:
            mr = statistics.median(tr)
            row += f" {_fmt(tr)} | {nbytes / mr / 1e3:.0f} | {mr / mk:.1f}x (min / max {min(tr) / max(tk):.1f}x) |"
        print(row, flush=True)


if __name__ == "__main__":
    main()
