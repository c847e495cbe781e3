#!/usr/bin/env python3
"""Time the fused residual add + dropout + LayerNorm kernels (csrc/kernels/layernorm.hip at H = 768 / 1024,
layernorm_wide.hip at H = 256 n from 1280 to 8192): forward and backward (the gamma / beta / dhsum finalize
included) at p = 0 and 0.1. us per call, bytes moved and achieved GB/s. The default shape is BERT-base b256 x S128
(32,768 rows of 768, profiles/r6/ln_bench.md); profiles/layernorm_wide.md uses --tokens 16384.

  python tools/ln_bench.py                                        # the four launches at 32,768 x 768
  python tools/ln_bench.py --tokens 16384 --hidden 4096 --ref     # also the torch composite on the same buffers
  python tools/ln_bench.py --tokens 16384 --hidden 4096 --mx      # forward + MX e4m3 copy of y against plain + quantize_mx

The bytes counted are what each pass has to move (bf16 tensors read or written once; mean, rstd, gamma, beta and
the fp32 partial rows are not counted):
  ln_fwd   x, h read; s, y written      4 T H * 2
  ln_bwd   dy, s read; dx, dh written   4 T H * 2
The composite's columns are charged the same bytes. Its backward is the autograd backward of
F.layer_norm(x + F.dropout(h)), whose graph is built once outside the timed window.

--mx: the forward that also writes the MX copy (q8 + E8M0 scales: 33/32 bytes per element on top of the plain pass)
against what it replaces, the plain forward followed by the stand-alone quantize_mx pass over the stored y (2 bytes
per element read again, 33/32 written); the three alternate inside a window.

Every figure comes from --repeats timed windows of --iters calls between two device events; with --ref the two
paths alternate inside a window. Printed: median (min - max) us and the rate at the median."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402

EPS, SEED = 1e-12, 7


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


def bench_mx(C, args, x, h, gamma, beta, step):
    from parameter_server_distributed_amd.ops import quantize_mx

    T, H, p = args.tokens, args.hidden, 0.1
    q8 = torch.empty(T, H, device=x.device, dtype=torch.float8_e4m3fn)
    sc8 = torch.empty(T * H // 32, device=x.device, dtype=torch.uint8)
    plain = (lambda: C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)[0])
    two = (lambda: quantize_mx(plain()))
    fused = (lambda: C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step, q8, sc8))
    tp, t2, tf = [], [], []
    for _ in range(args.repeats):
        tp.append(t_us(plain, args.iters))
        t2.append(t_us(two, args.iters))
        tf.append(t_us(fused, args.iters))
    nbytes, nq = 4 * T * H * 2, T * H
    copy = nq * 33 / 32
    print("| variant | plain MB | plain us | plain + quantize_mx MB | plain + quantize_mx us | fused MB | fused us "
          "| fused / (plain + quantize_mx) |")
    print("|" + "---:|" * 8)
    print(f"| ln_fwd p=0.1 + e4m3(y) | {nbytes / 1e6:.1f} | {_fmt(tp)} | {(nbytes + 2 * nq + copy) / 1e6:.1f} | {_fmt(t2)} | "
          f"{(nbytes + copy) / 1e6:.1f} | {_fmt(tf)} | {statistics.median(tf) / statistics.median(t2):.3f} |", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=32768, help="rows T")
    ap.add_argument("--hidden", type=int, default=768, help="hidden size H")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per window")
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per figure")
    ap.add_argument("--ref", action="store_true", help="also time the torch composite on the same buffers")
    ap.add_argument("--mx", action="store_true", help="time the MX side-output forward against plain + quantize_mx")
    args = ap.parse_args()
    if args.tokens < 1:
        ap.error("--tokens must be >= 1")
    if not torch.cuda.is_available():
        sys.exit("ln_bench: no GPU visible; timings are taken on the device only")
    C = native()
    dev = torch.device("cuda")
    T, H = args.tokens, args.hidden
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*shape):
        return torch.randn(*shape, device=dev, generator=g).to(torch.bfloat16)

    x, h, dy = rnd(T, H), rnd(T, H), rnd(T, H)
    gamma = (torch.rand(H, device=dev, generator=g) + 0.5).to(torch.bfloat16)
    beta = (torch.rand(H, device=dev, generator=g) - 0.5).to(torch.bfloat16)
    dhsum = torch.empty_like(gamma)
    step = torch.tensor([3], device=dev, dtype=torch.int64)
    print(f"T {T} tokens, H {H}; {args.repeats} windows of {args.iters} calls: median (min - max)")
    if args.mx:
        bench_mx(C, args, x, h, gamma, beta, step)
        return
    cases = []  # (name, kernel call, composite call or None)
    for p in (0.0, 0.1):
        _, s, mean, rstd = C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)
        ref_f = ref_b = None
        if args.ref:
            ins = [t.clone().requires_grad_(True) for t in (x, h, gamma, beta)]
            comp = (lambda a, b, w, c, p=p: F.layer_norm(a + F.dropout(b, p, True), (H,), w, c, EPS))
            out = comp(*ins)
            ref_f = (lambda comp=comp: comp(x, h, gamma, beta))
            ref_b = (lambda out=out, ins=ins: torch.autograd.grad(out, ins, dy, retain_graph=True))
        cases.append((f"ln_fwd p={p}", (lambda p=p: C.ln_fwd(x, h, gamma, beta, EPS, p, SEED, step)), ref_f))
        cases.append((f"ln_bwd p={p}", (lambda p=p, s=s, m=mean, r=rstd: C.ln_bwd(dy, s, m, r, gamma, p, SEED, step, None,
                                                                                 None, dhsum)), ref_b))
    nbytes = 4 * T * H * 2
    head = "| kernel | MB moved | kernel us | kernel GB/s |"
    if args.ref:
        head += " composite us | composite GB/s | composite / kernel |"
    print(head)
    print("|" + "---:|" * (head.count("|") - 1))
    for name, kern, ref in cases:
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
