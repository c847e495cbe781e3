#!/usr/bin/env python3
"""Time the rotary position embedding kernel (csrc/kernels/rope.hip, native ``rope_``): the forward and the
inverse (backward) pass over a packed qkv of 16,384 tokens with 12 heads of 64 at S = 1024, 2048 and 4096,
on plain rows, packed documents and padded rows. us per call and achieved bytes per second.

  python tools/rope_bench.py                 # the three shapes, three cases each
  python tools/rope_bench.py --ref           # also the torch composite rope_ref on the same buffers
  python tools/rope_bench.py --seq 2048      # one shape

The bytes counted are what the pass has to move: the Q and K thirds of qkv read and written once, 2/3 + 2/3
of the tensor (padded rows: of its valid rows; the tables, lens and doc_start are not counted). --docs MEAN
sets the mean document length (documents uniform in [MEAN/2, 3 MEAN/2], seeded), --min-len the shortest
padded row as a fraction of S. The kernel rotates its buffer in place call after call (a rotation keeps
the magnitudes); the composite is out of place, so its column also pays for the copy of V it returns.

Every figure comes from --repeats timed windows of --iters calls between two device events; with --ref the
two paths alternate inside a window. Printed: median (min - max) us and the rate at the median."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402
from parameter_server_distributed_amd.ops.attention import doc_starts  # noqa: E402
from parameter_server_distributed_amd.ops.rope import rope_ref, rope_tables  # noqa: E402

TOKENS, H, D = 16384, 12, 64


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


def _packed(B, S, mean, dev):
    g = torch.Generator(device="cpu").manual_seed(0)
    rows = []
    for _ in range(B):
        row, t = [], 0
        while t < S:
            n = min(int(torch.randint(mean // 2, mean * 3 // 2 + 1, (1,), generator=g)), S - t)
            row.append(n)
            t += n
        rows.append(row)
    return doc_starts(rows, S, dev), sum(len(r) for r in rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seq", type=int, default=None, help="one sequence length S (default: 1024, 2048 and 4096)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per window")
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per figure")
    ap.add_argument("--docs", type=int, default=256, help="mean document length of the packed case")
    ap.add_argument("--min-len", type=float, default=0.5, help="shortest padded row, as a fraction of S")
    ap.add_argument("--ref", action="store_true", help="also time the torch composite rope_ref on the same buffers")
    args = ap.parse_args()
    if args.seq is not None and (args.seq < 1 or TOKENS % args.seq):
        ap.error(f"--seq must divide {TOKENS}")
    if not torch.cuda.is_available():
        sys.exit("rope_bench: no GPU visible; timings are taken on the device only")
    C = native()
    dev = torch.device("cuda")
    seqs = [args.seq] if args.seq else [1024, 2048, 4096]
    head = "| S | B | case | dir | kernel us | kernel TB/s |"
    if args.ref:
        head += " composite us | composite TB/s | composite / kernel |"
    print(f"{TOKENS} tokens, H {H}, D {D}; {args.repeats} windows of {args.iters} calls: median (min - max)")
    print(head)
    print("|" + "---:|" * (head.count("|") - 1))
    for S in seqs:
        B = TOKENS // S
        qkv = (torch.randn(B, S, 3 * H * D, device=dev) * 0.5).to(torch.bfloat16)
        cos, sin = rope_tables(S, device=dev)
        doc, ndoc = _packed(B, S, args.docs, dev)
        g = torch.Generator(device="cpu").manual_seed(0)
        lc = torch.randint(int(S * args.min_len), S + 1, (B,), generator=g)
        lens = lc.to(torch.int32).to(dev)
        row_bytes = 2 * H * D * 2 * 2  # Q and K of one row, read and written
        cases = (("plain", None, None, B * S), (f"docs ({B * S / ndoc:.0f} mean)", None, doc, B * S),
                 (f"padded ({int(lc.sum())} of {B * S} rows)", lens, None, int(lc.sum())))
        for name, ln, dc, rows in cases:
            for inverse in (False, True):
                tk, tr = [], []
                for _ in range(args.repeats):  # the paths alternate inside a window
                    tk.append(t_us(lambda: C.rope_(qkv, H, cos, sin, ln, dc, inverse, 0), args.iters))
                    if args.ref:
                        tr.append(t_us(lambda: rope_ref(qkv, H, cos, sin, ln, dc, inverse), max(1, args.iters // 10)))
                mk = statistics.median(tk)
                row = (f"| {S} | {B} | {name} | {'inverse' if inverse else 'forward'} | {_fmt(tk)} | "
                       f"{rows * row_bytes / mk / 1e6:.2f} |")
                if args.ref:
                    mr = statistics.median(tr)
                    row += (f" {_fmt(tr)} | {rows * row_bytes / mr / 1e6:.2f} | {mr / mk:.1f}x "
                            f"(min / max {min(tr) / max(tk):.1f}x) |")
                print(row, flush=True)
        assert bool(torch.isfinite(qkv.float()).all())


if __name__ == "__main__":
    main()
