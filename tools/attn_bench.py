#!/usr/bin/env python3
"""Time the fused attention kernels (csrc/kernels/attention.hip, attention_long.hip) with and without
attention dropout: us per call, the compulsory HBM bytes over that time, and the MFMA rate. The
default shape is BERT-base pre-training (B 256, S 128, 12 heads of 64).

  python tools/attn_bench.py
  python tools/attn_bench.py --min-len 16   # padded batch: lengths uniform in [16, S], passed as lens
  python tools/attn_bench.py --seq 512 --batch 64 --sdpa   # the streaming kernels against the SDPA path
  python tools/attn_bench.py --seq 512 --batch 64 --causal # the causal instantiations (keys <= q)
  python tools/attn_bench.py --seq 512 --batch 64 --docs 128 --sdpa  # packed documents of mean length 128
  python tools/attn_bench.py --seq 2048 --batch 8 --causal --window 256 --sdpa  # sliding window of 256 keys

With --min-len the bytes count the valid rows only (what the variable-length kernels have to move)
and the FLOP rate counts the valid (query, key) pairs. With --causal the FLOP rate counts the visible
pairs (key <= q, and both < the length); the bytes are unchanged. --docs MEAN (causal only) packs every
row with documents of length uniform in [MEAN/2, 3 MEAN/2] (seeded) and passes doc_start: the document
copies of the kernels, and with --sdpa the SDPA path with the same boolean mask; the FLOP rate counts
the visible pairs (same document, key <= q). --window W (causal only, with or without --docs / --min-len)
passes window=W: the window copies of the streaming kernels (S >= 192), and with --sdpa the SDPA path with
the band AND-ed into its boolean mask; the FLOP rate counts the visible pairs, q - max(doc, q - W + 1, 0) + 1
per valid query.

--sdpa also times the module's SDPA path (F.scaled_dot_product_attention on transposed views, through
autograd, with its layout copies and, with lengths, its mask) on the same data as a second pair of
columns; both paths are then timed alternately in --windows windows and every figure is the median
(min - max) over the windows. TB/s and TF/s are from the kernel path's median.
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from parameter_server_distributed_amd import native  # noqa: E402


def t_us(fn, it=20):
    fn()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / it * 1e3


def _fmt(ts):
    if len(ts) == 1:
        return f"{ts[0]:.1f}"
    return f"{statistics.median(ts):.1f} ({min(ts):.1f} - {max(ts):.1f})"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-len", type=int, default=None, help="draw lengths uniformly in [N, S] and pass them as lens")
    ap.add_argument("--iters", type=int, default=20, help="timed calls per figure")
    ap.add_argument("--seq", type=int, default=128, help="sequence length S")
    ap.add_argument("--batch", type=int, default=256, help="batch size B")
    ap.add_argument("--sdpa", action="store_true", help="also time the module's SDPA path on the same data")
    ap.add_argument("--causal", action="store_true", help="causal mask (keys <= q), on both paths")
    ap.add_argument("--docs", type=int, default=None,
                    help="pack rows with documents of this mean length and pass doc_start (needs --causal)")
    ap.add_argument("--window", type=int, default=None,
                    help="sliding window: query q sees the W keys up to and including q (needs --causal)")
    ap.add_argument("--windows", type=int, default=None, help="timing windows per figure (default 1, with --sdpa 5)")
    args = ap.parse_args()
    C = native()
    dev = torch.device("cuda")
    B, S, H, D = args.batch, args.seq, 12, 64
    nwin = args.windows if args.windows is not None else (5 if args.sdpa else 1)
    qkv = (torch.randn(B, S, 3 * H * D, device=dev) * 0.5).to(torch.bfloat16)
    do = torch.randn(B, S, H * D, device=dev).to(torch.bfloat16)
    step = torch.tensor([3], device=dev, dtype=torch.int64)
    el = B * S * H * D * 2  # bytes of one [B, S, H, 64] bf16 tensor
    causal = args.causal
    flop_f = 4 * B * H * D * (S * (S + 1) // 2 if causal else S * S)
    lens = None
    if args.min_len is not None:
        if not 0 <= args.min_len <= S:
            ap.error(f"--min-len must be in [0, {S}]")
        g = torch.Generator(device="cpu").manual_seed(0)
        lc = torch.randint(args.min_len, S + 1, (B,), generator=g)
        lens = lc.to(torch.int32).to(dev)
        el = int(lc.sum()) * H * D * 2  # the valid rows only
        flop_f = 4 * H * D * int((lc * (lc + 1) // 2 if causal else lc * lc).sum())
        print(f"lens uniform in [{args.min_len}, {S}]: mean {lc.float().mean():.1f}, valid rows {int(lc.sum())} of {B * S}")
    # (doc_start,) with --docs, (doc_start or None, W) with --window: the last arguments of attn_fwd /
    # attn_bwd and of _sdpa
    extra = ()
    if args.docs is not None:
        if not causal or args.docs < 2 or args.min_len is not None:
            ap.error("--docs MEAN needs --causal, MEAN >= 2 and no --min-len")
        from parameter_server_distributed_amd.ops.attention import doc_starts

        g = torch.Generator(device="cpu").manual_seed(0)
        rows = []
        for _ in range(B):
            row, t = [], 0
            while t < S:
                n = min(int(torch.randint(args.docs // 2, args.docs * 3 // 2 + 1, (1,), generator=g)), S - t)
                row.append(n)
                t += n
            rows.append(row)
        extra = (doc_starts(rows, S, dev),)
        ndoc = sum(len(r) for r in rows)
        flop_f = 4 * H * D * sum(n * (n + 1) // 2 for r in rows for n in r)
        print(f"documents uniform in [{args.docs // 2}, {args.docs * 3 // 2}]: {ndoc / B:.1f} per row, "
              f"mean length {B * S / ndoc:.1f}")
    if args.window is not None:
        if not causal or args.window < 1:
            ap.error("--window W needs --causal and W >= 1")
        idx = torch.arange(S)
        lb = extra[0].cpu().long() if extra else torch.zeros(B, S, dtype=torch.long)
        lb = torch.maximum(lb, (idx - args.window + 1).clamp(min=0)[None, :])
        vq = idx[None, :] < (lc[:, None] if lens is not None else S)
        flop_f = 4 * H * D * int(((idx[None, :] - lb + 1) * vq).sum())
        extra = (extra[0] if extra else None, args.window)
        print(f"window {args.window}: {flop_f / (4 * H * D) / (B * S):.1f} visible keys per query")
    it = args.iters
    print(f"B {B}, S {S}, H {H}, D {D}{', causal' if causal else ''}; {nwin} window(s) of {it} calls")
    head = "| p | fwd us | fwd TB/s | fwd TF/s | bwd us | bwd TB/s | bwd TF/s |"
    if args.sdpa:
        from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

        mod = FusedSelfAttention(H, causal=causal).to(dev)
        xg = qkv.clone().requires_grad_(True)
        head += " sdpa fwd us | sdpa bwd us | fwd+bwd us | sdpa fwd+bwd us |"
    print(head)
    print("|" + "---:|" * (head.count("|") - 1))
    for p in (0.0, 0.1):
        o, lse = C.attn_fwd(qkv, H, p, 7, step, lens, 0, causal, *extra)
        tf, tb, sf, sb = [], [], [], []
        for _ in range(nwin):  # the paths alternate inside a window
            tf.append(t_us(lambda: C.attn_fwd(qkv, H, p, 7, step, lens, 0, causal, *extra), it))
            if args.sdpa:
                sf.append(t_us(lambda: mod._sdpa(xg, lens, p, *extra), it))
            tb.append(t_us(lambda: C.attn_bwd(do, qkv, o, lse, H, p, 7, step, None, lens, 0, causal, *extra), it))
            if args.sdpa:
                so = mod._sdpa(xg, lens, p, *extra)
                sb.append(t_us(lambda: torch.autograd.grad(so, xg, do, retain_graph=True), it))
                del so
        mf, mb = statistics.median(tf), statistics.median(tb)
        # fwd: read q, k, v; write o (+ lse). bwd: read q, k, v, o, dO; write dq, dk, dv
        row = (f"| {p} | {_fmt(tf)} | {4 * el / mf / 1e6:.2f} | {flop_f / mf / 1e6:.0f} | {_fmt(tb)} | "
               f"{8 * el / mb / 1e6:.2f} | {2.5 * flop_f / mb / 1e6:.0f} |")
        if args.sdpa:
            row += (f" {_fmt(sf)} | {_fmt(sb)} | {_fmt([a + b for a, b in zip(tf, tb)])} | "
                    f"{_fmt([a + b for a, b in zip(sf, sb)])} |")
        print(row, flush=True)


if __name__ == "__main__":
    main()
