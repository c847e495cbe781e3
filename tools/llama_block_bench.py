#!/usr/bin/env python3
"""Time the four kernels of the Llama-style block (csrc/kernels/rmsnorm.hip, swiglu.hip): the fused residual
add + dropout + RMSNorm forward and backward at p = 0 and 0.1, and the gated SiLU forward and backward, at
T = 16,384 tokens, H = 768, F = 2048 (--tokens, --hidden, --ffn; a hidden size of 512 n from 1536 to 8192 times
the wide kernels of rmsnorm_wide.hip). us per call, bytes moved and achieved GB/s.

  python tools/llama_block_bench.py            # the four kernels
  python tools/llama_block_bench.py --ref      # also the torch composites add_rmsnorm_ref / swiglu_ref
  python tools/llama_block_bench.py --mx       # the MX side-output variants against plain + quantize_mx
  python tools/llama_block_bench.py --layer    # one layer forward + backward: fp8 hand-overs on / off, bf16

The bytes counted are what each pass has to move (bf16 tensors read or written once; the fp32 rstd, gamma and
the dgamma partials are not counted):
  rms_fwd      r, h read; r_new, y written                          4 T H * 2
  rms_bwd      dy, dr_new, r_new read; dr written (p = 0: dh is dr)  4 T H * 2, with dropout + dh: 5 T H * 2
  swiglu_fwd   gu [T, 2F] read; a [T, F] written                    3 T F * 2
  swiglu_bwd   da, gu read; dgu [T, 2F] written                     5 T F * 2
The composites' columns are charged the same bytes, so their GB/s is the rate at which they do the same job
(they move more: every intermediate goes through memory). A composite backward is the autograd backward of
its forward, whose graph is built once outside the timed window.

--mx: each variant that also writes the MX fp8 copy of its output (q8 + E8M0 scales: 33/32 bytes per element on
top of the plain pass) against what it replaces, the plain kernel followed by the stand-alone quantize_mx pass
over the stored bf16 output (2 bytes per element read again, 33/32 written); the three alternate inside a window.
--layer: forward + backward of one LlamaLayer plus the norm that closes it (it takes the layer's branch, so the
down Linear's backward hand-over is in the figure), T tokens as [T / 512, 512], dropout 0.1, rope: the fp8 layer
with feature fp8_llama_handover on and off and the bf16 layer, alternating inside a window, ms per step.

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


def mx_cases(C, T, r, h, dy, drn, gamma, gu, da, step):
    """(name, plain bytes, MX copy elements, plain call -> the tensor that is quantised, e5m2, fused call)."""
    p = 0.1
    r_new, _, rstd = C.rms_fwd(r, h, gamma, EPS, p, SEED, step)

    def out8(n, cols, e5m2):
        return (torch.empty(n, cols, device=r.device, dtype=torch.float8_e5m2 if e5m2 else torch.float8_e4m3fn),
                torch.empty(n * cols // 32, device=r.device, dtype=torch.uint8))

    qy, qdh, qa, qdgu = out8(T, H, False), out8(T, H, True), out8(T, F, False), out8(T, 2 * F, True)
    return [
        ("rms_fwd p=0.1 + e4m3(y)", 4 * T * H * 2, T * H, lambda: C.rms_fwd(r, h, gamma, EPS, p, SEED, step)[1], False,
         lambda: C.rms_fwd(r, h, gamma, EPS, p, SEED, step, *qy)),
        ("rms_bwd p=0.1 + e5m2(dh)", 5 * T * H * 2, T * H,
         lambda: C.rms_bwd(dy, drn, r_new, rstd, gamma, p, SEED, step, True)[1], True,
         lambda: C.rms_bwd(dy, drn, r_new, rstd, gamma, p, SEED, step, True, None, *qdh)),
        ("swiglu_fwd + e4m3(a)", 3 * T * F * 2, T * F, lambda: C.swiglu_fwd(gu, 0), False,
         lambda: C.swiglu_fwd(gu, 0, *qa)),
        ("swiglu_bwd + e5m2(dgu)", 5 * T * F * 2, 2 * T * F, lambda: C.swiglu_bwd(da, gu, 0), True,
         lambda: C.swiglu_bwd(da, gu, 0, *qdgu)),
    ]


def bench_mx(C, args, tensors):
    from parameter_server_distributed_amd.ops import quantize_mx

    print("| variant | plain MB | plain us | plain + quantize_mx MB | plain + quantize_mx us | fused MB | fused us "
          "| fused / (plain + quantize_mx) |")
    print("|" + "---:|" * 8)
    for name, nbytes, nq, plain, e5m2, fused in mx_cases(C, args.tokens, *tensors):
        two = (lambda: quantize_mx(plain(), e5m2))
        tp, t2, tf = [], [], []
        for _ in range(args.repeats):
            tp.append(t_us(plain, args.iters))
            t2.append(t_us(two, args.iters))
            tf.append(t_us(fused, args.iters))
        copy = nq * 33 / 32
        ratio = statistics.median(tf) / statistics.median(t2)
        print(f"| {name} | {nbytes / 1e6:.1f} | {_fmt(tp)} | {(nbytes + 2 * nq + copy) / 1e6:.1f} | {_fmt(t2)} | "
              f"{(nbytes + copy) / 1e6:.1f} | {_fmt(tf)} | {ratio:.3f} |", flush=True)


def bench_layer(args, dev):
    from parameter_server_distributed_amd.models.llama_block import LlamaLayer
    from parameter_server_distributed_amd.ops.rmsnorm import FusedAddRMSNorm

    S = 512
    if args.tokens % S:
        sys.exit("llama_block_bench --layer: --tokens must be a multiple of 512")
    B = args.tokens // S
    g = torch.Generator(device=dev).manual_seed(1)
    r0 = torch.randn(B, S, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    h0 = torch.randn(B, S, H, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    dr, dy = (torch.randn(B, S, H, device=dev, generator=g).to(torch.bfloat16) for _ in range(2))
    step = torch.tensor([3], device=dev, dtype=torch.int64)

    def make(fp8):
        torch.manual_seed(0)
        layer = LlamaLayer(H, H // 64, F, 0.1, 0, rope=(S, 10000.0), fp8=fp8).to(dev).to(torch.bfloat16).train()
        close = FusedAddRMSNorm(H, p=0.1, seed=3).to(dev).to(torch.bfloat16).train()
        if fp8:
            close.psd_mx_grad_to(layer.down)
        for m in (layer.norm1, layer.norm2, close):
            m.step = step
        params = [r0, h0] + list(layer.parameters()) + list(close.parameters())

        def run():
            r, h = layer(r0, h0)
            torch.autograd.grad(close(r, h), params, (dr, dy))

        return run

    runs = [("fp8, fp8_llama_handover on", make("mx"), ""), ("fp8, fp8_llama_handover off", make("mx"),
                                                             "fp8_llama_handover=0"), ("bf16", make(False), "")]
    env0 = os.environ.get("PSD_FEATURES", "")
    ts = {name: [] for name, _, _ in runs}
    for _ in range(args.repeats):
        for name, run, feat in runs:
            os.environ["PSD_FEATURES"] = ",".join(filter(None, (env0, feat)))
            ts[name].append(t_us(run, args.layer_iters) / 1e3)
    os.environ["PSD_FEATURES"] = env0
    print(f"one LlamaLayer + closing norm, forward + backward, [{B}, {S}, {H}], F {F}: ms, median (min - max)")
    print("| layer | ms |")
    print("|---|---:|")
    for name, _, _ in runs:
        v = ts[name]
        print(f"| {name} | {statistics.median(v):.3f} ({min(v):.3f} - {max(v):.3f}) |", flush=True)


def main():
    global H, F
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", type=int, default=TOKENS, help="rows T")
    ap.add_argument("--hidden", type=int, default=H, help="hidden size H of the RMSNorm cases (and of --layer)")
    ap.add_argument("--ffn", type=int, default=F, help="FFN size F of the SwiGLU cases (and of --layer)")
    ap.add_argument("--iters", type=int, default=200, help="timed calls per window")
    ap.add_argument("--repeats", type=int, default=10, help="timed windows per figure")
    ap.add_argument("--ref", action="store_true", help="also time the torch composites on the same buffers")
    ap.add_argument("--mx", action="store_true", help="time the MX side-output variants against plain + quantize_mx")
    ap.add_argument("--layer", action="store_true", help="time one layer: fp8 hand-overs on / off and bf16")
    ap.add_argument("--layer-iters", type=int, default=20, help="timed steps per window of --layer")
    args = ap.parse_args()
    if args.tokens < 1:
        ap.error("--tokens must be >= 1")
    if args.hidden % 64 or args.hidden < 64 or args.ffn % 32 or args.ffn < 32:
        ap.error("--hidden must be a multiple of 64 and --ffn a multiple of 32")
    H, F = args.hidden, args.ffn
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
    if args.mx or args.layer:
        print(f"T {T} tokens, H {H}, F {F}; {args.repeats} windows: median (min - max)")
        if args.mx:
            bench_mx(C, args, (r, h, dy, drn, gamma, gu, da, step))
        if args.layer:
            bench_layer(args, dev)
        return
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
