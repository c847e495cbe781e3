"""Step time, peak memory and head-kernel times of gpt_small with GPTForLM(fused_head=...) on and off
(profiles/lmhead_xent.md): python tools/lmhead_bench.py [out.json]"""
import json, os, sys, time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from parameter_server_distributed_amd import native
from parameter_server_distributed_amd.models.gpt import GPTForLM, gpt_batch

dev = torch.device("cuda", 0)
out = {}

def step_time(B, S, fused, steps=8, warm=3):
    torch.manual_seed(0)
    m = GPTForLM(max_pos=S, dropout=0.1, fused_head=fused).to(dev).to(torch.bfloat16)
    batch, y = gpt_batch(B, S, m.vocab, dev, seed=1)
    lossf = m.head_loss if fused else m.loss
    def one():
        m.zero_grad(set_to_none=True)
        l = lossf(m(batch), y); l.backward(); return l
    for _ in range(warm): one()
    torch.cuda.synchronize(); torch.cuda.reset_peak_memory_stats(dev)
    t0 = time.perf_counter()
    for _ in range(steps): l = one()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    r = dict(ms=dt * 1e3, peak_gb=torch.cuda.max_memory_allocated(dev) / 2**30, loss=float(l.detach()))
    del m; torch.cuda.empty_cache(); return r

for (B, S) in ((8, 512), (2, 4096)):
    for rep in range(2):
        for fused in (False, True):
            k = f"{B}x{S}_{'fused' if fused else 'logits'}_{rep}"
            out[k] = step_time(B, S, fused); print(k, out[k], flush=True)

C = native()
for M in (4096, 8192):
    K, V = 768, 40512
    g = torch.Generator().manual_seed(0)
    x = torch.randn(M, K, generator=g).bfloat16().to(dev); w = (torch.randn(V, K, generator=g) * 0.02).bfloat16().to(dev)
    b = torch.zeros(V).bfloat16().to(dev); y = torch.randint(0, V, (M,), generator=g).to(dev)
    dz = torch.empty(M, V, dtype=torch.bfloat16, device=dev); sc = torch.ones(1, device=dev)
    logits = torch.empty(M, V, dtype=torch.bfloat16, device=dev)
    def ev(fn, n=10):
        for _ in range(3): fn()
        a, e = torch.cuda.Event(True), torch.cuda.Event(True); a.record()
        for _ in range(n): fn()
        e.record(); torch.cuda.synchronize(); return a.elapsed_time(e) / n
    lr, lse = C.lmhead_xent_fwd(x, w, b, y, 0)
    r = dict(slices=C.lmhead_xent_slices(M, V),
             fwd_ms=ev(lambda: C.lmhead_xent_fwd(x, w, b, y, 0)),
             dz_ms=ev(lambda: C.lmhead_xent_dz_(x, w, b, y, lse, sc, dz)),
             gemm_ms=ev(lambda: C.gemm_(x, w, True, True, logits, b)),
             xent_fwd_ms=ev(lambda: C.xent_fwd(logits, y)))
    r["tflops_fwd"] = 2 * M * K * V / r["fwd_ms"] / 1e9; r["tflops_dz"] = 2 * M * K * V / r["dz_ms"] / 1e9
    out[f"head_M{M}"] = r; print(f"head_M{M}", r, flush=True)
if len(sys.argv) > 1:
    json.dump(out, open(sys.argv[1], "w"), indent=1)
