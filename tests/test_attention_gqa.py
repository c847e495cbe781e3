"""Grouped-query attention on the GQA copies of the streaming kernels: B = 2, H = 4 query heads, Hkv = 2 / 1, S = 192
(a 64-row last tile, an even chunk count) and 320 (an odd one). o, lse and dQ must be bitwise the multi-head
kernels' on the tensor with every K/V head repeated G times (tests/test_attention_fp64.py pins those). dK, dV are
held per element in fp64, staged from the kernel's own o and lse as check_random does there: the reference is the
sum over the group of that file's dk_ref / dv_ref, the bound the sum over the group of the per-head operand terms,
scale * sum_g (W_g^T |Q_g|) and (U + E) * sum_g (Pb_g^T |dO_g|), plus ONE output rounding U |ref| (the accumulators
stay fp32 across the group). None of it is measured from a kernel; the ATTNERR lines are in profiles/attn_gqa.md."""
import pytest
import torch

from test_attention_fp64 import E, U, _Err, _heads, _split, _visible

B, H = 2, 4
MASKS = ("causal", "causal+lens", "window", "window+docs+lens")
_CACHE = {}


def _expand(x, hkv):
    """[B, S, (H + 2 hkv) * 64] -> [B, S, 3 * H * 64], each K/V head repeated for its group's query heads"""
    q, k, v = x.split((H * 64, hkv * 64, hkv * 64), -1)
    k, v = (t.reshape(*t.shape[:2], hkv, 64).repeat_interleave(H // hkv, dim=2).flatten(2) for t in (k, v))
    return torch.cat([q, k, v], -1).contiguous()


def _case(C, dev, S, hkv, mask, p, grid_cap=0):
    """(inputs, GQA (o, lse, dqkv), multi-head (o, lse, dqkv) on the expanded tensor), computed once per case"""
    key = (S, hkv, mask, p, grid_cap)
    if key not in _CACHE:
        from parameter_server_distributed_amd.ops.attention import doc_starts

        g = torch.Generator(device="cpu").manual_seed(S + hkv)
        x = (torch.randn(B, S, (H + 2 * hkv) * 64, generator=g) * 1.5).to(torch.bfloat16).to(dev)
        do = torch.randn(B, S, H * 64, generator=g).to(torch.bfloat16).to(dev)
        lens = torch.tensor([S - 31, 65], dtype=torch.int32, device=dev) if "lens" in mask else None
        doc = doc_starts([[97, 63, S - 160], [31, 33, 1, 64, S - 129]], S, dev) if "docs" in mask else None
        win = (65,) if "window" in mask else ()
        step = torch.tensor([3], device=dev, dtype=torch.int64)
        xe = _expand(x, hkv)
        o, lse = C.attn_fwd(x, H, p, 11, step, lens, grid_cap, True, doc, *win, kv_heads=hkv)
        dqkv = C.attn_bwd(do, x, o, lse, H, p, 11, step, None, lens, grid_cap, True, doc, *win, kv_heads=hkv)
        oe, lsee = C.attn_fwd(xe, H, p, 11, step, lens, 0, True, doc, *win)
        dqkve = C.attn_bwd(do, xe, oe, lsee, H, p, 11, step, None, lens, 0, True, doc, *win)
        _CACHE[key] = ((xe, do, lens, doc, win[0] if win else None), (o, lse, dqkv), (oe, lsee, dqkve))
    return _CACHE[key]


def _bits(t):
    return t.view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("S", [192, 320])
def test_forward_and_dq_are_the_multi_head_kernels_bitwise(gpu, C, S, hkv, mask, p):
    _, (o, lse, dqkv), (oe, lsee, dqkve) = _case(C, gpu, S, hkv, mask, p)
    assert dqkv.shape == (B, S, (H + 2 * hkv) * 64)
    for name, a, b in (("o", o, oe), ("lse", lse, lsee), ("dq", dqkv[..., :H * 64], dqkve[..., :H * 64])):
        assert torch.equal(_bits(a), _bits(b)), name


@pytest.mark.gpu
@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("hkv", [2, 1])
@pytest.mark.parametrize("S", [192, 320])
def test_dk_dv_per_element_fp64(gpu, C, S, hkv, mask):
    (xe, do, lens, doc, W), (o, lse, dqkv), _ = _case(C, gpu, S, hkv, mask, 0.0)
    scale, G = 0.125, H // hkv
    rep = _Err(f"gqa S={S} Hkv={hkv} {mask}")
    vis = _visible(B, S, lens, True, doc, W, gpu)[:, None]
    q, k, v = (t.double() for t in _split(xe, H))
    zero = torch.zeros((), dtype=torch.float64, device=gpu)
    s = (q @ k.transpose(-1, -2) * scale).masked_fill(~vis, float("-inf"))
    Pb = torch.where(vis, (s - lse.double()[..., None]).exp(), zero)  # from the lse the backward is given
    dod = _heads(do, H).double()
    D = (dod * _heads(o, H).double()).sum(-1)
    dP = dod @ v.transpose(-1, -2)
    dS = Pb * (dP - D[..., None])
    Wt = U * dS.abs() + E * (Pb * (dP.abs() + D.abs()[..., None]))

    def group(t):  # [B, H, S, 64] -> the sum over each K/V head's G query heads
        return t.view(B, hkv, G, S, 64).sum(2)

    dk_ref, dv_ref = group(scale * (dS.transpose(-1, -2) @ q)), group(Pb.transpose(-1, -2) @ dod)
    dk, dv = (_heads(t.contiguous(), hkv) for t in dqkv[..., H * 64:].split(hkv * 64, -1))
    rep.add("dk", dk, dk_ref, group(scale * (Wt.transpose(-1, -2) @ q.abs())) + U * dk_ref.abs())
    rep.add("dv", dv, dv_ref, group((U + E) * (Pb.transpose(-1, -2) @ dod.abs())) + U * dv_ref.abs())
    pad = ~vis.any(-1)[:, 0]
    if bool(pad.any()):
        rep.zero("o-pad", o[pad])
        rep.zero("dqkv-pad", dqkv[pad])
    rep.finish()


@pytest.mark.gpu
def test_results_do_not_depend_on_the_grid(gpu, C):
    _, full, _ = _case(C, gpu, 320, 2, "window+docs+lens", 0.1)
    _, capped, _ = _case(C, gpu, 320, 2, "window+docs+lens", 0.1, grid_cap=3)
    for name, a, b in zip(("o", "lse", "dqkv"), full, capped):
        assert torch.equal(_bits(a), _bits(b)), name


@pytest.mark.gpu
@pytest.mark.parametrize("inverse", [False, True])
@pytest.mark.parametrize("hkv", [2, 1])
def test_rope_rotates_q_and_the_k_heads_only(gpu, C, hkv, inverse):
    from parameter_server_distributed_amd.ops.rope import rope_tables

    cos, sin = rope_tables(256, device=gpu)
    g = torch.Generator(device="cpu").manual_seed(hkv)
    x = torch.randn(2, 200, (H + 2 * hkv) * 64, generator=g).to(torch.bfloat16).to(gpu)
    lens = torch.tensor([200, 131], dtype=torch.int32, device=gpu)
    want = C.rope_(_expand(x, hkv), H, cos, sin, lens, None, inverse)  # today's op: every copy of a K head alike
    got = C.rope_(x.clone(), H, cos, sin, lens, None, inverse, 0, kv_heads=hkv)
    assert torch.equal(_bits(_expand(got, hkv)[..., :2 * H * 64]), _bits(want[..., :2 * H * 64])), "Q / K"
    assert torch.equal(_bits(got[..., (H + hkv) * 64:]), _bits(x[..., (H + hkv) * 64:])), "V"


@pytest.mark.gpu
def test_module_agrees_with_its_sdpa_path(gpu, monkeypatch):
    from parameter_server_distributed_amd.ops.attention import FusedSelfAttention

    m = FusedSelfAttention(H, p=0.0, causal=True, kv_heads=2).to(gpu)
    g = torch.Generator(device="cpu").manual_seed(5)
    x = torch.randn(B, 192, (H + 4) * 64, generator=g).to(torch.bfloat16).to(gpu)
    do = torch.randn(B, 192, H * 64, generator=g).to(torch.bfloat16).to(gpu)
    outs = []
    for feats in ("", "attn_gqa=0"):
        monkeypatch.setenv("PSD_FEATURES", feats)
        assert m._long_kernel_ok(x) == (feats == "")
        xg = x.clone().requires_grad_(True)
        o = m(xg)
        o.backward(do)
        outs.append((o.detach().float(), xg.grad.float()))
    for a, b in zip(*outs):
        assert float((a - b).abs().max()) <= 1e-2 * float(b.abs().max())


def test_llama_block_and_model_take_kv_heads_on_the_cpu():
    from parameter_server_distributed_amd.models.gpt import GPTForLM
    from parameter_server_distributed_amd.models.llama_block import LlamaLayer

    layer = LlamaLayer(hidden=256, heads=4, kv_heads=2, ffn=512, rope=(64, 10000.0))
    assert tuple(layer.qkv.weight.shape) == (512, 256)
    r = torch.randn(2, 48, 256, requires_grad=True)
    r2, h = layer(r)
    (r2.sum() + h.sum()).backward()
    assert bool(torch.isfinite(r.grad).all()) and layer.qkv.weight.grad.abs().sum() > 0
    with pytest.raises(ValueError, match="kv_heads"):
        LlamaLayer(hidden=256, heads=4, kv_heads=3, ffn=512)
    with pytest.raises(ValueError, match="kv_heads"):
        GPTForLM(layers=1, hidden=256, heads=4, vocab=128, arch="gpt", kv_heads=2)


@pytest.mark.parametrize("kw,name", [
    (dict(kv_heads=3), "kv_heads"), (dict(kv_heads=-1), "kv_heads"), (dict(kv_heads=8), "kv_heads"),
    (dict(kv_heads=2, causal=False), "kv_heads"), (dict(kv_heads=2, S=128), "kv_heads"),
    (dict(kv_heads=2, width=3 * H * 64), "kv_heads"), (dict(kv_heads=2, bias=True), "bias_out"),
])
def test_native_refusals_name_the_argument(C, kw, name):
    """Raised before any launch, and before the tensors' device is looked at: CPU tensors here."""
    hkv, S, causal = kw["kv_heads"], kw.get("S", 192), kw.get("causal", True)
    x = torch.zeros(1, S, kw.get("width", (H + 2 * max(hkv, 0)) * 64), dtype=torch.bfloat16)
    o, lse = torch.zeros(1, S, H * 64, dtype=torch.bfloat16), torch.zeros(1, H, S)
    calls = [lambda: C.attn_bwd(o, x, o, lse, H, 0.0, 0, None, torch.zeros(x.shape[-1]) if "bias" in kw else None,
                                None, 0, causal, None, 0, kv_heads=hkv)]
    if "bias" not in kw:
        calls.append(lambda: C.attn_fwd(x, H, 0.0, 0, None, None, 0, causal, None, 0, kv_heads=hkv))
    if set(kw) == {"kv_heads"}:
        calls.append(lambda: C.rope_(x, H, torch.zeros(256, 32), torch.zeros(256, 32), None, None, False, 0, kv_heads=hkv))
    for call in calls:
        with pytest.raises(RuntimeError, match=name):
            call()
