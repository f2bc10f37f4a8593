"""fused_attention_prefill over an FP8 (float8_e4m3fn) KV cache with per-row scales
(csrc/hip/attention_prefill_fp8.hip) against the fp64 reference of test_attention_decode_gpu on
the dequantised cache, at that test's bounds (byte -> 16-bit is exact and the scales are applied
in fp32: the format adds no rounding).  Cache bytes at or past L_b are the NaN pattern 0x7F and
the scales there NaN: the kernel must never load them."""
import dataclasses

import pytest
import torch

from apex_example_amd.models import gpt2
from apex_example_amd.ops import fused_attention_prefill
from attn_ref import DEV, close, no_sdpa
from test_attention_decode_fp8_gpu import FP8, dequant, make, mirror
from test_attention_decode_gpu import BOUND, check, ref  # noqa: F401 (BOUND: check's)
from test_attention_prefill_gpu import CASES

pytestmark = pytest.mark.gpu
BF16, FP16 = torch.bfloat16, torch.float16


def call(q, kv, sc, cl, **kw):
    return fused_attention_prefill(q, kv.view(FP8)[:, :, 0], kv.view(FP8)[:, :, 1], cl,
                                   k_scale=sc[:, 0], v_scale=sc[:, 1], return_lse=True, **kw)


@pytest.mark.parametrize("case", CASES, ids=lambda c: "B%d-H%d-Hkv%d-Sq%d" % c[:4])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_forward(D, dtype, case):
    B, H, Hkv, Sq, lens, Smax = case
    q, kv, sc, cl = make(B, H, Hkv, Sq, lens, Smax, D, dtype)
    o, lse = call(q, kv, sc, cl)
    assert o.shape == q.shape and o.dtype == dtype and o.is_contiguous()
    assert lse.shape == (B, H, Sq)
    check(o, lse, *ref(q, *dequant(kv, sc), lens), dtype, "fp8 prefill")


@pytest.mark.parametrize("D", [64, 128])
def test_append(D):
    B, H, Hkv, Sq, Smax, lens = 2, 4, 2, 70, 256, [62, 130]
    q, kv, sc, cl = make(B, H, Hkv, Sq, lens, Smax, D, FP16, seed=2)
    new = torch.randn(B, Sq, 2, Hkv, D, device=DEV).to(FP16)
    nb, ns = mirror(new)  # [B, Sq, 2, Hkv, D], [B, Sq, 2, Hkv]
    kv0, sc0 = kv.clone(), sc.clone()
    filled, fsc = kv.clone(), sc.clone()  # the cache a call without append would be given
    for b, n in enumerate(lens):
        filled[b, n:n + Sq] = nb[b]
        fsc[b, :, :, n:n + Sq] = ns[b].permute(1, 2, 0)
    o, lse = call(q, kv, sc, cl, k_new=new[:, :, 0], v_new=new[:, :, 1])
    for b, n in enumerate(lens):
        assert torch.equal(kv[b, n:n + Sq], nb[b])
        assert torch.equal(sc[b, :, :, n:n + Sq], ns[b].permute(1, 2, 0))
        assert torch.equal(kv[b, :n], kv0[b, :n]) and torch.equal(sc[b, :, :, :n], sc0[b, :, :, :n])
        assert (kv[b, n + Sq:] == 0x7F).all() and torch.isnan(sc[b, :, :, n + Sq:]).all()
    o2, lse2 = call(q, filled, fsc, cl + Sq)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    check(o, lse, *ref(q, *dequant(filled, fsc), [n + Sq for n in lens]), FP16, "fp8 append")


def test_clip_and_determinism():
    """cache_seqlens above Smax: the results are those of L = Smax and the append writes nothing
    (the guard rows around the caches and scales keep their values); two calls, bitwise equal."""
    B, H, Hkv, Sq, Smax, D = 2, 4, 2, 40, 96, 64
    q, kv, sc, _ = make(B, H, Hkv, Sq, [Smax, Smax], Smax, D, BF16, seed=3)
    guarded = torch.full((B, Smax + 2, 2, Hkv, D), 7, device=DEV, dtype=torch.uint8)
    gsc = torch.full((B, 2, Hkv, Smax + 2), 7.0, device=DEV)
    guarded[:, 1:-1], gsc[..., 1:-1] = kv, sc
    cl = torch.tensor([Smax + 5, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    new = torch.randn(B, Sq, 2, Hkv, D, device=DEV).to(BF16)
    a, b = (call(q, guarded[:, 1:-1], gsc[..., 1:-1], cl, k_new=new[:, :, 0], v_new=new[:, :, 1])
            for _ in range(2))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(guarded[:, 1:-1], kv) and torch.equal(gsc[..., 1:-1], sc)
    assert (guarded[:, [0, -1]] == 7).all() and (gsc[..., [0, -1]] == 7).all()
    check(*a, *ref(q, *dequant(kv, sc), [Smax, Smax]), BF16, "fp8 clip")


REFUSALS = {
    "one scale": lambda a: a.update(v_scale=None),
    "scale dtype": lambda a: a.update(k_scale=a["k_scale"].double()),
    "scale shape": lambda a: a.update(k_scale=a["k_scale"][..., :32]),
    "scales with a 16-bit cache": lambda a: a.update(k_cache=a["k_cache"].to(BF16),
                                                    v_cache=a["v_cache"].to(BF16)),
    "e5m2": lambda a: a.update(k_cache=a["k_cache"].view(torch.float8_e5m2),
                               v_cache=a["v_cache"].view(torch.float8_e5m2)),
    "block_table": lambda a: a.update(block_table=torch.zeros(2, 1, dtype=torch.int32,
                                                              device=DEV)),
    "grad q": lambda a: a.update(q=a["q"].clone().requires_grad_(True)),
}


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(what):
    q, kv, sc, cl = make(2, 4, 2, 4, [8, 8], 64, 64, BF16)
    args = dict(q=q, k_cache=kv.view(FP8)[:, :, 0], v_cache=kv.view(FP8)[:, :, 1],
                cache_seqlens=cl, k_scale=sc[:, 0], v_scale=sc[:, 1])
    fused_attention_prefill(**args)  # the call every refusal is one edit away from
    REFUSALS[what](args)
    with pytest.raises(ValueError):
        fused_attention_prefill(**args)


@pytest.mark.parametrize("n_kv_head", [None, 2])
def test_gpt2_fp8_chunked_logits(n_kv_head, monkeypatch):
    """A 70-token prompt as two 35-token chunks over an FP8 cache (the second on the FP8 prefill
    kernels: 35 or 70 rows per group >= 33), then 8 single steps: the logits of the same weights
    with fused_attention=False, whose torch-mirror fallback attends the same cache contents (two
    16-bit paths: 3e-2)."""
    torch.manual_seed(0)
    cfg = gpt2.GPT2Config(vocab_size=512, n_positions=128, n_embd=256, n_layer=2, n_head=4,
                          n_kv_head=n_kv_head)
    model = gpt2.GPT2LMHeadModel(cfg).to(DEV, BF16).eval()
    plain = gpt2.GPT2LMHeadModel(dataclasses.replace(cfg, fused_attention=False))
    plain = plain.to(DEV, BF16).eval()
    plain.load_state_dict(model.state_dict())
    ids = torch.randint(0, cfg.vocab_size, (2, 78), device=DEV)
    monkeypatch.setattr(gpt2, "PREFILL_MIN_ROWS", 33)
    calls = []
    monkeypatch.setattr(gpt2.fused_attn, "fused_attention_prefill",
                        lambda *a, _f=gpt2.fused_attn.fused_attention_prefill, **k:
                        calls.append((a[0].size(1), k["k_scale"] is not None)) or _f(*a, **k))

    def run(m):
        cache = gpt2.KVCache(2, 78, kv_dtype=FP8)
        with torch.no_grad():
            steps = [m(ids[:, :35], cache=cache), m(ids[:, 35:70], cache=cache)]
            steps += [m(ids[:, t:t + 1], cache=cache) for t in range(70, 78)]
        assert cache.lengths.tolist() == [78, 78] and cache.kv[0].dtype == FP8
        return torch.cat(steps, 1)

    want = run(plain).float()
    assert calls == []
    no_sdpa(monkeypatch)
    got = run(model)
    assert calls == [(35, True)] * cfg.n_layer
    close(got, want, 3e-2, "fp8 chunked logits")
