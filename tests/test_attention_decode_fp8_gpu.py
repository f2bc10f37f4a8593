"""fused_attention_decode over an FP8 (float8_e4m3fn) KV cache with per-row scales
(csrc/hip/attention_decode_fp8.hip) against the fp64 reference of test_attention_decode_gpu on
the dequantised cache (bytes.double() * scale.double()), at that test's bounds: the kernel adds
no rounding the 16-bit kernel lacks.  Cache bytes at or past L_b are the NaN pattern 0x7F and
the scales there NaN: the kernels must never load them."""
import dataclasses

import pytest
import torch

from apex_example_amd.models.gpt2 import GPT2Config, GPT2LMHeadModel, KVCache
from apex_example_amd.ops import fp8_kv_append, fused_attention_decode
from attn_ref import DEV, close, no_sdpa
from test_attention_decode_gpu import BOUND, CASES, check, ref

pytestmark = pytest.mark.gpu
BF16, FP16, FP8 = torch.bfloat16, torch.float16, torch.float8_e4m3fn
FINITE = torch.tensor([b for b in range(256) if b & 0x7F != 0x7F], dtype=torch.uint8)
# either side of a 128-key slot; at num_splits = 5 every split owns one 64-key tile
FP8_CASES = CASES + [(2, 4, 2, 1, [127, 129], 256), (2, 4, 4, 1, [320, 129], 320)]


def make(B, H, Hkv, Sq, lens, Smax, D, dtype, seed=0):
    """q; a packed sequence-first cache of bytes uniform over the 254 finite e4m3 patterns, as
    uint8 [B, Smax, 2, Hkv, D]; packed scales 2^-7 * 2^u, u in [-2, 2], [B, 2, Hkv, Smax]; the
    lengths.  Rows at or past lens[b]: bytes 0x7F, scales NaN."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(B, Sq, H, D, generator=g).to(DEV, dtype)
    kv = FINITE[torch.randint(0, 254, (Smax, B, 2, Hkv, D), generator=g)].to(DEV).transpose(0, 1)
    sc = torch.ldexp(torch.ones(()), torch.randint(-9, -4, (B, 2, Hkv, Smax), generator=g)).to(DEV)
    for b, n in enumerate(lens):
        kv[b, min(n, Smax):] = 0x7F
        sc[b, :, :, min(n, Smax):] = float("nan")
    return q, kv, sc, torch.tensor(lens, dtype=torch.int32, device=DEV)


def call(q, kv, sc, cl, **kw):
    return fused_attention_decode(q, kv.view(FP8)[:, :, 0], kv.view(FP8)[:, :, 1], cl,
                                  k_scale=sc[:, 0], v_scale=sc[:, 1], return_lse=True, **kw)


def dequant(kv, sc):
    """fp64 k and v [B, Smax, Hkv, D] of a packed cache."""
    x = kv.view(FP8).float().double() * sc.double().permute(0, 3, 1, 2).unsqueeze(-1)
    return x[:, :, 0], x[:, :, 1]


def mirror(x):
    """The append kernel's quantiser in torch on the CPU: (uint8 bytes like x, scales)."""
    x = x.cpu().float()
    amax = x.abs().amax(-1, keepdim=True)
    s = torch.where(amax > 0, amax / 448, torch.ones_like(amax))
    return (x / s).clamp(-448, 448).to(FP8).view(torch.uint8).to(DEV), s.squeeze(-1).to(DEV)


@pytest.mark.parametrize("case", FP8_CASES, ids=lambda c: "B%d-H%d-Hkv%d-Sq%d-L%d" % (
    c[:4] + (c[4][0],)))
@pytest.mark.parametrize("nsplit", [1, 2, 5])
@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_forward(D, dtype, nsplit, case):
    B, H, Hkv, Sq, lens, Smax = case
    q, kv, sc, cl = make(B, H, Hkv, Sq, lens, Smax, D, dtype)
    o, lse = call(q, kv, sc, cl, num_splits=nsplit)
    assert o.shape == q.shape and o.dtype == dtype and o.is_contiguous()
    assert lse.shape == (B, H, Sq)
    check(o, lse, *ref(q, *dequant(kv, sc), lens), dtype, "fp8 decode")


@pytest.mark.parametrize("dtype", [BF16, FP16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("D", [64, 128])
def test_append_is_the_mirror(D, dtype):
    B, H, Hkv, Sq, Smax, lens = 2, 4, 2, 3, 256, [62, 130]
    q, kv, sc, cl = make(B, H, Hkv, Sq, lens, Smax, D, dtype, seed=2)
    new = torch.randn(B, Sq, 2, Hkv, D, device=DEV).to(dtype)
    new[0, 1, 0, 0] = 0  # an all-zero key row: scale 1
    nb, ns = mirror(new)  # [B, Sq, 2, Hkv, D], [B, Sq, 2, Hkv]
    assert ns[0, 1, 0, 0] == 1
    kv0, sc0 = kv.clone(), sc.clone()
    filled, fsc = kv.clone(), sc.clone()  # the cache a call without append would be given
    for b, n in enumerate(lens):
        filled[b, n:n + Sq] = nb[b]
        fsc[b, :, :, n:n + Sq] = ns[b].permute(1, 2, 0)
    o, lse = call(q, kv, sc, cl, k_new=new[:, :, 0], v_new=new[:, :, 1], num_splits=2)
    for b, n in enumerate(lens):
        assert torch.equal(kv[b, n:n + Sq], nb[b])
        assert torch.equal(sc[b, :, :, n:n + Sq], ns[b].permute(1, 2, 0))
        assert torch.equal(kv[b, :n], kv0[b, :n]) and torch.equal(sc[b, :, :, :n], sc0[b, :, :, :n])
        assert (kv[b, n + Sq:] == 0x7F).all() and torch.isnan(sc[b, :, :, n + Sq:]).all()
    o2, lse2 = call(q, filled, fsc, cl + Sq, num_splits=2)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    check(o, lse, *ref(q, *dequant(filled, fsc), [n + Sq for n in lens]), dtype, "fp8 append")
    # a 70-row prompt into an empty cache, on its own
    prompt = torch.randn(B, 70, 2, Hkv, D, device=DEV).to(dtype)
    pb, ps = mirror(prompt)
    kv[:], sc[:] = 0x7F, float("nan")
    fp8_kv_append(prompt[:, :, 0], prompt[:, :, 1], kv.view(FP8)[:, :, 0], kv.view(FP8)[:, :, 1],
                  sc[:, 0], sc[:, 1], torch.zeros_like(cl))
    assert torch.equal(kv[:, :70], pb) and torch.equal(sc[..., :70], ps.permute(0, 2, 3, 1))
    assert (kv[:, 70:] == 0x7F).all() and torch.isnan(sc[..., 70:]).all()


def test_default_splits_and_determinism():
    lens = [40, 1500, 2048]
    q, kv, sc, cl = make(3, 8, 2, 1, lens, 2048, 128, BF16, seed=1)
    a, b = call(q, kv, sc, cl), call(q, kv, sc, cl)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    check(*a, *ref(q, *dequant(kv, sc), lens), BF16, "fp8 default splits")


REFUSALS = {
    "no scales": lambda a: a.update(k_scale=None, v_scale=None),
    "one scale": lambda a: a.update(v_scale=None),
    "scale dtype": lambda a: a.update(k_scale=a["k_scale"].double()),
    "scale shape": lambda a: a.update(k_scale=a["k_scale"][..., :32]),
    "scale device": lambda a: a.update(v_scale=a["v_scale"].cpu()),
    "scale inner stride": lambda a: a.update(
        k_scale=a["k_scale"].transpose(1, 2).contiguous().transpose(1, 2)),
    "scales with a 16-bit cache": lambda a: a.update(k_cache=a["k_cache"].to(BF16),
                                                    v_cache=a["v_cache"].to(BF16)),
    "mixed caches": lambda a: a.update(v_cache=a["v_cache"].to(BF16)),
    "e5m2": lambda a: a.update(k_cache=a["k_cache"].view(torch.float8_e5m2),
                               v_cache=a["v_cache"].view(torch.float8_e5m2)),
    "int8": lambda a: a.update(k_cache=a["k_cache"].view(torch.int8),
                               v_cache=a["v_cache"].view(torch.int8)),
    "block_table": lambda a: a.update(block_table=torch.zeros(2, 1, dtype=torch.int32,
                                                              device=DEV)),
    "fp32 q": lambda a: a.update(q=a["q"].float()),
}


@pytest.mark.parametrize("what", REFUSALS)
def test_refusals(what):
    q, kv, sc, cl = make(2, 4, 2, 1, [8, 8], 64, 64, BF16)
    args = dict(q=q, k_cache=kv.view(FP8)[:, :, 0], v_cache=kv.view(FP8)[:, :, 1],
                cache_seqlens=cl, k_scale=sc[:, 0], v_scale=sc[:, 1])
    fused_attention_decode(**args)  # the call every refusal is one edit away from
    REFUSALS[what](args)
    with pytest.raises(ValueError):
        fused_attention_decode(**args)


@pytest.mark.parametrize("n_kv_head", [None, 2])
def test_gpt2_fp8_cached_logits(n_kv_head, monkeypatch):
    """A 70-token prompt, then 8 teacher-forced steps over an FP8 cache: the fused path's logits
    against those of the same weights with fused_attention=False, whose torch-mirror fallback
    attends the same cache contents (two 16-bit paths computing the same thing: 3e-2)."""
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_positions=128, n_embd=256, n_layer=2, n_head=4,
                     n_kv_head=n_kv_head)
    model = GPT2LMHeadModel(cfg).to(DEV, BF16).eval()
    plain = GPT2LMHeadModel(dataclasses.replace(cfg, fused_attention=False)).to(DEV, BF16).eval()
    plain.load_state_dict(model.state_dict())
    ids = torch.randint(0, cfg.vocab_size, (2, 78), device=DEV)

    def run(m):
        cache = KVCache(2, 78, kv_dtype=FP8)
        with torch.no_grad():
            steps = [m(ids[:, :70], cache=cache)[:, -1:]]
            steps += [m(ids[:, t:t + 1], cache=cache) for t in range(70, 78)]
        assert cache.length == 78 and cache.kv[0].dtype == FP8
        return torch.cat(steps, 1)

    want = run(plain).float()
    no_sdpa(monkeypatch)
    close(run(model), want, 3e-2, "fp8 cached logits")
