"""fused_attention_decode over a paged KV cache (csrc/hip/attention_decode_paged.hip): against
the fp64 reference of test_attention_decode_gpu on the contiguous cache, and bit for bit
against the contiguous kernels at the same num_splits.  Every pool row that holds no key below
L_b is NaN and every table entry at or past ceil(L_b / P) is 2**30: the kernels must read
neither."""
import pytest
import torch

from apex_example_amd.models.gpt2 import GPT2Config, GPT2LMHeadModel, KVCache, PagedKVCache
from apex_example_amd.ops import fused_attention_decode, paged_kv_append
from attn_ref import DEV, close, no_sdpa
from test_attention_decode_gpu import BF16, FP16, check, make, ref

pytestmark = pytest.mark.gpu


def page(kv, lens, P):
    """A contiguous [B, Smax, 2, Hkv, D] cache of make() (NaN at and past its lengths) scattered
    into a NaN pool of 2 B Smax / P + 1 pages by a random permutation (the last page, where a
    clamped bad id lands, is never used) -> the pool and the table, unallocated beyond ``lens``."""
    B, Smax = kv.shape[:2]
    n = Smax // P
    perm = torch.randperm(2 * B * n, generator=torch.Generator().manual_seed(P))[:B * n]
    pool = torch.full((2 * B * n + 1, P) + kv.shape[2:], float("nan"), dtype=kv.dtype, device=DEV)
    pool[perm.to(DEV)] = kv.reshape(B * n, P, *kv.shape[2:])
    table = perm.view(B, n).int()
    for b, L in enumerate(lens):
        table[b, -(-min(L, Smax) // P):] = 2 ** 30
    return pool, table.to(DEV)


def bits(t):
    return t.view(torch.int16)


def cases(P):
    return [(1, 1, 1, 1, [1], 256), (3, 8, 2, 1, [0, 65, 256], 256),
            (2, 6, 2, 5, [P + 1, 3 * P - 1], 512), (2, 16, 1, 3, [200, 17], 256)]


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("P", [16, 32, 64, 256])
def test_forward(P, D, nsplit, case):
    B, H, Hkv, Sq, lens, Smax = cases(P)[case]
    dtype = BF16 if P in (16, 64) else FP16
    q, kv, cl = make(B, H, Hkv, Sq, lens, Smax, D, dtype, seed=case)
    pool, table = page(kv, lens, P)
    o, lse = fused_attention_decode(q, pool[:, :, 0], pool[:, :, 1], cl, num_splits=nsplit,
                                    return_lse=True, block_table=table)
    assert o.shape == q.shape and o.is_contiguous() and lse.shape == (B, H, Sq)
    check(o, lse, *ref(q, kv[:, :, 0], kv[:, :, 1], lens), dtype, "paged")
    o2, lse2 = fused_attention_decode(q, kv[:, :, 0], kv[:, :, 1], cl, num_splits=nsplit,
                                      return_lse=True)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)


@pytest.mark.parametrize("D", [64, 128])
def test_append(D):
    """New rows across a page edge (14 .. 16 and 130 .. 132 at P = 16), and a 70-row prompt."""
    B, H, Hkv, Sq, Smax, lens, P = 2, 4, 2, 3, 256, [14, 130], 16
    q, kv, cl = make(B, H, Hkv, Sq, lens, Smax, D, FP16, seed=2)
    new = torch.randn(B, Sq, 2, Hkv, D, device=DEV).to(FP16)
    after = [n + Sq for n in lens]
    pool, table = page(kv, after, P)
    before = pool.clone()
    filled = kv.clone()  # the cache a call without append would be given
    for b, n in enumerate(lens):
        filled[b, n:n + Sq] = new[b]
    want, _ = page(filled, after, P)
    o, lse = fused_attention_decode(q, pool[:, :, 0], pool[:, :, 1], cl, k_new=new[:, :, 0],
                                    v_new=new[:, :, 1], num_splits=2, return_lse=True,
                                    block_table=table)
    assert torch.equal(bits(pool), bits(want))  # the new rows where expected ...
    changed = (bits(pool) != bits(before)).flatten(2).any(2)
    assert changed.sum().item() == B * Sq      # ... and every other row bit-identical
    o2, lse2 = fused_attention_decode(q, want[:, :, 0], want[:, :, 1], cl + Sq, num_splits=2,
                                      return_lse=True, block_table=table)
    assert torch.equal(o, o2) and torch.equal(lse, lse2)
    check(o, lse, *ref(q, filled[:, :, 0], filled[:, :, 1], after), FP16, "paged append")

    _, kv, _ = make(B, H, Hkv, 1, [70, 70], 80, D, FP16, seed=3)
    want, table = page(kv, [70, 70], P)
    pool = torch.full_like(want, float("nan"))
    paged_kv_append(kv[:, :70, 0], kv[:, :70, 1], pool[:, :, 0], pool[:, :, 1], table,
                    torch.zeros(B, dtype=torch.int32, device=DEV))
    assert torch.equal(bits(pool), bits(want))


def test_clip():
    """cache_seqlens above Smax: the results are those of L = Smax, an append writes nothing."""
    B, H, Hkv, Sq, Smax, D, P = 2, 2, 2, 1, 96, 64, 16
    q, kv, _ = make(B, H, Hkv, Sq, [Smax, Smax], Smax, D, BF16, seed=3)
    pool, table = page(kv, [Smax, Smax], P)
    before = pool.clone()
    cl = torch.tensor([Smax + 5, 2 ** 31 - 1], dtype=torch.int32, device=DEV)
    new = torch.randn(B, Sq, 2, Hkv, D, device=DEV).to(BF16)
    o, lse = fused_attention_decode(q, pool[:, :, 0], pool[:, :, 1], cl, k_new=new[:, :, 0],
                                    v_new=new[:, :, 1], num_splits=2, return_lse=True,
                                    block_table=table)
    assert torch.equal(bits(pool), bits(before))
    check(o, lse, *ref(q, kv[:, :, 0], kv[:, :, 1], [Smax, Smax]), BF16, "paged clip")


def test_refusals():
    q, kv, cl = make(2, 4, 2, 1, [8, 8], 64, 64, BF16)
    pool, table = page(kv, [8, 8], 16)
    k, v = pool[:, :, 0], pool[:, :, 1]
    p48 = pool.new_zeros(3, 48, 2, 2, 64)
    bad = [dict(block_table=table.long()), dict(block_table=table.cpu()),
           dict(block_table=table[:1]), dict(block_table=table[:, ::2]),
           dict(k_cache=p48[:, :, 0], v_cache=p48[:, :, 1]), dict(k_cache=k[:, :8], v_cache=v[:, :8]),
           dict(k_cache=k[:, :, :1]), dict(k_cache=k[..., :32], v_cache=v[..., :32]),
           dict(k_cache=k.half(), v_cache=v.half()), dict(q=q.clone().requires_grad_(True))]
    for kw in bad:
        args = dict(q=q, k_cache=k, v_cache=v, cache_seqlens=cl, block_table=table)
        args.update(kw)
        with pytest.raises(ValueError):
            fused_attention_decode(**args)


@pytest.mark.parametrize("n_kv_head", [None, 2])
def test_gpt2_paged_logits(n_kv_head, monkeypatch):
    """test_gpt2_cached_logits with 16-row pages: the logits of the contiguous cache bit for
    bit, and the full forward's within the two 16-bit paths' 3e-2."""
    torch.manual_seed(0)
    cfg = GPT2Config(vocab_size=512, n_positions=128, n_embd=256, n_layer=2, n_head=4,
                     n_kv_head=n_kv_head)
    model = GPT2LMHeadModel(cfg).to(DEV, BF16).eval()
    ids = torch.randint(0, cfg.vocab_size, (2, 78), device=DEV)
    no_sdpa(monkeypatch)
    got = []
    with torch.no_grad():
        full = model(ids).float()
        for cache in (PagedKVCache(2, 78, page_size=16), KVCache(2, 78)):
            steps = [model(ids[:, :70], cache=cache)[:, -1:]]
            steps += [model(ids[:, t:t + 1], cache=cache) for t in range(70, 78)]
            got.append(torch.cat(steps, 1))
            assert cache.length == 78 and cache.lengths.tolist() == [78, 78]
    assert torch.equal(got[0], got[1])
    close(got[0], full[:, 69:], 3e-2, "paged cached logits")
