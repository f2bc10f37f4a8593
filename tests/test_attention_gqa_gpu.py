"""Grouped-query fused attention (csrc/hip/attention_gqa.hip, Hkv < H key/value heads)
against the fp32 reference of tests/attn_ref.py on K / V expanded with repeat_interleave; the
reference dk / dv is the fp32 sum over each group.  Bounds as in the head dim 64 / 128 files
(2e-2 bf16, 6e-3 fp16, 3e-2 dropout, lse 1e-3): the group sum is fp32, rounded once."""
import pytest
import torch

from apex_example_amd.models.gpt2 import GPT2Block, GPT2Config
from apex_example_amd.ops import (fused_attention, fused_attention_kv, fused_attention_qkv,
                                  fused_attention_qkv_gqa, fused_attention_varlen)
from apex_example_amd.ops.attention import _C
from attn_ref import DEV, NEG, close, mask_kwargs, no_sdpa, ref_attention, ref_grads

pytestmark = pytest.mark.gpu
BF16 = torch.bfloat16
DIMS = pytest.mark.parametrize("D", [64, 128])


def _check(got, q, k, v, do, rel, **kw):
    """``got`` = (o, dq, dk, dv) against the reference on expanded k / v, group-summed."""
    G = q.size(2) // k.size(2)
    kx, vx = (t.detach().repeat_interleave(G, dim=2) for t in (k, v))
    fold = lambda t: t.view(*k.shape[:3], G, k.size(3)).sum(3)  # noqa: E731
    dq, dk, dv = ref_grads(q, kx, vx, do, **kw)
    want = (ref_attention(q.detach(), kx, vx, **kw)[0], dq, fold(dk), fold(dv))
    for g, w, n in zip(got, want, ("o", "dq", "dk", "dv")):
        close(g.detach(), w, rel, n)


def _qkv(B, Sq, Sk, H, Hkv, D, dt=BF16):
    return [torch.randn(B, s, h, D, device=DEV, dtype=dt, requires_grad=True)
            for s, h in ((Sq, H), (Sk, Hkv), (Sk, Hkv))]


@DIMS
@pytest.mark.parametrize("B,S,H,Hkv", [(1, 64, 2, 1), (2, 129, 4, 2), (2, 200, 6, 2)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", [BF16, torch.float16])
def test_fwd_bwd(B, S, H, Hkv, causal, dt, D):
    torch.manual_seed(0)
    q, k, v = _qkv(B, S, S, H, Hkv, D, dt)
    do = torch.randn_like(q)
    _, lse = _C().fwd(q, k, v, causal, 0.0, 0, D ** -0.5, None, None)
    kx, vx = (t.detach().repeat_interleave(H // Hkv, dim=2) for t in (k, v))
    lse_err = (lse - ref_attention(q.detach(), kx, vx, causal)[1]).abs().max().item()
    print("lse max abs err %.3e (bound 1.0e-03)" % lse_err)
    assert lse_err < 1e-3
    o = fused_attention(q, k, v, causal=causal)
    o.backward(do)
    _check([o, q.grad, k.grad, v.grad], q, k, v, do, 2e-2 if dt == BF16 else 6e-3, causal=causal)


@DIMS
@pytest.mark.parametrize("seq_first", [False, True])
def test_packed_qkv_dropout(seq_first, D):
    P, H, Hkv = 0.1, 6, 2
    torch.manual_seed(1)
    qkv = torch.randn(2, 200, H + 2 * Hkv, D, device=DEV, dtype=BF16)
    do = torch.randn(2, 200, H, D, device=DEV, dtype=BF16)
    if seq_first:
        qkv = qkv.transpose(0, 1).contiguous().transpose(0, 1)
    runs = []
    for _ in range(2):
        torch.manual_seed(2)
        seed = int(torch.randint(0, 2 ** 31 - 1, (1,)).item())  # what the call will draw
        torch.manual_seed(2)
        x = qkv.clone(memory_format=torch.preserve_format).requires_grad_(True)
        o = fused_attention_qkv_gqa(x, Hkv, dropout_p=P)
        o.backward(do)
        runs.append((o.detach(), x.grad))
    (o, g), (o2, g2) = runs
    assert g.shape == qkv.shape and g.stride() == qkv.stride()
    assert torch.equal(o, o2) and torch.equal(g, g2)
    _check([o, *g.split((H, Hkv, Hkv), 2)], *qkv.split((H, Hkv, Hkv), 2), do, 3e-2, p=P, seed=seed)


@DIMS
@pytest.mark.parametrize("Sq,Sk", [(40, 200), (200, 40)])
def test_cross_packed_kv(Sq, Sk, D):
    torch.manual_seed(3)
    q, k, v = _qkv(2, Sq, Sk, 4, 2, D)
    kv = torch.stack((k, v), 2).detach().requires_grad_(True)
    o = fused_attention_kv(q, kv)
    do = torch.randn_like(o)
    o.backward(do)
    assert kv.grad.shape == kv.shape and kv.grad.is_contiguous()  # ONE packed dkv
    _check([o, q.grad, *kv.grad.unbind(2)], q, k, v, do, 2e-2)


@DIMS
@pytest.mark.parametrize("boolean", [True, False])
def test_key_masks(boolean, D):
    torch.manual_seed(4)
    gone = torch.zeros(3, 256, dtype=torch.bool)
    gone[0, 64:128] = gone[0, 5::7] = gone[1, 150:] = gone[2] = True  # dead tile, holes, pad, all
    bias = (torch.zeros(3, 256) if boolean else torch.randn(3, 256)).masked_fill(gone, NEG)
    q, k, v = _qkv(3, 256, 256, 4, 2, D)
    o = fused_attention(q, k, v, **mask_kwargs(bias, boolean))
    do = torch.randn_like(o)
    o.backward(do)
    _check([o, q.grad, k.grad, v.grad], q, k, v, do, 2e-2, bias=bias.to(DEV))
    assert not o[2].any() and not q.grad[2].any()       # every key masked: o = 0, dq = 0
    assert not k.grad[gone.to(DEV)].any() and not v.grad[gone.to(DEV)].any()  # exact zeros


@DIMS
def test_equal_heads_is_the_packed_qkv_call_bitwise(D):
    a = torch.randn(2, 200, 3, 3, D, device=DEV, dtype=BF16, requires_grad=True)
    b = a.detach().view(2, 200, 9, D).requires_grad_(True)
    do = torch.randn(2, 200, 3, D, device=DEV, dtype=BF16)
    oa, ob = fused_attention_qkv(a, causal=True), fused_attention_qkv_gqa(b, 3, causal=True)
    oa.backward(do), ob.backward(do)
    assert torch.equal(oa, ob) and torch.equal(a.grad.view_as(b), b.grad)


def test_refusals():
    q, k, _ = _qkv(1, 64, 64, 4, 2, 64)
    with pytest.raises(ValueError, match="4 query heads do not split over 3 key/value heads"):
        fused_attention_qkv_gqa(torch.randn(1, 64, 10, 64, device=DEV, dtype=BF16), 3)
    with pytest.raises(ValueError, match=r"H = 4, Hkv = 2.*attn_mask"):
        fused_attention(q, k, k, attn_mask=torch.zeros(64, 64, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError, match=r"H = 4, Hkv = 2.*cu_seqlens"):
        fused_attention_varlen(q[0], k[0], k[0], torch.tensor([0, 64], dtype=torch.int32).to(DEV))


def test_gpt2_block_takes_the_fused_path(monkeypatch):
    kw = dict(n_layer=1, n_embd=256, n_head=4, n_kv_head=2, resid_pdrop=0.0, attn_pdrop=0.0)
    torch.manual_seed(6)
    fast = GPT2Block(GPT2Config(**kw)).to(DEV).to(BF16)
    ref = GPT2Block(GPT2Config(fused_attention=False, **kw)).to(DEV).to(BF16)
    ref.load_state_dict(fast.state_dict())
    x = torch.randn(2, 200, 256, device=DEV, dtype=BF16)
    xa, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    yr = ref(xr)
    dy = torch.randn_like(yr)
    yr.backward(dy)
    no_sdpa(monkeypatch)
    ya = fast(xa)
    ya.backward(dy)
    close(ya, yr.float(), 2e-2, "y")
    close(xa.grad, xr.grad.float(), 3e-2, "dx")  # two 16-bit paths, as the other files
