"""Head dim 128 fused attention kernels (csrc/hip/attention_d128.hip) against the fp32
reference of tests/attn_ref.py, through every public layout: forward, all gradients, the
exact dropout keep mask, key masks, cross-attention, packed sequences, bitwise
reproducibility and the module routing.

Bounds are those of the D = 64 files (the 16-bit rounding of P and of the stored results
does not depend on D, the accumulation is fp32): max error / max |reference| below 2e-2
for bf16 (6e-3 fp16), 3e-2 under dropout, lse within 1e-3.
"""
import pytest
import torch

from attn_ref import (DEV, NEG, close, finite, mask_kwargs, no_sdpa, ref_attention, ref_grads)

pytestmark = pytest.mark.gpu
D = 128
BF16 = torch.bfloat16


def _rel(dt, p=0.0):
    return 3e-2 if p > 0 else (2e-2 if dt == BF16 else 6e-3)


def _apply(layout, inputs, do, causal=False, p=0.0, seed=0, mask=(None, None), varlen=None):
    """The autograd op with an explicit dropout seed -> (o, [one gradient per input])."""
    from apex_example_amd.ops.attention import AttentionFunction

    xs = [t.detach().clone().requires_grad_(True) for t in inputs]
    o = AttentionFunction.apply(layout, causal, p, D ** -0.5, seed, *mask, varlen, *xs)
    o.backward(do)
    return o.detach(), [x.grad for x in xs]


def _check(got, want, rel, names):
    for g, w, n in zip(got, want, names):
        close(g, w, rel, n)


# ------------------------------------------------------------- 1. forward and backward
@pytest.mark.parametrize("B,S,H", [(1, 64, 1), (2, 129, 2), (1, 200, 3)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("dt", [BF16, torch.float16])
def test_fwd_bwd(B, S, H, causal, dt):
    from apex_example_amd.ops.attention import _C

    torch.manual_seed(0)
    q, k, v, do = (torch.randn(B, S, H, D, device=DEV, dtype=dt) for _ in range(4))
    _, lse = _C().fwd(q, k, v, causal, 0.0, 0, D ** -0.5, None, None)
    o, grads = _apply("qkv", (q, k, v), do, causal)
    ro, rlse, _ = ref_attention(q, k, v, causal)
    lse_err = (lse - rlse).abs().max().item()
    print("lse max abs err %.3e (bound 1.0e-03)" % lse_err)
    assert lse_err < 1e-3
    _check([o, *grads], [ro, *ref_grads(q, k, v, do, causal)], _rel(dt), ("o", "dq", "dk", "dv"))


# -------------------------------------------------------- 2. packed qkv, 6. determinism
P, SEED = 0.1, 4321


@pytest.fixture(scope="module")
def packed_case():
    """qkv [2, 200, 3, 3, 128], do and the reference's o and (dq, dk, dv) under dropout."""
    torch.manual_seed(1)
    qkv = torch.randn(2, 200, 3, 3, D, device=DEV, dtype=BF16)
    do = torch.randn(2, 200, 3, D, device=DEV, dtype=BF16)
    q, k, v = qkv.unbind(2)
    ro = ref_attention(q, k, v, p=P, seed=SEED)[0]
    return qkv, do, ro, ref_grads(q, k, v, do, p=P, seed=SEED)


@pytest.mark.parametrize("seq_first", [False, True])
def test_packed_qkv_dropout(seq_first, packed_case):
    qkv, do, ro, rg = packed_case
    x = qkv.transpose(0, 1).contiguous().transpose(0, 1) if seq_first else qkv
    assert x.is_contiguous() != seq_first
    o, (g,) = _apply("packed_qkv", (x,), do, p=P, seed=SEED)
    assert g.shape == qkv.shape and g.stride() == x.stride()  # ONE dqkv of qkv's layout
    _check([o, *g.unbind(2)], [ro, *rg], _rel(BF16, P), ("o", "dq", "dk", "dv"))


def test_bwd_deterministic(packed_case):
    qkv, do, _, _ = packed_case
    (a,), (b,) = (_apply("packed_qkv", (qkv,), do, p=P, seed=SEED)[1] for _ in range(2))
    assert torch.equal(a, b)


# ------------------------------------------------------------------ 3. cross-attention
@pytest.mark.parametrize("Sq,Sk", [(40, 200), (200, 40)])
def test_cross_packed_kv(Sq, Sk):
    from apex_example_amd.ops.attention import fused_attention_kv

    torch.manual_seed(2)
    q = torch.randn(2, Sq, 2, D, device=DEV, dtype=BF16, requires_grad=True)
    kv = torch.randn(2, Sk, 2, 2, D, device=DEV, dtype=BF16, requires_grad=True)
    o = fused_attention_kv(q, kv)
    do = torch.randn_like(o)
    o.backward(do)
    k, v = kv.detach().unbind(2)
    assert kv.grad.shape == kv.shape and kv.grad.is_contiguous()
    _check([o.detach(), q.grad, *kv.grad.unbind(2)],
           [ref_attention(q.detach(), k, v)[0], *ref_grads(q, k, v, do)], _rel(BF16),
           ("o", "dq", "dk", "dv"))


# ------------------------------------------------------------------------ 4. key masks
@pytest.mark.parametrize("boolean", [True, False])
def test_key_masks(boolean):
    """Sk = 256: batch 0 has a dead 64-key tile in the middle (keys 64..127) and scattered
    masked keys, batch 1 is padded from key 150, batch 2 has every key masked."""
    from apex_example_amd.ops.attention import fused_attention

    torch.manual_seed(3)
    B, S, H = 3, 256, 2
    gone = torch.zeros(B, S, dtype=torch.bool)
    gone[0, 64:128] = True
    gone[0, 5::7] = True
    gone[1, 150:] = True
    gone[2] = True
    bias = (torch.zeros(B, S) if boolean else torch.randn(B, S)).masked_fill(gone, NEG)
    q, k, v = (torch.randn(B, S, H, D, device=DEV, dtype=BF16, requires_grad=True)
               for _ in range(3))
    o = fused_attention(q, k, v, **mask_kwargs(bias, boolean))
    do = torch.randn_like(o)
    o.backward(do)
    ro = ref_attention(q.detach(), k.detach(), v.detach(), bias=bias.to(DEV))[0]
    _check([o.detach(), q.grad, k.grad, v.grad], [ro, *ref_grads(q, k, v, do, bias=bias.to(DEV))],
           _rel(BF16), ("o", "dq", "dk", "dv"))
    finite(o, q.grad, k.grad, v.grad)
    assert not o[2].any() and not q.grad[2].any()       # every key masked: o = 0, dq = 0
    assert not k.grad[gone.to(DEV)].any() and not v.grad[gone.to(DEV)].any()  # exact zeros


# ------------------------------------------------------------------ 5. packed sequences
LENS = (0, 1, 64, 65, 200)


@pytest.mark.parametrize("causal,p", [(False, 0.0), (True, 0.0), (False, P)])
def test_varlen_equals_padded_masked_call(causal, p):
    """The packed call against the reference of the padded problem with the key-padding
    mask, read at the real rows (the hash indices are local to the sequence)."""
    torch.manual_seed(4)
    B, S, H, T = len(LENS), max(LENS), 2, sum(LENS)
    cu = torch.tensor([0, *torch.tensor(LENS).cumsum(0).tolist()], dtype=torch.int32, device=DEV)
    real = (torch.arange(S).view(1, S) < torch.tensor(LENS).view(B, 1)).to(DEV)  # [B, S]
    q, k, v, do = (torch.randn(T, H, D, device=DEV, dtype=BF16) for _ in range(4))

    def pad(x):
        y = torch.zeros(B, S, H, D, device=DEV, dtype=BF16)
        y[real] = x
        return y

    o, grads = _apply("varlen_qkv", (q, k, v), do, causal, p, SEED, varlen=(cu, S))
    bias = torch.zeros(B, S, device=DEV).masked_fill(~real, NEG)
    pq, pk, pv, pdo = pad(q), pad(k), pad(v), pad(do)
    ro = ref_attention(pq, pk, pv, causal, bias, p=p, seed=SEED)[0]
    rg = ref_grads(pq, pk, pv, pdo, causal, bias, p=p, seed=SEED)
    _check([o, *grads], [t[real] for t in (ro, *rg)], _rel(BF16, p), ("o", "dq", "dk", "dv"))


# ------------------------------------------------------------------------ 7. interface
@pytest.mark.parametrize("encdec", [False, True])
def test_multihead_attn_modules_take_the_fused_path(encdec, monkeypatch):
    from apex_example_amd.contrib.multihead_attn import EncdecMultiheadAttn, SelfMultiheadAttn

    torch.manual_seed(5)
    cls = EncdecMultiheadAttn if encdec else SelfMultiheadAttn
    fast = cls(256, 2, bias=True).to(DEV).to(BF16)
    ref = cls(256, 2, bias=True, impl="default").to(DEV).to(BF16)
    ref.load_state_dict(fast.state_dict())
    x = torch.randn(70, 2, 256, device=DEV, dtype=BF16)
    mem = torch.randn(130 if encdec else 70, 2, 256, device=DEV, dtype=BF16)
    xa, xr = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    args = (lambda t: (t, mem)) if encdec else (lambda t: (t, t, t))
    yr, _ = ref(*args(xr), is_training=False)
    dy = torch.randn_like(yr)
    yr.backward(dy)
    no_sdpa(monkeypatch)
    ya, _ = fast(*args(xa), is_training=False)
    ya.backward(dy)
    close(ya, yr.float(), 2e-2, "y")
    close(xa.grad, xr.grad.float(), 3e-2, "dx")  # two 16-bit paths, as the D = 64 files


def test_supported_head_dims():
    from apex_example_amd.ops.attention import fused_attention, supported

    t = torch.empty(1, device=DEV, dtype=BF16)
    assert supported(t, 128) and supported(t, 64) and not supported(t, 96)
    q = torch.randn(1, 64, 1, 96, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match=r"\[B,S,H,64\] or \[B,S,H,128\]"):
        fused_attention(q, q, q)
