"""The shared fp32 attention reference (tests/attn_ref.py) is right: against
F.scaled_dot_product_attention on the CPU at small equal and unequal lengths, on a fully
masked batch element, and in the keep mask it applies under dropout."""
import math

import pytest
import torch
import torch.nn.functional as F

import dropout_hash
from attn_ref import NEG, ref_attention, ref_grads

B, H, D = 2, 2, 64
LENGTHS = [(5, 5), (5, 9), (9, 5)]


def _inputs(Sq, Sk):
    g = torch.Generator().manual_seed(100 * Sq + Sk)
    q, k, v = (torch.randn(B, S, H, D, generator=g) for S in (Sq, Sk, Sk))
    return q, k, v, torch.randn(B, Sq, H, D, generator=g)


def _key_bias(Sk):
    """Additive [B, Sk]: finite biases, and -inf on the last third of batch element 1."""
    bias = 0.5 * torch.randn(B, Sk, generator=torch.Generator().manual_seed(7))
    bias[1, Sk - Sk // 3:] = NEG
    return bias


# the causal mask is defined for equal lengths only
@pytest.mark.parametrize("Sq,Sk,form", [(Sq, Sk, f) for Sq, Sk in LENGTHS
                                        for f in ("plain", "causal", "bias")
                                        if f != "causal" or Sq == Sk])
def test_ref_matches_sdpa(Sq, Sk, form):
    """o, lse and the three gradients; assert_close's fp32 defaults suffice everywhere."""
    q, k, v, do = _inputs(Sq, Sk)
    bias = _key_bias(Sk) if form == "bias" else None
    o, lse, dead = ref_attention(q, k, v, form == "causal", bias)
    assert o.shape == (B, Sq, H, D) and lse.shape == dead.shape == (B, H, Sq)
    assert not dead.any()
    qs, ks, vs = (t.clone().requires_grad_(True) for t in (q, k, v))
    so = F.scaled_dot_product_attention(
        *(t.transpose(1, 2) for t in (qs, ks, vs)),
        attn_mask=None if bias is None else bias.view(B, 1, 1, Sk),
        is_causal=form == "causal").transpose(1, 2)
    so.backward(do)
    torch.testing.assert_close(o, so.detach())
    for g, sg in zip(ref_grads(q, k, v, do, form == "causal", bias), (qs.grad, ks.grad, vs.grad)):
        torch.testing.assert_close(g, sg)
    # lse = log2 of the softmax denominator, written out in fp64
    s = torch.einsum("bqhd,bkhd->bhqk", q.double(), k.double()) / math.sqrt(D)
    if bias is not None:
        s = s + bias.double().view(B, 1, 1, Sk)
    if form == "causal":
        s = s + torch.full((Sq, Sk), NEG, dtype=torch.float64).triu(1)
    torch.testing.assert_close(lse, s.exp().sum(-1).log2().float())


@pytest.mark.parametrize("Sq,Sk", LENGTHS)
def test_fully_masked_batch_element(Sq, Sk):
    q, k, v, do = _inputs(Sq, Sk)
    bias = _key_bias(Sk)
    bias[1] = NEG
    o, lse, dead = ref_attention(q, k, v, bias=bias)
    assert dead[1].all() and not dead[0].any()
    assert (o[1] == 0).all() and (lse[1] == NEG).all()
    assert torch.isfinite(o).all() and torch.isfinite(lse[0]).all()
    grads = ref_grads(q, k, v, do, bias=bias)
    for g in grads:
        assert torch.isfinite(g).all() and (g[1] == 0).all()
    assert all(g[0].abs().max() > 0 for g in grads)


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_keep_mask_forms_agree(p):
    """keep_mask and the hash_bytes(..., SK=) >= thr8 form the reference uses are one mask
    at equal lengths, and the reference applies it to the softmax."""
    S, seed = 9, 4321
    keep, scale = dropout_hash.keep_mask(B, H, S, seed, p)
    t = dropout_hash.thr8(p)
    assert torch.equal(keep, dropout_hash.hash_bytes(B, H, S, seed, SK=S) >= t)
    assert scale == 256.0 / (256 - t)
    assert 0 < keep.sum() < keep.numel()
    q, k, v, _ = _inputs(S, S)
    o, _, _ = ref_attention(q, k, v, p=p, seed=seed)
    pr = torch.softmax(torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D), -1)
    torch.testing.assert_close(o, torch.einsum("bhqk,bkhd->bqhd", pr * keep * scale, v))
