"""fp32 reference of the fused attention kernels (csrc/hip/attention.hip) and the small
helpers around it, shared by tests/test_attention_gpu.py, tests/test_attention_mask_gpu.py
and tests/test_attention_cross_gpu.py (the kernels match it) and tests/test_attn_ref_cpu.py
(the reference is right).

``ref_attention`` writes the kernels' definition out in plain torch ops: [Sq, Sk] scores
q k^T / sqrt(D), an additive per-batch key bias, the causal mask at equal lengths, a softmax
whose fully masked rows are zero (o = 0, lse = -inf, finite zero gradients - not NaN), and
dropout by the kernels' own keep mask (tests/dropout_hash.py), the kept probabilities
scaled by 256 / (256 - thr8)."""
import math

import torch
import torch.nn.functional as F

import dropout_hash

DEV = "cuda"
NEG = float("-inf")


def _C():
    from apex_example_amd import _native

    return _native.require().attn


def ref_attention(q, k, v, causal=False, bias=None, p=0.0, seed=0):
    """fp32 reference on q [B, Sq, H, D], k / v [B, Sk, H, D] and an additive [B, Sk] key
    bias -> (o [B, Sq, H, D], lse [B, H, Sq] log2, dead [B, H, Sq]: rows with no live
    key).  ``causal`` needs Sq == Sk."""
    B, Sq, H, D = q.shape
    Sk = k.size(1)
    qf, kf, vf = (t.float().permute(0, 2, 1, 3) for t in (q, k, v))
    s = qf @ kf.transpose(-1, -2) / math.sqrt(D)
    if bias is not None:
        s = s + bias.float().view(B, 1, 1, Sk)
    if causal:
        assert Sq == Sk, "the causal mask is defined for equal lengths only"
        s = s.masked_fill(torch.ones(Sq, Sk, device=q.device).triu(1).bool(), NEG)
    dead = (s == NEG).all(-1, keepdim=True)
    lse = torch.logsumexp(s, -1) / math.log(2.0)
    pr = torch.softmax(torch.where(dead, torch.zeros_like(s), s), -1)
    pr = torch.where(dead, torch.zeros_like(pr), pr)  # fully masked rows: p = 0, finite grads
    if p > 0:
        # the mask mirror runs where the scores are (production shapes: 134 M entries)
        t = dropout_hash.thr8(p)
        keep = dropout_hash.hash_bytes(B, H, Sq, seed, SK=Sk, device=q.device) >= t
        pr = pr * keep * (256.0 / (256 - t))
    return (pr @ vf).permute(0, 2, 1, 3), lse, dead.squeeze(-1)


def ref_grads(q, k, v, do, causal=False, bias=None, p=0.0, seed=0):
    """The reference's (dq, dk, dv) for the output gradient ``do``, in fp32."""
    qf, kf, vf = (t.detach().float().clone().requires_grad_(True) for t in (q, k, v))
    o, _, _ = ref_attention(qf, kf, vf, causal, bias, p=p, seed=seed)
    o.backward(do.float())
    return qf.grad, kf.grad, vf.grad


def close(a, b, rel, what="", floor=0.0):
    """max |a - b| / max |b| < rel.  ``floor``: a lower limit of the denominator, for a
    reference that is identically zero (see test_cross_fwd_bwd)."""
    err = (a.float() - b).abs().max().item()
    scale = max(b.abs().max().item(), floor) + 1e-6
    print("%s max err %.3e / max magnitude %.3e = %.3e (bound %.1e)" % (
        what, err, scale, err / scale, rel))
    assert err / scale < rel, (what, err, scale)


def finite(*ts):
    for t in ts:
        assert torch.isfinite(t.float()).all()


def mask_kwargs(bias, boolean):
    """An additive [B, Sk] bias (CPU) as the mask argument of the fused entry points:
    key_padding_mask where it is a boolean one (bias in {0, -inf}), else key_bias."""
    if boolean:
        return {"key_padding_mask": (bias == NEG).to(DEV)}
    return {"key_bias": bias.to(DEV)}


def no_sdpa(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("F.scaled_dot_product_attention was called")

    monkeypatch.setattr(F, "scaled_dot_product_attention", boom)
