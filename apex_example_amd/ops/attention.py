"""Fused multi-head attention (head dim 64, bf16 / fp16) on the gfx950 MFMA
kernels of csrc/hip/attention.hip: flash-attention style forward (online
softmax, never materialises the S x S scores) and backward (dK/dV and dQ
kernels recomputing P from the saved log-sum-exp; no atomics, so gradients are
bitwise reproducible), with an optional causal mask and dropout whose keep
mask is a counter-based hash of (seed, batch*head, query, key) regenerated
exactly by the backward.

``fused_attention_qkv(qkv)`` takes the packed [B, S, 3, H, 64] output of a
fused QKV projection and returns o as [B, S, H, 64] (``.view(B, S, H*64)`` is
free); its backward writes dQ/dK/dV straight into ONE packed buffer, so the
projection's input gradient needs no concatenation.  Layout-generic views
([S, B, ...] sequence-first included) work: the kernels take strides.

Cross-attention: q may be [B, Sq, H, 64] against k / v of another length
[B, Sk, H, 64] (``fused_attention``), and ``fused_attention_kv(q, kv)`` takes the packed
[B, Sk, 2, H, 64] output of a fused KV projection, its backward writing dK/dV into ONE
packed buffer of kv's layout.  The causal mask is defined for Sq == Sk only.

Key masks: ``key_padding_mask`` ([B, S] bool with S the KEY length, True = masked key,
Apex's convention) or ``key_bias`` ([B, S] float, added to the scaled scores, ``-inf``
allowed) mask keys per batch element inside the kernels.  ``prepare_key_mask`` turns either into the
form the kernels read (an fp32 bias row in log2 units plus one liveness byte per
64-key tile) in one launch without a host sync; pass the returned ``PreparedKeyMask``
in place of the mask to share it between the layers of a model.  64-key tiles whose
keys are all masked are skipped (no loads, no math) wherever they lie, masked keys
get exactly zero dK / dV, and a query whose keys are all masked gets o = 0 and
dq = 0 (its lse is unspecified) instead of NaN.

Packed variable-length sequences: ``fused_attention_varlen(q, k, v, cu_seqlens)`` takes
[T, H, 64] views holding only the real tokens of B sequences, sequence b owning rows
``cu_seqlens[b] .. cu_seqlens[b+1]-1`` (int32 [B + 1] on the GPU, read by the kernels), and
attends within each sequence (``causal`` per sequence): no padded query, key or token-wise
work around the attention.  ``fused_attention_varlen_qkv`` takes the packed [T, 3, H, 64]
output of a fused QKV projection and returns one dqkv of its layout.  The results are
those of the padded call with a key-padding mask, read at the real rows; not combined
with key masks or unequal query / key lengths.

Eligibility (``supported``): GPU tensor, bf16/fp16, head dim 64, q and k / v of one
batch size and head count (the query and key lengths may differ), no mask other than
a per-batch key mask (a [Tq, Tk] ``attn_mask`` is not fused) or, at equal lengths, the
causal mask; packed sequences ([T, H, 64] with ``cu_seqlens``): q, k and v of one token
and head count, self-attention per sequence, optional causal mask, no key mask.  Callers
fall back to ``F.scaled_dot_product_attention`` otherwise.
"""
from __future__ import annotations

import math

import torch

from .. import _native


def _C():
    return _native.require().attn


def supported(t: torch.Tensor, head_dim: int) -> bool:
    return (t.is_cuda and head_dim == 64 and t.dtype in (torch.bfloat16, torch.float16)
            and _native.available())


_WARNED = set()


def effective_dropout(p: float) -> float:
    """The dropout rate the kernels apply for a requested ``p``: one hash byte per
    (query, key) is compared with round(256 p), so the rate is a multiple of 1/256
    (p = 0.1 runs at 26/256 = 0.1016), and any p > 0 drops at least 1/256."""
    if p <= 0.0:
        return 0.0
    return min(256, max(1, int(p * 256.0 + 0.5))) / 256.0


def _check_rate(p: float) -> None:
    """Warn (once per rate) where the 1/256 quantisation moves the rate by more than 2 %."""
    q = effective_dropout(p)
    if p > 0.0 and abs(q - p) > 0.02 * p and p not in _WARNED:
        import warnings

        _WARNED.add(p)
        warnings.warn("fused attention: dropout p=%g runs at %g (the kernels quantise the rate "
                      "to 1/256)" % (p, q))


def _seed(dropout_p: float) -> int:
    """Per-call dropout seed from torch's CPU generator (no device sync; follows
    torch.manual_seed)."""
    if dropout_p <= 0.0:
        return 0
    _check_rate(dropout_p)
    return int(torch.randint(0, 2 ** 31 - 1, (1,)).item())


class PreparedKeyMask:
    """A [B, S] key mask in the form the kernels read (``prepare_key_mask``):
    ``bias`` fp32 [B, round_up(S, 64)] in log2 units (-inf = masked, -inf past S) and
    ``live`` uint8 [B, round_up(S, 64) / 64] (0 = every key of the 64-key tile masked)."""

    __slots__ = ("bias", "live", "B", "S")

    def __init__(self, bias, live, B, S):
        self.bias, self.live, self.B, self.S = bias, live, B, S


def prepare_key_mask(mask: torch.Tensor) -> PreparedKeyMask:
    """mask [B, S] on the GPU: bool / uint8 (True / non-zero = masked key) or floating
    (additive, added to the scaled scores; -inf masks).  One kernel launch, no host sync
    (graph-capture safe).  The result serves every fused attention call with the same
    (B, S), forward and backward."""
    if not isinstance(mask, torch.Tensor) or mask.dim() != 2:
        raise ValueError("key mask must be a [B, S] tensor, got %s" % (
            tuple(mask.shape) if isinstance(mask, torch.Tensor) else type(mask).__name__))
    if not mask.is_cuda:
        raise ValueError("key mask must be on the GPU, got a %s tensor" % mask.device)
    B, S = mask.shape
    bias, live = _C().prepare_key_mask(mask.detach().contiguous(), S)
    return PreparedKeyMask(bias, live, B, S)


def _key_mask(key_padding_mask, key_bias, like):
    """The (bias, live) pair of a call's mask arguments for the keys ``like``
    [B, S, ...] (k, or a packed qkv / kv whose dim 1 is the key length; ``q`` in the
    messages), or (None, None)."""
    if key_padding_mask is None and key_bias is None:
        return None, None
    if key_padding_mask is not None and key_bias is not None:
        raise ValueError("give key_padding_mask (boolean) or key_bias (additive), not both")
    B, S = like.size(0), like.size(1)
    m = key_padding_mask if key_bias is None else key_bias
    if not isinstance(m, PreparedKeyMask):
        if key_bias is None and m.dtype not in (torch.bool, torch.uint8):
            raise ValueError("key_padding_mask must be bool (True = masked key), got %s; an "
                             "additive mask goes to key_bias" % m.dtype)
        if key_bias is not None and not m.is_floating_point():
            raise ValueError("key_bias must be a floating additive mask, got %s" % m.dtype)
        if tuple(m.shape) != (B, S):
            raise ValueError("key mask must be [B, S] = [%d, %d], got %s" % (B, S, tuple(m.shape)))
        if m.device != like.device:
            raise ValueError("key mask is on %s, q on %s" % (m.device, like.device))
        m = prepare_key_mask(m)
    if (m.B, m.S) != (B, S):
        raise ValueError("prepared key mask is for [B, S] = [%d, %d], the call's keys are "
                         "[%d, %d]" % (m.B, m.S, B, S))
    if m.bias.device != like.device:
        raise ValueError("key mask is on %s, q on %s" % (m.bias.device, like.device))
    return m.bias, m.live


def _check_causal(causal, Sq, Sk):
    if causal and Sq != Sk:
        raise ValueError("causal attention needs equal query and key lengths, got Sq = %d, "
                         "Sk = %d" % (Sq, Sk))


# How a call's tensor inputs split into the q [B, Sq, H, 64] and k, v [B, Sk, H, 64] views
# the kernels take (packed variable-length layouts: [T, H, 64] views); the gradient
# buffers, one per input, split the same way.
_SPLIT = {
    "qkv": lambda ts: ts,                                # q, k, v
    "packed_qkv": lambda ts: ts[0].unbind(2),            # qkv [B, S, 3, H, 64]
    "q_packed_kv": lambda ts: (ts[0], *ts[1].unbind(2)),  # q, kv [B, Sk, 2, H, 64]
    "varlen_qkv": lambda ts: ts,                         # q, k, v [T, H, 64]
    "varlen_packed_qkv": lambda ts: ts[0].unbind(1),     # qkv [T, 3, H, 64]
}


class AttentionFunction(torch.autograd.Function):
    """o = softmax(q k^T * scale [+ key bias] [+ causal mask]) [dropout] v -> [B, Sq, H, 64]
    on the q / k / v views of ``inputs`` (any strides) under ``layout``, a key of ``_SPLIT``;
    (kbias, klive) is a prepared key mask of the Sk keys or (None, None).  ``varlen`` is
    None or, with the "varlen_*" layouts ([T, H, 64] views of packed sequences, o
    [T, H, 64]), the pair (cu_seqlens int32 [B + 1], max_seqlen); it rides in ``ctx``
    outside autograd's saved tensors, so a captured graph may be replayed on new offsets
    written into the same tensor.  The backward
    returns one gradient per input: packed inputs (and the q beside a packed kv: a
    time-first projection gets its gradient back as a view, no transpose copy) get theirs
    in their own layout, separate q, k, v dense ones."""

    @staticmethod
    def forward(ctx, layout, causal, dropout_p, scale, seed, kbias, klive, varlen, *inputs):
        q, k, v = _SPLIT[layout](inputs)
        ctx.cfg = (layout, bool(causal), float(dropout_p), int(seed), float(scale))
        ctx.varlen = varlen
        if varlen is None:
            o, lse = _C().fwd(q, k, v, *ctx.cfg[1:], kbias, klive)
        else:
            o, lse = _C().fwd_varlen(q, k, v, *varlen, *ctx.cfg[1:])
        ctx.save_for_backward(*inputs, o, lse, kbias, klive)
        return o

    @staticmethod
    def backward(ctx, do):
        *inputs, o, lse, kbias, klive = ctx.saved_tensors
        layout, *cfg = ctx.cfg
        if layout in ("qkv", "varlen_qkv"):
            grads = [torch.empty_like(t, memory_format=torch.contiguous_format) for t in inputs]
        else:
            grads = [torch.empty_like(t) for t in inputs]
        if ctx.varlen is None:
            _C().bwd(do, *_SPLIT[layout](inputs), o, lse, *cfg, *_SPLIT[layout](grads), kbias,
                     klive)
        else:
            _C().bwd_varlen(do, *_SPLIT[layout](inputs), o, lse, *ctx.varlen, *cfg,
                            *_SPLIT[layout](grads))
        return (None,) * 8 + tuple(grads)


# The per-layout names, each ``.apply`` in its own argument order.
class FusedAttentionFunction:
    @staticmethod
    def apply(q, k, v, causal, dropout_p, scale, seed, kbias=None, klive=None):
        return AttentionFunction.apply("qkv", causal, dropout_p, scale, seed, kbias, klive,
                                       None, q, k, v)


class FusedQKVAttentionFunction:
    @staticmethod
    def apply(qkv, causal, dropout_p, scale, seed, kbias=None, klive=None):
        return AttentionFunction.apply("packed_qkv", causal, dropout_p, scale, seed, kbias,
                                       klive, None, qkv)


class FusedKVAttentionFunction:
    @staticmethod
    def apply(q, kv, dropout_p, scale, seed, kbias=None, klive=None):
        return AttentionFunction.apply("q_packed_kv", False, dropout_p, scale, seed, kbias,
                                       klive, None, q, kv)


def fused_attention(q, k, v, causal=False, dropout_p=0.0, scale=None, key_padding_mask=None,
                    key_bias=None):
    """q: [B, Sq, H, 64], k, v: [B, Sk, H, 64] -> o [B, Sq, H, 64] (Sq != Sk is
    cross-attention; ``causal`` needs Sq == Sk).  key_padding_mask: [B, Sk] bool, True =
    masked key; key_bias: [B, Sk] float, added to the scaled scores; either may be a
    ``PreparedKeyMask``."""
    _check_causal(causal, q.size(1), k.size(1))
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    kbias, klive = _key_mask(key_padding_mask, key_bias, k)
    return FusedAttentionFunction.apply(q, k, v, causal, dropout_p, scale, _seed(dropout_p),
                                        kbias, klive)


def fused_attention_kv(q, kv, dropout_p=0.0, scale=None, key_padding_mask=None, key_bias=None):
    """q: [B, Sq, H, 64], kv: [B, Sk, 2, H, 64] (the packed output of a fused KV
    projection, any strides) -> o [B, Sq, H, 64]; the backward writes dK and dV into one
    packed dkv of kv's layout.  Masks are [B, Sk], as in ``fused_attention``."""
    if kv.dim() != 5 or kv.size(2) != 2:
        raise ValueError("kv must be [B, Sk, 2, H, 64], got %s" % (tuple(kv.shape),))
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    kbias, klive = _key_mask(key_padding_mask, key_bias, kv)
    return FusedKVAttentionFunction.apply(q, kv, dropout_p, scale, _seed(dropout_p),
                                          kbias, klive)


def fused_attention_qkv(qkv, causal=False, dropout_p=0.0, scale=None, key_padding_mask=None,
                        key_bias=None):
    """qkv: [B, S, 3, H, 64] (any strides) -> o [B, S, H, 64]; the backward returns one
    packed dqkv of qkv's layout.  Masks as in ``fused_attention``."""
    scale = 1.0 / math.sqrt(qkv.size(-1)) if scale is None else scale
    kbias, klive = _key_mask(key_padding_mask, key_bias, qkv)
    return FusedQKVAttentionFunction.apply(qkv, causal, dropout_p, scale, _seed(dropout_p),
                                           kbias, klive)


def _varlen(cu_seqlens, max_seqlen, like, key_padding_mask, key_bias):
    """The (cu_seqlens, max_seqlen) pair of a packed call on ``like`` ([T, ...]) after the
    checks that need no look at the offsets' values - and, with max_seqlen=None, the one
    host copy that computes it and checks them."""
    if key_padding_mask is not None or key_bias is not None:
        raise ValueError("key masks are not combined with packed sequences (cu_seqlens): the "
                         "offsets already keep every sequence to itself")
    if not isinstance(cu_seqlens, torch.Tensor) or cu_seqlens.dim() != 1 or \
            cu_seqlens.numel() < 1:
        raise ValueError("cu_seqlens must be a 1-D int32 tensor of B + 1 offsets")
    if cu_seqlens.dtype != torch.int32:
        raise ValueError("cu_seqlens must be int32, got %s" % cu_seqlens.dtype)
    if cu_seqlens.device != like.device:
        raise ValueError("cu_seqlens is on %s, q on %s" % (cu_seqlens.device, like.device))
    cu_seqlens = cu_seqlens.detach().contiguous()
    T = like.size(0)
    if max_seqlen is None:
        cu = cu_seqlens.tolist()  # the host sync
        lens = [b - a for a, b in zip(cu, cu[1:])]
        if cu[0] != 0:
            raise ValueError("cu_seqlens must start at 0, got %d" % cu[0])
        if any(n < 0 for n in lens):
            raise ValueError("cu_seqlens must be non-decreasing")
        if cu[-1] != T:
            raise ValueError("cu_seqlens must end at T = %d tokens, got %d" % (T, cu[-1]))
        max_seqlen = max(lens + [1])
    max_seqlen = int(max_seqlen)
    if max_seqlen <= 0:
        raise ValueError("max_seqlen must be positive, got %d" % max_seqlen)
    return cu_seqlens, max_seqlen


def fused_attention_varlen(q, k, v, cu_seqlens, max_seqlen=None, causal=False, dropout_p=0.0,
                           scale=None, key_padding_mask=None, key_bias=None):
    """Attention over packed variable-length sequences.  q, k, v: [T, H, 64] views (any
    token / head strides) of the real tokens of B sequences; cu_seqlens: int32 [B + 1] on
    the GPU, non-decreasing from 0 to T: sequence b owns rows cu[b] .. cu[b+1]-1, and its
    queries see its own keys only (``causal``: key j <= query i, indices local to the
    sequence).  -> o [T, H, 64], equal to the padded call with a key-padding mask read at
    the real rows (same dropout mask for the same seed).  Empty sequences are legal.

    max_seqlen=None: computed from cu_seqlens with ONE host sync, which also checks the
    offsets (ValueError).  max_seqlen given (any value >= the longest sequence; the results
    do not depend on it): no sync, so the call is graph-capture safe and a captured graph
    may be replayed on other offsets written into the same tensor - but cu_seqlens is then
    TRUSTED, and a max_seqlen below a sequence's length silently drops the tail of that
    sequence (its rows past max_seqlen are neither attended to nor written; rows of o and
    of the gradients that are not written are unspecified).

    Key masks are not combined with packing (ValueError)."""
    cu_seqlens, max_seqlen = _varlen(cu_seqlens, max_seqlen, q, key_padding_mask, key_bias)
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    return AttentionFunction.apply("varlen_qkv", causal, dropout_p, scale, _seed(dropout_p),
                                   None, None, (cu_seqlens, max_seqlen), q, k, v)


def fused_attention_varlen_qkv(qkv, cu_seqlens, max_seqlen=None, causal=False, dropout_p=0.0,
                               scale=None, key_padding_mask=None, key_bias=None):
    """qkv: [T, 3, H, 64] (the packed output of a fused QKV projection over packed
    sequences, any strides) -> o [T, H, 64]; the backward returns one packed dqkv of qkv's
    layout.  cu_seqlens / max_seqlen as in ``fused_attention_varlen``."""
    if qkv.dim() != 4 or qkv.size(1) != 3:
        raise ValueError("qkv must be [T, 3, H, 64], got %s" % (tuple(qkv.shape),))
    cu_seqlens, max_seqlen = _varlen(cu_seqlens, max_seqlen, qkv, key_padding_mask, key_bias)
    scale = 1.0 / math.sqrt(qkv.size(-1)) if scale is None else scale
    return AttentionFunction.apply("varlen_packed_qkv", causal, dropout_p, scale,
                                   _seed(dropout_p), None, None, (cu_seqlens, max_seqlen), qkv)
