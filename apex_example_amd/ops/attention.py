"""Fused multi-head attention (head dim D = 64 or 128, bf16 / fp16) on the gfx950 MFMA
kernels of csrc/hip/attention.hip (D = 64) and csrc/hip/attention_d128.hip (D = 128):
flash-attention style forward (online softmax, never materialises the S x S scores) and backward (dK/dV and dQ
kernels recomputing P from the saved log-sum-exp; no atomics, so gradients are
bitwise reproducible), with an optional causal mask and dropout whose keep
mask is a counter-based hash of (seed, batch*head, query, key) regenerated
exactly by the backward.

``fused_attention_qkv(qkv)`` takes the packed [B, S, 3, H, D] output of a
fused QKV projection and returns o as [B, S, H, D] (``.view(B, S, H*D)`` is
free); its backward writes dQ/dK/dV straight into ONE packed buffer, so the
projection's input gradient needs no concatenation.  Layout-generic views
([S, B, ...] sequence-first included) work: the kernels take strides.

Cross-attention: q may be [B, Sq, H, D] against k / v of another length
[B, Sk, H, D] (``fused_attention``), and ``fused_attention_kv(q, kv)`` takes the packed
[B, Sk, 2, H, D] output of a fused KV projection, its backward writing dK/dV into ONE
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

Pair masks: ``attn_mask`` is a boolean [Sq, Sk] or [B, Sq, Sk] tensor, True = masked pair
(Apex's time mask; sliding windows, block-diagonal document masks, prefix-LM, causal plus
padding).  ``prepare_attn_mask`` packs it into bit tiles in one launch without a host sync
(csrc/hip/attention_pairmask.hip): one 64-bit word per (query, 64-key tile) for the forward
and dQ kernels, its transpose for dK/dV, and a class byte per tile, so that tiles with no
attended pair are skipped wherever they lie, tiles where every pair attends run the
mask-free math and only mixed tiles test bits.  A boolean ``key_padding_mask`` is OR-ed in
by the prepare step; pass the returned ``PreparedAttnMask`` in place of the tensor to share
it between layers.  Fully masked queries and keys behave as under a key mask.  It excludes
``causal`` (put the triangle in the mask) and ``key_bias`` (an additive bias beside a pair
mask stays on SDPA).  Timings against SDPA with the same mask and against the causal
kernel: docs/PERF.md, "Attention: boolean pair masks".

Packed variable-length sequences: ``fused_attention_varlen(q, k, v, cu_seqlens)`` takes
[T, H, D] views holding only the real tokens of B sequences, sequence b owning rows
``cu_seqlens[b] .. cu_seqlens[b+1]-1`` (int32 [B + 1] on the GPU, read by the kernels), and
attends within each sequence (``causal`` per sequence): no padded query, key or token-wise
work around the attention.  ``fused_attention_varlen_qkv`` takes the packed [T, 3, H, D]
output of a fused QKV projection and returns one dqkv of its layout.  The results are
those of the padded call with a key-padding mask, read at the real rows; not combined
with key masks or unequal query / key lengths.

Grouped-query and multi-query heads: k and v (and a packed kv) may have Hkv < H heads with
H % Hkv == 0; query head h reads key/value head h // (H // Hkv) (torch's ``enable_gqa``,
the Llama / Megatron layout), without expanding K / V: the dK/dV kernel walks the query heads
of a group and writes each dK / dV row once (csrc/hip/attention_gqa.hip).
``fused_attention_qkv_gqa(qkv, num_kv_heads)`` takes the [B, S, H + 2 Hkv, D] output of one
fused projection (query heads, then key heads, then value heads) and returns one dqkv of
that layout.  The dropout mask is that of the same call on K / V expanded to H heads.  Not
combined with ``attn_mask`` or packed sequences (ValueError).  docs/PERF.md, "Attention:
grouped-query heads".

Decode over a KV cache: ``fused_attention_decode(q, k_cache, v_cache, cache_seqlens)`` attends
the Sq newest tokens q [B, Sq, H, D] (Sq of 1 to a few) to the keys of [B, Smax, Hkv, D] cache
views (any strides: the halves of one packed [B, Smax, 2, Hkv, D] buffer), of which
``cache_seqlens`` (int32 [B] on the GPU, read by the kernels only: no host sync, graph-capture
safe, a captured graph may be replayed after ``cache_seqlens += Sq``) says how many rows are
filled.  With ``k_new`` / ``v_new`` the new rows are first appended behind them.  The mask is
causal and aligned bottom-right (query i sees keys j <= L_b - Sq + i), rows at or past L_b are
never read, a query that sees no key gets o = 0 and lse = -inf.  Forward only: no dropout,
no key or pair mask, no gradient.  Its kernels (csrc/hip/attention_decode.hip) are not the
training forward: the G query heads of a group times the Sq tokens fill one MFMA tile so K / V
are read once per group, the four waves of a workgroup and ``num_splits`` workgroups split
the keys, and a second launch joins the splits in a fixed order (bitwise reproducible for a
given ``num_splits``).  docs/PERF.md, "Attention: decode over a KV cache".

Paged KV cache: with ``block_table`` (int32 [B, max_pages] on the GPU) the caches of
``fused_attention_decode`` are [num_pages, P, Hkv, D] page views of one pool (any strides: the
halves of a packed [num_pages, P, 2, Hkv, D] pool; P in 16, 32, 64, 128, 256) and key j of
batch element b is row j % P of page ``block_table[b][j // P]``, so memory follows the tokens
held and sequences of any lengths share the pool.  The kernels (csrc/hip/
attention_decode_paged.hip) walk the table in scalar registers one tile ahead of the K / V
DMA; table entries at or past ceil(L_b / P) are never read, page ids are clamped to the pool,
and a captured graph may be replayed after table entries are rewritten in place.  The work
split is the contiguous kernels': for a given ``num_splits`` the result is bitwise that of the
contiguous call on the same keys.  ``paged_kv_append`` stores new rows (a whole prompt at
prefill) through the table on its own.  docs/PERF.md, "Attention: decode over a paged KV cache".

FP8 KV cache: with ``torch.float8_e4m3fn`` caches and ``k_scale`` / ``v_scale`` (fp32 [B, Hkv,
Smax], one scale per batch element, key/value head and key) ``fused_attention_decode`` reads
half the K / V bytes: key j of head hk is ``k_cache[b, j, hk].float() * k_scale[b, hk, j]``.
q, o and the new rows stay bf16 / fp16 and so do the MFMAs; the kernels (csrc/hip/
attention_decode_fp8.hip) turn the bytes into 16-bit fragments in registers (exact) and apply
the scales to the scores and to p, so quantisation is the only error the format adds.
``k_new`` / ``v_new`` are quantised per row by the append kernel (scale = amax / 448), as
``fp8_kv_append`` does on its own and ``fp8_quantize_rows`` mirrors in torch bit for bit.  Not
paged yet.  docs/PERF.md, "Attention: decode over an FP8 KV cache".

Chunked prefill over a KV cache: ``fused_attention_prefill(q, k_cache, v_cache, cache_seqlens)``
is the decode call for many new tokens (a later chunk of a long prompt, the next turn of a
conversation, a prompt behind a shared prefix) over a contiguous bf16 / fp16 cache: the same
tensors, lengths on the device, bottom-right mask, clip and ``k_new`` / ``v_new`` append, but
kernels (csrc/hip/attention_prefill.hip) that split the rows instead of the keys: the G * Sq rows
of a key/value head's group in token order, 128 per workgroup, every 64-key K / V tile shared by
four waves through LDS, each workgroup's key loop ending at the last key its tokens see.  One
launch, no ``num_splits``, bitwise reproducible.  It wins where the row tiles fill the device
and loses to decode's split-KV where they do not (B = 1 with a few hundred rows): docs/PERF.md,
"Attention: chunked prefill over a KV cache".  With float8_e4m3fn caches and ``k_scale`` /
``v_scale`` the same call runs the FP8 variant of those kernels (csrc/hip/
attention_prefill_fp8.hip): the row split and causal skipping above over shared 64-key byte
tiles (half the LDS), the bytes converted in registers and the scales applied as in FP8 decode,
the new rows quantised by the same append; docs/PERF.md, "Attention: chunked prefill over an FP8
KV cache".  Paged caches are refused here, 16-bit or FP8.

Eligibility (``supported``): GPU tensor, bf16/fp16, head dim 64 or 128, q and k / v of one
batch size (the query and key lengths may differ) and H query heads over Hkv key/value heads
with H % Hkv == 0 (Hkv < H neither with a pair mask nor packed), no mask other than
a per-batch key mask, a boolean pair mask (an additive [Tq, Tk] ``attn_mask`` is not
fused) or, at equal lengths, the causal mask; packed sequences ([T, H, D] with ``cu_seqlens``): q, k and v of one token
and head count, self-attention per sequence, optional causal mask, no key mask.  A decode
step over a KV cache (``fused_attention_decode``) takes the same dtypes, head dims and head
groupings, forward only, over a contiguous cache or, with ``block_table``, over pages of
16 to 256 rows; a contiguous cache may instead be float8_e4m3fn with fp32 per-row scales (q
still bf16 / fp16).  Callers
fall back to ``F.scaled_dot_product_attention`` otherwise.
"""
from __future__ import annotations

import math

import torch

from .. import _native


def _C():
    return _native.require().attn


HEAD_DIMS = (64, 128)  # the head dims that have kernels


def supported(t: torch.Tensor, head_dim: int) -> bool:
    return (t.is_cuda and head_dim in HEAD_DIMS and t.dtype in (torch.bfloat16, torch.float16)
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


class PreparedAttnMask:
    """A boolean pair mask as the bit tiles the kernels read (``prepare_attn_mask``), set
    bit = attend, Bm = 1 (``B`` None: shared by the batch) or B:
    ``wq`` uint64 [Bm, ceil(Sq/128), ceil(Sk/64), 128] (a query's 64 keys per word) with the
    tile classes ``cq`` uint8 [Bm, ceil(Sq/128), ceil(Sk/64)] (0 dead, 1 mixed, 2 full), and
    the transpose ``wk`` [Bm, ceil(Sk/128), ceil(Sq/64), 128], ``ck`` for dK/dV."""

    __slots__ = ("wq", "cq", "wk", "ck", "B", "Sq", "Sk")

    def __init__(self, wq, cq, wk, ck, B, Sq, Sk):
        self.wq, self.cq, self.wk, self.ck, self.B, self.Sq, self.Sk = wq, cq, wk, ck, B, Sq, Sk


def _bool_mask(m, what, dims, shape_text):
    if not isinstance(m, torch.Tensor) or m.dim() not in dims:
        raise ValueError("%s must be a %s tensor, got %s" % (
            what, shape_text, tuple(m.shape) if isinstance(m, torch.Tensor) else type(m).__name__))
    if m.dtype not in (torch.bool, torch.uint8):
        raise ValueError("%s must be bool (True = masked), got %s" % (what, m.dtype))
    if not m.is_cuda:
        raise ValueError("%s must be on the GPU, got a %s tensor" % (what, m.device))
    return m.detach().contiguous()


def prepare_attn_mask(attn_mask: torch.Tensor, key_padding_mask=None) -> PreparedAttnMask:
    """attn_mask: bool / uint8 [Sq, Sk] or [B, Sq, Sk] on the GPU, True / non-zero = masked
    pair; key_padding_mask: optional bool [B, Sk], True = masked key, OR-ed in (the result
    is then per batch element).  One kernel launch, no host sync (graph-capture safe); the
    result serves every fused attention call of the same (B, Sq, Sk), forward and backward."""
    m = _bool_mask(attn_mask, "attn_mask", (2, 3), "[Sq, Sk] or [B, Sq, Sk]")
    Sq, Sk = m.shape[-2:]
    B = m.size(0) if m.dim() == 3 else None
    kp = None
    if key_padding_mask is not None:
        kp = _bool_mask(key_padding_mask, "key_padding_mask", (2,), "[B, Sk]")
        if kp.size(1) != Sk or (B is not None and kp.size(0) != B) or kp.device != m.device:
            raise ValueError("key_padding_mask %s on %s does not fit attn_mask %s on %s" % (
                tuple(kp.shape), kp.device, tuple(m.shape), m.device))
        B = kp.size(0)
    if Sq == 0 or Sk == 0:
        raise ValueError("attn_mask must have queries and keys, got %s" % (tuple(m.shape),))
    words, cls = _C().prepare_attn_mask(m, kp)
    Bm = 1 if B is None else B
    nq = (-(-Sq // 128), -(-Sk // 64))
    nk = (-(-Sk // 128), -(-Sq // 64))
    nwq, ncq = Bm * nq[0] * nq[1] * 128, Bm * nq[0] * nq[1]
    words = words.view(torch.uint64)
    return PreparedAttnMask(words[:nwq].view(Bm, *nq, 128), cls[:ncq].view(Bm, *nq),
                            words[nwq:].view(Bm, *nk, 128), cls[ncq:].view(Bm, *nk), B, Sq, Sk)


def _attn_mask(attn_mask, causal, key_padding_mask, key_bias, q, like):
    """The ``PreparedAttnMask`` of a call with ``attn_mask`` for the queries ``q``
    [B, Sq, ...] and the keys ``like`` [B, Sk, ...]."""
    if causal:
        raise ValueError("attn_mask excludes causal=True: put the triangle in the mask")
    if key_bias is not None:
        raise ValueError("attn_mask excludes key_bias: an additive bias beside a pair mask is "
                         "not fused")
    B, Sq, Sk = q.size(0), q.size(1), like.size(1)
    m = attn_mask
    if isinstance(m, PreparedAttnMask):
        if key_padding_mask is not None:
            raise ValueError("a PreparedAttnMask already holds its key_padding_mask")
    else:
        if not isinstance(m, torch.Tensor) or m.dim() not in (2, 3) or \
                tuple(m.shape[-2:]) != (Sq, Sk) or (m.dim() == 3 and m.size(0) != B):
            raise ValueError("attn_mask must be [Sq, Sk] = [%d, %d] or [B, Sq, Sk] with B = %d, "
                             "got %s" % (Sq, Sk, B, tuple(m.shape) if isinstance(m, torch.Tensor)
                                         else type(m).__name__))
        if isinstance(key_padding_mask, PreparedKeyMask):
            raise ValueError("attn_mask takes the boolean key_padding_mask tensor, not a "
                             "PreparedKeyMask")
        if key_padding_mask is not None and tuple(key_padding_mask.shape) != (B, Sk):
            raise ValueError("key mask must be [B, S] = [%d, %d], got %s" % (
                B, Sk, tuple(key_padding_mask.shape)))
        m = prepare_attn_mask(m, key_padding_mask)
    if (m.Sq, m.Sk) != (Sq, Sk) or m.B not in (None, B):
        raise ValueError("prepared attn_mask is for [B, Sq, Sk] = [%s, %d, %d], the call's is "
                         "[%d, %d, %d]" % (m.B, m.Sq, m.Sk, B, Sq, Sk))
    if m.wq.device != q.device:
        raise ValueError("attn_mask is on %s, q on %s" % (m.wq.device, q.device))
    return m


def _check_causal(causal, Sq, Sk):
    if causal and Sq != Sk:
        raise ValueError("causal attention needs equal query and key lengths, got Sq = %d, "
                         "Sk = %d" % (Sq, Sk))


# How a call's tensor inputs split into the q [B, Sq, H, D] and k, v [B, Sk, H, D] views
# the kernels take (packed variable-length layouts: [T, H, D] views); the gradient
# buffers, one per input, split the same way.
_SPLIT = {
    "qkv": lambda ts: ts,                                # q, k, v
    "packed_qkv": lambda ts: ts[0].unbind(2),            # qkv [B, S, 3, H, D]
    "q_packed_kv": lambda ts: (ts[0], *ts[1].unbind(2)),  # q, kv [B, Sk, 2, H, D]
    "varlen_qkv": lambda ts: ts,                         # q, k, v [T, H, D]
    "varlen_packed_qkv": lambda ts: ts[0].unbind(1),     # qkv [T, 3, H, D]
}


def _split(layout, ts):
    """The (q, k, v) views of the tensors ``ts`` under ``layout``: a key of ``_SPLIT`` or
    ("gqa_qkv", Hkv), one qkv [B, S, H + 2 Hkv, D] with the query heads first, then the key
    heads, then the value heads."""
    if isinstance(layout, tuple):
        hkv = layout[1]
        return ts[0].split((ts[0].size(2) - 2 * hkv, hkv, hkv), 2)
    return _SPLIT[layout](ts)


def _check_heads(q, k, excluded=None):
    """ValueError for H query heads that do not split over k's Hkv heads (dim -2 of both)
    or, with ``excluded`` naming an argument they are not combined with, for Hkv < H."""
    H, Hkv = q.size(-2), k.size(-2)
    if Hkv <= 0 or H % Hkv != 0:
        raise ValueError("%d query heads do not split over %d key/value heads" % (H, Hkv))
    if excluded is not None and Hkv != H:
        raise ValueError("grouped-query heads (H = %d, Hkv = %d) are not combined with %s: "
                         "expand k / v to H heads for that" % (H, Hkv, excluded))


class AttentionFunction(torch.autograd.Function):
    """o = softmax(q k^T * scale [+ key bias] [+ causal mask]) [dropout] v -> [B, Sq, H, D]
    on the q / k / v views of ``inputs`` (any strides) under ``layout`` (``_split``);
    (kbias, klive) is a prepared key mask of the Sk keys or (None, None).  ``varlen`` is
    None or, with the "varlen_*" layouts ([T, H, D] views of packed sequences, o
    [T, H, D]), the pair (cu_seqlens int32 [B + 1], max_seqlen); it rides in ``ctx``
    outside autograd's saved tensors, so a captured graph may be replayed on new offsets
    written into the same tensor.  The same slot takes a ``PreparedAttnMask`` instead (a
    pair mask: no causal flag, no key mask; it takes no gradient).  The backward
    returns one gradient per input: packed inputs (and the q beside a packed kv: a
    time-first projection gets its gradient back as a view, no transpose copy) get theirs
    in their own layout, separate q, k, v dense ones."""

    @staticmethod
    def forward(ctx, layout, causal, dropout_p, scale, seed, kbias, klive, varlen, *inputs):
        q, k, v = _split(layout, inputs)
        ctx.cfg = (layout, bool(causal), float(dropout_p), int(seed), float(scale))
        ctx.varlen = varlen
        if varlen is None:
            o, lse = _C().fwd(q, k, v, *ctx.cfg[1:], kbias, klive)
        elif isinstance(varlen, PreparedAttnMask):
            m = varlen
            o, lse = _C().fwd_amask(q, k, v, *ctx.cfg[2:], m.wq, m.cq, m.wk, m.ck)
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
            _C().bwd(do, *_split(layout, inputs), o, lse, *cfg, *_split(layout, grads), kbias,
                     klive)
        elif isinstance(ctx.varlen, PreparedAttnMask):
            m = ctx.varlen
            _C().bwd_amask(do, *_split(layout, inputs), o, lse, *cfg[1:],
                           *_split(layout, grads), m.wq, m.cq, m.wk, m.ck)
        else:
            _C().bwd_varlen(do, *_split(layout, inputs), o, lse, *ctx.varlen, *cfg,
                            *_split(layout, grads))
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
                    key_bias=None, attn_mask=None):
    """q: [B, Sq, H, D], k, v: [B, Sk, Hkv, D] -> o [B, Sq, H, D] (Sq != Sk is
    cross-attention; ``causal`` needs Sq == Sk; Hkv < H with H % Hkv == 0 is grouped-query
    attention, query head h reading key/value head h // (H // Hkv), not under ``attn_mask``).
    key_padding_mask: [B, Sk] bool, True =
    masked key; key_bias: [B, Sk] float, added to the scaled scores; either may be a
    ``PreparedKeyMask``.  attn_mask: bool [Sq, Sk] / [B, Sq, Sk], True = masked pair, or a
    ``PreparedAttnMask``; it excludes ``causal`` and ``key_bias`` and merges a boolean
    ``key_padding_mask``."""
    _check_causal(causal, q.size(1), k.size(1))
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    if attn_mask is not None:
        _check_heads(q, k, "attn_mask")
        m = _attn_mask(attn_mask, causal, key_padding_mask, key_bias, q, k)
        return AttentionFunction.apply("qkv", False, dropout_p, scale, _seed(dropout_p), None,
                                       None, m, q, k, v)
    kbias, klive = _key_mask(key_padding_mask, key_bias, k)
    return FusedAttentionFunction.apply(q, k, v, causal, dropout_p, scale, _seed(dropout_p),
                                        kbias, klive)


def fused_attention_kv(q, kv, dropout_p=0.0, scale=None, key_padding_mask=None, key_bias=None,
                       attn_mask=None):
    """q: [B, Sq, H, D], kv: [B, Sk, 2, Hkv, D] (the packed output of a fused KV
    projection, any strides) -> o [B, Sq, H, D]; the backward writes dK and dV into one
    packed dkv of kv's layout.  Masks and Hkv as in ``fused_attention``."""
    if kv.dim() != 5 or kv.size(2) != 2:
        raise ValueError("kv must be [B, Sk, 2, H, D], got %s" % (tuple(kv.shape),))
    if attn_mask is not None:
        _check_heads(q, kv, "attn_mask")
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    if attn_mask is not None:
        m = _attn_mask(attn_mask, False, key_padding_mask, key_bias, q, kv)
        return AttentionFunction.apply("q_packed_kv", False, dropout_p, scale, _seed(dropout_p),
                                       None, None, m, q, kv)
    kbias, klive = _key_mask(key_padding_mask, key_bias, kv)
    return FusedKVAttentionFunction.apply(q, kv, dropout_p, scale, _seed(dropout_p),
                                          kbias, klive)


def fused_attention_qkv(qkv, causal=False, dropout_p=0.0, scale=None, key_padding_mask=None,
                        key_bias=None, attn_mask=None):
    """qkv: [B, S, 3, H, D] (any strides) -> o [B, S, H, D]; the backward returns one
    packed dqkv of qkv's layout.  Masks as in ``fused_attention``."""
    scale = 1.0 / math.sqrt(qkv.size(-1)) if scale is None else scale
    if attn_mask is not None:
        m = _attn_mask(attn_mask, causal, key_padding_mask, key_bias, qkv, qkv)
        return AttentionFunction.apply("packed_qkv", False, dropout_p, scale, _seed(dropout_p),
                                       None, None, m, qkv)
    kbias, klive = _key_mask(key_padding_mask, key_bias, qkv)
    return FusedQKVAttentionFunction.apply(qkv, causal, dropout_p, scale, _seed(dropout_p),
                                           kbias, klive)


def fused_attention_qkv_gqa(qkv, num_kv_heads, causal=False, dropout_p=0.0, scale=None,
                            key_padding_mask=None, key_bias=None):
    """qkv: [B, S, H + 2 Hkv, D] with Hkv = ``num_kv_heads`` (the output of one fused
    projection: H query heads, then Hkv key heads, then Hkv value heads; any strides,
    sequence-first included) -> o [B, S, H, D]; query head h reads key/value head
    h // (H // Hkv).  The backward returns one packed dqkv of qkv's layout.  Key masks as in
    ``fused_attention``.  With Hkv == H the results are bitwise those of
    ``fused_attention_qkv`` on the same data."""
    hkv = int(num_kv_heads)
    if qkv.dim() != 4 or hkv <= 0 or qkv.size(2) <= 2 * hkv:
        raise ValueError("qkv must be [B, S, H + 2 * num_kv_heads, D] with num_kv_heads = %d > 0, "
                         "got %s" % (hkv, tuple(qkv.shape)))
    if (qkv.size(2) - 2 * hkv) % hkv != 0:
        raise ValueError("%d query heads do not split over %d key/value heads" % (
            qkv.size(2) - 2 * hkv, hkv))
    scale = 1.0 / math.sqrt(qkv.size(-1)) if scale is None else scale
    kbias, klive = _key_mask(key_padding_mask, key_bias, qkv)
    return AttentionFunction.apply(("gqa_qkv", hkv), causal, dropout_p, scale, _seed(dropout_p),
                                   kbias, klive, None, qkv)


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
    """Attention over packed variable-length sequences.  q, k, v: [T, H, D] views (any
    token / head strides) of the real tokens of B sequences; cu_seqlens: int32 [B + 1] on
    the GPU, non-decreasing from 0 to T: sequence b owns rows cu[b] .. cu[b+1]-1, and its
    queries see its own keys only (``causal``: key j <= query i, indices local to the
    sequence).  -> o [T, H, D], equal to the padded call with a key-padding mask read at
    the real rows (same dropout mask for the same seed).  Empty sequences are legal.

    max_seqlen=None: computed from cu_seqlens with ONE host sync, which also checks the
    offsets (ValueError).  max_seqlen given (any value >= the longest sequence; the results
    do not depend on it): no sync, so the call is graph-capture safe and a captured graph
    may be replayed on other offsets written into the same tensor - but cu_seqlens is then
    TRUSTED, and a max_seqlen below a sequence's length silently drops the tail of that
    sequence (its rows past max_seqlen are neither attended to nor written; rows of o and
    of the gradients that are not written are unspecified).

    Key masks are not combined with packing (ValueError)."""
    _check_heads(q, k, "packed sequences (cu_seqlens)")
    cu_seqlens, max_seqlen = _varlen(cu_seqlens, max_seqlen, q, key_padding_mask, key_bias)
    scale = 1.0 / math.sqrt(q.size(-1)) if scale is None else scale
    return AttentionFunction.apply("varlen_qkv", causal, dropout_p, scale, _seed(dropout_p),
                                   None, None, (cu_seqlens, max_seqlen), q, k, v)


def fused_attention_varlen_qkv(qkv, cu_seqlens, max_seqlen=None, causal=False, dropout_p=0.0,
                               scale=None, key_padding_mask=None, key_bias=None):
    """qkv: [T, 3, H, D] (the packed output of a fused QKV projection over packed
    sequences, any strides) -> o [T, H, D]; the backward returns one packed dqkv of qkv's
    layout.  cu_seqlens / max_seqlen as in ``fused_attention_varlen``."""
    if qkv.dim() != 4 or qkv.size(1) != 3:
        raise ValueError("qkv must be [T, 3, H, D], got %s" % (tuple(qkv.shape),))
    cu_seqlens, max_seqlen = _varlen(cu_seqlens, max_seqlen, qkv, key_padding_mask, key_bias)
    scale = 1.0 / math.sqrt(qkv.size(-1)) if scale is None else scale
    return AttentionFunction.apply("varlen_packed_qkv", causal, dropout_p, scale,
                                   _seed(dropout_p), None, None, (cu_seqlens, max_seqlen), qkv)


PAGE_SIZES = (16, 32, 64, 128, 256)  # the page sizes the paged decode kernels take


def _check_paged(first, k_pages, v_pages, block_table, cache_seqlens):
    """The pools, table and lengths of a paged call whose batch, dtype and device are those of
    ``first`` = (name, [B, S, heads, D] tensor); ValueError on anything the kernels refuse."""
    name0, t0 = first
    for name, t in (first, ("k_pages", k_pages), ("v_pages", v_pages)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError("%s must be a 4-d tensor, got %s" % (
                name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU, got a %s tensor" % (name, t.device))
        if t.device != t0.device or t.dtype != t0.dtype:
            raise ValueError("%s is %s on %s, %s %s on %s" % (name, t.dtype, t.device, name0,
                                                             t0.dtype, t0.device))
    if t0.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("decode takes bf16 / fp16 tensors, got %s" % t0.dtype)
    B, D = t0.size(0), t0.size(3)
    if D not in HEAD_DIMS:
        raise ValueError("head dim must be one of %s, got %d" % (HEAD_DIMS, D))
    if k_pages.shape != v_pages.shape or k_pages.size(3) != D:
        raise ValueError("k_pages and v_pages must be [num_pages, P, Hkv, D] with D = %d, got %s "
                         "and %s" % (D, tuple(k_pages.shape), tuple(v_pages.shape)))
    P = k_pages.size(1)
    if P not in PAGE_SIZES:
        raise ValueError("the page size must be one of %s, got %d" % (PAGE_SIZES, P))
    if k_pages.size(0) < 1:
        raise ValueError("the page pool is empty")
    if not isinstance(block_table, torch.Tensor) or block_table.dtype != torch.int32 or \
            block_table.dim() != 2 or block_table.size(0) != B or block_table.size(1) < 1:
        raise ValueError("block_table must be an int32 [B, max_pages] = [%d, >= 1] tensor" % B)
    if block_table.device != t0.device:
        raise ValueError("block_table is on %s, %s on %s" % (block_table.device, name0,
                                                            t0.device))
    if not block_table.is_contiguous():
        raise ValueError("block_table must be contiguous: the kernels read the tensor itself")
    if block_table.size(1) * P >= 1 << 24:
        raise ValueError("max_pages * page size must be below 2^24, got %d" % (
            block_table.size(1) * P))
    if any(P * t.stride(1) * 2 >= 1 << 32 for t in (k_pages, v_pages)):
        raise ValueError("page size x row stride must stay below 2^32 bytes: the kernels' "
                         "offsets within a page are 32-bit")
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or \
            tuple(cache_seqlens.shape) != (B,):
        raise ValueError("cache_seqlens must be an int32 [B] = [%d] tensor" % B)
    if cache_seqlens.device != t0.device:
        raise ValueError("cache_seqlens is on %s, %s on %s" % (cache_seqlens.device, name0,
                                                              t0.device))
    if not cache_seqlens.is_contiguous():
        raise ValueError("cache_seqlens must be contiguous: the kernels read the tensor itself")


def _check_new_rows(k_new, v_new, like, want):
    for name, t in (("k_new", k_new), ("v_new", v_new)):
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != want or not t.is_cuda or \
                t.device != like.device or t.dtype != like.dtype:
            raise ValueError("%s must be a %s %s tensor on %s, got %s" % (
                name, like.dtype, list(want), like.device,
                (t.dtype, tuple(t.shape), t.device) if isinstance(t, torch.Tensor)
                else type(t).__name__))


def _decode_paged(q, k_pages, v_pages, cache_seqlens, k_new, v_new, scale, num_splits,
                  return_lse, block_table):
    if (k_new is None) != (v_new is None):
        raise ValueError("k_new and v_new come as a pair")
    _check_paged(("q", q), k_pages, v_pages, block_table, cache_seqlens)
    _check_heads(q, k_pages)
    B, Sq, _, D = q.shape
    named = [q, k_pages, v_pages]
    if k_new is not None:
        _check_new_rows(k_new, v_new, q, (B, Sq, k_pages.size(2), D))
        named += [k_new, v_new]
    if torch.is_grad_enabled() and any(t.requires_grad for t in named):
        raise ValueError("fused_attention_decode is forward only: call it under torch.no_grad() "
                         "or on detached tensors")
    cap = _C().DECODE_MAX_SPLITS
    if num_splits is not None and not 1 <= int(num_splits) <= cap:
        raise ValueError("num_splits must be in [1, %d], got %s" % (cap, num_splits))
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    o, lse = _C().decode_paged(q, k_pages, v_pages, block_table, cache_seqlens, k_new, v_new,
                               float(scale), 0 if num_splits is None else int(num_splits))
    return (o, lse) if return_lse else o


def paged_kv_append(k_new, v_new, k_pages, v_pages, block_table, cache_seqlens):
    """Store k_new / v_new [B, Sn, Hkv, D] (any Sn: a prompt at prefill) in the pages of a paged
    KV cache (``fused_attention_decode(..., block_table=)``): row i of batch element b becomes
    key cache_seqlens[b] + i, row (cache_seqlens[b] + i) % P of page block_table[b][(cache_seqlens
    [b] + i) // P].  Keys outside [0, max_pages * P) are skipped, page ids are clamped to the
    pool.  One launch, no host sync; cache_seqlens is not advanced."""
    _check_paged(("k_new", k_new), k_pages, v_pages, block_table, cache_seqlens)
    want = (k_new.size(0), k_new.size(1), k_pages.size(2), k_new.size(3))
    _check_new_rows(k_new, v_new, k_new, want)
    _C().paged_append(k_new, v_new, k_pages, v_pages, block_table, cache_seqlens)


FP8 = torch.float8_e4m3fn  # the one 8-bit cache dtype (OCP e4m3: finite up to 448, no inf)


def fp8_quantize_rows(x):
    """The quantiser of the FP8 KV cache in plain torch, bit for bit the append kernel's: per
    row (last dim) scale = amax / 448 in fp32 (1.0 for an all-zero row) and bytes = e4m3_rne(
    clamp(x / scale, -448, 448)).  -> (float8_e4m3fn like x, fp32 scales x.shape[:-1])."""
    xf = x.float()
    amax = xf.abs().amax(-1)
    scale = torch.where(amax > 0, amax / 448.0, torch.ones_like(amax))
    return (xf / scale.unsqueeze(-1)).clamp(-448.0, 448.0).to(FP8), scale


def _check_fp8(first, k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table=None):
    """The caches, scales and lengths of an FP8 call whose batch, 16-bit dtype and device are
    those of ``first`` = (name, [B, S, heads, D] tensor); ValueError on anything refused."""
    name0, t0 = first
    if block_table is not None:
        raise ValueError("an FP8 KV cache is not paged yet: block_table takes bf16 / fp16 pages")
    for name, t in (first, ("k_cache", k_cache), ("v_cache", v_cache)):
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError("%s must be a 4-d tensor, got %s" % (
                name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
        if not t.is_cuda or t.device != t0.device:
            raise ValueError("%s must be on %s's GPU, got a %s tensor" % (name, name0, t.device))
    if k_cache.dtype != FP8 or v_cache.dtype != FP8:
        if k_cache.dtype.itemsize > 1 and v_cache.dtype.itemsize > 1:
            raise ValueError("k_scale / v_scale come with a float8_e4m3fn cache, not with %s"
                             % k_cache.dtype)
        raise ValueError("an 8-bit KV cache is float8_e4m3fn in both halves, got %s and %s" % (
            k_cache.dtype, v_cache.dtype))
    if t0.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("an FP8 KV cache takes bf16 / fp16 %s, got %s" % (name0, t0.dtype))
    B, D = t0.size(0), t0.size(3)
    if D not in HEAD_DIMS:
        raise ValueError("head dim must be one of %s, got %d" % (HEAD_DIMS, D))
    if k_cache.shape != v_cache.shape or k_cache.size(0) != B or k_cache.size(3) != D:
        raise ValueError("k_cache and v_cache must be [B, Smax, Hkv, D] with B = %d, D = %d, got "
                         "%s and %s" % (B, D, tuple(k_cache.shape), tuple(v_cache.shape)))
    want = (B, k_cache.size(2), k_cache.size(1))
    for name, t in (("k_scale", k_scale), ("v_scale", v_scale)):
        if not isinstance(t, torch.Tensor) or t.dtype != torch.float32 or \
                tuple(t.shape) != want or t.device != t0.device or t.stride(2) != 1:
            raise ValueError("%s must be an fp32 [B, Hkv, Smax] = %s tensor on %s with the key "
                             "index contiguous, got %s" % (
                                 name, list(want), t0.device,
                                 (t.dtype, tuple(t.shape), t.stride(), t.device)
                                 if isinstance(t, torch.Tensor) else type(t).__name__))
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or \
            tuple(cache_seqlens.shape) != (B,):
        raise ValueError("cache_seqlens must be an int32 [B] = [%d] tensor" % B)
    if cache_seqlens.device != t0.device:
        raise ValueError("cache_seqlens is on %s, %s on %s" % (cache_seqlens.device, name0,
                                                              t0.device))
    if not cache_seqlens.is_contiguous():
        raise ValueError("cache_seqlens must be contiguous: the kernels read the tensor itself")


def _check_fp8_call(what, q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale, block_table,
                    k_scale, v_scale):
    """The tensors of a call over an FP8 KV cache (``what``: "decode" or "prefill"), ValueError
    on anything refused; -> the softmax scale."""
    if (k_new is None) != (v_new is None):
        raise ValueError("k_new and v_new come as a pair")
    _check_fp8(("q", q), k_cache, v_cache, k_scale, v_scale, cache_seqlens, block_table)
    _check_heads(q, k_cache)
    B, Sq, _, D = q.shape
    named = [q]
    if k_new is not None:
        _check_new_rows(k_new, v_new, q, (B, Sq, k_cache.size(2), D))
        named += [k_new, v_new]
    if torch.is_grad_enabled() and any(t.requires_grad for t in named):
        raise ValueError("fused_attention_%s is forward only: call it under torch.no_grad() "
                         "or on detached tensors" % what)
    return 1.0 / math.sqrt(D) if scale is None else scale


def _decode_fp8(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale, num_splits,
                return_lse, block_table, k_scale, v_scale):
    scale = _check_fp8_call("decode", q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale,
                            block_table, k_scale, v_scale)
    cap = _C().DECODE_MAX_SPLITS
    if num_splits is not None and not 1 <= int(num_splits) <= cap:
        raise ValueError("num_splits must be in [1, %d], got %s" % (cap, num_splits))
    o, lse = _C().decode_fp8(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, k_new, v_new,
                             float(scale), 0 if num_splits is None else int(num_splits))
    return (o, lse) if return_lse else o


def _prefill_fp8(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale, return_lse,
                 block_table, k_scale, v_scale):
    scale = _check_fp8_call("prefill", q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale,
                            block_table, k_scale, v_scale)
    o, lse = _C().prefill_fp8(q, k_cache, v_cache, k_scale, v_scale, cache_seqlens, k_new, v_new,
                              float(scale))
    return (o, lse) if return_lse else o


def fp8_kv_append(k_new, v_new, k_cache, v_cache, k_scale, v_scale, cache_seqlens):
    """Quantise k_new / v_new [B, Sn, Hkv, D] (bf16 / fp16, any Sn: a prompt at prefill) into an
    FP8 KV cache (``fused_attention_decode(..., k_scale=, v_scale=)``): row i of batch element b
    becomes key cache_seqlens[b] + i, its bytes and its scale as ``fp8_quantize_rows`` gives
    them.  Keys outside [0, Smax) are skipped.  One launch, no host sync; cache_seqlens is not
    advanced."""
    _check_fp8(("k_new", k_new), k_cache, v_cache, k_scale, v_scale, cache_seqlens)
    want = (k_new.size(0), k_new.size(1), k_cache.size(2), k_new.size(3))
    _check_new_rows(k_new, v_new, k_new, want)
    _C().fp8_append(k_new, v_new, k_cache, v_cache, k_scale, v_scale, cache_seqlens)


def _check_cache16(what, q, k_cache, v_cache, cache_seqlens, k_new, v_new):
    """The tensors of a call over a contiguous 16-bit KV cache (``what``: "decode" or
    "prefill"), ValueError on anything refused; -> the head dim."""
    named = [("q", q), ("k_cache", k_cache), ("v_cache", v_cache)]
    if (k_new is None) != (v_new is None):
        raise ValueError("k_new and v_new come as a pair")
    if k_new is not None:
        named += [("k_new", k_new), ("v_new", v_new)]
    for name, t in named:
        if not isinstance(t, torch.Tensor) or t.dim() != 4:
            raise ValueError("%s must be a 4-d tensor, got %s" % (
                name, tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__))
        if not t.is_cuda:
            raise ValueError("%s must be on the GPU, got a %s tensor" % (name, t.device))
        if t.device != q.device or t.dtype != q.dtype:
            raise ValueError("%s is %s on %s, q %s on %s" % (name, t.dtype, t.device, q.dtype,
                                                            q.device))
    if q.dtype not in (torch.bfloat16, torch.float16):
        raise ValueError("%s takes bf16 / fp16 tensors, got %s" % (what, q.dtype))
    B, Sq, H, D = q.shape
    if D not in HEAD_DIMS:
        raise ValueError("head dim must be one of %s, got %d" % (HEAD_DIMS, D))
    if k_cache.shape != v_cache.shape or k_cache.size(0) != B or k_cache.size(3) != D:
        raise ValueError("k_cache and v_cache must be [B, Smax, Hkv, D] with B = %d, D = %d, got "
                         "%s and %s" % (B, D, tuple(k_cache.shape), tuple(v_cache.shape)))
    _check_heads(q, k_cache)
    Hkv = k_cache.size(2)
    if k_new is not None and not (tuple(k_new.shape) == tuple(v_new.shape) == (B, Sq, Hkv, D)):
        raise ValueError("k_new and v_new must be [B, Sq, Hkv, D] = [%d, %d, %d, %d], got %s and "
                         "%s" % (B, Sq, Hkv, D, tuple(k_new.shape), tuple(v_new.shape)))
    if not isinstance(cache_seqlens, torch.Tensor) or cache_seqlens.dtype != torch.int32 or \
            tuple(cache_seqlens.shape) != (B,):
        raise ValueError("cache_seqlens must be an int32 [B] = [%d] tensor" % B)
    if cache_seqlens.device != q.device:
        raise ValueError("cache_seqlens is on %s, q on %s" % (cache_seqlens.device, q.device))
    if not cache_seqlens.is_contiguous():
        raise ValueError("cache_seqlens must be contiguous: the kernels read the tensor itself")
    if torch.is_grad_enabled() and any(t.requires_grad for _, t in named):
        raise ValueError("fused_attention_%s is forward only: call it under torch.no_grad() "
                         "or on detached tensors" % what)
    return D


def fused_attention_decode(q, k_cache, v_cache, cache_seqlens, k_new=None, v_new=None,
                           scale=None, num_splits=None, return_lse=False, block_table=None,
                           k_scale=None, v_scale=None):
    """One decode step over a KV cache.  q: [B, Sq, H, D], the Sq newest tokens; k_cache,
    v_cache: [B, Smax, Hkv, D] views (any batch / sequence / head strides; H % Hkv == 0, D = 64
    or 128, bf16 / fp16); cache_seqlens: int32 [B] on the GPU, the keys already in the cache,
    read by the kernels only (no host sync).  With k_new and v_new [B, Sq, Hkv, D] the rows are
    first written into the caches at rows cache_seqlens[b] .. cache_seqlens[b] + Sq - 1 and the
    visible length is L_b = cache_seqlens[b] + Sq, else L_b = cache_seqlens[b]; L_b is clipped
    to Smax on the device and no row outside the views is read or written.  Query i sees keys
    j <= L_b - Sq + i; a query that sees no key gets o = 0 and lse = -inf.  cache_seqlens is not
    advanced: the caller adds Sq (on the device) after the call.

    num_splits: workgroups that split each cache (None: chosen from the shapes and the device's
    CU count, never from the lengths); results are bitwise reproducible for a given value.
    -> o [B, Sq, H, D] contiguous and, with return_lse, the fp32 [B, H, Sq] lse in log2 units.
    Forward only: ValueError if a gradient is asked of it.

    block_table: int32 [B, max_pages] on the GPU makes the cache a paged one: k_cache, v_cache
    are then [num_pages, P, Hkv, D] page views of a pool (any page / row / head strides; P in
    16, 32, 64, 128, 256), key j of batch element b is row j % P of page block_table[b][j // P],
    Smax = max_pages * P, and k_new / v_new are appended through the table.  Entries at or
    past ceil(L_b / P) are never read and page ids are clamped to the pool on the device.  For
    a given num_splits the result is bitwise that of the contiguous call on the same keys.

    k_scale, v_scale: with float8_e4m3fn k_cache and v_cache (both), the fp32 [B, Hkv, Smax]
    per-row scales (key index contiguous, any batch / head strides: the halves of one [B, 2, Hkv,
    Smax] buffer): key j of head hk is k_cache[b, j, hk].float() * k_scale[b, hk, j].  q, k_new
    and v_new stay bf16 / fp16; k_new / v_new are quantised per row on their way in
    (``fp8_quantize_rows``), and everything above holds.  ValueError without the scales, with
    scales on a 16-bit cache, with caches of two dtypes or another 8-bit dtype, and with
    block_table: the paged FP8 cache is not built yet (the follow-up to this path)."""
    if k_scale is not None or v_scale is not None or any(
            isinstance(t, torch.Tensor) and t.dtype.itemsize == 1 for t in (k_cache, v_cache)):
        return _decode_fp8(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale, num_splits,
                           return_lse, block_table, k_scale, v_scale)
    if block_table is not None:
        return _decode_paged(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale,
                             num_splits, return_lse, block_table)
    D = _check_cache16("decode", q, k_cache, v_cache, cache_seqlens, k_new, v_new)
    cap = _C().DECODE_MAX_SPLITS
    if num_splits is not None and not 1 <= int(num_splits) <= cap:
        raise ValueError("num_splits must be in [1, %d], got %s" % (cap, num_splits))
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    o, lse = _C().decode(q, k_cache, v_cache, cache_seqlens, k_new, v_new, float(scale),
                         0 if num_splits is None else int(num_splits))
    return (o, lse) if return_lse else o


def fused_attention_prefill(q, k_cache, v_cache, cache_seqlens, k_new=None, v_new=None,
                            scale=None, return_lse=False, block_table=None, k_scale=None,
                            v_scale=None):
    """Sq new tokens (a prompt chunk, the next turn, a draft: any Sq >= 1) over a contiguous
    KV cache that holds a prefix.  Every tensor and every contract is
    ``fused_attention_decode``'s: q [B, Sq, H, D]; k_cache, v_cache [B, Smax, Hkv, D] views;
    cache_seqlens int32 [B] on the GPU, read by the kernels only; with k_new and v_new [B, Sq,
    Hkv, D] the rows are first stored at rows cache_seqlens[b] + i and L_b = cache_seqlens[b] +
    Sq, else L_b = cache_seqlens[b], clipped to Smax on the device; query i sees keys j <= L_b -
    Sq + i, a query that sees no key gets o = 0 and lse = -inf; cache_seqlens is not advanced.
    -> o [B, Sq, H, D] contiguous and, with return_lse, the fp32 [B, H, Sq] lse in log2 units.
    One launch without a workspace: there is no num_splits and results are bitwise
    reproducible.  Forward only.

    k_scale, v_scale: with float8_e4m3fn k_cache and v_cache (both), the fp32 [B, Hkv, Smax]
    per-row scales of ``fused_attention_decode``, whose FP8 contract holds word for word: q,
    k_new and v_new stay bf16 / fp16, k_new / v_new are quantised per row on their way in
    (``fp8_quantize_rows``) and the chunk attends the quantised rows, its own included.
    ValueError without the scales or with one of them, with scales on a 16-bit cache, with
    caches of two dtypes or another 8-bit dtype, and for a block_table with either cache dtype:
    a paged cache goes to ``fused_attention_decode``."""
    if k_scale is not None or v_scale is not None or any(
            isinstance(t, torch.Tensor) and t.dtype.itemsize == 1 for t in (k_cache, v_cache)):
        return _prefill_fp8(q, k_cache, v_cache, cache_seqlens, k_new, v_new, scale, return_lse,
                            block_table, k_scale, v_scale)
    if block_table is not None:
        raise ValueError("fused_attention_prefill takes a contiguous KV cache: a paged one "
                         "(block_table) is served by fused_attention_decode only")
    D = _check_cache16("prefill", q, k_cache, v_cache, cache_seqlens, k_new, v_new)
    scale = 1.0 / math.sqrt(D) if scale is None else scale
    o, lse = _C().prefill(q, k_cache, v_cache, cache_seqlens, k_new, v_new, float(scale))
    return (o, lse) if return_lse else o
