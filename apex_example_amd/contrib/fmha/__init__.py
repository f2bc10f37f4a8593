"""apex.contrib.fmha counterpart: multi-head self-attention over PACKED variable-length
sequences (unpadded BERT pre-training).  The real tokens of a batch sit in one [T, ...]
buffer, ``cu_seqlens`` (int32 [B + 1]) gives each sequence's first row, and attention runs
per sequence inside the gfx950 fused attention kernels (``ops.attention``'s
``fused_attention_varlen_qkv``: no padded query, key or output row exists anywhere).

Off the fused path (CPU, fp32, head dim != 64) a per-sequence
``F.scaled_dot_product_attention`` loop over ``cu_seqlens`` gives the same result."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from ...ops import attention as fused_attn

__all__ = ["FMHA", "packed_self_attention"]


def packed_self_attention(qkv, cu_seqlens, max_s=None, dropout_p=0.0, causal=False, fused=True):
    """qkv [T, 3, H, D] (any strides), cu_seqlens int32 [B + 1] from 0 to T -> o [T, H, D]:
    every sequence attends within itself.  The fused kernels when ``fused`` and
    ``ops.attention.supported`` holds (``max_s`` given: no host sync), else one SDPA call
    per sequence (one host copy of ``cu_seqlens``)."""
    T, _, H, D = qkv.shape
    if fused and fused_attn.supported(qkv, D):
        return fused_attn.fused_attention_varlen_qkv(qkv, cu_seqlens, max_s, causal=causal,
                                                     dropout_p=dropout_p)
    cu = [int(c) for c in cu_seqlens.tolist()]
    if cu[0] != 0 or cu[-1] != T or any(b < a for a, b in zip(cu, cu[1:])):
        raise ValueError("cu_seqlens must be non-decreasing from 0 to T = %d, got %s" % (T, cu))
    outs = []
    for a, b in zip(cu, cu[1:]):
        if b == a:
            continue
        q, k, v = qkv[a:b].permute(1, 2, 0, 3).unsqueeze(1)  # each [1, H, L, D]
        o = F.scaled_dot_product_attention(q, k, v, dropout_p=dropout_p, is_causal=causal)
        outs.append(o[0].transpose(0, 1))
    return torch.cat(outs) if outs else qkv.new_zeros(T, H, D)


class FMHA(nn.Module):
    """``apex.contrib.fmha.FMHA``: ``forward(qkv [T, 3 * hidden], cu_seqlens, max_s)`` ->
    [T, hidden], qkv laid out as [T, 3, heads, head dim].  ``config`` supplies
    ``attention_probs_dropout_prob``, ``num_attention_heads`` and ``hidden_size``."""

    def __init__(self, config):
        super().__init__()
        self.p_dropout = config.attention_probs_dropout_prob
        self.h = config.num_attention_heads
        self.hidden_size = config.hidden_size
        self.d = self.hidden_size // self.h
        assert self.d * self.h == self.hidden_size, "Invalid hidden size/num_heads"

    def forward(self, qkv, cu_seqlens, max_s, is_training=True, zero_tensors=False):
        # zero_tensors: accepted for Apex's signature; nothing here needs pre-zeroed outputs
        T = qkv.size(0)
        p = self.p_dropout if is_training else 0.0
        o = packed_self_attention(qkv.view(T, 3, self.h, self.d), cu_seqlens, max_s, p)
        return o.reshape(T, self.hidden_size)
