"""Shared attention core of the contrib multi-head attention modules."""
from __future__ import annotations

import math

import torch
import torch.nn.functional as F

from ...ops import attention as fused_attn


def sdpa_masks(key_padding_mask, attn_mask, mask_additive, B, Tq, Tk, dtype, device):
    """Apex mask conventions -> one additive SDPA mask [B, 1, Tq, Tk] (or None).
    key_padding_mask [B, Tk]: True / 1 = padded key (or an additive float mask when
    ``mask_additive``); attn_mask [Tq, Tk]: True / 1 = masked (or additive)."""
    m = None
    if key_padding_mask is not None:
        kp = key_padding_mask.to(device)
        if mask_additive:
            m = kp.to(dtype).view(B, 1, 1, Tk)
        else:
            m = torch.zeros(B, 1, 1, Tk, dtype=dtype, device=device).masked_fill(
                kp.bool().view(B, 1, 1, Tk), float("-inf"))
    if attn_mask is not None:
        am = attn_mask.to(device)
        if mask_additive or am.is_floating_point():
            a = am.to(dtype).view(1, 1, Tq, Tk)
        else:
            a = torch.zeros(1, 1, Tq, Tk, dtype=dtype, device=device).masked_fill(
                am.bool().view(1, 1, Tq, Tk), float("-inf"))
        m = a if m is None else m + a
    return m


def _fused_key_mask(key_padding_mask, mask_additive, device):
    """The modules' key-padding mask as the fused ops' keyword arguments."""
    if key_padding_mask is None:
        return {}
    if isinstance(key_padding_mask, fused_attn.PreparedKeyMask):
        return {"key_bias": key_padding_mask}
    kp = key_padding_mask.to(device)
    if mask_additive:
        return {"key_bias": kp.float()}
    return {"key_padding_mask": kp.bool()}


def attention_bshd(q, k, v, dropout_p, key_padding_mask=None, attn_mask=None,
                   mask_additive=False, allow_fused=True, kv=None):
    """q [B, Tq, H, D], k/v [B, Tk, H, D] (any strides) -> [B, Tq, H, D].
    gfx950 fused kernels when eligible (no attn_mask, D == 64, 16-bit; Tq and Tk may
    differ; a key-padding mask [B, Tk] - boolean / byte, or additive under
    ``mask_additive``, or an ops.attention.PreparedKeyMask - is applied inside the
    kernels), PyTorch SDPA otherwise.  ``kv``: the packed [B, Tk, 2, H, D] tensor that k
    and v are the two halves of, when there is one: the fused path then takes it whole
    (``fused_attention_kv``: one packed dkv in the backward); the SDPA path uses k and v."""
    B, Tq, H, D = q.shape
    Tk = k.size(1)
    if allow_fused and attn_mask is None and fused_attn.supported(q, D):
        mask_kw = _fused_key_mask(key_padding_mask, mask_additive, q.device)
        if kv is not None:
            return fused_attn.fused_attention_kv(q, kv, dropout_p=dropout_p, **mask_kw)
        return fused_attn.fused_attention(q, k, v, causal=False, dropout_p=dropout_p, **mask_kw)
    mask = sdpa_masks(key_padding_mask, attn_mask, mask_additive, B, Tq, Tk, q.dtype, q.device)
    o = F.scaled_dot_product_attention(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2),
                                       attn_mask=mask, dropout_p=dropout_p,
                                       scale=1.0 / math.sqrt(D))
    return o.transpose(1, 2)
