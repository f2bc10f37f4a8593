"""BERT (Devlin et al. 2018) for pre-training, defined in-repo (no transformers
download): post-LN encoder with FusedLayerNorm, fused QKV projection, the gfx950 fused
attention kernels (ops/attention.py, with the padding mask applied inside them;
PyTorch SDPA off-GPU, in fp32 or with fused_attention=False), masked-LM head on the
gathered masked positions only (NVIDIA's pretraining recipe, max_predictions
per sequence) with the decoder tied to the word embeddings, and the NSP head.
``BertConfig(unpad=True)`` runs the encoder layers on the non-padding tokens only (packed
sequences, attention per sequence through ``cu_seqlens``; contrib/fmha).

bert_large(): 24 layers, hidden 1024, 16 heads, FFN 4096, vocab 30522 (padded to
a multiple of 8 optionally), 512 positions.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.embedding import Embedding
from .. import _native
from ..normalization import FusedLayerNorm, fused_add_dropout_layer_norm
from ..fused_dense import (fused_dense_function, fused_dense_gelu_dense_skip_function,
                           fused_dense_skip_function)
from ..ops import attention as fused_attn


@dataclass
class BertConfig:
    vocab_size: int = 30522
    hidden_size: int = 1024
    num_hidden_layers: int = 24
    num_attention_heads: int = 16
    intermediate_size: int = 4096
    hidden_dropout_prob: float = 0.1
    attention_probs_dropout_prob: float = 0.1
    max_position_embeddings: int = 512
    type_vocab_size: int = 2
    initializer_range: float = 0.02
    layer_norm_eps: float = 1e-12
    fused_layer_norm: bool = True
    fused_attention: bool = True
    fused_dense: bool = True  # fused bias-grad / GELU-backward dense layers (fused_dense)
    # FFN activation: "gelu_tanh" (apex fused_dense's GELU, the tanh approximation:
    # forward and backward run inside hipBLASLt GEMM epilogues; |erf - tanh| GELU is
    # < 1e-3, below bf16 resolution at FFN magnitudes) or "gelu" (erf).  The stock
    # path (fused_dense=False) uses the same function, so comparisons stay like for like.
    hidden_act: str = "gelu_tanh"
    # Unpadded encoder: with an attention_mask, run the layers on the kept tokens only,
    # packed into one [1, T, hidden] buffer, attention per sequence through cu_seqlens
    # (contrib.fmha); the padded positions of the output are zero.  See BertModel.forward.
    unpad: bool = False


def _ln(cfg, n):
    if cfg.fused_layer_norm:
        return FusedLayerNorm(n, eps=cfg.layer_norm_eps)
    return nn.LayerNorm(n, eps=cfg.layer_norm_eps)


class BertEmbeddings(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.word_embeddings = Embedding(cfg.vocab_size, cfg.hidden_size)
        self.position_embeddings = Embedding(cfg.max_position_embeddings, cfg.hidden_size)
        self.token_type_embeddings = Embedding(cfg.type_vocab_size, cfg.hidden_size)
        self.LayerNorm = _ln(cfg, cfg.hidden_size)
        self.dropout = nn.Dropout(cfg.hidden_dropout_prob)

    def forward(self, input_ids, token_type_ids):
        s = input_ids.size(1)
        pos = torch.arange(s, device=input_ids.device).unsqueeze(0)
        e = self.word_embeddings(input_ids) + self.position_embeddings(pos) + \
            self.token_type_embeddings(token_type_ids)
        return self.dropout(self.LayerNorm(e))


class BertSelfAttention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.h = cfg.num_attention_heads
        self.d = cfg.hidden_size // cfg.num_attention_heads
        self.qkv = nn.Linear(cfg.hidden_size, 3 * cfg.hidden_size)
        self.dense = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.p = cfg.attention_probs_dropout_prob
        self.fused = cfg.fused_attention
        self.fused_dense = cfg.fused_dense

    def _lin(self, m, x):
        return fused_dense_function(x, m.weight, m.bias) if self.fused_dense else m(x)

    def forward(self, x, attn_mask=None, key_mask=None, cu_seqlens=None, max_s=None):
        """Returns (attention output, x as the residual branch).  With fused_dense the
        residual is the QKV layer's skip output, so the input gradient of the block
        is one accumulating GEMM (no separate residual-gradient add).  attn_mask: additive
        [b, 1, 1, s] for the SDPA path; key_mask: the same padding mask prepared for the
        fused kernels (ops.attention.PreparedKeyMask), which then take it instead.
        cu_seqlens / max_s: x is [1, T, hidden], the packed tokens of the sequences that
        cu_seqlens (int32 [B + 1]) delimits, each attending within itself (no mask)."""
        b, s, hd = x.shape
        if self.fused_dense:
            qkv, skip = fused_dense_skip_function(x, self.qkv.weight, self.qkv.bias)
        else:
            qkv, skip = self.qkv(x), x
        p = self.p if self.training else 0.0
        if cu_seqlens is not None:
            from ..contrib.fmha import packed_self_attention

            o = packed_self_attention(qkv.view(b * s, 3, self.h, self.d), cu_seqlens, max_s, p,
                                      fused=self.fused)
            return self._lin(self.dense, o.reshape(b, s, hd)), skip
        qkv = qkv.view(b, s, 3, self.h, self.d)
        if (self.fused and (attn_mask is None or key_mask is not None)
                and fused_attn.supported(qkv, self.d)):
            o = fused_attn.fused_attention_qkv(qkv, causal=False, dropout_p=p, key_bias=key_mask)
            return self._lin(self.dense, o.view(b, s, hd)), skip
        if attn_mask is None and key_mask is not None:
            raise ValueError("key_mask is for the fused attention path; pass attn_mask too")
        qkv = qkv.permute(2, 0, 3, 1, 4)
        q, k, v = qkv[0], qkv[1], qkv[2]
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=attn_mask, dropout_p=p)
        o = o.transpose(1, 2).reshape(b, s, hd)
        return self._lin(self.dense, o), skip


class BertLayer(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.attention = BertSelfAttention(cfg)
        self.attn_dropout = nn.Dropout(cfg.hidden_dropout_prob)
        self.attn_ln = _ln(cfg, cfg.hidden_size)
        self.intermediate = nn.Linear(cfg.hidden_size, cfg.intermediate_size)
        self.output = nn.Linear(cfg.intermediate_size, cfg.hidden_size)
        self.out_dropout = nn.Dropout(cfg.hidden_dropout_prob)
        self.out_ln = _ln(cfg, cfg.hidden_size)
        self.fused_dense = cfg.fused_dense
        self.approximate = {"gelu_tanh": "tanh", "gelu": "none"}[cfg.hidden_act]

    def forward(self, x, attn_mask=None, key_mask=None, cu_seqlens=None, max_s=None):
        a, x = self.attention(x, attn_mask, key_mask, cu_seqlens, max_s)
        x, _ = fused_add_dropout_layer_norm(x, a, self.attn_ln, self.attn_dropout.p,
                                            self.training)
        if self.fused_dense:
            f, x = fused_dense_gelu_dense_skip_function(x, self.intermediate.weight,
                                                        self.intermediate.bias,
                                                        self.output.weight, self.output.bias,
                                                        self.approximate)
        else:
            f = self.output(F.gelu(self.intermediate(x), approximate=self.approximate))
        return fused_add_dropout_layer_norm(x, f, self.out_ln, self.out_dropout.p,
                                            self.training)[0]


def additive_attention_mask(attention_mask, dtype):
    """BERT's [b, s] attention_mask (1 = attend, 0 = padding) as an additive key bias:
    0 on kept keys, -10000 on padded ones."""
    return (1.0 - attention_mask.to(dtype)) * -10000.0


class BertModel(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.config = cfg
        self.embeddings = BertEmbeddings(cfg)
        self.layers = nn.ModuleList([BertLayer(cfg) for _ in range(cfg.num_hidden_layers)])
        self.pooler = nn.Linear(cfg.hidden_size, cfg.hidden_size)

    def forward(self, input_ids, token_type_ids, attention_mask=None):
        """Returns (sequence output [b, s, hidden], pooled output [b, hidden]).

        config.unpad with an attention_mask ([b, s], non-zero = keep, any pattern): the kept
        tokens, in order and with their own position embeddings, are gathered after the
        embeddings into one [1, T, hidden] buffer, every layer (GEMMs, LayerNorms, attention
        per sequence) runs on those T rows alone, and the result is scattered back into a
        zero [b, s, hidden] before the pooler - padded positions of the sequence output
        are exactly zero.  Costs ONE host sync per forward (the per-sequence token counts:
        T and the longest sequence size the buffers and the attention grid)."""
        x = self.embeddings(input_ids, token_type_ids)
        if self.config.unpad and attention_mask is not None:
            return self._forward_unpadded(x, attention_mask)
        mask = key_mask = None
        if attention_mask is not None:
            # [b, s] 1 = keep -> additive [b, 1, 1, s]
            mask = additive_attention_mask(attention_mask, x.dtype)[:, None, None, :]
            head_dim = self.config.hidden_size // self.config.num_attention_heads
            if (self.config.fused_attention and x.is_cuda and head_dim == 64
                    and _native.available()):
                # the same -10000 bias (never -inf: no row is fully masked), prepared once
                # for the fused kernels of all layers (each layer takes them when its qkv
                # is 16-bit, the SDPA path with `mask` otherwise)
                key_mask = fused_attn.prepare_key_mask(
                    additive_attention_mask(attention_mask, torch.float32))
        for layer in self.layers:
            x = layer(x, mask, key_mask)
        pooled = torch.tanh(self.pooler(x[:, 0]))
        return x, pooled

    def _forward_unpadded(self, x, attention_mask):
        b, s, hd = x.shape
        keep = attention_mask.reshape(-1) != 0
        counts = keep.view(b, s).sum(1)
        lens = counts.tolist()  # the host sync
        T, max_s = sum(lens), max(lens + [1])
        cu_seqlens = F.pad(counts.cumsum(0), (1, 0)).to(torch.int32)
        # attention_mask.flatten().nonzero(), its size known from the counts (no second sync)
        idx = torch.nonzero_static(keep, size=T).squeeze(1)
        t = x.reshape(b * s, hd).index_select(0, idx).unsqueeze(0)
        for layer in self.layers:
            t = layer(t, cu_seqlens=cu_seqlens, max_s=max_s)
        x = x.new_zeros(b * s, hd).index_copy(0, idx, t.squeeze(0)).view(b, s, hd)
        pooled = torch.tanh(self.pooler(x[:, 0]))
        return x, pooled


class BertForPreTraining(nn.Module):
    """Returns (masked-LM logits at the masked positions, NSP logits)."""

    def __init__(self, cfg: BertConfig):
        super().__init__()
        self.config = cfg
        self.bert = BertModel(cfg)
        self.transform = nn.Linear(cfg.hidden_size, cfg.hidden_size)
        self.transform_ln = _ln(cfg, cfg.hidden_size)
        self.decoder_bias = nn.Parameter(torch.zeros(cfg.vocab_size))
        self.nsp = nn.Linear(cfg.hidden_size, 2)
        self.apply(self._init)

    def _init(self, m):
        std = self.config.initializer_range
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=std)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=std)

    def forward(self, input_ids, token_type_ids, masked_positions, attention_mask=None):
        seq, pooled = self.bert(input_ids, token_type_ids, attention_mask)
        b, s, h = seq.shape
        idx = masked_positions + (torch.arange(b, device=seq.device) * s).unsqueeze(1)
        sel = seq.reshape(b * s, h).index_select(0, idx.reshape(-1))
        t = self.transform_ln(F.gelu(self.transform(sel)))
        logits = F.linear(t, self.bert.embeddings.word_embeddings.weight, self.decoder_bias)
        return logits, self.nsp(pooled)


def pretraining_loss(mlm_logits, nsp_logits, mlm_labels, nsp_labels, fused=True):
    """Masked-LM (labels -1 = not predicted) + NSP cross entropy.  ``fused``: the
    MLM term runs the gfx950 softmax-cross-entropy kernel on the 16-bit logits."""
    labels = mlm_labels.reshape(-1)
    if fused and mlm_logits.is_cuda and _native.available():
        from ..contrib.xentropy import SoftmaxCrossEntropyLoss

        losses = SoftmaxCrossEntropyLoss.apply(mlm_logits, labels, 0.0, -1, True)
        mlm = losses.sum() / (labels != -1).sum().clamp_min(1)
    else:
        mlm = F.cross_entropy(mlm_logits.float(), labels, ignore_index=-1)
    nsp = F.cross_entropy(nsp_logits.float(), nsp_labels)
    return mlm + nsp


def bert_large(**kw):
    return BertForPreTraining(BertConfig(**kw))


def bert_base(**kw):
    kw.setdefault("hidden_size", 768)
    kw.setdefault("num_hidden_layers", 12)
    kw.setdefault("num_attention_heads", 12)
    kw.setdefault("intermediate_size", 3072)
    return BertForPreTraining(BertConfig(**kw))


def synthetic_batch(cfg: BertConfig, batch, seq_len, max_pred, device, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    ids = torch.randint(0, cfg.vocab_size, (batch, seq_len), generator=g)
    tt = torch.zeros(batch, seq_len, dtype=torch.long)
    tt[:, seq_len // 2:] = 1
    pos = torch.stack([torch.randperm(seq_len, generator=g)[:max_pred].sort().values
                       for _ in range(batch)])
    labels = torch.randint(0, cfg.vocab_size, (batch, max_pred), generator=g)
    nsp = torch.randint(0, 2, (batch,), generator=g)
    return [t.to(device) for t in (ids, tt, pos, labels, nsp)]
