"""GPT-2 (Radford et al. 2019) language model defined in-repo: pre-LN decoder
blocks with FusedLayerNorm, causal attention on the gfx950 fused attention
kernels (ops/attention.py; PyTorch SDPA off-GPU / fp32),
tanh-GELU MLP and an LM head tied to the token embedding.  ``generate`` samples with a
``KVCache``: the prompt runs through the causal kernels once, every further token through the
split-KV decode kernels (``fused_attention_decode``), later chunks of a prompt fed in pieces
(``prefill_chunk``) through the chunked-prefill kernels (``fused_attention_prefill``); with
``page_size`` the cache is a
``PagedKVCache``, a page pool and a block table read by the paged decode kernels; with
``kv_dtype=torch.float8_e4m3fn`` the ``KVCache`` holds FP8 rows and one fp32 scale per row, read
by the FP8 variants of the decode and chunked-prefill kernels.

gpt2_medium(): 24 layers, d_model 1024, 16 heads, vocab 50257, 1024 positions
= 354,823,168 parameters in 292 tensors.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
import torch.nn as nn
import torch.nn.functional as F

from ..ops.embedding import Embedding
from .. import _native
from ..normalization import FusedLayerNorm, fused_add_dropout_layer_norm
from ..fused_dense import cast_params_once, fused_dense_function, fused_dense_gelu_dense_function
from ..ops import attention as fused_attn


@dataclass
class GPT2Config:
    vocab_size: int = 50257
    n_positions: int = 1024
    n_embd: int = 1024
    n_layer: int = 24
    n_head: int = 16
    # key/value heads shared by n_head // n_kv_head query heads each (grouped-query attention;
    # 1 = multi-query).  None: n_head of them, the GPT-2 module and state dict as published.
    n_kv_head: int | None = None
    resid_pdrop: float = 0.1
    embd_pdrop: float = 0.1
    attn_pdrop: float = 0.1
    layer_norm_epsilon: float = 1e-5
    initializer_range: float = 0.02
    fused_layer_norm: bool = True
    fused_attention: bool = True
    fused_dense: bool = True  # fused bias-grad / GELU-backward dense layers (fused_dense)
    # residual add + dropout + the next LayerNorm as one kernel per sublayer join
    # (fp32 residual stream, 16-bit sublayer output under O1)
    fused_residual_ln: bool = True


# New rows (tokens x query heads of a group) from which a chunk behind a filled contiguous cache
# goes to the chunked-prefill kernels instead of the decode kernels: the smallest measured row
# count at which they beat decode at every measured cache length (docs/PERF.md, "Attention:
# chunked prefill over a KV cache": below it decode's split-KV wins at batch 1; the section also
# names the small grids above it where decode is still faster).  The FP8 cache's own table gives
# the same 2048 by the same rule ("Attention: chunked prefill over an FP8 KV cache"), so one
# constant serves both cache dtypes.
PREFILL_MIN_ROWS = 2048


def _ln(cfg, n):
    if cfg.fused_layer_norm:
        return FusedLayerNorm(n, eps=cfg.layer_norm_epsilon)
    return nn.LayerNorm(n, eps=cfg.layer_norm_epsilon)


class KVCache:
    """Keys and values of the tokens a model has seen, for ``GPT2LMHeadModel.forward(...,
    cache=)``: per layer one packed [B, max_len, 2, Hkv, D] buffer (allocated at the layer's
    first use, in its activations' dtype), one int32 [B] length tensor on the device, which the
    decode kernels read, and the same length as a host integer, so that choosing between the
    prefill and the decode path costs no sync.  One length per batch: ragged prompts are not
    served.  With ``kv_dtype=torch.float8_e4m3fn`` a layer's buffer is FP8 and comes with fp32
    per-row scales [B, 2, Hkv, max_len] (``scales``): half the bytes a decode step reads."""

    def __init__(self, batch, max_len, kv_dtype=None):
        if kv_dtype not in (None, fused_attn.FP8):
            raise ValueError("kv_dtype must be None (the activations' dtype) or "
                             "torch.float8_e4m3fn, got %s" % kv_dtype)
        self.batch, self.max_len, self.kv_dtype = int(batch), int(max_len), kv_dtype
        self.kv = {}         # layer -> [B, max_len, 2, Hkv, D]
        self.scales = {}     # FP8: layer -> fp32 [B, 2, Hkv, max_len]
        self.lengths = None  # int32 [B], on the device of the first layer's buffer
        self.length = 0

    def layer(self, idx, like):
        """The buffer of layer ``idx`` for keys shaped and typed like ``like`` [B, s, Hkv, D]."""
        if idx not in self.kv:
            self.kv[idx] = like.new_empty(self.batch, self.max_len, 2, like.size(2), like.size(3),
                                          dtype=self.kv_dtype or like.dtype)
            if self.kv_dtype is not None:
                self.scales[idx] = like.new_empty(self.batch, 2, like.size(2), self.max_len,
                                                  dtype=torch.float32)
            if self.lengths is None:
                self.lengths = torch.full((self.batch,), self.length, dtype=torch.int32,
                                          device=like.device)
        return self.kv[idx]

    def advance(self, n):
        """After every layer has stored ``n`` new tokens."""
        self.length += n
        if self.lengths is not None:
            self.lengths += n


class PagedKVCache:
    """A ``KVCache`` kept in pages of ``page_size`` rows: per layer one packed pool [num_pages,
    P, 2, Hkv, D] (allocated at the layer's first use) and, shared by the layers, one int32
    block table [B, ceil(max_len / P)], built here with the pages of a sequence interleaved
    across the batch (page(b, j) = j * B + b) and moved to the device with the first pool.
    ``lengths`` / ``length`` / ``advance`` are those of ``KVCache``.  16-bit pages only: an FP8
    cache (``kv_dtype``) is not paged yet."""
    kv_dtype = None

    def __init__(self, batch, max_len, page_size=64, kv_dtype=None):
        if kv_dtype is not None:
            raise ValueError("a paged KV cache holds the activations' dtype: kv_dtype = %s is "
                             "served by the contiguous KVCache only" % kv_dtype)
        if page_size not in fused_attn.PAGE_SIZES:
            raise ValueError("page_size must be one of %s, got %s" % (fused_attn.PAGE_SIZES,
                                                                      page_size))
        self.batch, self.max_len, self.page_size = int(batch), int(max_len), int(page_size)
        self.max_pages = -(-self.max_len // self.page_size)
        self.num_pages = self.batch * self.max_pages
        self.block_table = (torch.arange(self.max_pages, dtype=torch.int32)[None] * self.batch
                            + torch.arange(self.batch, dtype=torch.int32)[:, None]).contiguous()
        self.kv = {}         # layer -> [num_pages, P, 2, Hkv, D]
        self.lengths = None  # int32 [B], on the device of the first layer's pool
        self.length = 0

    def layer(self, idx, like):
        """The pool of layer ``idx`` for keys shaped and typed like ``like`` [B, s, Hkv, D]."""
        if idx not in self.kv:
            self.kv[idx] = like.new_empty(self.num_pages, self.page_size, 2, like.size(2),
                                          like.size(3))
            if self.lengths is None:
                self.lengths = torch.full((self.batch,), self.length, dtype=torch.int32,
                                          device=like.device)
                self.block_table = self.block_table.to(like.device)
        return self.kv[idx]

    def rows(self, lo, hi):
        """(page ids [B, hi - lo], rows [hi - lo]) of keys lo .. hi - 1, as index tensors."""
        pos = torch.arange(lo, hi, device=self.block_table.device)
        return self.block_table[:, pos // self.page_size].long(), pos % self.page_size

    advance = KVCache.advance


class GPT2Attention(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.h = cfg.n_head
        self.d = cfg.n_embd // cfg.n_head
        self.hkv = cfg.n_kv_head
        if self.hkv is not None and (self.hkv <= 0 or self.h % self.hkv != 0):
            raise ValueError("n_head = %d does not split over n_kv_head = %d" % (self.h, self.hkv))
        # grouped: one projection to [query heads | key heads | value heads]
        self.c_attn = nn.Linear(cfg.n_embd, 3 * cfg.n_embd if self.hkv is None
                                else (self.h + 2 * self.hkv) * self.d)
        self.c_proj = nn.Linear(cfg.n_embd, cfg.n_embd)
        self.p = cfg.attn_pdrop
        self.resid_dropout = nn.Dropout(cfg.resid_pdrop)
        self.fused = cfg.fused_attention
        self.fused_dense = cfg.fused_dense
        self.layer_idx = 0  # its slot in a KVCache; GPT2LMHeadModel numbers its blocks

    def _lin(self, m, x):
        return fused_dense_function(x, m.weight, m.bias) if self.fused_dense else m(x)

    def forward(self, x, resid_dropout=True, cache=None):
        b, s, e = x.shape
        drop = self.resid_dropout if resid_dropout else (lambda t: t)
        if cache is not None:
            return drop(self._lin(self.c_proj, self._cached(x, cache)))
        if self.hkv is not None:
            return drop(self._lin(self.c_proj, self._grouped(x)))
        qkv = self._lin(self.c_attn, x).view(b, s, 3, self.h, self.d)
        p = self.p if self.training else 0.0
        if self.fused and fused_attn.supported(qkv, self.d):
            o = fused_attn.fused_attention_qkv(qkv, causal=True, dropout_p=p).view(b, s, e)
            return drop(self._lin(self.c_proj, o))
        qkv = qkv.permute(2, 0, 3, 1, 4)
        o = F.scaled_dot_product_attention(qkv[0], qkv[1], qkv[2], is_causal=True, dropout_p=p)
        o = o.transpose(1, 2).reshape(b, s, e)
        return drop(self._lin(self.c_proj, o))

    def _cached(self, x, cache):
        """Attention output [b, s, e] of s new tokens behind the ``cache.length`` tokens of a
        ``KVCache`` or ``PagedKVCache``, storing their keys and values (the model advances the
        lengths).  An empty cache is a prefill on the causal kernels (a paged one stores the
        prompt's rows through ``paged_kv_append``); a filled one a decode step, which appends in
        its own launch - or, for a contiguous cache (16-bit or FP8) and s * (h / hkv) >=
        PREFILL_MIN_ROWS new rows, a chunk on the chunked-prefill kernels, which append the same
        way.  Off the GPU / in fp32: SDPA over the filled rows (a paged cache's gathered through
        the table).  An FP8 cache: the new rows are quantised on their way in (``fp8_kv_append``
        or the decode / chunked-prefill call's own append; off the kernels by their torch mirror
        ``fp8_quantize_rows``), a decode step or a chunk behind a filled cache attends the
        quantised rows, its own included, and a prefill into an empty cache the prompt's own
        16-bit keys and values, on either path."""
        b, s, e = x.shape
        h, hkv, d = self.h, self.hkv or self.h, self.d
        y = self._lin(self.c_attn, x)
        if self.hkv is None:
            q, k, v = y.view(b, s, 3, h, d).unbind(2)
        else:
            q, k, v = y.view(b, s, h + 2 * hkv, d).split((h, hkv, hkv), 2)
        L = cache.length
        if b != cache.batch or L + s > cache.max_len:
            raise ValueError("the KV cache holds %d x %d tokens: no room for batch %d, %d + %d "
                             "tokens" % (cache.batch, cache.max_len, b, L, s))
        kv = cache.layer(self.layer_idx, k)
        paged = isinstance(cache, PagedKVCache)  # kv: [num_pages, P, 2, Hkv, D] behind a table
        fused = self.fused and fused_attn.supported(q, d)
        sc = cache.scales[self.layer_idx] if cache.kv_dtype is not None else None
        if fused and L > 0 and not paged and s * (h // hkv) >= PREFILL_MIN_ROWS:
            return fused_attn.fused_attention_prefill(
                q, kv[:, :, 0], kv[:, :, 1], cache.lengths, k_new=k, v_new=v,
                k_scale=None if sc is None else sc[:, 0],
                v_scale=None if sc is None else sc[:, 1]).view(b, s, e)
        if fused and L > 0:
            return fused_attn.fused_attention_decode(
                q, kv[:, :, 0], kv[:, :, 1], cache.lengths, k_new=k, v_new=v,
                block_table=cache.block_table if paged else None,
                k_scale=None if sc is None else sc[:, 0],
                v_scale=None if sc is None else sc[:, 1]).view(b, s, e)
        if sc is not None and fused:
            fused_attn.fp8_kv_append(k, v, kv[:, :, 0], kv[:, :, 1], sc[:, 0], sc[:, 1],
                                     cache.lengths)
        elif sc is not None:
            for i, t in enumerate((k, v)):
                kv[:, L:L + s, i], rows = fused_attn.fp8_quantize_rows(t)
                sc[:, i, :, L:L + s] = rows.transpose(1, 2)
        elif not paged:
            kv[:, L:L + s, 0] = k
            kv[:, L:L + s, 1] = v
        elif fused:
            fused_attn.paged_kv_append(k, v, kv[:, :, 0], kv[:, :, 1], cache.block_table,
                                       cache.lengths)
        else:
            kv[cache.rows(L, L + s)] = torch.stack((k, v), 2)
        if fused:
            return fused_attn.fused_attention(q, k, v, causal=True).view(b, s, e)
        g = h // hkv
        filled = kv[cache.rows(0, L + s)] if paged else kv[:, :L + s]  # [b, L + s, 2, Hkv, D]
        if sc is not None and L == 0:
            filled = torch.stack((k, v), 2)
        elif sc is not None:
            rows = sc[..., :L + s].permute(0, 3, 1, 2).unsqueeze(-1)  # [b, L + s, 2, Hkv, 1]
            filled = (filled.float() * rows).to(q.dtype)
        kk, vv = (filled[:, :, i].transpose(1, 2).repeat_interleave(g, 1) for i in (0, 1))
        # bottom-right causal mask: new token i sees keys j <= L + i
        keep = torch.ones(s, L + s, dtype=torch.bool, device=x.device).tril(L)
        o = F.scaled_dot_product_attention(q.transpose(1, 2), kk, vv, attn_mask=keep)
        return o.transpose(1, 2).reshape(b, s, e)

    def _grouped(self, x):
        """Attention output [b, s, e] with n_kv_head key/value heads."""
        b, s, e = x.shape
        h, hkv = self.h, self.hkv
        qkv = self._lin(self.c_attn, x).view(b, s, h + 2 * hkv, self.d)
        p = self.p if self.training else 0.0
        if self.fused and fused_attn.supported(qkv, self.d):
            return fused_attn.fused_attention_qkv_gqa(qkv, hkv, causal=True,
                                                      dropout_p=p).view(b, s, e)
        q, k, v = (t.transpose(1, 2) for t in qkv.split((h, hkv, hkv), 2))
        k, v = (t.repeat_interleave(h // hkv, 1) for t in (k, v))
        o = F.scaled_dot_product_attention(q, k, v, is_causal=True, dropout_p=p)
        return o.transpose(1, 2).reshape(b, s, e)


class GPT2MLP(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.c_fc = nn.Linear(cfg.n_embd, 4 * cfg.n_embd)
        self.c_proj = nn.Linear(4 * cfg.n_embd, cfg.n_embd)
        self.dropout = nn.Dropout(cfg.resid_pdrop)
        self.fused_dense = cfg.fused_dense

    def forward(self, x, dropout=True):
        drop = self.dropout if dropout else (lambda t: t)
        if self.fused_dense:
            return drop(fused_dense_gelu_dense_function(
                x, self.c_fc.weight, self.c_fc.bias, self.c_proj.weight, self.c_proj.bias,
                "tanh"))
        return drop(self.c_proj(F.gelu(self.c_fc(x), approximate="tanh")))


class GPT2Block(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.ln_1 = _ln(cfg, cfg.n_embd)
        self.attn = GPT2Attention(cfg)
        self.ln_2 = _ln(cfg, cfg.n_embd)
        self.mlp = GPT2MLP(cfg)

    def forward(self, x, cache=None):
        x = x + self.attn(self.ln_1(x), cache=cache)
        return x + self.mlp(self.ln_2(x))

    def forward_joined(self, x, y, next_ln, cache=None):
        """Same block with the sublayer joins fused: ``y`` = ln_1(x) is given,
        returns (next_ln(x'), x') for the block output x'.  Each join (dropout,
        residual add, the following LayerNorm) is one kernel each way."""
        # y only feeds autocast GEMMs (c_attn / c_fc / the tied LM head): under O1 it
        # leaves the join in the GEMM dtype instead of fp32 + a cast kernel
        y16 = torch.is_autocast_enabled("cuda")
        y, x = fused_add_dropout_layer_norm(x, self.attn(y, resid_dropout=False, cache=cache),
                                            self.ln_2,
                                            self.attn.resid_dropout.p, self.training, y16)
        return fused_add_dropout_layer_norm(x, self.mlp(y, dropout=False), next_ln,
                                            self.mlp.dropout.p, self.training, y16)


class GPT2LMHeadModel(nn.Module):
    def __init__(self, cfg: GPT2Config):
        super().__init__()
        self.config = cfg
        self.wte = Embedding(cfg.vocab_size, cfg.n_embd)
        self.wpe = Embedding(cfg.n_positions, cfg.n_embd)
        self.drop = nn.Dropout(cfg.embd_pdrop)
        self.h = nn.ModuleList([GPT2Block(cfg) for _ in range(cfg.n_layer)])
        self.ln_f = _ln(cfg, cfg.n_embd)
        for i, block in enumerate(self.h):
            block.attn.layer_idx = i
        self.apply(self._init)
        # GPT-2: scale the residual projections by 1/sqrt(2 * n_layer)
        for name, p in self.named_parameters():
            if name.endswith("c_proj.weight"):
                nn.init.normal_(p, std=cfg.initializer_range / (2 * cfg.n_layer) ** 0.5)

    def _init(self, m):
        if isinstance(m, nn.Linear):
            nn.init.normal_(m.weight, std=self.config.initializer_range)
            if m.bias is not None:
                nn.init.zeros_(m.bias)
        elif isinstance(m, nn.Embedding):
            nn.init.normal_(m.weight, std=self.config.initializer_range)

    def forward(self, input_ids, cache=None):
        """Logits [B, S, vocab].  With a ``KVCache`` / ``PagedKVCache``, ``input_ids`` are the tokens that follow
        the ``cache.length`` ones it holds: their keys and values are stored, their positions
        start at that length and they attend to everything before them (inference only)."""
        s = input_ids.size(1)
        p0 = 0 if cache is None else cache.length
        if cache is not None and p0 + s > self.config.n_positions:
            raise ValueError("%d + %d tokens exceed n_positions = %d" % (
                p0, s, self.config.n_positions))
        pos = torch.arange(p0, p0 + s, device=input_ids.device).unsqueeze(0)
        x = self.drop(self.wte(input_ids) + self.wpe(pos))
        if self.config.fused_dense and x.is_cuda and torch.is_autocast_enabled("cuda"):
            # O1: every dense weight / bias cast to the GEMM dtype in one launch
            dense = [p for blk in self.h for m in (blk.attn.c_attn, blk.attn.c_proj,
                                                   blk.mlp.c_fc, blk.mlp.c_proj)
                     for p in (m.weight, m.bias)]
            with cast_params_once(dense, torch.get_autocast_dtype("cuda")):
                return self._blocks(x, cache)
        return self._blocks(x, cache)

    def _blocks(self, x, cache=None):
        if self.config.fused_residual_ln:
            y = self.h[0].ln_1(x)
            for i, block in enumerate(self.h):
                nxt = self.h[i + 1].ln_1 if i + 1 < len(self.h) else self.ln_f
                y, x = block.forward_joined(x, y, nxt, cache)
        else:
            for block in self.h:
                x = block(x, cache)
            y = self.ln_f(x)
        if cache is not None:
            cache.advance(x.size(1))
        return F.linear(y, self.wte.weight)  # tied LM head

    @torch.no_grad()
    def generate(self, input_ids, max_new_tokens, temperature=0.0, page_size=None, kv_dtype=None,
                 prefill_chunk=None):
        """input_ids [B, S0] (one prompt length per batch) -> [B, S0 + max_new_tokens]: greedy
        at temperature 0, else sampled from softmax(logits / temperature).  Runs in eval mode
        with a ``KVCache`` or, with ``page_size``, a ``PagedKVCache`` of such pages: one forward
        over the prompt, then one token per step.  ``kv_dtype=torch.float8_e4m3fn`` keeps the
        (contiguous) cache in FP8 with per-row scales.  ``prefill_chunk``: feed the prompt in
        chunks of that many tokens (bounded activation memory for a long prompt), the first on
        the causal kernels, the later ones behind the filled cache; None: one forward."""
        b, s0 = input_ids.shape
        if prefill_chunk is not None and prefill_chunk < 1:
            raise ValueError("prefill_chunk must be a positive token count, got %s" % prefill_chunk)
        if s0 + max_new_tokens > self.config.n_positions:
            raise ValueError("%d prompt + %d new tokens exceed n_positions = %d" % (
                s0, max_new_tokens, self.config.n_positions))
        training = self.training
        self.eval()
        try:
            cache = KVCache(b, s0 + max_new_tokens, kv_dtype) if page_size is None else \
                PagedKVCache(b, s0 + max_new_tokens, page_size, kv_dtype)
            out, step = input_ids, input_ids
            if prefill_chunk is not None and max_new_tokens > 0:
                # all but the last chunk of the prompt: only their keys and values are needed
                while s0 - cache.length > prefill_chunk:
                    self(input_ids[:, cache.length:cache.length + prefill_chunk], cache=cache)
                step = input_ids[:, cache.length:]
            for n in range(max_new_tokens):
                logits = self(step, cache=cache)[:, -1].float()
                if temperature > 0.0:
                    step = torch.multinomial(torch.softmax(logits / temperature, -1), 1)
                else:
                    step = logits.argmax(-1, keepdim=True)
                out = torch.cat([out, step], 1)
            return out
        finally:
            self.train(training)


def lm_loss(logits, input_ids, fused=True):
    """Next-token cross entropy with an fp32 softmax.  ``fused``: the gfx950
    softmax-cross-entropy kernel (contrib.xentropy) reads the 16-bit logits
    directly (the last position's label is padding) instead of materialising a
    sliced fp32 copy of the [B*S, vocab] logits."""
    if fused and logits.is_cuda and _native.available():
        from ..contrib.xentropy import SoftmaxCrossEntropyLoss

        b, s, v = logits.shape
        labels = torch.cat([input_ids[:, 1:], input_ids.new_full((b, 1), -1)], 1).reshape(-1)
        losses = SoftmaxCrossEntropyLoss.apply(logits.reshape(b * s, v), labels, 0.0, -1, True)
        return losses.sum() / (b * (s - 1))
    return F.cross_entropy(logits[:, :-1].reshape(-1, logits.size(-1)).float(),
                           input_ids[:, 1:].reshape(-1))


def gpt2_medium(**kw):
    return GPT2LMHeadModel(GPT2Config(**kw))


def gpt2_small(**kw):
    kw.setdefault("n_embd", 768)
    kw.setdefault("n_layer", 12)
    kw.setdefault("n_head", 12)
    return GPT2LMHeadModel(GPT2Config(**kw))
