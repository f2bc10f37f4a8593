"""Fused MI355X operators used by the model zoo (BatchNorm+ReLU, ...)."""
from .batch_norm import BatchNorm2dReLU, BatchNormFunction, batch_norm_act  # noqa: F401
from .attention import (PreparedAttnMask, PreparedKeyMask, fp8_kv_append, fused_attention,  # noqa: F401
                        fused_attention_decode, fused_attention_kv, fused_attention_prefill,
                        fused_attention_qkv, fused_attention_qkv_gqa, fused_attention_varlen, fused_attention_varlen_qkv, paged_kv_append,
                        prepare_attn_mask, prepare_key_mask)
