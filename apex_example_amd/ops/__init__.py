"""Fused MI355X operators used by the model zoo (BatchNorm+ReLU, ...)."""
from .batch_norm import BatchNorm2dReLU, BatchNormFunction, batch_norm_act  # noqa: F401
from .attention import (PreparedKeyMask, fused_attention, fused_attention_kv,  # noqa: F401
                        fused_attention_qkv, fused_attention_varlen,
                        fused_attention_varlen_qkv, prepare_key_mask)
