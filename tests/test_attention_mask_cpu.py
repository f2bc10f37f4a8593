"""Key-mask plumbing off the GPU: the new keyword arguments of attention_bshd and
BertModel still give the SDPA result on CPU tensors, and the mask conventions
(True = masked key; BERT's 1/0 attention_mask -> 0 / -10000) hold."""
import math

import pytest
import torch
import torch.nn.functional as F


def _manual(q, k, v, bias):
    """softmax(q k^T / sqrt(D) + bias[b, key]) v on [B, T, H, D] tensors."""
    B, T, H, D = q.shape
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / math.sqrt(D) + bias.view(B, 1, 1, T)
    return torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)


def _qkv(B=3, T=10, H=2, D=64):
    torch.manual_seed(0)
    return tuple(torch.randn(B, T, H, D) for _ in range(3))


def test_attention_bshd_bool_key_padding_mask_true_is_masked():
    from apex_example_amd.contrib.multihead_attn._common import attention_bshd

    q, k, v = _qkv()
    kpm = torch.zeros(3, 10, dtype=torch.bool)
    kpm[0, 7:] = True
    kpm[1, :4] = True
    bias = torch.zeros(3, 10).masked_fill(kpm, float("-inf"))
    want = _manual(q, k, v, bias)
    for allow in (True, False):  # CPU tensors: SDPA either way
        got = attention_bshd(q, k, v, 0.0, key_padding_mask=kpm, allow_fused=allow)
        torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    # a byte mask means the same (Apex passes uint8)
    got = attention_bshd(q, k, v, 0.0, key_padding_mask=kpm.to(torch.uint8))
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)
    # masked keys carry no weight: changing their values changes nothing
    v2 = v.clone()
    v2[0, 7:] += 100.0
    torch.testing.assert_close(attention_bshd(q, k, v2, 0.0, key_padding_mask=kpm)[0], want[0],
                               rtol=1e-5, atol=1e-5)


def test_attention_bshd_additive_key_padding_mask():
    from apex_example_amd.contrib.multihead_attn._common import attention_bshd

    q, k, v = _qkv()
    torch.manual_seed(1)
    bias = torch.randn(3, 10)
    bias[2, 5:] = float("-inf")
    got = attention_bshd(q, k, v, 0.0, key_padding_mask=bias, mask_additive=True)
    torch.testing.assert_close(got, _manual(q, k, v, bias), rtol=1e-5, atol=1e-5)


def test_attention_bshd_attn_mask_with_key_padding_mask():
    from apex_example_amd.contrib.multihead_attn._common import attention_bshd

    q, k, v = _qkv()
    kpm = torch.zeros(3, 10, dtype=torch.bool)
    kpm[:, 8:] = True
    am = torch.ones(10, 10).triu(1).bool()
    got = attention_bshd(q, k, v, 0.0, key_padding_mask=kpm, attn_mask=am)
    s = torch.einsum("bqhd,bkhd->bhqk", q, k) / 8.0
    s = s.masked_fill(am.view(1, 1, 10, 10) | kpm.view(3, 1, 1, 10), float("-inf"))
    want = torch.einsum("bhqk,bkhd->bqhd", torch.softmax(s, -1), v)
    torch.testing.assert_close(got, want, rtol=1e-5, atol=1e-5)


def test_bert_additive_mask_convention():
    from apex_example_amd.models.bert import additive_attention_mask

    am = torch.tensor([[1, 1, 0], [1, 0, 0]])
    got = additive_attention_mask(am, torch.float32)
    assert torch.equal(got, torch.tensor([[0.0, 0.0, -10000.0], [0.0, -10000.0, -10000.0]]))
    assert additive_attention_mask(am.bool(), torch.float32).equal(got)
    assert additive_attention_mask(am, torch.bfloat16).dtype == torch.bfloat16


@pytest.mark.parametrize("fused_attention", [True, False])
def test_bert_model_attention_mask_on_cpu_is_sdpa(fused_attention, monkeypatch):
    """fp32 on the CPU is ineligible for the fused kernels whatever the config says: the
    model must take SDPA with the -10000 additive mask, and padded keys must not matter."""
    from apex_example_amd.models.bert import BertConfig, BertModel

    calls = []
    real = F.scaled_dot_product_attention

    def spy(q, k, v, attn_mask=None, **kw):
        calls.append(attn_mask)
        return real(q, k, v, attn_mask=attn_mask, **kw)

    monkeypatch.setattr(F, "scaled_dot_product_attention", spy)
    torch.manual_seed(0)
    cfg = BertConfig(vocab_size=100, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
                     intermediate_size=256, hidden_dropout_prob=0.0,
                     attention_probs_dropout_prob=0.0, max_position_embeddings=32,
                     fused_layer_norm=False, fused_dense=False, fused_attention=fused_attention)
    m = BertModel(cfg).eval()
    ids = torch.randint(0, 100, (2, 12))
    tt = torch.zeros(2, 12, dtype=torch.long)
    am = torch.ones(2, 12, dtype=torch.long)
    am[1, 8:] = 0
    y, _ = m(ids, tt, am)
    assert len(calls) == 2 and all(c is not None and c.shape == (2, 1, 1, 12) for c in calls)
    assert torch.equal(calls[0][1, 0, 0], torch.tensor([0.0] * 8 + [-10000.0] * 4))
    # tokens under the padding do not reach the kept positions
    ids2 = ids.clone()
    ids2[1, 8:] = (ids[1, 8:] + 1) % 100
    y2, _ = m(ids2, tt, am)
    torch.testing.assert_close(y2[1, :8], y[1, :8], rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(y2[0], y[0], rtol=1e-6, atol=1e-6)
    # and without a mask they do
    y3, _ = m(ids, tt)
    assert not torch.allclose(y3[1, :8], y[1, :8], atol=1e-4)


def test_fused_ops_reject_conflicting_or_cpu_masks():
    """Argument checks that need no GPU: both mask forms at once, wrong shapes, CPU masks."""
    from apex_example_amd.ops.attention import _key_mask, prepare_key_mask

    q = torch.zeros(2, 8, 1, 64)
    assert _key_mask(None, None, q) == (None, None)
    with pytest.raises(ValueError, match="not both"):
        _key_mask(torch.zeros(2, 8, dtype=torch.bool), torch.zeros(2, 8), q)
    with pytest.raises(ValueError, match=r"\[B, S\]"):
        _key_mask(torch.zeros(2, 9, dtype=torch.bool), None, q)
    with pytest.raises(ValueError, match="GPU"):
        prepare_key_mask(torch.zeros(2, 8, dtype=torch.bool))
