"""Packed variable-length attention without a GPU: ``contrib.fmha.FMHA``'s per-sequence
SDPA fallback against an explicit per-sequence softmax(q k^T / 8) v, BERT's ``unpad``
option against the padded model at the kept positions, and the argument checks of the
packed ops that run before any native call."""
import itertools
from types import SimpleNamespace

import pytest
import torch


def _cu(lens):
    return torch.tensor([0] + list(itertools.accumulate(lens)), dtype=torch.int32)


def _fmha(hidden=128, heads=2, p=0.0):
    from apex_example_amd.contrib.fmha import FMHA

    return FMHA(SimpleNamespace(attention_probs_dropout_prob=p, num_attention_heads=heads,
                                hidden_size=hidden))


def _ref(qkv, lens, heads):
    """qkv [T, 3 * hidden] laid out [T, 3, H, 64] -> [T, hidden], sequence by sequence"""
    T = qkv.size(0)
    x = qkv.view(T, 3, heads, 64)
    outs, s = [], 0
    for n in lens:
        q, k, v = x[s:s + n].unbind(1)          # [n, H, 64]
        pr = torch.softmax(torch.einsum("qhd,khd->hqk", q, k) / 8.0, -1)
        outs.append(torch.einsum("hqk,khd->qhd", pr, v))
        s += n
    return torch.cat(outs).reshape(T, heads * 64)


def test_fmha_fallback_matches_per_sequence_softmax():
    lens, heads = [3, 0, 17, 1], 2
    T = sum(lens)
    torch.manual_seed(0)
    qkv = torch.randn(T, 3 * heads * 64)
    dy = torch.randn(T, heads * 64)
    a = qkv.clone().requires_grad_(True)
    y = _fmha()(a, _cu(lens), max(lens), is_training=True, zero_tensors=True)   # p = 0
    y.backward(dy)
    r = qkv.clone().requires_grad_(True)
    yr = _ref(r, lens, heads)
    yr.backward(dy)
    assert y.shape == (T, heads * 64) and a.grad.shape == qkv.shape
    torch.testing.assert_close(y, yr, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(a.grad, r.grad, rtol=1e-5, atol=1e-5)


def test_fmha_eval_ignores_dropout_and_sequences_do_not_mix():
    lens = [4, 9]
    m = _fmha(p=0.5)
    torch.manual_seed(1)
    qkv = torch.randn(sum(lens), 3 * 128)
    y = m(qkv, _cu(lens), 9, is_training=False)
    torch.testing.assert_close(y, _ref(qkv, lens, 2), rtol=1e-5, atol=1e-5)
    other = qkv.clone()
    other[4:] = torch.randn(9, 3 * 128)
    assert torch.equal(m(other, _cu(lens), 9, is_training=False)[:4], y[:4])


def test_fmha_rejects_offsets_that_do_not_cover_the_tokens():
    qkv = torch.randn(10, 3 * 128)
    for cu in ([0, 4, 9], [1, 4, 10], [0, 6, 4, 10]):
        with pytest.raises(ValueError, match="cu_seqlens"):
            _fmha()(qkv, torch.tensor(cu, dtype=torch.int32), 10)


@pytest.mark.parametrize("pattern", ["right", "holes"])
def test_bert_unpad_matches_padded_model_cpu(pattern):
    from apex_example_amd.models.bert import BertConfig, BertForPreTraining, BertModel

    kw = dict(vocab_size=128, hidden_size=128, num_hidden_layers=2, num_attention_heads=2,
              intermediate_size=256, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0,
              max_position_embeddings=64)
    torch.manual_seed(0)
    a = BertModel(BertConfig(unpad=True, **kw))
    r = BertModel(BertConfig(**kw))
    r.load_state_dict(a.state_dict())
    B, S = 4, 24
    ids = torch.randint(0, 128, (B, S))
    tt = torch.zeros(B, S, dtype=torch.long)
    keep = torch.arange(S).view(1, S) < torch.tensor([24, 13, 1, 8]).view(B, 1)
    if pattern == "holes":      # left padding and holes: tokens keep their positions
        keep = keep.roll(5, 1)
        keep[:, 0] = True       # the pooler reads position 0
        keep[0, 7] = False
    am = keep.long()
    ya, pa = a(ids, tt, am)
    yr, pr = r(ids, tt, am)
    dy = torch.randn_like(yr) * keep.unsqueeze(-1)
    (ya * dy).sum().backward()
    (yr * dy).sum().backward()
    assert ya.shape == yr.shape
    torch.testing.assert_close(ya[keep], yr[keep], rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(pa, pr, rtol=1e-4, atol=1e-4)
    assert (ya[~keep] == 0).all()
    torch.testing.assert_close(a.layers[0].attention.qkv.weight.grad,
                               r.layers[0].attention.qkv.weight.grad, rtol=1e-4, atol=1e-4)
    # without a mask unpad changes nothing, and the pre-training head indexes as before
    torch.testing.assert_close(a(ids, tt)[0], r(ids, tt)[0], rtol=0, atol=0)
    torch.manual_seed(0)
    full = BertForPreTraining(BertConfig(unpad=True, **kw))
    logits, nsp = full(ids, tt, torch.tensor([[0, 3]] * B), am)
    assert logits.shape == (B * 2, 128) and nsp.shape == (B, 2)


def test_varlen_argument_validation_cpu():
    from apex_example_amd.ops import fused_attention_varlen, fused_attention_varlen_qkv

    q = torch.randn(10, 1, 64)
    ok = _cu([4, 6])
    with pytest.raises(ValueError, match="key masks"):
        fused_attention_varlen(q, q, q, ok, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="key masks"):
        fused_attention_varlen(q, q, q, ok, key_bias=torch.zeros(2, 6))
    with pytest.raises(ValueError, match="int32"):
        fused_attention_varlen(q, q, q, ok.long())
    with pytest.raises(ValueError, match="1-D"):
        fused_attention_varlen(q, q, q, ok.view(1, 3))
    with pytest.raises(ValueError, match="1-D"):
        fused_attention_varlen(q, q, q, [0, 4, 10])
    with pytest.raises(ValueError, match="start at 0"):
        fused_attention_varlen(q, q, q, torch.tensor([2, 4, 10], dtype=torch.int32))
    with pytest.raises(ValueError, match="non-decreasing"):
        fused_attention_varlen(q, q, q, torch.tensor([0, 12, 10], dtype=torch.int32))
    with pytest.raises(ValueError, match="end at T"):
        fused_attention_varlen(q, q, q, torch.tensor([0, 4, 9], dtype=torch.int32))
    with pytest.raises(ValueError, match="max_seqlen"):
        fused_attention_varlen(q, q, q, ok, max_seqlen=-3)
    with pytest.raises(ValueError, match="qkv must be"):
        fused_attention_varlen_qkv(q, ok)
