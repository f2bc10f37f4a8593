"""GPT2Config(n_kv_head=): runs on the SDPA fallback; None leaves the state dict as it was."""
import torch

from apex_example_amd.models.gpt2 import GPT2Config, GPT2LMHeadModel

KW = dict(vocab_size=64, n_positions=32, n_embd=64, n_layer=1, n_head=4, fused_layer_norm=False,
          fused_dense=False, fused_residual_ln=False)


def test_n_kv_head_runs_on_the_fallback_and_none_changes_nothing():
    torch.manual_seed(0)
    m = GPT2LMHeadModel(GPT2Config(n_kv_head=2, **KW)).eval()
    y = m(torch.randint(0, 64, (2, 16)))
    y.sum().backward()
    assert y.shape == (2, 16, 64) and torch.isfinite(y).all()
    shapes = {k: tuple(v.shape) for k, v in GPT2LMHeadModel(GPT2Config(**KW)).state_dict().items()}
    assert shapes["h.0.attn.c_attn.weight"] == (3 * 64, 64)
    grouped = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    assert (grouped.pop("h.0.attn.c_attn.weight"), grouped.pop("h.0.attn.c_attn.bias")) == ((128, 64), (128,))
    assert all(shapes[k] == s for k, s in grouped.items()) and len(grouped) == len(shapes) - 2
