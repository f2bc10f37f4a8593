"""generate(prefill_chunk=) and chunked cached forwards on the CPU in fp32 (the SDPA fallback)."""
import pytest
import torch

from apex_example_amd.models.gpt2 import KVCache
from test_gpt2_generate_cpu import tiny


@pytest.mark.parametrize("n_kv_head", [None, 2])
def test_chunked_generate_and_logits(n_kv_head):
    model = tiny(n_kv_head)
    ids = torch.randint(0, 97, (2, 12))
    assert torch.equal(model.generate(ids, 6, prefill_chunk=5), model.generate(ids, 6))
    with torch.no_grad():
        cache = KVCache(2, 12)
        parts = [model(ids[:, c:c + 5], cache=cache) for c in (0, 5, 10)]
        assert (torch.cat(parts, 1) - model(ids)).abs().max().item() < 1e-4
    with pytest.raises(ValueError):
        model.generate(ids, 6, prefill_chunk=0)
