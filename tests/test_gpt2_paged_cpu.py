"""GPT-2 with a PagedKVCache on the CPU in fp32: the filled rows gathered through the table
for the SDPA fallback of the cached attention path."""
import pytest
import torch

from apex_example_amd.models.gpt2 import PagedKVCache
from test_gpt2_generate_cpu import tiny


@pytest.mark.parametrize("n_kv_head", [None, 2])
def test_paged_generate_gives_the_contiguous_tokens(n_kv_head):
    model = tiny(n_kv_head)
    ids = torch.randint(0, 97, (2, 15))  # 15 + 6 tokens: the decode steps cross a page edge
    assert torch.equal(model.generate(ids, 6, page_size=16), model.generate(ids, 6))


def test_table_is_disjoint_and_interleaved():
    cache = PagedKVCache(3, 70, page_size=16)
    t = cache.block_table
    assert t.dtype == torch.int32 and t.shape == (3, 5) and cache.num_pages == 15
    assert sorted(t.flatten().tolist()) == list(range(15))
    assert t[:, 0].tolist() == [0, 1, 2] and t[1].tolist() == [1, 4, 7, 10, 13]
    with pytest.raises(ValueError):
        PagedKVCache(3, 70, page_size=48)
