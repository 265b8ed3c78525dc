"""CPU checks of the paged KV cache (inference.kv_cache): the allocator, the
gather / scatter reference path, and generate(kv_format="paged") against the
dense per-sequence generation in fp32, both the same exact eager chain."""

import pytest
import torch

from dist_utils import run_distributed
from neuronx_distributed_amd.inference.kv_cache import (
    PAGE_ROWS, PagedKVCache, PagePool, build_kv_caches)


def test_pool_allocate_release_reuse():
    pool = PagePool(5, 2, 3, "cpu")
    pool.allocate(0, 17)                      # 2 pages
    pool.allocate(1, 1)
    pool.allocate(0, 20)                      # still 2 pages
    assert pool.block_table.tolist() == [[0, 1, -1], [2, -1, -1]]
    pool.allocate(0, 48)
    with pytest.raises(RuntimeError):         # needs 2, 1 is free
        pool.allocate(1, 48)
    with pytest.raises(ValueError):           # more than pages_per_seq
        pool.allocate(1, 49)
    assert pool.block_table[1].tolist() == [2, -1, -1] and pool.num_free == 1
    pool.release(0)
    assert pool.block_table[0].tolist() == [-1, -1, -1] and pool.num_free == 4
    pool.allocate(1, 48)
    assert sorted(pool.block_table[1].tolist() + pool._free) == [0, 1, 2, 3, 4]


def test_update_gather_round_trip():
    B, H, D, S = 3, 2, 8, 21
    pool = PagePool(7, B, 3, "cpu")
    # unordered; 7 = num_pages and -1 name no page; sequence 2 has one page
    table = torch.tensor([[4, 0, 6], [2, 5, 7], [3, -1, -1]]).int()
    pool.block_table.copy_(table)
    cache, = build_kv_caches(1, B, H, 48, D, dtype=torch.float32,
                             device="cpu", kv_format="paged", page_pool=pool)
    assert type(cache) is PagedKVCache
    torch.manual_seed(0)
    k, v = torch.randn(2, B, H, S, D)
    assert cache.update(k, v, 0)[0] is k
    want = torch.zeros(2, B, H, 3 * PAGE_ROWS, D)
    for b in range(B):
        for r in range(S):
            if 0 <= table[b, r // PAGE_ROWS] < 7:
                want[:, b, :, r] = torch.stack((k[b, :, r], v[b, :, r]))
    assert not want[0, 2, :, 16:21].any() and want[0, 1, :, 16:21].any()
    assert all(torch.equal(a, w) for a, w in zip(cache.gather(), want))
    # decode: a position outside [0, 48) or an invalid page is inactive
    pos = torch.tensor([-1, 21, 48])
    assert cache.active(pos).tolist() == [False, True, False]
    assert cache.active(torch.tensor([16, 32, 15])).tolist() == [
        True, False, True]
    assert cache.active(torch.tensor([46, 30, 16]), 2).tolist() == [
        True, True, False]
    k1, v1 = torch.randn(2, B, H, 1, D)
    got = cache.update(k1, v1, pos)
    want[0, 1, :, 21], want[1, 1, :, 21] = k1[1, :, 0], v1[1, :, 0]
    assert all(torch.equal(a, w) for a, w in zip(got, want))
    with pytest.raises(NotImplementedError):
        cache.update(k, v, 5)
    with pytest.raises(NotImplementedError):
        build_kv_caches(1, B, H, 48, D, window=8, kv_format="paged",
                        page_pool=pool)


def _generate_worker(rank, world):
    from neuronx_distributed_amd.inference import generation
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg = get_config("tiny")
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    lens, N = [9, 4, 6], 8
    x = torch.randint(1, cfg.vocab_size, (3, 9))
    for b, n in enumerate(lens):
        x[b, n:] = 0
    dense = generation.generate(model, x, max_new_tokens=N, prompt_lens=lens)
    paged = generation.generate(model, x, max_new_tokens=N, prompt_lens=lens,
                                kv_format="paged")
    assert paged.shape == (3, 9 + N) and torch.equal(paged, dense), \
        (paged, dense)
    return True


def test_generate_paged_equals_dense_fp32():
    run_distributed(_generate_worker, world_size=1)
