"""CPU checks of the chunked prefill on the paged KV cache through the torch
chain: generate(kv_format="paged", prefill_chunk=N) against the one-shot
prefill in fp32 on right-padded prompts of different lengths, and
PagedKVCache.update / active with ``chunk_lens``.

Prompt lengths (37, 16, 5) against N = 9 (chunk seams inside pages, a last
chunk of one token), 16 (seams on page seams, a sequence that ends exactly on
one) and 24 (a last chunk shorter than N); from the second chunk on the
shorter sequences run with n[b] = 0.  Tokens must be equal.  Pages are
compared on the rows real tokens wrote, [0, len_b + new - 1): beyond them the
one-shot prefill leaves the K/V of its padding, the chunked one nothing."""

import pytest
import torch

from dist_utils import run_distributed
from neuronx_distributed_amd.inference.kv_cache import PagedKVCache, PagePool

LENS, NEW = (37, 16, 5), 4


def _generate_worker(rank, world, chunk):
    from neuronx_distributed_amd.inference import generation
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg = get_config("tiny", max_position_embeddings=64)
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    x = torch.randint(1, cfg.vocab_size, (len(LENS), max(LENS)))
    for b, n in enumerate(LENS):
        x[b, n:] = 0
    built, real = [], generation.build_kv_caches
    generation.build_kv_caches = lambda *a, **kw: (
        built.append(real(*a, **kw)) or built[-1])
    kw = dict(max_new_tokens=NEW, prompt_lens=LENS, kv_format="paged")
    want = generation.generate(model, x, **kw)
    got = generation.generate(model, x, prefill_chunk=chunk, **kw)
    assert torch.equal(got, want), (got, want)
    for a, b in zip(*built):                  # layer by layer
        for ga, gb in zip(a.gather(), b.gather()):
            for i, n in enumerate(LENS):
                torch.testing.assert_close(ga[i, :, :n + NEW - 1],
                                           gb[i, :, :n + NEW - 1],
                                           atol=1e-5, rtol=0)
    for bad in (dict(kv_format=None), dict(prefill_chunk=8)):
        with pytest.raises(ValueError):
            generation.generate(model, x, **{**kw, "prefill_chunk": chunk,
                                             **bad})
    return True


@pytest.mark.parametrize("chunk", (9, 16, 24))
def test_generate_chunked_prefill_equals_one_shot_fp32(chunk):
    run_distributed(_generate_worker, world_size=1, args=(chunk,))


def test_update_active_with_chunk_lens():
    B, H, D, S = 4, 2, 8, 12
    pool = PagePool(8, B, 2, "cpu")
    pool.block_table.copy_(torch.tensor(
        [[4, 0], [2, -1], [3, 7], [6, 1]]).int())
    cache = PagedKVCache(pool, H, D, torch.float32, "cpu")
    torch.manual_seed(0)
    cache._k.normal_()
    cache._v.normal_()
    before = [t.clone() for t in cache.gather()]
    pos = torch.tensor([10, 10, 3, 30])
    # the real rows of sequence 1 end in page 0: its entry -1 is not needed;
    # 0 tokens, and more than S, are inactive; sequence 3 ends on the last row
    lens = torch.tensor([9, 6, 0, 2])
    assert cache.active(pos, S, lens).tolist() == [True, True, False, True]
    assert cache.active(pos, S, torch.tensor([9, 7, 13, 3])).tolist() == [
        True, False, False, False]
    assert cache.active(pos, S).tolist() == [True, False, True, False]
    k, v = torch.randn(2, B, H, S, D)
    got = cache.update(k, v, pos, lens)
    want = [t.clone() for t in before]
    for b, (p, n) in enumerate(zip(pos.tolist(), lens.tolist())):
        want[0][b, :, p:p + n], want[1][b, :, p:p + n] = k[b, :, :n], v[b, :, :n]
    assert all(torch.equal(a, w) for a, w in zip(got, want))
    with pytest.raises(ValueError):
        cache.update(k, v, 0, lens)
