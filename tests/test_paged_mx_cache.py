"""CPU checks of the paged MXFP8 KV cache (inference.kv_cache.PagedMXKVCache)
against MXKVCache on the same rows, through a permuted block table: stored
bytes, dequantized views, inactive sequences, chunk_lens padding and
build_kv_caches(kv_format="paged_mxfp8")."""

import pytest
import torch

from neuronx_distributed_amd.inference.kv_cache import (
    PAGE_ROWS, MXKVCache, PagedMXKVCache, PagePool, build_kv_caches)
from neuronx_distributed_amd.quantization.microscaling import (
    pack_mx, quantize_mx)

B, H, D, PPS, NP = 3, 2, 64, 3, 9
SMAX = PPS * PAGE_ROWS


@pytest.fixture
def caches():
    pool = PagePool(NP, B, PPS, "cpu")
    pool.block_table.copy_(torch.tensor([[4, 0, 6], [2, 8, 7], [3, 5, 1]]))
    paged, = build_kv_caches(1, B, H, SMAX, D, dtype=torch.float32,
                             device="cpu", kv_format="paged_mxfp8",
                             page_pool=pool)
    assert type(paged) is PagedMXKVCache and paged.max_seq == SMAX
    return pool, paged, MXKVCache(B, H, SMAX, D, torch.float32, "cpu")


def _pools(c):
    return [t.clone() for t in (c._k, c._ks, c._v, c._vs)]


def _rows(pages, table):   # (B, H, SMAX, W): every sequence's rows in order
    x = pages[table.long()].transpose(1, 2)
    return x.reshape(B, H, SMAX, pages.shape[-1])


def test_prefill_and_ragged_decode_equal_dense_mx(caches):
    pool, paged, dense = caches
    torch.manual_seed(0)
    S = 21
    k, v = torch.randn(2, B, H, S, D) * torch.exp2(
        torch.randint(-6, 7, (2, B, H, S, D // 32, 1)).float()
    ).expand(2, B, H, S, D // 32, 32).reshape(2, B, H, S, D)
    assert paged.update(k, v, 0)[0] is k
    dense.update(k, v, 0)
    pos = torch.tensor([21, 16, 47])      # mid-page, page start, last row
    for step in range(2):
        k1, v1 = torch.randn(2, B, H, 1, D)
        got = paged.update(k1, v1, pos + step * torch.tensor([1, 1, 0]))
        want = dense.update(k1, v1, pos + step * torch.tensor([1, 1, 0]))
        assert all(torch.equal(a, w) for a, w in zip(got, want))
    assert all(torch.equal(a, w) for a, w in zip(paged.gather(), got))
    # stored bytes: MXKVCache's, i.e. pack_mx(quantize_mx(row))
    for pay, scl, dp, ds in (
            (paged.k_pages, paged.k_scale_pages, dense.k, dense.k_scale),
            (paged.v_pages, paged.v_scale_pages, dense.v, dense.v_scale)):
        assert torch.equal(_rows(pay, pool.block_table), dp)
        assert torch.equal(_rows(scl, pool.block_table), ds)
    ep, es = pack_mx(*quantize_mx(k[1, :, 5], "fp8_e4m3"), "fp8_e4m3")
    assert torch.equal(paged.k_pages[2, :, 5], ep)
    assert torch.equal(paged.k_scale_pages[2, :, 5], es)
    with pytest.raises(NotImplementedError):
        paged.update(k, v, 5)


@pytest.mark.parametrize("pos,poison", [
    ((-1, 20, SMAX), {}),                       # positions out of range
    ((20, 20, 40), {0: (1, -1), 2: (0, NP)})])  # entry at / before the page
def test_inactive_sequences_leave_the_pools(caches, pos, poison):
    pool, paged, _ = caches
    for b, (j, entry) in poison.items():
        pool.block_table[b, j] = entry
    pos = torch.tensor(pos)
    assert paged.active(pos).tolist() == [False, True, False]
    before = _pools(paged)
    k1, v1 = torch.randn(2, B, H, 1, D) + 3.0
    paged.update(k1, v1, pos)
    after = _pools(paged)
    pg, slot = int(pool.block_table[1, 20 // PAGE_ROWS]), 20 % PAGE_ROWS
    assert after[0][pg, :, slot].any() and after[3][pg, :, slot].any()
    for a, b in zip(after, before):   # all four pools, but sequence 1's row
        b[pg, :, slot] = a[pg, :, slot]
        assert torch.equal(a[:NP], b[:NP])


def test_chunk_lens_padding_stores_nothing(caches):
    pool, paged, dense = caches
    S, pos = 12, torch.tensor([10, 0, 30])
    lens = torch.tensor([12, 0, 3])            # sequence 1 is inactive
    k, v = torch.randn(2, B, H, S, D)
    before = _pools(paged)
    paged.update(k, v, pos, lens)
    want = torch.zeros(B, H, SMAX, D, dtype=torch.uint8)
    for b in (0, 2):
        n, p = int(lens[b]), int(pos[b])
        want[b, :, p:p + n] = pack_mx(
            *quantize_mx(k[b, :, :n], "fp8_e4m3"), "fp8_e4m3")[0]
    assert torch.equal(_rows(paged.k_pages, pool.block_table), want)
    assert not _rows(paged.v_scale_pages, pool.block_table)[2, :, 33:].any()
    assert torch.equal(paged.v_pages[2], before[2][2])   # sequence 1, page 0


def test_build_kv_caches_contract():
    pool = PagePool(4, 2, 2, "cpu")
    kw = dict(dtype=torch.float32, device="cpu", kv_format="paged_mxfp8")
    assert len(build_kv_caches(2, 2, H, 32, D, page_pool=pool, **kw)) == 2
    with pytest.raises(NotImplementedError):
        build_kv_caches(1, 2, H, 32, D, window=8, page_pool=pool, **kw)
    with pytest.raises(ValueError):
        build_kv_caches(1, 2, H, 32, D, **kw)
    with pytest.raises(ValueError):             # no whole MX block
        build_kv_caches(1, 2, H, 32, 48, page_pool=pool, **kw)
