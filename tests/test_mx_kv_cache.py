"""MXFP8 KV cache (inference/kv_cache.py MXKVCache) on the CPU: the stored
layout is pack_mx(quantize_mx(.)) along D byte for byte, both update modes
agree, a model run on it is torch.equal to the same model run on a cache that
fake-quantizes K and V (and differs from the unquantized run), construction
and the public interface, byte accounting."""

import pytest
import torch

from dist_utils import run_distributed

from neuronx_distributed_amd.inference import (KVCache, MXKVCache,
                                               RollingKVCache,
                                               build_kv_caches)
from neuronx_distributed_amd.quantization.microscaling import (
    dequantize_mx, pack_mx, quantize_mx)

FMT = "fp8_e4m3"


def _packed(x):
    return pack_mx(*quantize_mx(x, FMT), FMT)


def _rand(B, H, S, D, seed):
    g = torch.Generator().manual_seed(seed)
    # a spread of block magnitudes, so the scale bytes differ
    mag = torch.exp2(torch.randint(-6, 7, (B, H, S, D // 32, 1),
                                   generator=g).float())
    x = torch.randn(B, H, S, D // 32, 32, generator=g) * mag
    return x.reshape(B, H, S, D)


def _buffers(c):
    return c.k, c.k_scale, c.v, c.v_scale


def test_layout_matches_pack_mx():
    B, H, Smax, D = 2, 3, 16, 64
    c = MXKVCache(B, H, Smax, D, dtype=torch.float32, device="cpu")
    for t in _buffers(c):
        assert t.dtype == torch.uint8 and not t.any()
    assert c.k.shape == (B, H, Smax, D) and c.k_scale.shape == (B, H, Smax, 2)
    k0, v0 = _rand(B, H, 5, D, 0), _rand(B, H, 5, D, 1)
    K, V = c.update(k0, v0, 0)
    assert K.shape == (B, H, 5, D) and K.dtype == torch.float32
    # the returned view is what the cache holds, the pos-0 prefill included
    assert torch.equal(K, dequantize_mx(*quantize_mx(k0, FMT),
                                        dtype=torch.float32))
    assert torch.equal(V, dequantize_mx(*quantize_mx(v0, FMT),
                                        dtype=torch.float32))
    k1, v1 = _rand(B, H, 3, D, 2), _rand(B, H, 3, D, 3)
    K, V = c.update(k1, v1, 7)
    assert K.shape == (B, H, 10, D)
    for buf, sbuf, a, b in ((c.k, c.k_scale, k0, k1), (c.v, c.v_scale, v0, v1)):
        p0, s0 = _packed(a)
        p1, s1 = _packed(b)
        assert torch.equal(buf[:, :, 0:5], p0)
        assert torch.equal(sbuf[:, :, 0:5], s0)
        assert torch.equal(buf[:, :, 7:10], p1)
        assert torch.equal(sbuf[:, :, 7:10], s1)
        for lo, hi in ((5, 7), (10, Smax)):   # never written: still zero
            assert not buf[:, :, lo:hi].any() and not sbuf[:, :, lo:hi].any()
    assert torch.equal(K[:, :, 7:10], dequantize_mx(*quantize_mx(k1, FMT),
                                                    dtype=torch.float32))
    assert not K[:, :, 5:7].any()


@pytest.mark.parametrize("p", [0, 4, 11])
def test_tensor_pos_equals_int_pos(p):
    B, H, Smax, D = 2, 2, 12, 32
    a = MXKVCache(B, H, Smax, D, dtype=torch.float32, device="cpu")
    b = MXKVCache(B, H, Smax, D, dtype=torch.float32, device="cpu")
    pre_k, pre_v = _rand(B, H, 3, D, 4), _rand(B, H, 3, D, 5)
    a.update(pre_k, pre_v, 0)
    b.update(pre_k, pre_v, 0)
    k, v = _rand(B, H, 1, D, 6), _rand(B, H, 1, D, 7)
    Ka, Va = a.update(k, v, p)
    Kb, Vb = b.update(k, v, torch.tensor([p]))
    for x, y in zip(_buffers(a), _buffers(b)):
        assert torch.equal(x, y)
    assert Ka.shape == (B, H, p + 1, D)
    assert Kb.shape == (B, H, Smax, D) and Vb.shape == (B, H, Smax, D)
    assert torch.equal(Kb[:, :, :p + 1], Ka)
    assert torch.equal(Vb[:, :, :p + 1], Va)


class _FakeQuantKVCache(KVCache):
    """A plain fp32 cache that stores K and V after a quantize-dequantize
    round trip: what MXKVCache must be indistinguishable from."""

    def update(self, k_new, v_new, pos):
        fq = lambda x: dequantize_mx(*quantize_mx(x, FMT),  # noqa: E731
                                     dtype=torch.float32)
        return super().update(fq(k_new), fq(v_new), pos)


def _parity_worker(rank, world):
    from neuronx_distributed_amd.inference import generate
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    # tiny with head_dim 32 (one MX block per head row)
    cfg = get_config("tiny", hidden_size=128, max_position_embeddings=64)
    assert cfg.head_dim == 32
    torch.manual_seed(0)
    model = LlamaForCausalLM(cfg).eval()
    B, S, steps = 2, 6, 5
    n_kv, L = cfg.num_key_value_heads, cfg.num_hidden_layers
    Smax = S + 2 * steps + 1

    def run(make):
        caches = [make() for _ in range(L)]
        torch.manual_seed(1)
        x = torch.randint(0, 256, (B, S))
        got = []
        with torch.no_grad():
            logits = model(x, kv_caches=caches, pos_offset=0)
            got.append(logits)
            tok = logits[:, -1, :].argmax(-1, keepdim=True)
            pos = S
            for step in range(2 * steps):
                # int positions first, then device-tensor positions
                po = pos if step < steps else torch.tensor([pos])
                logits = model(tok, kv_caches=caches, pos_offset=po)
                got.append(logits)
                # feed a fixed token stream so the three runs see one input
                tok = (tok + 7) % 256
                pos += 1
        return got

    mx = run(lambda: MXKVCache(B, n_kv, Smax, cfg.head_dim,
                               dtype=torch.float32, device="cpu"))
    fake = run(lambda: _FakeQuantKVCache(B, n_kv, Smax, cfg.head_dim,
                                         dtype=torch.float32, device="cpu"))
    plain = run(lambda: KVCache(B, n_kv, Smax, cfg.head_dim,
                                dtype=torch.float32, device="cpu"))
    assert len(mx) == 1 + 2 * steps
    for i, (a, b) in enumerate(zip(mx, fake)):
        assert torch.equal(a, b), (i, (a - b).abs().max())
    # not a no-op: the quantized cache changes every logit tensor
    for i, (a, b) in enumerate(zip(mx, plain)):
        assert not torch.equal(a, b), i

    # generate() threads kv_format down to the caches
    torch.manual_seed(2)
    x = torch.randint(0, 256, (B, S))
    out = generate(model, x, max_new_tokens=4, kv_format="mxfp8")
    assert out.shape == (B, S + 4) and torch.equal(out[:, :S], x)
    return True


def test_model_parity_with_fake_quant_cache():
    run_distributed(_parity_worker, world_size=1)


def test_construction_and_interface():
    with pytest.raises(ValueError):
        MXKVCache(1, 1, 8, 48, device="cpu")
    with pytest.raises(NotImplementedError):
        build_kv_caches(2, 1, 1, 16, 32, device="cpu", window=8,
                        kv_format="mxfp8")
    with pytest.raises(ValueError):
        build_kv_caches(2, 1, 1, 16, 32, device="cpu", kv_format="fp4")
    # a window that does not bind is no rolling cache
    cs = build_kv_caches(2, 1, 1, 16, 32, device="cpu", window=16,
                         kv_format="mxfp8")
    assert [type(c) for c in cs] == [MXKVCache, MXKVCache]
    assert cs[0].dtype == torch.bfloat16
    cs = build_kv_caches(2, 1, 1, 16, 32, dtype=torch.float32, device="cpu",
                         kv_format="mxfp8")
    assert cs[0].dtype == torch.float32 and cs[0].k.dtype == torch.uint8
    # kv_format=None: exactly today's classes
    cs = build_kv_caches(2, 1, 1, 16, 32, device="cpu", kv_format=None)
    assert [type(c) for c in cs] == [KVCache, KVCache]
    assert cs[0].k.dtype == torch.bfloat16
    cs = build_kv_caches(2, 1, 1, 16, 32, device="cpu", window=8)
    assert [type(c) for c in cs] == [RollingKVCache, RollingKVCache]
    cs = build_kv_caches(1, 1, 1, 16, 32, device="cpu", window=16)
    assert type(cs[0]) is KVCache


def test_byte_accounting():
    B, H, Smax, D = 3, 2, 40, 128
    c = MXKVCache(B, H, Smax, D, device="cpu")
    total = sum(t.nbytes for t in _buffers(c))
    assert total == 2 * B * H * Smax * (D + D // 32)
    bf16 = KVCache(B, H, Smax, D, device="cpu")
    assert total / (bf16.k.nbytes + bf16.v.nbytes) == 132 / 256
