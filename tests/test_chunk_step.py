"""The multi-token decode step with a device position, on the CPU in fp32
(models/llama.py LlamaAttention._cached_step, the eager chain that is also
the reference of the fused GPU kernels of test_chunk_attn_gpu.py):

* a tensor-position forward of S in {2, 5, 8} tokens equals the int-position
  forward on a copy of the caches, logits and cache contents, for KVCache and
  MXKVCache,
* S == 1 with a tensor position is still exactly _cached_step,
* eight one-token steps into a RollingKVCache (sliding window 4) equal the
  int-position steps,
* RollingKVCache refuses a multi-token tensor-position update,
* speculative_generate / medusa_generate with fused_verify=True return the
  tokens of the default path and of plain greedy generation.
"""

import copy

import pytest
import torch

from dist_utils import run_distributed


def _models(seed, **cfg_over):
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config

    cfg = get_config("tiny", **cfg_over)
    torch.manual_seed(seed)
    return cfg, LlamaForCausalLM(cfg).eval()


def _caches(cfg, B, max_seq, kv_format, window=None):
    from neuronx_distributed_amd.inference.kv_cache import build_kv_caches

    return build_kv_caches(cfg.num_hidden_layers, B, cfg.num_key_value_heads,
                           max_seq, cfg.head_dim, dtype=torch.float32,
                           device="cpu", kv_format=kv_format, window=window)


def _buffers(c):
    return [getattr(c, n) for n in ("k", "v", "k_scale", "v_scale")
            if hasattr(c, n)]


def _chunk_worker(rank, world, kv_format):
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    # head_dim 32: the smallest an MXKVCache takes
    cfg, model = _models(0, hidden_size=128)
    B, P, Smax = 2, 11, 24
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (B, P + 8))
    with torch.no_grad():
        base = _caches(cfg, B, Smax, kv_format)
        model(x[:, :P], kv_caches=base, pos_offset=0)
        for S in (2, 5, 8):
            c_t, c_i = copy.deepcopy(base), copy.deepcopy(base)
            chunk = x[:, P:P + S]
            got = model(chunk, kv_caches=c_t, pos_offset=torch.tensor([P]))
            want = model(chunk, kv_caches=c_i, pos_offset=P)
            assert got.shape == want.shape == (B, S, cfg.vocab_size)
            assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), \
                (kv_format, S, (got - want).abs().max())
            for a, b in zip(c_t, c_i):
                for ta, tb in zip(_buffers(a), _buffers(b)):
                    if ta.dtype == torch.uint8:
                        assert torch.equal(ta, tb), (kv_format, S)
                    else:
                        assert torch.allclose(ta, tb, atol=1e-6, rtol=0)
                # rows beyond the chunk were not touched
                for ta, t0 in zip(_buffers(a), _buffers(base[0])):
                    assert not ta[:, :, P + S:].any()
    return True


@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_chunk_forward_equals_int_position(kv_format):
    run_distributed(_chunk_worker, world_size=1, args=(kv_format,))


def _single_worker(rank, world):
    """S == 1: forward() still hands a tensor position to _cached_step."""
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, model = _models(0)
    attn = model.model.layers[0].self_attn
    B, P, Smax = 2, 7, 16
    torch.manual_seed(2)
    hidden = torch.randn(B, 1, cfg.hidden_size)
    cos, sin = model.model.rope_cos, model.model.rope_sin
    pos_t = torch.tensor([P])
    with torch.no_grad():
        base = _caches(cfg, B, Smax, None)[0]
        base.k.normal_()
        base.v.normal_()
        c1, c2 = copy.deepcopy(base), copy.deepcopy(base)
        got = attn(hidden, cos, sin, pos_t, c1)
        q, k, v = attn.qkv_proj(hidden)
        shp = lambda t, h: t.reshape(B, 1, h, attn.head_dim)  # noqa: E731
        want = attn._cached_step(shp(q, attn.num_heads_local),
                                 shp(k, attn.num_kv_local),
                                 shp(v, attn.num_kv_local), cos, sin, pos_t,
                                 c2, False)
    assert torch.equal(got, want)
    assert torch.equal(c1.k, c2.k) and torch.equal(c1.v, c2.v)
    assert not torch.equal(c1.k, base.k)
    return True


def test_single_token_tensor_position_unchanged():
    run_distributed(_single_worker, world_size=1)


def _rolling_worker(rank, world):
    """The rolling branch of the eager chain: slots masked by their global
    position, and by the window, from a device position."""
    from neuronx_distributed_amd.inference.kv_cache import RollingKVCache
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, model = _models(0, sliding_window=4)
    B, P, Smax = 2, 6, 16
    torch.manual_seed(4)
    x = torch.randint(0, cfg.vocab_size, (B, P + 8))
    with torch.no_grad():
        c_t = _caches(cfg, B, Smax, None, window=4)
        assert all(type(c) is RollingKVCache for c in c_t)
        # the int-position steps: a plain cache, windowed by the attention
        # (a rolling cache takes an int position only for its prefill)
        c_i = _caches(cfg, B, Smax, None)
        model(x[:, :P], kv_caches=c_t, pos_offset=0)
        model(x[:, :P], kv_caches=c_i, pos_offset=0)
        for i in range(P, P + 8):   # the window wraps twice
            tok = x[:, i:i + 1]
            got = model(tok, kv_caches=c_t, pos_offset=torch.tensor([i]))
            want = model(tok, kv_caches=c_i, pos_offset=i)
            assert got.shape == want.shape == (B, 1, cfg.vocab_size)
            assert torch.allclose(got, want, atol=1e-5, rtol=1e-5), \
                (i, (got - want).abs().max())
            for c in c_t:   # the slots hold the last four positions
                assert sorted(c.slot_pos.tolist()) == list(range(i - 3, i + 1))
    return True


def test_rolling_single_token_tensor_position():
    run_distributed(_rolling_worker, world_size=1)


def test_rolling_cache_refuses_chunk():
    from neuronx_distributed_amd.inference.kv_cache import RollingKVCache

    c = RollingKVCache(1, 2, 4, 16, dtype=torch.float32, device="cpu")
    k = torch.randn(1, 2, 3, 16)
    with pytest.raises(NotImplementedError):
        c.update(k, k, torch.tensor([5]))
    assert not c.k.any() and (c.slot_pos == -1).all()
    c.update(k[:, :, :1], k[:, :, :1], torch.tensor([5]))   # one token: fine
    assert c.slot_pos[1] == 5


def test_kv_cache_chunk_update_rows():
    from neuronx_distributed_amd.inference.kv_cache import KVCache, MXKVCache

    for cls in (KVCache, MXKVCache):
        a = cls(2, 2, 12, 32, dtype=torch.float32, device="cpu")
        b = cls(2, 2, 12, 32, dtype=torch.float32, device="cpu")
        torch.manual_seed(3)
        k, v = torch.randn(2, 2, 4, 32), torch.randn(2, 2, 4, 32)
        K, V = a.update(k, v, torch.tensor([5]))
        Ki, Vi = b.update(k, v, 5)
        assert K.shape[2] == 12           # tensor position: the full buffers
        assert torch.equal(K[:, :, :9], Ki) and torch.equal(V[:, :, :9], Vi)
        for ta, tb in zip(_buffers(a), _buffers(b)):
            assert torch.equal(ta, tb)


def _spec_worker(rank, world, kv_format):
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.inference.speculation import (
        medusa_generate, speculative_generate)
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.utils.medusa_utils import MedusaHead

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    over = {"hidden_size": 128} if kv_format else {}
    cfg, target = _models(0, **over)
    _, draft = _models(99, **over)
    torch.manual_seed(7)
    heads = torch.nn.ModuleList(
        [MedusaHead(cfg.hidden_size, cfg.vocab_size) for _ in range(3)])
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (2, 9))

    seen = []
    attn_cls = type(target.model.layers[0].self_attn)
    real = attn_cls._cached_step

    def spy(self, q, *a, **kw):
        if q.shape[1] > 1:   # one-token decode steps take the method too
            seen.append(q.shape[1])
        return real(self, q, *a, **kw)

    attn_cls._cached_step = spy
    try:
        ref = generate(target, x, max_new_tokens=12, kv_format=kv_format)
        assert not seen
        for d in (target, draft):
            dflt, _ = speculative_generate(target, d, x, max_new_tokens=12,
                                           spec_len=3, kv_format=kv_format)
            assert not seen           # the default path never takes the step
            out, rate = speculative_generate(target, d, x, max_new_tokens=12,
                                             spec_len=3, kv_format=kv_format,
                                             fused_verify=True)
            assert torch.equal(out, dflt), (out, dflt)
            if kv_format is None:
                assert torch.equal(out, ref), (out, ref)
            assert 0.0 <= rate <= 1.0
            # the verify chunk (up to spec_len + 1) and the draft's two tokens
            assert 2 in seen and max(seen) == 4 and min(seen) >= 2
            del seen[:]
        dflt, _ = medusa_generate(target, heads, x, max_new_tokens=10,
                                  kv_format=kv_format)
        assert not seen
        out, rate = medusa_generate(target, heads, x, max_new_tokens=10,
                                    kv_format=kv_format, fused_verify=True)
        assert seen and max(seen) == 4
        assert torch.equal(out, dflt), (out, dflt)
        if kv_format is None:
            assert torch.equal(out, generate(target, x, max_new_tokens=10))
    finally:
        attn_cls._cached_step = real
    return True


@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_fused_verify_tokens(kv_format):
    run_distributed(_spec_worker, world_size=1, args=(kv_format,))
