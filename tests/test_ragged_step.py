"""Per-sequence positions on the CPU in fp32 (the eager chain of
models/llama.py LlamaAttention._cached_step, which is also the reference of
the fused ragged kernels of test_ragged_attn_gpu.py):

* a forward of S in {1, 3, 8} tokens with positions (3, 11, -1) equals, row by
  row, the int-position forward of that row alone on its slice of the caches,
  logits and cache contents, for KVCache and MXKVCache; the inactive third row
  keeps its cache bitwise and gets a zero attention output,
* generate(prompt_lens=[5, 9, 2]) returns, row by row, what generate returns
  for the unpadded prompt alone, for both cache formats,
* speculative_generate(per_sequence=True) returns the tokens of greedy
  generate, with and without prompt_lens, and accepts everything when the
  draft is the target,
* RollingKVCache refuses a (B,) position,
* _cached_step refuses a position tensor of neither 1 nor B elements.
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


def _caches(cfg, B, max_seq, kv_format):
    from neuronx_distributed_amd.inference.kv_cache import build_kv_caches

    return build_kv_caches(cfg.num_hidden_layers, B, cfg.num_key_value_heads,
                           max_seq, cfg.head_dim, dtype=torch.float32,
                           device="cpu", kv_format=kv_format)


_NAMES = ("k", "v", "k_scale", "v_scale")


def _buffers(c):
    return [getattr(c, n) for n in _NAMES if hasattr(c, n)]


def _row_caches(cfg, caches, b, max_seq, kv_format):
    """B = 1 caches holding copies of row b of ``caches``."""
    out = _caches(cfg, 1, max_seq, kv_format)
    for src, dst in zip(caches, out):
        for n in _NAMES:
            if hasattr(src, n):
                getattr(dst, n).copy_(getattr(src, n)[b:b + 1])
    return out


def _forward_worker(rank, world, kv_format):
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    # head_dim 32: the smallest an MXKVCache takes
    cfg, model = _models(0, hidden_size=128)
    B, P, Smax = 3, 11, 24
    positions = (3, 11, -1)
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (B, P + 8))
    attn_in = []
    hooks = [layer.self_attn.o_proj.register_forward_pre_hook(
        lambda mod, inp: attn_in.append(inp[0])) for layer in model.model.layers]
    with torch.no_grad():
        base = _caches(cfg, B, Smax, kv_format)
        # every row holds P rows; the ones beyond a row's position are stale
        model(x[:, :P], kv_caches=base, pos_offset=0)
        for S in (1, 3, 8):
            c_t = copy.deepcopy(base)
            chunk = x[:, P:P + S]
            del attn_in[:]
            got = model(chunk, kv_caches=c_t,
                        pos_offset=torch.tensor(positions))
            assert got.shape == (B, S, cfg.vocab_size)
            assert len(attn_in) == cfg.num_hidden_layers
            for a in attn_in:   # the inactive row: zero before o_proj
                assert a.shape[:2] == (B, S)
                assert not a[2].any() and a[0].any() and a[1].any()
            for b in (0, 1):
                c_b = _row_caches(cfg, base, b, Smax, kv_format)
                want = model(chunk[b:b + 1], kv_caches=c_b,
                             pos_offset=positions[b])
                assert torch.allclose(got[b:b + 1], want, atol=1e-5,
                                      rtol=1e-5), \
                    (kv_format, S, b, (got[b:b + 1] - want).abs().max())
                for ct, cb in zip(c_t, c_b):
                    for ta, tb in zip(_buffers(ct), _buffers(cb)):
                        if ta.dtype == torch.uint8:
                            assert torch.equal(ta[b:b + 1], tb), \
                                (kv_format, S, b)
                        else:
                            assert torch.allclose(ta[b:b + 1], tb, atol=1e-6,
                                                  rtol=0)
            for ct, c0 in zip(c_t, base):
                # the active rows were written, the inactive one was not
                assert not torch.equal(ct.k[:2], c0.k[:2])
                for ta, t0 in zip(_buffers(ct), _buffers(c0)):
                    assert torch.equal(ta[2], t0[2]), (kv_format, S)
    for h in hooks:
        h.remove()
    return True


@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_ragged_forward_equals_per_row(kv_format):
    run_distributed(_forward_worker, world_size=1, args=(kv_format,))


_LENS = [5, 9, 2]


def _padded_prompts(cfg, seed=1, fill=7):
    torch.manual_seed(seed)
    x = torch.randint(1, cfg.vocab_size, (len(_LENS), max(_LENS)))
    for b, n in enumerate(_LENS):
        x[b, n:] = fill     # what the padding holds must not matter
    return x


def _check_layout(out, x, lens, refs, n_new, pad):
    """Row b of ``out``: its prompt, then the new tokens of refs[b] (the
    (1, len_b + n_new) result for the unpadded prompt alone), then pad."""
    assert out.shape == (len(lens), x.shape[1] + n_new)
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], x[b, :n]), b
        assert torch.equal(out[b, n:n + n_new], refs[b][0, n:]), \
            (b, out[b], refs[b])
        assert (out[b, n + n_new:] == pad).all(), b


def _generate_worker(rank, world, kv_format):
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    over = {"hidden_size": 128} if kv_format else {}
    cfg, model = _models(0, **over)
    x = _padded_prompts(cfg)
    N = 6
    refs = [generate(model, x[b:b + 1, :n], max_new_tokens=N,
                     kv_format=kv_format) for b, n in enumerate(_LENS)]
    out = generate(model, x, max_new_tokens=N, kv_format=kv_format,
                   prompt_lens=_LENS)
    _check_layout(out, x, _LENS, refs, N, 0)
    out = generate(model, x, max_new_tokens=N, kv_format=kv_format,
                   prompt_lens=torch.tensor(_LENS), pad_token_id=3)
    _check_layout(out, x, _LENS, refs, N, 3)
    for bad in ([5, 9], [5, 10, 2], [0, 9, 2]):
        with pytest.raises(ValueError):
            generate(model, x, max_new_tokens=N, prompt_lens=bad)
    return True


@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_generate_prompt_lens_matches_per_row(kv_format):
    run_distributed(_generate_worker, world_size=1, args=(kv_format,))


def _window_worker(rank, world):
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, model = _models(0, sliding_window=4)
    with pytest.raises(NotImplementedError):
        generate(model, _padded_prompts(cfg), max_new_tokens=4,
                 prompt_lens=_LENS)
    return True


def test_generate_prompt_lens_refuses_rolling_cache():
    run_distributed(_window_worker, world_size=1)


def _spec_worker(rank, world):
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.inference.speculation import (
        speculative_generate)
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, target = _models(0)
    _, draft = _models(99)
    x = _padded_prompts(cfg)
    N = 12
    full = generate(target, x, max_new_tokens=N)
    ragged = generate(target, x, max_new_tokens=N, prompt_lens=_LENS)
    refs = [generate(target, x[b:b + 1, :n], max_new_tokens=N)
            for b, n in enumerate(_LENS)]
    _check_layout(ragged, x, _LENS, refs, N, 0)
    for d in (draft, target):
        out, rate = speculative_generate(target, d, x, max_new_tokens=N,
                                         spec_len=3, per_sequence=True)
        assert torch.equal(out, full), (out, full)
        out_l, rate_l = speculative_generate(target, d, x, max_new_tokens=N,
                                             spec_len=3, per_sequence=True,
                                             prompt_lens=_LENS)
        assert torch.equal(out_l, ragged), (out_l, ragged)
        if d is target:
            assert rate == 1.0 and rate_l == 1.0, (rate, rate_l)
        else:
            assert 0.0 <= rate < 1.0 and 0.0 <= rate_l < 1.0, (rate, rate_l)
    with pytest.raises(ValueError):   # prompt_lens is a per_sequence option
        speculative_generate(target, draft, x, max_new_tokens=N,
                             prompt_lens=_LENS)
    return True


def test_per_sequence_speculation_tokens():
    run_distributed(_spec_worker, world_size=1)


def test_rolling_cache_refuses_per_sequence_position():
    from neuronx_distributed_amd.inference.kv_cache import RollingKVCache

    c = RollingKVCache(2, 2, 4, 16, dtype=torch.float32, device="cpu")
    k = torch.randn(2, 2, 1, 16)
    with pytest.raises(NotImplementedError):
        c.update(k, k, torch.tensor([5, 2]))
    assert not c.k.any() and (c.slot_pos == -1).all()


def test_kv_cache_per_sequence_rows():
    """The (B,) mode of both caches against int-position updates of each row
    alone; the inactive rows (-1, and one row short of fitting) stay."""
    from neuronx_distributed_amd.inference.kv_cache import KVCache, MXKVCache

    B, Smax, S = 4, 12, 3
    pos = [5, 0, -1, Smax - S + 1]
    for cls in (KVCache, MXKVCache):
        a = cls(B, 2, Smax, 32, dtype=torch.float32, device="cpu")
        torch.manual_seed(3)
        for t in _buffers(a):
            t.copy_(torch.randint(0, 200, t.shape).to(t.dtype))
        before = [t.clone() for t in _buffers(a)]
        k, v = torch.randn(B, 2, S, 32), torch.randn(B, 2, S, 32)
        K, V = a.update(k, v, torch.tensor(pos))
        assert K.shape == V.shape == (B, 2, Smax, 32)
        for b in (0, 1):
            one = cls(1, 2, Smax, 32, dtype=torch.float32, device="cpu")
            for t, t0 in zip(_buffers(one), before):
                t.copy_(t0[b:b + 1])
            one.update(k[b:b + 1], v[b:b + 1], pos[b])
            for ta, tb in zip(_buffers(a), _buffers(one)):
                assert torch.equal(ta[b:b + 1], tb), (cls, b)
        for b in (2, 3):
            for ta, t0 in zip(_buffers(a), before):
                assert torch.equal(ta[b], t0[b]), (cls, b)


def _numel_worker(rank, world):
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, model = _models(0)
    attn = model.model.layers[0].self_attn
    B, Smax = 3, 16
    torch.manual_seed(2)
    hidden = torch.randn(B, 1, cfg.hidden_size)
    cos, sin = model.model.rope_cos, model.model.rope_sin
    cache = _caches(cfg, B, Smax, None)[0]
    with torch.no_grad():
        for bad in (torch.tensor([4, 5]), torch.tensor([1, 2, 3, 4]),
                    torch.zeros(0, dtype=torch.long)):
            with pytest.raises(ValueError):
                attn(hidden, cos, sin, bad, cache)
            assert not cache.k.any() and not cache.v.any()
        attn(hidden, cos, sin, torch.tensor([4, 5, 6]), cache)   # B: fine
        assert cache.k[0, :, 4].any() and cache.k[2, :, 6].any()
        assert not cache.k[0, :, 5].any()
    return True


def test_cached_step_rejects_other_numel():
    run_distributed(_numel_worker, world_size=1)


def test_ragged_attn_step_switch_restores():
    from neuronx_distributed_amd import ops

    import threading

    assert ops._RAGGED_STEP.get()
    with ops.ragged_attn_step(False):
        assert not ops.ragged_attn_enabled()
        seen = []   # another thread is not affected
        t = threading.Thread(target=lambda: seen.append(ops._RAGGED_STEP.get()))
        t.start()
        t.join()
        assert seen == [True]
        with ops.ragged_attn_step(True):
            assert ops.ragged_attn_enabled() == ops.ragged_attn_available()
        assert not ops.ragged_attn_enabled()
    with pytest.raises(KeyError):
        with ops.ragged_attn_step(False):
            raise KeyError("x")
    assert ops._RAGGED_STEP.get()


def _edge_worker(rank, world):
    """The eager ragged chain: a RoPE table shorter than the cache is refused
    before anything is written, and an inactive row whose cache holds NaN
    still gets an exactly zero attention output; generate and
    speculative_generate refuse max_new_tokens < 1 with prompt_lens."""
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.inference.speculation import (
        speculative_generate)
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg, model = _models(0)
    attn = model.model.layers[0].self_attn
    B, Smax = 3, 16
    torch.manual_seed(2)
    hidden = torch.randn(B, 2, cfg.hidden_size)
    cos, sin = model.model.rope_cos, model.model.rope_sin
    pos = torch.tensor([4, 5, -1])
    seen = []
    hook = attn.o_proj.register_forward_pre_hook(
        lambda mod, inp: seen.append(inp[0]))
    with torch.no_grad():
        cache = _caches(cfg, B, Smax, None)[0]
        with pytest.raises(ValueError):
            attn(hidden, cos[:Smax - 1], sin[:Smax - 1], pos, cache)
        assert not cache.k.any() and not seen
        cache.k[2] = float("nan")
        cache.v[2] = float("nan")
        out = attn(hidden, cos, sin, pos, cache)
        assert torch.isfinite(out).all() and not seen[0][2].any()
        assert seen[0][0].any() and cache.k[2].isnan().all()
    hook.remove()
    x = _padded_prompts(cfg)
    with pytest.raises(ValueError):
        generate(model, x, max_new_tokens=0, prompt_lens=_LENS)
    with pytest.raises(ValueError):
        speculative_generate(model, model, x, max_new_tokens=0,
                             per_sequence=True, prompt_lens=_LENS)
    return True


def test_ragged_chain_edges():
    run_distributed(_edge_worker, world_size=1)
