"""GPU checks of the per-sequence-position ("ragged") entries of the four
fused decode-attention kernels: ops.decode_attn_step, decode_attn_mx_step,
chunk_attn_step and chunk_attn_mx_step with ``ragged=True`` and a (B,)
position tensor.

The reference is the uniform entry itself (``ragged=False``), which the other
GPU files check against fp64: for every active row b, the ragged call must
leave exactly the bytes, in the output row and in the row's cache slice, that
the uniform op leaves when run on row b alone (B = 1 slices of the same
inputs and starting cache) at position pos[b].  No tolerance is involved: a
workgroup serves one (b, kvh, split) and nothing crosses rows.

* one token: B 4, Hkv 2, rep 1 / 4, Smax 96, positions (0, 1, 17, 70) and
  (95, 3, 0, 40): an empty cache, fewer rows than splits, an uneven split,
  more than 16 rows per split, the last row,
* a chunk: B 4, Smax 160, T 2 / 5 / 8, rep 1 / 8 (rep 8 with T 8: two query
  blocks), positions (0, 31, 33, 130) around the 32-row tile,
* inactive rows (pos < 0 or pos + T > Smax): their cache slices, filled with a
  0xAB byte pattern, stay bitwise, their output rows are zero, and their
  neighbours still equal the uniform runs,
* the Python guards, hipGraph replay with ``pos_t += 1``, and the model level
  (fused ragged step against the eager chain of LlamaAttention._cached_step).
"""

import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from neuronx_distributed_amd.quantization.microscaling import (
    pack_mx, quantize_mx)

FMT = "fp8_e4m3"
D = 128
B, HKV = 4, 2
FORMATS = ("bf16", "mxfp8")
SCALE = 1.0 / math.sqrt(D)


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    from neuronx_distributed_amd.ops import build as _build

    _build.build()
    assert ops.is_available(), ops._LIB_ERR
    assert ops.ragged_attn_available()


def _pos_t(pos):
    pos = [pos] if isinstance(pos, int) else list(pos)
    return torch.tensor(pos, dtype=torch.int64, device="cuda")


def _step(fmt, T):
    if T == 1:
        return ops.decode_attn_step if fmt == "bf16" \
            else ops.decode_attn_mx_step
    return ops.chunk_attn_step if fmt == "bf16" else ops.chunk_attn_mx_step


def _case(fmt, rep, T, Smax, seed, nb=B):
    """A cache with every row written (the rows at and beyond a position are
    stale ones), and q, k, v: (nb, W) for T = 1, (nb, T, W) for a chunk."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g) * 0.5   # noqa: E731
    K, V = rnd(nb, HKV, Smax, D), rnd(nb, HKV, Smax, D)
    if fmt == "bf16":
        cache = (K.bfloat16().cuda(), V.bfloat16().cuda())
    else:
        cache = tuple(t.cuda() for t in
                      pack_mx(*quantize_mx(K, FMT), FMT)
                      + pack_mx(*quantize_mx(V, FMT), FMT))
    shp = (nb,) if T == 1 else (nb, T)
    q = rnd(*shp, HKV * rep * D).bfloat16().cuda()
    k = rnd(*shp, HKV * D).bfloat16().cuda()
    v = rnd(*shp, HKV * D).bfloat16().cuda()
    return cache, q, k, v


def _table(Smax):
    return ops.precompute_rope_freqs(Smax, D, device="cuda")


def _check_rows(fmt, rep, T, Smax, positions, seed, sentinel=False):
    """One ragged call against the uniform op on every active row alone;
    inactive rows: cache untouched, output zero."""
    nb = len(positions)
    table = _table(Smax)
    start, q, k, v = _case(fmt, rep, T, Smax, seed, nb)
    active = [0 <= p and p + T <= Smax for p in positions]
    if sentinel:
        for t in start:
            for b in range(nb):
                if not active[b]:
                    t[b].view(torch.uint8).fill_(0xAB)
    cache = tuple(t.clone() for t in start)
    fn = _step(fmt, T)
    out = fn(q, k, v, *cache, *table, _pos_t(positions), HKV * rep, HKV,
             SCALE, ragged=True)
    assert out.shape == q.shape
    for b, p in enumerate(positions):
        if not active[b]:
            assert not out[b].any(), (fmt, rep, T, positions, b)
            for t, t0 in zip(cache, start):
                assert torch.equal(t[b], t0[b]), (fmt, rep, T, positions, b)
            continue
        one = tuple(t[b:b + 1].clone() for t in start)
        want = fn(q[b:b + 1], k[b:b + 1], v[b:b + 1], *one, *table, _pos_t(p),
                  HKV * rep, HKV, SCALE)
        assert torch.equal(out[b:b + 1], want), (fmt, rep, T, positions, b)
        assert out[b].any()
        for t, t1, t0 in zip(cache, one, start):
            assert torch.equal(t[b:b + 1], t1), (fmt, rep, T, positions, b)
        assert not torch.equal(cache[0][b, :, p:p + T], start[0][b, :, p:p + T])
    return active


@pytest.mark.parametrize("positions", [(0, 1, 17, 70), (95, 3, 0, 40)])
@pytest.mark.parametrize("rep", (1, 4))
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_token_equals_uniform_rows(fmt, rep, positions):
    assert all(_check_rows(fmt, rep, 1, 96, positions, 3 + rep))


@pytest.mark.parametrize("T", (2, 5, 8))
@pytest.mark.parametrize("rep", (1, 8))
@pytest.mark.parametrize("fmt", FORMATS)
def test_chunk_equals_uniform_rows(fmt, rep, T):
    assert all(_check_rows(fmt, rep, T, 160, (0, 31, 33, 130), 10 * rep + T))


@pytest.mark.parametrize("T", (1, 2, 5, 8))
@pytest.mark.parametrize("fmt", FORMATS)
def test_inactive_rows(fmt, T):
    Smax = 96 if T == 1 else 160
    positions = (-1, 5, Smax - T + 1, 9)
    for rep in (1, 8):
        active = _check_rows(fmt, rep, T, Smax, positions, 50 + T,
                             sentinel=True)
        assert active == [False, True, False, True]


def test_guards():
    nb, rep, T, Smax = 2, 2, 3, 8
    cos, sin = _table(Smax)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    mx = (z(nb, HKV, Smax, D, dt=torch.uint8),
          z(nb, HKV, Smax, D // 32, dt=torch.uint8),
          z(nb, HKV, Smax, D, dt=torch.uint8),
          z(nb, HKV, Smax, D // 32, dt=torch.uint8))
    bf = (z(nb, HKV, Smax, D), z(nb, HKV, Smax, D))
    ones = lambda *s: torch.ones(*s, dtype=torch.bfloat16,  # noqa: E731
                                 device="cuda")
    good = _pos_t((2, 3))
    bad = (_pos_t(2),                                     # (1,) when B = 2
           good.int(),                                    # int32
           good.cpu(),                                    # on the CPU
           _pos_t((2, 0, 3, 0)).view(nb, 2)[:, :1],       # (B, 1) strided view
           _pos_t((2, 0, 3, 0))[::2],                     # (B,) strided view
           _pos_t((2, 3, 4)))                             # B + 1 of them
    assert not bad[3].is_contiguous() and bad[3].shape == (nb, 1)
    for fmt, cache in (("bf16", bf), ("mxfp8", mx)):
        for t in (1, T):
            shp = (nb,) if t == 1 else (nb, t)
            q, kv = ones(*shp, HKV * rep * D), ones(*shp, HKV * D)
            for pos_t in bad:
                with pytest.raises(ValueError):
                    _step(fmt, t)(q, kv, kv, *cache, cos, sin, pos_t,
                                  HKV * rep, HKV, SCALE, ragged=True)
            # a (B,) position is no uniform one
            with pytest.raises(ValueError):
                _step(fmt, t)(q, kv, kv, *cache, cos, sin, good, HKV * rep,
                              HKV, SCALE)
    torch.cuda.synchronize()
    for t in mx + bf:                        # nothing was launched
        assert not t.any()


@pytest.mark.parametrize("fmt", FORMATS)
def test_graph_replay_matches_eager(fmt):
    rep, steps, Smax, nb = 4, 3, 48, 2
    pos0 = (2, 40)
    table = _table(Smax)
    cache, _, _, _ = _case(fmt, rep, 1, Smax, 22, nb)
    ins = [_case(fmt, rep, 1, 1, 23 + i, nb)[1:] for i in range(steps)]
    fn = _step(fmt, 1)
    call = lambda q, k, v, c, p: fn(  # noqa: E731
        q, k, v, *c, *table, p, HKV * rep, HKV, SCALE, ragged=True)
    eager_cache = tuple(t.clone() for t in cache)
    eager = [call(*ins[i], eager_cache, _pos_t([p + i for p in pos0]))
             for i in range(steps)]

    q_s, k_s, v_s = (t.clone() for t in ins[0])
    pos_t = _pos_t(pos0)
    warm = tuple(t.clone() for t in cache)   # warm-up touches a copy only
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(q_s, k_s, v_s, warm, pos_t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = call(q_s, k_s, v_s, cache, pos_t)
    for i in range(steps):
        for dst, src in zip((q_s, k_s, v_s), ins[i]):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out_s, eager[i]), i
        pos_t += 1
    for a, b in zip(cache, eager_cache):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------

def _llama(seed=0):
    import torch.distributed as dist
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29558")
        dist.init_process_group("nccl", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg = get_config("test-d128")   # 2 layers, hidden 512, Hq 4, Hkv 2, D 128
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    torch.manual_seed(seed)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg)
    torch.set_default_dtype(prev)
    return cfg, model.eval()


LOGIT_ATOL = 5e-2   # test_chunk_attn_gpu.py, the same fused-vs-eager check


@pytest.mark.parametrize("S", (1, 4))
@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_model_ragged_matches_eager_chain(kv_format, S, monkeypatch):
    """model(tokens, pos_offset=(B,) tensor) through the fused ragged step
    against the eager chain of LlamaAttention._cached_step on a copy of the
    caches (the ragged kernels made unavailable).  The third row is
    inactive."""
    from neuronx_distributed_amd.inference.kv_cache import build_kv_caches

    cfg, model = _llama()
    names = ("decode_attn_step", "decode_attn_mx_step", "chunk_attn_step",
             "chunk_attn_mx_step")
    calls = dict.fromkeys(names, 0)

    def wrap(name, real):
        def f(*a, **kw):
            assert kw.get("ragged") is True
            calls[name] += 1
            return real(*a, **kw)
        return f

    for n in names:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))
    Bm, P, Smax = 3, 11, 32
    positions = _pos_t((5, 11, -1))
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (Bm, P + S), device="cuda")
    mk = lambda: build_kv_caches(  # noqa: E731
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, Smax,
        cfg.head_dim, device="cuda", kv_format=kv_format)
    c1, c2 = mk(), mk()
    used = ("decode_attn" if S == 1 else "chunk_attn") \
        + ("_mx" if kv_format else "") + "_step"
    with torch.no_grad():
        for c in (c1, c2):
            model(x[:, :P], kv_caches=c, pos_offset=0)
        before = [c.k[2].clone() for c in c1]
        got = model(x[:, P:], kv_caches=c1, pos_offset=positions)
        assert calls[used] == cfg.num_hidden_layers == sum(calls.values())
        monkeypatch.setattr(ops, "ragged_attn_available", lambda: False)
        want = model(x[:, P:], kv_caches=c2, pos_offset=positions)
        assert sum(calls.values()) == cfg.num_hidden_layers
    assert got.shape == want.shape == (Bm, S, cfg.vocab_size)
    err = (got.float() - want.float()).abs().max().item()
    print(f"model ragged step {kv_format} S {S}: max logit diff {err:.3e} "
          f"(logits up to {want.float().abs().max().item():.2f})")
    assert err <= LOGIT_ATOL
    for a, b, k0 in zip(c1, c2, before):
        assert torch.equal(a.k[2], k0) and torch.equal(b.k[2], k0)
        assert torch.equal(a.v[2], b.v[2])
    # layer 0 of both runs sees the same hidden states: the same V rows
    assert torch.equal(c1[0].v, c2[0].v)


@pytest.mark.parametrize("kv_format", [None, "mxfp8"])
def test_per_sequence_speculation_takes_ragged_kernels(kv_format, monkeypatch):
    """speculative_generate(per_sequence=True): with fused_verify every draft
    step and verify chunk of the batch goes through the ragged entries,
    without it none does (the eager chain).  Tokens are not compared with
    per-row runs here: bf16 library GEMMs may choose kernels by batch size;
    tests/test_ragged_step.py compares them in fp32."""
    from neuronx_distributed_amd.inference.speculation import (
        speculative_generate)

    cfg, target = _llama(0)
    _, draft = _llama(5)
    names = ("decode_attn_step", "decode_attn_mx_step", "chunk_attn_step",
             "chunk_attn_mx_step")
    calls = dict.fromkeys(names, 0)

    def wrap(name, real):
        def f(*a, **kw):
            if kw.get("ragged"):
                calls[name] += 1
            return real(*a, **kw)
        return f

    for n in names:
        monkeypatch.setattr(ops, n, wrap(n, getattr(ops, n)))
    lens = [9, 4, 6]
    torch.manual_seed(2)
    x = torch.randint(1, cfg.vocab_size, (3, 9), device="cuda")
    for b, n in enumerate(lens):
        x[b, n:] = 0
    N = 8
    out, rate = speculative_generate(target, draft, x, max_new_tokens=N,
                                     spec_len=3, kv_format=kv_format,
                                     per_sequence=True, prompt_lens=lens)
    assert sum(calls.values()) == 0 and ops._RAGGED_STEP.get()
    fused, rate_f = speculative_generate(target, draft, x, max_new_tokens=N,
                                         spec_len=3, kv_format=kv_format,
                                         per_sequence=True, prompt_lens=lens,
                                         fused_verify=True)
    mx = "_mx" if kv_format else ""
    assert calls[f"decode_attn{mx}_step"] > 0
    assert calls[f"chunk_attn{mx}_step"] > 0
    assert sum(calls.values()) == calls[f"decode_attn{mx}_step"] \
        + calls[f"chunk_attn{mx}_step"]
    for o, r in ((out, rate), (fused, rate_f)):
        assert o.shape == (3, 9 + N) and 0.0 <= r <= 1.0
        for b, n in enumerate(lens):
            assert torch.equal(o[b, :n], x[b, :n])
            assert (o[b, n + N:] == 0).all()
