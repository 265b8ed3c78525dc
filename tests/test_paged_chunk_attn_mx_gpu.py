"""GPU checks of the fused multi-token decode attention over the paged MXFP8
KV cache (paged_chunk_attn_mx of csrc/paged_chunk_attn.hip,
ops.paged_chunk_attn_mx_step) and its route from LlamaAttention._cached_step
and speculative_generate(kv_format="paged_mxfp8").

Layout of test_paged_attn_mx_gpu.py, its bound min(2 * e_bf16, 3e-2) against
fp64 attention over the pools as stored after the call, e_bf16 from
ops.paged_chunk_attn_step on bf16 pools of the dequantized values; appended
bytes against ops.chunk_attn_mx_step(ragged=True) on a dense copy.  Pools and
new k, v are randn * 0.5 * 2^e, e in {-2..1} varying with (page, head, row,
32-block): a scale from the wrong row, block or page is off by 2 or more.
Rows at or beyond an active position hold 0xFF (NaN in e4m3 and e8m0).

Measured on MI355X, test_numerics_bytes_inactive: largest error 6.609e-3
(rep 4, T 2, set 0; the bf16 paged kernel 6.080e-3 there, 7.977e-3 at its
worst), MX / bf16 ratio of one case 0.55..1.11 against the allowed 2.
test_steady_state_tile_loop: 1.959e-4 (T 2), 1.869e-4 (T 8), ratios 1.008,
1.009.  Model level: max logit difference 1.56e-2 against the torch chain."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from test_decode_attn_mx_gpu import (
    ATOL_CAP, REPS, _deq, _deq64, _packed, _ref64)
from test_paged_attn_gpu import D, NP, PAGE, SCALE, _table
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    LOGIT_ATOL, _llama, _pos_t, _require_lib)

SMALL = (4, 2, NP, 6)     # B, Hkv, pages, pages per sequence (96 rows)
LONG = (2, 1, 144, 72)    # 1152 rows per sequence


def _dense(pages, table):   # (nb, hkv, rows, w): the rows in order
    x = pages[table.long()].transpose(1, 2)
    return x.reshape(table.shape[0], x.shape[1], -1, x.shape[-1]).contiguous()


def _setup(layout, rep, T, seed):
    """The clean table, the four written pools, q, k, v, the RoPE table."""
    nb, hkv, npg, pps = layout
    g = torch.Generator().manual_seed(1234)
    table = torch.randperm(npg, generator=g).int()[:nb * pps].view(nb, pps)
    g.manual_seed(seed)

    def rnd(*s):   # (..., D): an exponent per (leading indices, 32-block)
        idx = sum(torch.arange(n).view([n] + [1] * (len(s) - 1 - i))
                  for i, n in enumerate(s[:-1]))
        e = (idx + 2 * torch.arange(D // 32)) % 4 - 2
        x = torch.randn(*s[:-1], D // 32, 32, generator=g) * 0.5
        return (x * torch.exp2(e.float()).unsqueeze(-1)).reshape(*s)

    pools = [t.cuda() for _ in range(2)
             for t in _packed(rnd(npg, hkv, PAGE, D))]
    q = torch.randn(nb, T, hkv * rep * D, generator=g) * 0.5
    k, v = (rnd(nb, T, hkv, D).bfloat16().reshape(nb, T, -1).cuda()
            for _ in range(2))
    return (table.cuda(), pools, q.bfloat16().cuda(), k, v,
            ops.precompute_rope_freqs(pps * PAGE, D, device="cuda"))


def _check(layout, rep, T, positions, seed, poison=None):
    nb, hkv, npg, pps = layout
    clean, pools, q, k, v, rope = _setup(layout, rep, T, seed)
    table = clean.clone()
    for b, (j, entry) in (poison or {}).items():
        table[b, j] = entry
    active = [0 <= p and p + T <= pps * PAGE and all(
        0 <= int(e) < npg for e in table[b, :(p + T - 1) // PAGE + 1])
        for b, p in enumerate(positions)]
    on = [b for b in range(nb) if active[b]]
    off = [b for b in range(nb) if not active[b]]
    for t in pools:                    # an inactive sequence's pages
        t[clean[off].long()] = 0xAB
    tail = (_pos_t(positions), hkv * rep, hkv, SCALE)
    # the bf16 kernel on the very values the MX pools hold
    bf = [_deq(*pools[:2], torch.bfloat16), _deq(*pools[2:], torch.bfloat16)]
    out_b = ops.paged_chunk_attn_step(q, k, v, *bf, table, *rope, *tail)
    for b in on:                       # stale rows: NaN payload, NaN scale
        rows = torch.arange(positions[b], pps * PAGE, device="cuda")
        for t in pools:
            t[clean[b, rows // PAGE].long(), :, rows % PAGE] = 0xFF
    want = [t.clone() for t in pools]
    dense = [_dense(t, clean) for t in pools]
    ops.chunk_attn_mx_step(q, k, v, *dense, *rope, *tail, ragged=True)
    for b in on:
        for r in range(positions[b], positions[b] + T):
            for t, dt in zip(want, dense):
                t[int(clean[b, r // PAGE]), :, r % PAGE] = dt[b, :, r]
    out = ops.paged_chunk_attn_mx_step(q, k, v, *pools, table, *rope, *tail)
    assert out.shape == q.shape
    assert all(torch.equal(a, w) for a, w in zip(pools, want))  # every byte
    assert all((t[clean[b].long()] == 0xAB).all() for b in off for t in pools)
    assert not out[off].any() and torch.isfinite(out.float()).all()

    def err(o, Kd, Vd):   # fp64 attention over the cache as stored now
        return max((o[b:b + 1, t].double() - _ref64(
            q[b:b + 1, t], Kd[b:b + 1], Vd[b:b + 1], rope, positions[b] + t,
            rep)).abs().max().item() for b in on for t in range(T))

    if on:
        dense = [_dense(t, clean) for t in pools]
        e = err(out, _deq64(*dense[:2]), _deq64(*dense[2:]))
        e_b = err(out_b, *(_dense(t, clean).double() for t in bf))
        print(f"paged chunk mx rep {rep} T {T} pos {positions}: max err "
              f"{e:.3e}, bf16 paged kernel {e_b:.3e}, ratio {e / e_b:.3f}")
        assert e <= min(2.0 * e_b, ATOL_CAP), (e, e_b)
    return active


# the position sets of test_paged_chunk_attn_gpu.py; the -1 at page 1 of
# sequence 2 is never read for T 2, which leaves that sequence active
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("T", (2, 3, 5, 8))
@pytest.mark.parametrize("rep", REPS)
def test_numerics_bytes_inactive(rep, T, which):
    if which == 0:
        active = _check(SMALL, rep, T, (0, 14, 30, 96 - T), 7 + rep)
        assert active == [True] * 4
    else:
        active = _check(SMALL, rep, T, (-1, 97 - T, 14, 40), 11 + rep,
                        {2: (1, -1), 3: (0, NP)})
        assert active == [False, False, T == 2, False]


@pytest.mark.parametrize("T", (2, 8))
def test_steady_state_tile_loop(T):
    """33 or more tiles, 9 per split: wave 0 of a split walks three."""
    assert _check(LONG, 4, T, (1030, 1151 - T), 5) == [True, True]


def test_guards():
    nb, rep, (_, hkv, npg, pps) = 2, 2, SMALL
    cos, sin = ops.precompute_rope_freqs(pps * PAGE, D, device="cuda")
    z = lambda *s, dt=torch.uint8: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    pools = [z(npg, hkv, PAGE, w) for w in (D, D // 32, D, D // 32)]
    good = dict(kp=pools[0], ks=pools[1], T=3, pos=_pos_t((2, 3)),
                table=_table()[:nb].contiguous())
    for over in (dict(kp=z(npg, hkv, PAGE, D, dt=torch.bfloat16)),
                 dict(ks=z(npg, hkv, PAGE, 2)),          # scale-pool width
                 dict(table=good["table"].long()), dict(T=1), dict(T=9),
                 dict(pos=_pos_t((2,)))):
        a = {**good, **over}
        q = z(nb, a["T"], hkv * rep * D, dt=torch.bfloat16) + 1
        kv = z(nb, a["T"], hkv * D, dt=torch.bfloat16) + 1
        with pytest.raises(ValueError):
            ops.paged_chunk_attn_mx_step(
                q, kv, kv, a["kp"], a["ks"], *pools[2:], a["table"], cos,
                sin, a["pos"], hkv * rep, hkv, SCALE)
    assert not any(t.any() for t in pools)   # nothing was launched


def test_graph_replay_matches_eager():
    rep, T, hkv, pos0 = 4, 4, SMALL[1], (10, 27, 40, 59)   # across page seams
    table, pools, q, k, v, rope = _setup(SMALL, rep, T, 22)
    call = lambda c, p: ops.paged_chunk_attn_mx_step(  # noqa: E731
        q, k, v, *c, table, *rope, p, hkv * rep, hkv, SCALE)
    eager_pools = [t.clone() for t in pools]
    eager = [call(eager_pools, _pos_t([p + i * T for p in pos0]))
             for i in range(3)]
    pos_t, side = _pos_t(pos0), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):            # warm-up touches a copy only
        call([t.clone() for t in pools], pos_t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = call(pools, pos_t)
    for want in eager:
        graph.replay()
        assert torch.equal(out_s, want)
        pos_t += T
    assert all(torch.equal(a, b) for a, b in zip(pools, eager_pools))


def test_model_chunk_and_speculative_generate(monkeypatch):
    from neuronx_distributed_amd.inference import speculation
    from neuronx_distributed_amd.inference.kv_cache import (
        PagePool, build_kv_caches)

    cfg, model = _llama()
    calls = []
    for name in ("paged_chunk_attn_mx_step", "paged_chunk_attn_step"):
        monkeypatch.setattr(ops, name, lambda *a, _n=name, _f=getattr(
            ops, name), **kw: calls.append(_n) or _f(*a, **kw))
    Bm, P, S = 3, 11, 4
    pool = PagePool(2 * Bm, Bm, 2, "cuda")
    for b in reversed(range(Bm)):
        pool.allocate(b, 2 * PAGE)
    c1, c2 = (build_kv_caches(
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, 2 * PAGE,
        cfg.head_dim, device="cuda", kv_format="paged_mxfp8", page_pool=pool)
        for _ in range(2))
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (Bm, P + S), device="cuda")
    positions = _pos_t((5, 11, -1))          # the third row is inactive
    once = ["paged_chunk_attn_mx_step"] * cfg.num_hidden_layers
    with torch.no_grad():
        for c in (c1, c2):
            model(x[:, :P], kv_caches=c, pos_offset=0)
        got = model(x[:, P:], kv_caches=c1, pos_offset=positions)
        assert calls == once                 # once per layer
        with monkeypatch.context() as m:     # the eager chain on gather()
            m.setattr(ops, "paged_chunk_attn_mx_available", lambda: False)
            want = model(x[:, P:], kv_caches=c2, pos_offset=positions)
        assert calls == once
    err = (got.float() - want.float()).abs().max().item()
    print(f"model paged chunk mx step: max logit diff {err:.3e}")
    assert got.shape == (Bm, S, cfg.vocab_size) and err <= LOGIT_ATOL

    _, draft = _llama(5)
    pools, real = [], speculation.build_kv_caches
    monkeypatch.setattr(
        speculation, "build_kv_caches",
        lambda *a, **kw: pools.append(kw["page_pool"]) or real(*a, **kw))
    lens = (9, 4, 6)
    x = torch.randint(1, cfg.vocab_size, (3, 9), device="cuda")
    for b, n in enumerate(lens):
        x[b, n:] = 0
    gen = lambda x, **kw: speculation.speculative_generate(  # noqa: E731
        model, draft, x, max_new_tokens=8, spec_len=3, fused_verify=True, **kw)
    dense, _ = gen(x, kv_format="mxfp8", per_sequence=True, prompt_lens=lens)
    paged, _ = gen(x, kv_format="paged_mxfp8", per_sequence=True,
                   prompt_lens=lens)
    assert len(calls) > len(once) and "paged_chunk_attn_step" not in calls
    assert torch.equal(paged, dense), (paged, dense)
    # pages of (21, 16, 18) rows: 2 + 1 + 2, in both models' pools
    assert [p.num_pages for p in pools[-2:]] == [5, 5]
    with pytest.raises(ValueError, match="per_sequence"):
        gen(x[:, :4], kv_format="paged_mxfp8")
