"""GPU checks of the fused multi-token decode attention over the paged KV
cache (csrc/paged_chunk_attn.hip, ops.paged_chunk_attn_step) and its route
from LlamaAttention._cached_step and speculative_generate(kv_format="paged").

Layouts as in test_paged_attn_gpu.py: pools behind a fixed random permutation
as the table.  Numerics against fp64 (rows gathered through the table after
the call, RoPE in fp32) within 3e-2 + 2e-2 max|ref|, and against the fp64
error of ops.chunk_attn_step(ragged=True) on the dense gather of the same
inputs, computed in the same run; the appended rows bit for bit against that
kernel's.

Measured on MI355X over the 24 cases (3 reps x 4 T x 2 position sets, 51
active sequences) of test_numerics_append_inactive: max |out - fp64| 4.988e-3
for the paged kernel and 4.988e-3 for the dense one (rep 4, T 2, pos 0: the
rounding of an output near 1 to bf16); the ratio of the two errors is 1.000
for every sequence, the outputs being bit-equal: the paged kernel walks the
same tiles in the same order with the same arithmetic.  ALLOWED_RATIO = 2.0
is twice that worst ratio.  test_steady_state_tile_loop: at most 2.565e-4.
Model level: max logit difference 1.17e-2 against the torch chain.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    LOGIT_ATOL, _llama, _pos_t, _require_lib)

D, PAGE = 128, 16
SCALE = 1.0 / math.sqrt(D)
SMALL = (4, 2, 24, 6)     # B, Hkv, pages, pages per sequence (96 rows)
LONG = (2, 1, 144, 72)    # 1152 rows per sequence
ALLOWED_RATIO = 2.0       # twice the worst measured ratio (docstring)


def _setup(layout, rep, T, seed):
    """The clean table, pools with every row written, and q, k, v."""
    nb, hkv, npg, pps = layout
    g = torch.Generator().manual_seed(1234)
    table = torch.randperm(npg, generator=g).int()[:nb * pps].view(nb, pps)
    g.manual_seed(seed)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5  # noqa: E731
                      ).bfloat16().cuda()
    return (table.cuda(), (rnd(npg, hkv, PAGE, D), rnd(npg, hkv, PAGE, D)),
            rnd(nb, T, hkv * rep * D), rnd(nb, T, hkv * D),
            rnd(nb, T, hkv * D),
            ops.precompute_rope_freqs(pps * PAGE, D, device="cuda"))


def _dense(pages, table):   # (nb, hkv, rows, D): every sequence's rows in order
    x = pages[table.long()].transpose(1, 2)
    return x.reshape(table.shape[0], x.shape[1], -1, D).contiguous()


def _err(out, q, K, V, cos, sin, p, rep):
    """max |out - fp64 attention| and max |ref| of one sequence's chunk: out
    (T, hkv*rep*D), q alike, at position p over its rows K, V (hkv, rows, D)
    as stored."""
    hkv, err, top = K.shape[0], 0.0, 0.0
    K, V = K.double().cpu(), V.double().cpu()
    for t in range(q.shape[0]):
        c, s = cos[p + t].cpu(), sin[p + t].cpu()
        x = q[t].float().cpu().view(hkv, rep, D)
        x0, x1 = x[..., :D // 2], x[..., D // 2:]
        qr = torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1).double()
        w = torch.softmax(qr @ K[:, :p + t + 1].transpose(1, 2) * SCALE, -1)
        ref = (w @ V[:, :p + t + 1]).reshape(-1)
        err = max(err, (out[t].double().cpu() - ref).abs().max().item())
        top = max(top, ref.abs().max().item())
    return err, top


def _check(layout, rep, T, positions, seed, poison=None, against_dense=True):
    """One paged chunk step.  ``poison``: {b: (page index j, entry)} written
    into the table before the call.  A sequence is active by the rule of
    PagedKVCache.active; the pages of the others hold 0xAB bytes."""
    nb, hkv, npg, pps = layout
    poison = poison or {}
    clean, (kp, vp), q, k, v, (cos, sin) = _setup(layout, rep, T, seed)
    table = clean.clone()
    for b, (j, entry) in poison.items():
        table[b, j] = entry
    active = [0 <= p and p + T <= pps * PAGE and all(
        0 <= int(e) < npg for e in table[b, :(p + T - 1) // PAGE + 1])
        for b, p in enumerate(positions)]
    for b in range(nb):
        if not active[b]:
            for t in (kp, vp):
                t[clean[b].long()] = t[clean[b].long()].view(
                    torch.uint8).fill_(0xAB).view(torch.bfloat16)
    pos_t = _pos_t(positions)
    K1, V1 = _dense(kp, clean), _dense(vp, clean)
    want_k, want_v = kp.clone(), vp.clone()
    if against_dense:
        dense_out = ops.chunk_attn_step(q, k, v, K1, V1, cos, sin, pos_t,
                                        hkv * rep, hkv, SCALE, ragged=True)
        for b, p in enumerate(positions):
            for r in range(p, p + T) if active[b] else ():
                want_k[clean[b, r // PAGE], :, r % PAGE] = K1[b, :, r]
                want_v[clean[b, r // PAGE], :, r % PAGE] = V1[b, :, r]
    out = ops.paged_chunk_attn_step(q, k, v, kp, vp, table, cos, sin, pos_t,
                                    hkv * rep, hkv, SCALE)
    assert out.shape == q.shape
    if against_dense:                   # every byte of both pools
        assert torch.equal(kp, want_k) and torch.equal(vp, want_v)
    Kd, Vd = _dense(kp, clean), _dense(vp, clean)
    for b, p in enumerate(positions):
        if not active[b]:
            assert not out[b].any(), (rep, T, positions, b)
            continue
        err, top = _err(out[b], q[b], Kd[b], Vd[b], cos, sin, p, rep)
        msg = f"paged chunk rep {rep} T {T} pos {p}: max err {err:.3e}"
        assert err <= 3e-2 + 2e-2 * top, msg
        if against_dense:
            err_d, _ = _err(dense_out[b], q[b], K1[b], V1[b], cos, sin, p, rep)
            print(f"{msg}, dense {err_d:.3e}, ratio {err / err_d:.3f}, "
                  f"bit-equal {torch.equal(out[b], dense_out[b])}")
            assert err <= ALLOWED_RATIO * err_d, msg
        else:
            print(msg)
    return active


# set 0, all active: an empty cache, a chunk across a page seam, across a
# tile seam (all with fewer tiles than splits), one ending on the last row.
# set 1: a position below 0, one row too many, entry -1 at page 1 (the page
# of the last row for T >= 3; never read, and the sequence active, for T 2),
# entry num_pages in an earlier page.
@pytest.mark.parametrize("which", (0, 1))
@pytest.mark.parametrize("T", (2, 3, 5, 8))
@pytest.mark.parametrize("rep", (1, 4, 8))
def test_numerics_append_inactive(rep, T, which):
    if which == 0:
        active = _check(SMALL, rep, T, (0, 14, 30, 96 - T), 7 + rep)
        assert active == [True] * 4
    else:
        active = _check(SMALL, rep, T, (-1, 97 - T, 14, 40), 11 + rep,
                        {2: (1, -1), 3: (0, SMALL[2])})
        assert active == [False, False, T == 2, False]


@pytest.mark.parametrize("T", (2, 8))
def test_steady_state_tile_loop(T):
    """pos + T > 1024: 33 or more 32-row tiles, 9 per split (whole tiles,
    DA_SPLIT 4), so wave 0 of a split walks three of them."""
    assert _check(LONG, 4, T, (1030, 1151 - T), 5, against_dense=False) \
        == [True, True]


def test_graph_replay_matches_eager():
    rep, T, steps, pos0 = 4, 4, 3, (10, 27)      # across a page boundary
    nb, hkv = 2, SMALL[1]
    table, pools, _, _, _, (cos, sin) = _setup(SMALL, rep, T, 22)
    table = table[:nb].contiguous()
    ins = [tuple(t[:nb] for t in _setup(SMALL, rep, T, 23 + i)[2:5])
           for i in range(steps)]
    call = lambda q, k, v, c, p: ops.paged_chunk_attn_step(  # noqa: E731
        q, k, v, *c, table, cos, sin, p, hkv * rep, hkv, SCALE)
    eager_pools = tuple(t.clone() for t in pools)
    eager = [call(*ins[i], eager_pools, _pos_t([p + i * T for p in pos0]))
             for i in range(steps)]
    q_s, k_s, v_s = (t.clone() for t in ins[0])
    pos_t = _pos_t(pos0)
    warm = tuple(t.clone() for t in pools)   # warm-up touches a copy only
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        call(q_s, k_s, v_s, warm, pos_t)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = call(q_s, k_s, v_s, pools, pos_t)
    for i in range(steps):
        for dst, src in zip((q_s, k_s, v_s), ins[i]):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out_s, eager[i]), i
        pos_t += T
    assert all(torch.equal(a, b) for a, b in zip(pools, eager_pools))


def test_guards():
    nb, rep, T, (_, hkv, npg, pps) = 2, 2, 3, SMALL
    table, _, _, _, _, (cos, sin) = _setup(SMALL, rep, T, 1)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    good = dict(kp=z(npg, hkv, PAGE, D), vp=z(npg, hkv, PAGE, D), T=T,
                table=table[:nb].contiguous(), pos=_pos_t((2, 3)))
    bad = [dict(kp=z(npg, hkv, PAGE, D, dt=torch.float16)),
           dict(kp=z(npg, hkv, 32, D), vp=z(npg, hkv, 32, D)),
           dict(vp=z(npg, hkv, PAGE, 2 * D)[..., :D]),     # not contiguous
           dict(table=good["table"].long()), dict(table=good["table"].cpu()),
           dict(table=table[:nb + 1].contiguous()), dict(T=1), dict(T=9),
           dict(pos=_pos_t((2,)))]
    for over in bad:
        a = {**good, **over}
        q, kv = z(nb, a["T"], hkv * rep * D) + 1, z(nb, a["T"], hkv * D) + 1
        with pytest.raises(ValueError):
            ops.paged_chunk_attn_step(q, kv, kv, a["kp"], a["vp"], a["table"],
                                      cos, sin, a["pos"], hkv * rep, hkv,
                                      SCALE)
    torch.cuda.synchronize()
    for a in bad + [good]:                   # nothing was launched
        assert not any(a[n].any() for n in ("kp", "vp") if n in a)


def test_model_chunk_and_speculative_generate(monkeypatch):
    from neuronx_distributed_amd.inference import speculation
    from neuronx_distributed_amd.inference.kv_cache import (
        PagePool, build_kv_caches)

    cfg, model = _llama()
    calls, real_step = [], ops.paged_chunk_attn_step
    monkeypatch.setattr(ops, "paged_chunk_attn_step", lambda *a, **kw: (
        calls.append(1) or real_step(*a, **kw)))
    Bm, P, S = 3, 11, 4
    pool = PagePool(2 * Bm, Bm, 2, "cuda")
    for b in reversed(range(Bm)):
        pool.allocate(b, 2 * PAGE)
    c1, c2 = (build_kv_caches(
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, 2 * PAGE,
        cfg.head_dim, device="cuda", kv_format="paged", page_pool=pool)
        for _ in range(2))
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (Bm, P + S), device="cuda")
    positions = _pos_t((5, 11, -1))          # the third row is inactive
    with torch.no_grad():
        for c in (c1, c2):
            model(x[:, :P], kv_caches=c, pos_offset=0)
        got = model(x[:, P:], kv_caches=c1, pos_offset=positions)
        assert len(calls) == cfg.num_hidden_layers   # once per layer
        with monkeypatch.context() as m:     # the eager chain on gather()
            m.setattr(ops, "paged_chunk_attn_available", lambda: False)
            want = model(x[:, P:], kv_caches=c2, pos_offset=positions)
        assert len(calls) == cfg.num_hidden_layers
    err = (got.float() - want.float()).abs().max().item()
    print(f"model paged chunk step: max logit diff {err:.3e}")
    assert got.shape == (Bm, S, cfg.vocab_size) and err <= LOGIT_ATOL

    _, draft = _llama(5)
    pools, real = [], speculation.build_kv_caches
    monkeypatch.setattr(
        speculation, "build_kv_caches",
        lambda *a, **kw: pools.append(kw["page_pool"]) or real(*a, **kw))
    lens, N, k = (9, 4, 6), 8, 3
    x = torch.randint(1, cfg.vocab_size, (3, 9), device="cuda")
    for b, n in enumerate(lens):
        x[b, n:] = 0
    kw = dict(max_new_tokens=N, spec_len=k, fused_verify=True,
              prompt_lens=lens)
    dense, _ = speculation.speculative_generate(model, draft, x,
                                                per_sequence=True, **kw)
    n_model = len(calls)
    paged, rate = speculation.speculative_generate(
        model, draft, x, kv_format="paged", per_sequence=True, **kw)
    assert len(calls) > n_model and 0.0 <= rate <= 1.0
    assert torch.equal(paged, dense), (paged, dense)
    # pages of (21, 16, 18) rows: 2 + 1 + 2, in both models' pools
    assert [p.num_pages for p in pools[-2:]] == [5, 5]
    assert 5 < 3 * math.ceil((9 + N + k + 1) / PAGE)
    with pytest.raises(ValueError, match="per_sequence"):
        speculation.speculative_generate(model, draft, x[:, :4],
                                         kv_format="paged")
