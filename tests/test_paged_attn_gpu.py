"""GPU checks of the paged KV cache kernels (csrc/paged_attn.hip) and their
route from LlamaAttention._cached_step and generate(kv_format="paged").

B 4, Hkv 2, D 128; 24 pages behind a fixed random permutation as the table
(an identity mapping or a wrong indirection fails); 6 pages per sequence.
Numerics against fp64 (rows gathered through the table, RoPE in fp32) within
test_ops_gpu.py's atol 3e-2 + 2e-2 max|ref| for this operation; the append
bit for bit against ops.decode_attn_step(ragged=True) on the dense gather."""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    LOGIT_ATOL, _llama, _pos_t, _require_lib)

D, B, HKV, NP, PPS, PAGE = 128, 4, 2, 24, 6, 16
SCALE = 1.0 / math.sqrt(D)


def _table(nb=B):
    g = torch.Generator().manual_seed(1234)
    return torch.randperm(NP, generator=g).int().view(B, PPS)[:nb].cuda()


def _case(rep, seed, nb=B):
    """Pools with every row written, and q, k, v of one step."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5  # noqa: E731
                      ).bfloat16().cuda()
    return ((rnd(NP, HKV, PAGE, D), rnd(NP, HKV, PAGE, D)),
            rnd(nb, HKV * rep * D), rnd(nb, HKV * D), rnd(nb, HKV * D))


def _dense(pages, table):   # (nb, HKV, 96, D): every sequence's rows in order
    x = pages[table.long()].transpose(1, 2)
    return x.reshape(table.shape[0], HKV, PPS * PAGE, D).contiguous()


def _rope_table():
    return ops.precompute_rope_freqs(PPS * PAGE, D, device="cuda")


def _ref(q, k, v, Kd, Vd, cos, sin, p, rep):
    """fp64 attention of one sequence at position p: (HKV * rep * D,)."""
    c, s = cos[p].cpu(), sin[p].cpu()

    def rope(x):
        x0, x1 = x[..., :D // 2], x[..., D // 2:]
        return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1).double()

    qb = rope(q.float().cpu().view(HKV, rep, D))
    K = torch.cat([Kd[:, :p].cpu(), rope(k.float().cpu().view(HKV, 1, D))], 1)
    V = torch.cat([Vd[:, :p].cpu(), v.cpu().view(HKV, 1, D)], 1).double()
    w = torch.softmax(qb @ K.double().transpose(1, 2) * SCALE, -1)
    return (w @ V).reshape(-1)


def _check(rep, positions, seed, poison=None):
    """One paged step.  ``poison``: {b: (page index j, entry)} written into
    the table after the pages of b were filled with 0xAB.  Active sequences
    against fp64 and the dense kernel's append; inactive ones: zero output."""
    poison = poison or {}
    table, (cos, sin) = _table(), _rope_table()
    (kp, vp), q, k, v = _case(rep, seed)
    active = [0 <= p < PPS * PAGE and b not in poison
              for b, p in enumerate(positions)]
    for b in range(B):
        if not active[b]:
            for t in (kp, vp):
                t[table[b].long()] = t[table[b].long()].view(
                    torch.uint8).fill_(0xAB).view(torch.bfloat16)
    Kd, Vd = _dense(kp, table), _dense(vp, table)
    K1, V1 = Kd.clone(), Vd.clone()
    ops.decode_attn_step(q, k, v, K1, V1, cos, sin, _pos_t(positions),
                         HKV * rep, HKV, SCALE, ragged=True)
    want_k, want_v = kp.clone(), vp.clone()
    for b, p in enumerate(positions):
        if active[b]:
            pg = int(table[b, p // PAGE])
            want_k[pg, :, p % PAGE] = K1[b, :, p]
            want_v[pg, :, p % PAGE] = V1[b, :, p]
    for b, (j, entry) in poison.items():
        table[b, j] = entry
    out = ops.paged_attn_step(q, k, v, kp, vp, table, cos, sin,
                              _pos_t(positions), HKV * rep, HKV, SCALE)
    assert out.shape == q.shape         # every byte of both pools:
    assert torch.equal(kp, want_k) and torch.equal(vp, want_v)
    for b, p in enumerate(positions):
        if not active[b]:
            assert not out[b].any(), (rep, positions, b)
            continue
        ref = _ref(q[b], k[b], v[b], Kd[b], Vd[b], cos, sin, p, rep)
        err = (out[b].double().cpu() - ref).abs().max().item()
        print(f"paged rep {rep} pos {p}: max err {err:.3e}")
        assert err <= 3e-2 + 2e-2 * ref.abs().max().item(), (rep, positions, b)
    return active


# an empty cache, fewer pages than splits, both sides of a page boundary; an
# uneven page split, the last row of the last page; inactive: a position out
# of range; entry -1 at the append page, num_pages among the earlier pages
@pytest.mark.parametrize("positions,poison,off", [
    ((0, 1, 15, 16), None, ()), ((17, 63, 64, 95), None, ()),
    ((-1, 20, 96, 40), None, (0, 2)),
    ((37, 20, 50, 40), {0: (2, -1), 2: (1, NP)}, (0, 2))])
@pytest.mark.parametrize("rep", (1, 4, 8))
def test_numerics_append_inactive(rep, positions, poison, off):
    assert _check(rep, positions, 7 + rep, poison) == [
        b not in off for b in range(B)]


def test_kv_store_matches_scatter():
    S = 37
    table = _table()
    table[1, 2:] = -1                 # two pages: rows 32..36 are dropped
    (kp, vp), _, _, _ = _case(1, 40)
    g = torch.Generator().manual_seed(41)
    k, v = (torch.randn(B, S, HKV, D, generator=g).bfloat16().cuda()
            .transpose(1, 2) for _ in range(2))
    rows = torch.arange(S, device="cuda")
    pg = table[:, rows // PAGE].long()                  # (B, S)
    keep, slot = pg >= 0, (rows % PAGE).expand(B, S)
    assert int(keep.sum()) == B * S - 5
    want = [kp.clone(), vp.clone()]
    for w, new in zip(want, (k, v)):
        w[pg[keep], :, slot[keep]] = new.transpose(1, 2)[keep]
    ops.paged_kv_store(k, v, kp, vp, table)
    assert torch.equal(kp, want[0]) and torch.equal(vp, want[1])


def test_guards():
    nb, rep, (cos, sin) = 2, 2, _rope_table()
    z = lambda *s, dt=torch.bfloat16: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    good = dict(kp=z(NP, HKV, PAGE, D), vp=z(NP, HKV, PAGE, D),
                table=_table(nb), pos=_pos_t((2, 3)))
    q, kv = z(nb, HKV * rep * D) + 1, z(nb, HKV * D) + 1
    bad = [dict(kp=z(NP, HKV, PAGE, D, dt=torch.float16)),
           dict(kp=z(NP, HKV, 32, D), vp=z(NP, HKV, 32, D)),
           dict(vp=z(NP, HKV, PAGE, 2 * D)[..., :D]),     # not contiguous
           dict(table=good["table"].long()), dict(table=good["table"].cpu()),
           dict(table=_table(nb + 1)), dict(pos=_pos_t((2,)))]
    for over in bad:
        a = {**good, **over}
        with pytest.raises(ValueError):
            ops.paged_attn_step(q, kv, kv, a["kp"], a["vp"], a["table"], cos,
                                sin, a["pos"], HKV * rep, HKV, SCALE)
    torch.cuda.synchronize()
    for a in bad + [good]:                   # nothing was launched
        assert not any(a[n].any() for n in ("kp", "vp") if n in a)


def test_graph_replay_matches_eager():
    rep, steps, nb, pos0 = 4, 3, 2, (14, 30)     # across a page boundary
    table, (cos, sin) = _table(nb), _rope_table()
    pools, _, _, _ = _case(rep, 22)
    ins = [_case(rep, 23 + i, nb)[1:] for i in range(steps)]
    call = lambda q, k, v, c, p: ops.paged_attn_step(  # noqa: E731
        q, k, v, *c, table, cos, sin, p, HKV * rep, HKV, SCALE)
    eager_pools = tuple(t.clone() for t in pools)
    eager = [call(*ins[i], eager_pools, _pos_t([p + i for p in pos0]))
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
        pos_t += 1
    assert all(torch.equal(a, b) for a, b in zip(pools, eager_pools))


def test_model_paged_step_and_generate(monkeypatch):
    from neuronx_distributed_amd.inference import generation
    from neuronx_distributed_amd.inference.kv_cache import (
        PagePool, build_kv_caches)

    cfg, model = _llama()
    calls, real_step = [], ops.paged_attn_step
    monkeypatch.setattr(ops, "paged_attn_step", lambda *a, **kw: (
        calls.append(1) or real_step(*a, **kw)))
    Bm, P = 3, 11
    pool = PagePool(2 * Bm, Bm, 2, "cuda")
    for b in reversed(range(Bm)):
        pool.allocate(b, 2 * PAGE)
    c1, c2 = (build_kv_caches(
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, 2 * PAGE,
        cfg.head_dim, device="cuda", kv_format="paged", page_pool=pool)
        for _ in range(2))
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (Bm, P + 1), device="cuda")
    positions = _pos_t((5, 11, -1))          # the third row is inactive
    with torch.no_grad():
        for c in (c1, c2):
            model(x[:, :P], kv_caches=c, pos_offset=0)
        got = model(x[:, P:], kv_caches=c1, pos_offset=positions)
        with monkeypatch.context() as m:     # the eager chain on gather()
            m.setattr(ops, "paged_attn_available", lambda: False)
            want = model(x[:, P:], kv_caches=c2, pos_offset=positions)
        assert len(calls) == cfg.num_hidden_layers   # once per layer, in got
    err = (got.float() - want.float()).abs().max().item()
    print(f"model paged step: max logit diff {err:.3e}")
    assert err <= LOGIT_ATOL
    pools, real = [], generation.build_kv_caches
    monkeypatch.setattr(
        generation, "build_kv_caches",
        lambda *a, **kw: pools.append(kw["page_pool"]) or real(*a, **kw))
    lens, N = (9, 4, 6), 8
    x = torch.randint(1, cfg.vocab_size, (3, 9), device="cuda")
    for b, n in enumerate(lens):
        x[b, n:] = 0
    out = generation.generate(model, x, max_new_tokens=N, kv_format="paged",
                              prompt_lens=lens)
    assert len(calls) > cfg.num_hidden_layers and out.shape == (3, 9 + N)
    for b, n in enumerate(lens):
        assert torch.equal(out[b, :n], x[b, :n])
        assert (out[b, n + N:] == 0).all()
    assert pools[0].num_pages == 4 < 3 * math.ceil((9 + N) / PAGE)
