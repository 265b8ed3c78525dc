"""GPU checks of the fused chunked-prefill attention over the paged KV cache
(csrc/paged_prefill_attn.hip, ops.paged_prefill_attn_step) and its route from
LlamaAttention._cached_step and generate(kv_format="paged", prefill_chunk=N).

Layouts as in test_paged_chunk_attn_gpu.py: pools behind a fixed random
permutation as the table.  Numerics against fp64 (rows gathered through the
table after the call, RoPE in fp32) within 3e-2 + 2e-2 max|ref| per sequence.
Both pools must equal, byte for byte, a copy that received the same real
tokens through ops.paged_chunk_attn_step in pieces of 8 (ops.paged_attn_step
for a remainder of 1): the appended rows are those kernels' bit for bit and
every other byte is unchanged.

Measured on MI355X, worst |out - fp64| over the active sequences:
test_numerics_append 3.910e-3 (rep 8, T 40, pos 0: the rounding of an output
near 1 to bf16), test_inactive 1.617e-3, test_steady_state_tile_loop
2.579e-4; the bound is at least 3e-2.  Model level: max logit difference
1.562e-2 against the torch chain.
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from test_paged_chunk_attn_gpu import _dense, _err
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    LOGIT_ATOL, _llama, _pos_t, _require_lib)

D, PAGE = 128, 16
SCALE = 1.0 / math.sqrt(D)
WIDE = (4, 2, 100, 24)    # B, Hkv, pages, pages per sequence (384 rows)
SMALL = (8, 2, 56, 6)     # 96 rows per sequence
LONG = (2, 1, 144, 72)    # 1152 rows per sequence


def _setup(layout, rep, T, seed):
    """The clean table, pools with every row written, q, k, v and cos/sin."""
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


def _by_steps(q, k, v, kp, vp, table, cos, sin, b, p, n, hq, hkv):
    """The first n tokens of sequence b into (kp, vp) through the existing
    steps of at most 8 tokens."""
    for t0 in range(0, n, 8):
        m = min(8, n - t0)
        sl = lambda x: x[b:b + 1, t0:t0 + m]   # noqa: E731
        if m == 1:
            ops.paged_attn_step(q[b:b + 1, t0], k[b:b + 1, t0], v[b:b + 1, t0],
                                kp, vp, table[b:b + 1], cos, sin,
                                _pos_t([p + t0]), hq, hkv, SCALE)
        else:
            ops.paged_chunk_attn_step(sl(q), sl(k), sl(v), kp, vp,
                                      table[b:b + 1], cos, sin,
                                      _pos_t([p + t0]), hq, hkv, SCALE)


def _check(layout, rep, T, positions, lens, seed, poison=None):
    """One paged prefill step.  ``lens``: n[b], None for T.  ``poison``:
    {b: (page index j, entry)} written into the table before the call.  The
    pages of inactive sequences hold 0xAB bytes.  Returns the activity."""
    nb, hkv, npg, pps = layout
    clean, (kp, vp), q, k, v, (cos, sin) = _setup(layout, rep, T, seed)
    table = clean.clone()
    for b, (j, entry) in (poison or {}).items():
        table[b, j] = entry
    ns = list(lens) if lens is not None else [T] * nb
    active = [1 <= n <= T and 0 <= p and p + n <= pps * PAGE and all(
        0 <= int(e) < npg for e in table[b, :(p + n - 1) // PAGE + 1])
        for b, (p, n) in enumerate(zip(positions, ns))]
    for b in range(nb):
        if not active[b]:
            for t in (kp, vp):
                t[clean[b].long()] = t[clean[b].long()].view(
                    torch.uint8).fill_(0xAB).view(torch.bfloat16)
    want_k, want_v = kp.clone(), vp.clone()
    for b in range(nb):
        if active[b]:
            _by_steps(q, k, v, want_k, want_v, table, cos, sin, b,
                      positions[b], ns[b], hkv * rep, hkv)
    out = ops.paged_prefill_attn_step(
        q, k, v, kp, vp, table, cos, sin, _pos_t(positions), hkv * rep, hkv,
        SCALE, None if lens is None else _pos_t(lens))
    assert out.shape == q.shape
    assert torch.equal(kp, want_k) and torch.equal(vp, want_v)
    Kd, Vd = _dense(kp, clean), _dense(vp, clean)
    for b, (p, n) in enumerate(zip(positions, ns)):
        if not active[b]:
            assert not out[b].any(), (rep, T, positions, b)
            continue
        assert not out[b, n:].any(), (rep, T, b, n)       # padding rows
        err, top = _err(out[b, :n], q[b, :n], Kd[b], Vd[b], cos, sin, p, rep)
        msg = f"paged prefill rep {rep} T {T} pos {p} n {n}: max err {err:.3e}"
        print(msg)
        assert err <= 3e-2 + 2e-2 * top, msg
    return active


# T just above one token block (256 / rep tokens): two workgroups, waves of
# pure padding.  An empty cache; a position off the page grid with a chunk
# across 64-row tile seams; a chunk ending on the last row of the table; a
# sequence whose real tokens end inside the first block (the second writes
# zeros only).
@pytest.mark.parametrize("rep", (1, 4, 8))
def test_numerics_append(rep):
    T, rows = 256 // rep + 8, WIDE[3] * PAGE
    assert _check(WIDE, rep, T, (0, 37, rows - T, 21),
                  (T, T, T, 256 // rep - 5), 7 + rep) == [True] * 4


# pos < 0; one row too many; entry -1 inside the range; entry num_pages in an
# earlier page; n = 0; n > T; entry -1 BEYOND the last page (active); a plain
# active sequence with padding.
@pytest.mark.parametrize("rep", (1, 4, 8))
def test_inactive(rep):
    T = 24
    active = _check(SMALL, rep, T, (-1, 97 - T, 10, 40, 5, 5, 14, 50),
                    (T, T, T, T, 0, T + 1, T, 20), 11 + rep,
                    {2: (1, -1), 3: (0, SMALL[2]), 6: (3, -1)})
    assert active == [False] * 6 + [True] * 2


@pytest.mark.parametrize("rep", (1, 4, 8))
def test_steady_state_tile_loop(rep):
    """A prefix beyond 1024 rows: 16 or more unmasked 64-row tiles and the
    page-id prefetch across them before the diagonal."""
    assert _check(LONG, rep, 40, (1030, 1152 - 40), None, 5) == [True, True]


def test_guards():
    nb, rep, T, (_, hkv, npg, pps) = 2, 2, 12, SMALL
    table, _, _, _, _, (cos, sin) = _setup(SMALL, rep, T, 1)
    z = lambda *s, dt=torch.bfloat16: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    good = dict(kp=z(npg, hkv, PAGE, D), vp=z(npg, hkv, PAGE, D),
                table=table[:nb].contiguous(), pos=_pos_t((2, 3)),
                lens=_pos_t((T, 5)), cos=cos)
    bad = [dict(kp=z(npg, hkv, PAGE, D, dt=torch.float16)),
           dict(kp=z(npg, hkv, 32, D), vp=z(npg, hkv, 32, D)),
           dict(vp=z(npg, hkv, PAGE, 2 * D)[..., :D]),     # not contiguous
           dict(table=good["table"].long()), dict(table=good["table"].cpu()),
           dict(pos=_pos_t((2,))), dict(pos=_pos_t((2, 3)).int()),
           dict(lens=_pos_t((T,))), dict(lens=_pos_t((T, 5)).int()),
           dict(lens=_pos_t((T, 5)).cpu()), dict(cos=cos[:pps * PAGE - 1])]
    for over in bad:
        a = {**good, **over}
        q, kv = z(nb, T, hkv * rep * D) + 1, z(nb, T, hkv * D) + 1
        with pytest.raises(ValueError):
            ops.paged_prefill_attn_step(q, kv, kv, a["kp"], a["vp"],
                                        a["table"], a["cos"], sin, a["pos"],
                                        hkv * rep, hkv, SCALE, a["lens"])
    torch.cuda.synchronize()
    for a in bad + [good]:                   # nothing was launched
        assert not any(a[n].any() for n in ("kp", "vp") if n in a)


def test_model_chunk_and_generate(monkeypatch):
    from neuronx_distributed_amd.inference import generation
    from neuronx_distributed_amd.inference.kv_cache import (
        PagePool, build_kv_caches)

    cfg, model = _llama()
    calls, real_step = [], ops.paged_prefill_attn_step
    monkeypatch.setattr(ops, "paged_prefill_attn_step", lambda *a, **kw: (
        calls.append(1) or real_step(*a, **kw)))
    Bm, P, S = 4, 11, 24
    pool = PagePool(3 * Bm, Bm, 3, "cuda")
    for b in reversed(range(Bm)):
        pool.allocate(b, 3 * PAGE)
    c1, c2 = (build_kv_caches(
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, 3 * PAGE,
        cfg.head_dim, device="cuda", kv_format="paged", page_pool=pool)
        for _ in range(2))
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (Bm, P + S), device="cuda")
    # the third sequence is inactive, the fourth has no real token
    kw = dict(pos_offset=_pos_t((5, 11, -1, 7)),
              chunk_lens=_pos_t((S, 17, S, 0)))
    with torch.no_grad():
        for c in (c1, c2):
            model(x[:, :P], kv_caches=c, pos_offset=0)
        got = model(x[:, P:], kv_caches=c1, **kw)
        assert len(calls) == cfg.num_hidden_layers   # once per layer
        with monkeypatch.context() as m:     # the eager chain on gather()
            m.setattr(ops, "paged_prefill_attn_available", lambda: False)
            want = model(x[:, P:], kv_caches=c2, **kw)
        assert len(calls) == cfg.num_hidden_layers
        with pytest.raises(ValueError):      # S <= 8 has no chunk_lens
            model(x[:, :4], kv_caches=c1, pos_offset=kw["pos_offset"],
                  chunk_lens=_pos_t((4,) * Bm))
    err = (got.float() - want.float()).abs().max().item()
    print(f"model paged prefill step: max logit diff {err:.3e}")
    assert got.shape == (Bm, S, cfg.vocab_size) and err <= LOGIT_ATOL

    lens, N = (37, 16, 5), 4
    x = torch.randint(1, cfg.vocab_size, (3, 37), device="cuda")
    n_model = len(calls)
    out = generation.generate(model, x, max_new_tokens=N, prompt_lens=lens,
                              kv_format="paged", prefill_chunk=16)
    assert out.shape == (3, 37 + N)
    assert len(calls) == n_model + 3 * cfg.num_hidden_layers   # three chunks
