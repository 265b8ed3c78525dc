"""GPU checks of the fused chunked-prefill attention over the paged MXFP8 KV
cache (ops.paged_prefill_attn_mx_step, the MX forms of
csrc/paged_prefill_attn.hip) and its route from LlamaAttention._cached_step
and generate(kv_format="paged_mxfp8", prefill_chunk=N).

Data of test_paged_chunk_attn_mx_gpu.py (0xFF, NaN in e4m3 and e8m0, in the
rows at or beyond an active position), cases of
test_paged_prefill_attn_gpu.py.  All four pools must equal, byte for byte, a
copy that received the same real tokens through ops.paged_chunk_attn_mx_step
in pieces of 8 (ops.paged_attn_mx_step for a remainder of 1).  Numerics
against fp64 attention over the pools as stored after the call, within
min(2 * e_bf16, 3e-2) of test_paged_attn_mx_gpu.py, e_bf16 the error of
ops.paged_prefill_attn_step on bf16 pools of the dequantized values.

Measured on MI355X, worst error of a call (MX, bf16, ratio; 2 is allowed):
test_numerics_bytes rep 1 4.557e-3, 4.269e-3, 1.068; rep 4 4.486e-3, 4.069e-3,
1.103; rep 8 7.006e-3, 4.825e-3, 1.452; test_inactive 1.499e-3 .. 2.485e-3,
ratios 0.932 .. 0.977; test_steady_state_tile_loop 2.053e-4, 2.200e-4, 0.933.
Bytes equal in every case.  Model level: max logit difference 1.562e-2."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from test_decode_attn_mx_gpu import ATOL_CAP, _deq, _deq64
from test_paged_chunk_attn_gpu import _err
from test_paged_chunk_attn_mx_gpu import _dense, _setup
from test_paged_prefill_attn_gpu import LONG, PAGE, SCALE, SMALL, WIDE, D
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    LOGIT_ATOL, _llama, _pos_t, _require_lib)


def _by_steps(q, k, v, pools, table, rope, b, p, n, hq, hkv):
    # the first n tokens of sequence b through the MX steps of at most 8
    for t0 in range(0, n, 8):
        m = min(8, n - t0)
        tail = (table[b:b + 1], *rope, _pos_t([p + t0]), hq, hkv, SCALE)
        if m == 1:
            ops.paged_attn_mx_step(q[b:b + 1, t0], k[b:b + 1, t0],
                                   v[b:b + 1, t0], *pools, *tail)
        else:
            ops.paged_chunk_attn_mx_step(*(x[b:b + 1, t0:t0 + m]
                                           for x in (q, k, v)), *pools, *tail)


def _check(layout, rep, T, positions, lens, seed, poison=None):
    """One step; arguments and result as _check of
    test_paged_prefill_attn_gpu.py."""
    nb, hkv, npg, pps = layout
    clean, pools, q, k, v, rope = _setup(layout, rep, T, seed)
    table = clean.clone()
    for b, (j, entry) in (poison or {}).items():
        table[b, j] = entry
    ns = list(lens) if lens is not None else [T] * nb
    active = [1 <= n <= T and 0 <= p and p + n <= pps * PAGE and all(
        0 <= int(e) < npg for e in table[b, :(p + n - 1) // PAGE + 1])
        for b, (p, n) in enumerate(zip(positions, ns))]
    on = [b for b in range(nb) if active[b]]
    off = [b for b in range(nb) if not active[b]]
    for t in pools:                    # an inactive sequence's pages
        t[clean[off].long()] = 0xAB
    tail = (table, *rope, _pos_t(positions), hkv * rep, hkv, SCALE,
            None if lens is None else _pos_t(lens))
    # the bf16 kernel on the very values the MX pools hold
    bf = [_deq(*pools[:2], torch.bfloat16), _deq(*pools[2:], torch.bfloat16)]
    out_b = ops.paged_prefill_attn_step(q, k, v, *bf, *tail)
    for b in on:                       # stale rows: NaN payload, NaN scale
        rows = torch.arange(positions[b], pps * PAGE, device="cuda")
        for t in pools:
            t[clean[b, rows // PAGE].long(), :, rows % PAGE] = 0xFF
    want = [t.clone() for t in pools]
    for b in on:
        _by_steps(q, k, v, want, table, rope, b, positions[b], ns[b],
                  hkv * rep, hkv)
    out = ops.paged_prefill_attn_mx_step(q, k, v, *pools, *tail)
    assert out.shape == q.shape and torch.isfinite(out.float()).all()
    assert all(torch.equal(a, w) for a, w in zip(pools, want))  # every byte
    assert all((t[clean[b].long()] == 0xAB).all() for b in off for t in pools)
    assert not out[off].any()
    assert not any(out[b, ns[b]:].any() for b in on)      # padding rows

    def err(o, Kd, Vd):   # fp64 attention over the cache as stored now
        return max(_err(o[b, :ns[b]], q[b, :ns[b]], Kd[b], Vd[b], *rope,
                        positions[b], rep)[0] for b in on)

    dense = [_dense(t, clean) for t in pools]
    e = err(out, _deq64(*dense[:2]), _deq64(*dense[2:]))
    e_b = err(out_b, *(_dense(t, clean) for t in bf))
    print(f"paged prefill mx rep {rep} T {T} pos {positions}: max err "
          f"{e:.3e}, bf16 paged kernel {e_b:.3e}, ratio {e / e_b:.3f}")
    assert e <= min(2.0 * e_b, ATOL_CAP), (e, e_b)
    return active


# the cases of test_paged_prefill_attn_gpu.py, where their reasons stand
@pytest.mark.parametrize("rep", (1, 4, 8))
def test_numerics_bytes(rep):
    T, rows = 256 // rep + 8, WIDE[3] * PAGE
    assert _check(WIDE, rep, T, (0, 37, rows - T, 21),
                  (T, T, T, 256 // rep - 5), 7 + rep) == [True] * 4


@pytest.mark.parametrize("rep", (1, 4, 8))
def test_inactive(rep):
    T = 24
    active = _check(SMALL, rep, T, (-1, 97 - T, 10, 40, 5, 5, 14, 50),
                    (T, T, T, T, 0, T + 1, T, 20), 11 + rep,
                    {2: (1, -1), 3: (0, SMALL[2]), 6: (3, -1)})
    assert active == [False] * 6 + [True] * 2


def test_steady_state_tile_loop():
    assert _check(LONG, 4, 40, (1030, 1152 - 40), None, 5) == [True, True]


def test_guards():
    nb, rep, T, (_, hkv, npg, pps) = 2, 2, 12, SMALL
    table, _, _, _, _, (cos, sin) = _setup(SMALL, rep, T, 1)
    z = lambda *s, dt=torch.uint8: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    pools = [z(npg, hkv, PAGE, w) for w in (D, D // 32, D, D // 32)]
    good = dict(kp=pools[0], ks=pools[1], table=table[:nb].contiguous(),
                pos=_pos_t((2, 3)), lens=_pos_t((T, 5)), cos=cos)
    for over in (dict(kp=z(npg, hkv, PAGE, D, dt=torch.bfloat16)),
                 dict(ks=z(npg, hkv, PAGE, 2)),          # scale-pool width
                 dict(table=good["table"].long()),
                 dict(pos=_pos_t((2,))), dict(pos=_pos_t((2, 3)).int()),
                 dict(lens=_pos_t((T,))), dict(lens=_pos_t((T, 5)).int()),
                 dict(lens=_pos_t((T, 5)).cpu()),
                 dict(cos=cos[:pps * PAGE - 1])):
        a = {**good, **over}
        q = z(nb, T, hkv * rep * D, dt=torch.bfloat16) + 1
        kv = z(nb, T, hkv * D, dt=torch.bfloat16) + 1
        with pytest.raises(ValueError):
            ops.paged_prefill_attn_mx_step(
                q, kv, kv, a["kp"], a["ks"], *pools[2:], a["table"],
                a["cos"], sin, a["pos"], hkv * rep, hkv, SCALE, a["lens"])
    assert not any(t.any() for t in pools)   # nothing was launched


def test_model_chunk_and_generate(monkeypatch):
    from neuronx_distributed_amd.inference import generation
    from neuronx_distributed_amd.inference.kv_cache import (
        PagePool, build_kv_caches)

    cfg, model = _llama()
    calls, real_step = [], ops.paged_prefill_attn_mx_step
    monkeypatch.setattr(ops, "paged_prefill_attn_mx_step", lambda *a, **kw: (
        calls.append(1) or real_step(*a, **kw)))
    Bm, P, S = 4, 11, 24
    pool = PagePool(3 * Bm, Bm, 3, "cuda")
    for b in reversed(range(Bm)):
        pool.allocate(b, 3 * PAGE)
    c1, c2 = (build_kv_caches(
        cfg.num_hidden_layers, Bm, cfg.num_key_value_heads, 3 * PAGE,
        cfg.head_dim, device="cuda", kv_format="paged_mxfp8", page_pool=pool)
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
            m.setattr(ops, "paged_prefill_attn_mx_available", lambda: False)
            want = model(x[:, P:], kv_caches=c2, **kw)
        assert len(calls) == cfg.num_hidden_layers
    err = (got.float() - want.float()).abs().max().item()
    print(f"model paged prefill mx step: max logit diff {err:.3e}")
    assert got.shape == (Bm, S, cfg.vocab_size) and err <= LOGIT_ATOL

    lens, N = (37, 16, 5), 4
    x = torch.randint(1, cfg.vocab_size, (3, 37), device="cuda")
    n_model = len(calls)
    out = generation.generate(model, x, max_new_tokens=N, prompt_lens=lens,
                              kv_format="paged_mxfp8", prefill_chunk=16)
    assert out.shape == (3, 37 + N)
    assert len(calls) == n_model + 3 * cfg.num_hidden_layers   # three chunks
