"""GPU checks of the paged MXFP8 KV cache kernels (csrc/paged_attn_mx.hip) and
their route from LlamaAttention._cached_step and
generate(kv_format="paged_mxfp8").

Shapes of test_paged_attn_gpu.py: B 4, Hkv 2, D 128; 24 pages behind a fixed
random permutation as the table (an identity mapping or a wrong indirection
fails); 6 pages per sequence.  Addressing exactly (the one-hot construction of
test_decode_attn_mx_gpu.py); numerics against fp64 attention over the pools
as stored after the call, under min(2 * e_bf16, 3e-2) with e_bf16 measured in
the same run from ops.paged_attn_step on bf16 pools that hold the dequantized
values; the appended bytes against ops.decode_attn_mx_step(ragged=True) on a
dense copy.  Rows at or beyond a position hold 0xFF, the NaN encodings of
e4m3 and e8m0.

Measured on MI355X over the 20 cases of test_numerics_bytes_inactive: largest
error 3.772e-3 (rep 1, positions 0..16; the bf16 paged kernel 3.858e-3),
MX / bf16 ratio of one case 0.83..1.15 against the allowed 2."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from neuronx_distributed_amd.quantization.microscaling import pack_mx
from test_decode_attn_mx_gpu import (
    ATOL_CAP, FMT, REPS, _deq, _deq64, _packed, _ref64)
from test_paged_attn_gpu import (
    B, D, HKV, NP, PAGE, PPS, SCALE, _rope_table, _table)
from test_ragged_attn_gpu import (  # noqa: F401 (the fixture builds the lib)
    _llama, _pos_t, _require_lib)

SMAX = PPS * PAGE
W = (D, D // 32, D, D // 32)    # row bytes of the four pools: K, Ks, V, Vs


def _dense(pages, table):   # (B, HKV, 96, w): every sequence's rows in order
    x = pages[table.long()].transpose(1, 2)
    return x.reshape(B, HKV, SMAX, pages.shape[-1]).contiguous()


def _step(q, k, v, pools, table, rope, positions, rep):
    return ops.paged_attn_mx_step(q, k, v, *pools, table, *rope,
                                  _pos_t(positions), HKV * rep, HKV, SCALE)


@pytest.mark.parametrize("pos", (0, 15, 16, 31, 32, 33, 95))
@pytest.mark.parametrize("rep", REPS)
def test_one_hot(rep, pos):
    """q = 4 against one K row of 4s: that row takes all the weight and the
    output is its dequantized V, bit for bit.  Every call probes one target
    per (b, kvh); the calls sweep it over rows 0..pos, the appended one
    included.  V: e4m3-grid integers, a power-of-two scale per (page, head,
    row, block).  RoPE is the identity."""
    table, tl = _table(), _table().tolist()
    rope = (torch.ones(SMAX, D // 2, device="cuda"),
            torch.zeros(SMAX, D // 2, device="cuda"))
    pg, h = torch.arange(NP).view(NP, 1, 1, 1), torch.arange(HKV).view(
        1, HKV, 1, 1)
    r, d = torch.arange(PAGE).view(1, 1, PAGE, 1), torch.arange(D)
    v = ((3 * r + 5 * d + 7 * pg + 11 * h) % 17 - 8).float()
    sv = ((r + 2 * torch.arange(D // 32) + pg + h) % 4 - 1).float()
    vp0, vs0 = (t.cuda() for t in pack_mx(v, sv, FMT))
    four_p, four_s = (t.cuda() for t in _packed(torch.full((D,), 4.0)))
    g = torch.Generator().manual_seed(100 * pos + rep)
    q2 = torch.full((B, HKV * rep * D), 4.0, dtype=torch.bfloat16,
                    device="cuda")
    for base in range(0, pos + 1, B * HKV):
        rstar = [min(base + i, pos) for i in range(B * HKV)]
        kp, ks = (torch.zeros(NP, HKV, PAGE, w, dtype=torch.uint8,
                              device="cuda") for w in W[:2])
        vp, vs = vp0.clone(), vs0.clone()
        k2 = torch.zeros(B, HKV, D)
        for i, t in enumerate(rstar):
            if t < pos:
                kp[tl[i // HKV][t // PAGE], i % HKV, t % PAGE] = four_p
                ks[tl[i // HKV][t // PAGE], i % HKV, t % PAGE] = four_s
            else:
                k2[i // HKV, i % HKV] = 4.0
        v2 = (torch.randn(B, HKV * D, generator=g) * 0.5).bfloat16().cuda()
        out = _step(q2, k2.bfloat16().view(B, -1).cuda(), v2,
                    (kp, ks, vp, vs), table, rope, [pos] * B, rep)
        vd = _deq(vp, vs, torch.bfloat16)   # as stored after the call
        for i, t in enumerate(rstar):
            want = vd[tl[i // HKV][t // PAGE], i % HKV, t % PAGE]
            got = out.view(B, HKV, rep, D)[i // HKV, i % HKV]
            assert torch.equal(got, want.expand(rep, D)), (rep, pos, i, t)


# an empty cache, both sides of a page seam; a pair seam (32) and fewer
# pairs than splits; an uneven split and the last row of the last page;
# inactive: positions out of range; entry -1 at the append page, num_pages
# among the earlier pages
@pytest.mark.parametrize("positions,poison,off", [
    ((0, 1, 15, 16), {}, ()), ((17, 31, 32, 33), {}, ()),
    ((63, 64, 65, 95), {}, ()), ((-1, 20, 96, 40), {}, (0, 2)),
    ((37, 20, 50, 40), {0: (2, -1), 2: (1, NP)}, (0, 2))])
@pytest.mark.parametrize("rep", REPS)
def test_numerics_bytes_inactive(rep, positions, poison, off):
    clean, table, rope = _table(), _table(), _rope_table()
    for b, (j, entry) in poison.items():
        table[b, j] = entry
    g = torch.Generator().manual_seed(7 + rep)
    rnd = lambda *s: torch.randn(*s, generator=g) * 0.5   # noqa: E731
    pools = [t.cuda() for _ in range(2)
             for t in _packed(rnd(NP, HKV, PAGE, D))]
    q, k, v = (rnd(B, n * D).bfloat16().cuda()
               for n in (HKV * rep, HKV, HKV))
    active = [b for b in range(B) if b not in off]
    for b in off:                      # an inactive sequence's pages
        for t in pools:
            t[clean[b].long()] = 0xAB
    # the bf16 kernel on the very values the MX pools hold
    bf = [_deq(pools[0], pools[1], torch.bfloat16),
          _deq(pools[2], pools[3], torch.bfloat16)]
    out_b = ops.paged_attn_step(q, k, v, *bf, table, *rope,
                                _pos_t(positions), HKV * rep, HKV, SCALE)
    for b in active:                   # stale rows: NaN payload, NaN scale
        rows = torch.arange(positions[b], SMAX, device="cuda")
        for t in pools:
            t[clean[b, rows // PAGE].long(), :, rows % PAGE] = 0xFF
    want = [t.clone() for t in pools]
    dense = [_dense(t, clean) for t in pools]
    ops.decode_attn_mx_step(q, k, v, *dense, *rope, _pos_t(positions),
                            HKV * rep, HKV, SCALE, ragged=True)
    for b in active:
        p = positions[b]
        for t, dt in zip(want, dense):
            t[int(clean[b, p // PAGE]), :, p % PAGE] = dt[b, :, p]

    out = _step(q, k, v, pools, table, rope, positions, rep)
    assert all(torch.equal(a, w) for a, w in zip(pools, want))  # every byte
    assert all((t[clean[b].long()] == 0xAB).all() for b in off for t in pools)
    assert not out[list(off)].any() and torch.isfinite(out.float()).all()

    def err(o, Kd, Vd):   # fp64 attention over the cache as stored now
        return max((o[b:b + 1].double() - _ref64(
            q[b:b + 1], Kd[b:b + 1], Vd[b:b + 1], rope, positions[b], rep)
        ).abs().max().item() for b in active)

    dense = [_dense(t, clean) for t in pools]
    e = err(out, _deq64(*dense[:2]), _deq64(*dense[2:]))
    e_b = err(out_b, *(_dense(t, clean).double() for t in bf))
    print(f"paged mx rep {rep} pos {positions}: max err {e:.3e}, bf16 paged "
          f"kernel {e_b:.3e}")
    assert e <= min(2.0 * e_b, ATOL_CAP), (e, e_b)


@pytest.mark.parametrize("pos0,S", [(0, 1), (0, 33), (5, 33)])
def test_kv_store(pos0, S):
    table = _table()
    table[1, 1] = -1                   # rows 16..31 of sequence 1 are dropped
    g = torch.Generator().manual_seed(pos0 + 10 * S)
    k, v = (torch.randn(B, S, HKV, D, generator=g).bfloat16().cuda()
            .transpose(1, 2) for _ in range(2))
    pools = [torch.full((NP, HKV, PAGE, w), 0xAB, dtype=torch.uint8,
                        device="cuda") for w in W]
    with pytest.raises(ValueError):    # fp32 K: nothing is launched
        ops.paged_mx_kv_store(k.float(), v, *pools, table, pos0)
    torch.cuda.synchronize()
    assert all((t == 0xAB).all() for t in pools)
    rows = pos0 + torch.arange(S, device="cuda")
    pg = table[:, rows // PAGE].long()                  # (B, S)
    keep, slot = pg >= 0, (rows % PAGE).expand(B, S)
    assert int(keep.sum()) == B * S - len(set(range(16, 32))
                                          & set(rows.tolist()))
    want = [t.clone() for t in pools]
    for x, w in ((k, want[:2]), (v, want[2:])):
        for t, e in zip(w, _packed(x.cpu().float())):
            t[pg[keep], :, slot[keep]] = e.cuda().transpose(1, 2)[keep]
    ops.paged_mx_kv_store(k, v, *pools, table, pos0)
    assert all(torch.equal(a, w) for a, w in zip(pools, want))


def test_guards():
    nb, rep, (cos, sin) = 2, 2, _rope_table()
    z = lambda *s, dt=torch.uint8: torch.zeros(  # noqa: E731
        *s, dtype=dt, device="cuda")
    pools = [z(NP, HKV, PAGE, w) for w in W]
    good = dict(kp=pools[0], ks=pools[1], table=_table()[:nb].contiguous(),
                pos=_pos_t((2, 3)), cos=cos, sin=sin, rep=rep)
    bad = [dict(kp=z(NP, HKV, PAGE, D, dt=torch.bfloat16)),   # bf16 pools
           dict(ks=z(NP, HKV, PAGE, 2)),                      # scale shape
           dict(table=good["table"].long()), dict(pos=_pos_t((2, 3)).int()),
           dict(rep=3), dict(cos=cos[:SMAX - 1], sin=sin[:SMAX - 1])]
    for over in bad:
        a = {**good, **over}
        q = z(nb, HKV * a["rep"] * D, dt=torch.bfloat16) + 1
        kv = z(nb, HKV * D, dt=torch.bfloat16) + 1
        with pytest.raises(ValueError):
            ops.paged_attn_mx_step(q, kv, kv, a["kp"], a["ks"], *pools[2:],
                                   a["table"], a["cos"], a["sin"], a["pos"],
                                   HKV * a["rep"], HKV, SCALE)
    torch.cuda.synchronize()
    assert not any(t.any() for t in pools)   # nothing was launched


def test_generate_route_and_graph(monkeypatch):
    from neuronx_distributed_amd.inference.generation import generate

    cfg, model = _llama()
    calls = {"paged_attn_mx_step": 0, "paged_attn_step": 0,
             "decode_attn_mx_step": 0}
    for name in calls:
        def count(*a, _n=name, _f=getattr(ops, name), **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(ops, name, count)
    torch.manual_seed(1)
    x = torch.randint(1, cfg.vocab_size, (3, 33), device="cuda")
    lens, new = (33, 4, 18), 9
    kw = dict(max_new_tokens=new, kv_format="paged_mxfp8", prompt_lens=lens)
    eager = generate(model, x, use_cuda_graph=False, **kw)
    assert calls == {"paged_attn_mx_step": cfg.num_hidden_layers * (new - 1),
                     "paged_attn_step": 0, "decode_attn_mx_step": 0}
    graph = generate(model, x, use_cuda_graph=True, **kw)
    assert calls["paged_attn_step"] == calls["decode_attn_mx_step"] == 0
    assert eager.shape == (3, 33 + new) and torch.equal(eager, graph)
