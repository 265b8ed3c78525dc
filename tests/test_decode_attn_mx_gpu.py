"""GPU checks of the MXFP8 KV cache kernels (ops/csrc/decode_attn_mx.hip):
the fused decode attention that reads and appends the quantized cache, and
the prefill store mx_kv_store.

* exact V path and row addressing ("one-hot"): one cached row takes all the
  softmax weight (every other weight is exp2(-261) = 0 in fp32), so the output
  is bit-equal to that row's dequantized V, for every row position of every
  split, wave, quarter-wave and unroll slot, and for the appended row,
* exact K dim map ("probe"): one q dim against K rows that are zero only
  there, all 128 dims,
* random numerics against fp64 attention over the cache as stored after the
  call, under a bound MEASURED in the same run from the bf16 kernel
  (ops.decode_attn_step) on the same values: at most twice its max error and
  never above the 3e-2 of test_ops_gpu.py::test_decode_attn_numerics,
* the appended bytes, mx_kv_store, edge blocks, determinism, hipGraph replay,
  the Python guards and generate(kv_format="mxfp8") end to end.

Measured on MI355X, max |out - fp64 reference| over the 40 cases of
test_random_numerics: MX kernel 3.894e-3, bf16 kernel 3.792e-3 (both at rep 8,
pos 1: the rounding of an output near 1 to bf16); largest MX / bf16 ratio of
one case 1.10, against the allowed 2.
"""

import functools
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from neuronx_distributed_amd.quantization.microscaling import (
    dequantize_mx, pack_mx, quantize_mx, unpack_mx)

FMT = "fp8_e4m3"
D = 128
B, HKV = 2, 2
REPS = (1, 2, 4, 8)
POS = (0, 1, 3, 15, 16, 17, 63, 64, 65, 257)
SCALE = 1.0 / math.sqrt(D)
ATOL_CAP = 3e-2   # test_ops_gpu.py::test_decode_attn_numerics


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    from neuronx_distributed_amd.ops import build as _build

    _build.build()
    assert ops.is_available(), ops._LIB_ERR
    assert ops.decode_attn_available()
    assert ops.decode_attn_mx_available()


def _packed(x):
    return pack_mx(*quantize_mx(x, FMT), FMT)


def _deq(payload, scale, dtype):
    return dequantize_mx(*unpack_mx(payload, scale, FMT), dtype=dtype)


def _deq64(payload, scale):
    """Dequantized in fp64 throughout: 256 * 2^120 (the bf16 maximum,
    quantized) is 2^128, past fp32."""
    q, e = unpack_mx(payload, scale, FMT)
    return q.double() * torch.exp2(e.double()).repeat_interleave(32, dim=-1)


@functools.lru_cache(maxsize=None)
def _identity_table(n):
    return (torch.ones(n, D // 2, device="cuda"),
            torch.zeros(n, D // 2, device="cuda"))


@functools.lru_cache(maxsize=None)
def _rope_table(n):
    return ops.precompute_rope_freqs(n, D, device="cuda")


def _pos_t(pos):
    return torch.tensor([pos], dtype=torch.int64, device="cuda")


@functools.lru_cache(maxsize=None)
def _grid_v(nb, nh, Smax, pos):
    """V rows [0, pos) from e4m3-grid integers with a different power-of-two
    scale per (pair, row, block); rows from pos on are zero."""
    pair = torch.arange(nb * nh).reshape(nb, nh, 1, 1)
    r = torch.arange(Smax).reshape(1, 1, Smax, 1)
    d = torch.arange(D).reshape(1, 1, 1, D)
    blk = torch.arange(D // 32).reshape(1, 1, 1, D // 32)
    v = ((3 * r + 5 * d + 7 * pair) % 17 - 8).float()
    sv = ((r + 2 * blk + pair) % 4 - 1).float().expand(nb, nh, Smax, D // 32)
    vp, vs = pack_mx(v, sv, FMT)
    vp[:, :, pos:] = 0
    vs[:, :, pos:] = 0
    return vp.cuda(), vs.cuda()


def _call(q2, k2, v2, cache, table, pos, rep, nh=HKV):
    cos, sin = table
    return ops.decode_attn_mx_step(q2, k2, v2, *cache, cos, sin, _pos_t(pos),
                                   nh * rep, nh, SCALE)


# ---------------------------------------------------------------------------
# 1. exact V path and row addressing
# ---------------------------------------------------------------------------

# Smax = pos + 3 everywhere, and pos = Smax - 1 at three sizes
ONE_HOT = [(p, False) for p in POS] + [(p, True) for p in (0, 17, 257)]


@pytest.mark.parametrize("pos,last_row", ONE_HOT)
@pytest.mark.parametrize("rep", REPS)
def test_one_hot(rep, pos, last_row):
    """q = 4 everywhere against one K row of 4s (4 quantizes losslessly:
    e = -6, 4 * 64 = 256 is an e4m3 value): log2-score 128*16/sqrt(128)*log2 e
    ~ 261 against 0 for every other row, so l = 1 and out == dequantized V
    row r*, bit for bit.  Each call probes four target rows, one per
    (b, kvh) pair; together the calls sweep r* over every row 0..pos."""
    Smax = pos + 1 if last_row else pos + 3
    npair = B * HKV
    table = _identity_table(Smax)
    vp0, vs0 = _grid_v(B, HKV, Smax, pos)
    four_p, four_s = (t.cuda() for t in _packed(torch.full((D,), 4.0)))
    g = torch.Generator().manual_seed(100 * pos + rep)
    q2 = torch.full((B, HKV * rep * D), 4.0, dtype=torch.bfloat16,
                    device="cuda")
    for base in range(0, pos + 1, npair):
        rstar = torch.tensor([min(base + i, pos) for i in range(npair)])
        new = (rstar == pos).reshape(B, HKV).cuda()
        kp = torch.zeros(B, HKV, Smax, D, dtype=torch.uint8, device="cuda")
        ks = torch.zeros(B, HKV, Smax, D // 32, dtype=torch.uint8,
                         device="cuda")
        vp, vs = vp0.clone(), vs0.clone()
        for i in range(npair):
            if rstar[i] < pos:
                kp[i // HKV, i % HKV, rstar[i]] = four_p
                ks[i // HKV, i % HKV, rstar[i]] = four_s
        k2 = (new[:, :, None] * torch.full((D,), 4.0, device="cuda")) \
            .bfloat16().reshape(B, HKV * D)
        v2 = (torch.randn(B, HKV * D, generator=g) * 0.5).bfloat16().cuda()
        out = _call(q2, k2, v2, (kp, ks, vp, vs), table, pos, rep)

        # appended bytes (identity table: the roped K row is k2 itself)
        for buf, sbuf, row in ((kp, ks, k2), (vp, vs, v2)):
            ep, es = _packed(row.cpu().float().reshape(B, HKV, D))
            assert torch.equal(buf[:, :, pos].cpu(), ep)
            assert torch.equal(sbuf[:, :, pos].cpu(), es)
        assert torch.equal(vp[:, :, :pos], vp0[:, :, :pos])
        assert not vp[:, :, pos + 1:].any() and not kp[:, :, pos + 1:].any()
        # the cache as stored after the call, the appended row included
        vd = _deq(vp, vs, torch.bfloat16)
        idx = rstar.cuda().reshape(B, HKV, 1, 1).expand(B, HKV, 1, D)
        want = vd.gather(2, idx).expand(B, HKV, rep, D)
        got = out.view(B, HKV, rep, D)
        assert torch.equal(got, want), (
            f"rep {rep} pos {pos} targets {rstar.tolist()}: "
            f"{(got != want).any(-1).nonzero()[:8].tolist()}")


# ---------------------------------------------------------------------------
# 2. exact K dim map
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("run", range(4))
def test_probe_k_dims(run):
    """q is 64 at dim d only; the target row's K is 64 at d only, every
    other row (the appended one included) is 64 everywhere BUT d.  Target
    log2-score 64*64/sqrt(128)*log2 e ~ 522, all others 0: out == the
    target's dequantized V row.  A lane that read K bytes of another dim
    would see the target's zeros and lose the weight to the other rows."""
    nb, nh, pos = 16, 8, 40
    Smax = pos + 3
    pair = torch.arange(nb * nh)
    d = (pair + 32 * run) % D
    rstar = (7 * pair + 11 * run) % pos
    onehot = torch.nn.functional.one_hot(d, D).float() * 64.0   # (pairs, D)
    k = (64.0 - onehot).reshape(nb, nh, 1, D).repeat(1, 1, Smax, 1)
    k[pair // nh, pair % nh, rstar] = onehot
    k[:, :, pos:] = 0
    kp, ks = (t.cuda() for t in _packed(k))
    vp, vs = (t.clone() for t in _grid_v(nb, nh, Smax, pos))
    q2 = onehot.bfloat16().reshape(nb, nh * D).cuda()
    k2 = (64.0 - onehot).bfloat16().reshape(nb, nh * D).cuda()
    v2 = torch.ones(nb, nh * D, dtype=torch.bfloat16, device="cuda")
    out = _call(q2, k2, v2, (kp, ks, vp, vs), _identity_table(Smax), pos, 1,
                nh=nh)
    vd = _deq(vp, vs, torch.bfloat16)
    want = vd[(pair // nh).cuda(), (pair % nh).cuda(), rstar.cuda()]
    got = out.view(nb * nh, D)
    bad = (got != want).any(-1).nonzero().flatten()
    assert torch.equal(got, want), (
        f"run {run}: pairs {bad[:8].tolist()} dims {d[bad.cpu()][:8].tolist()}")


# ---------------------------------------------------------------------------
# 3. random numerics
# ---------------------------------------------------------------------------

def _rope32(x, cos, sin, pos):   # x (B, H, D), fp32 like the kernels
    c, s = cos[pos].float(), sin[pos].float()
    x = x.float()
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)


def _ref64(q2, Kd, Vd, table, pos, rep):
    """fp64 attention of the fp32-roped q over rows [0, pos] of Kd, Vd."""
    nb, nh = Kd.shape[:2]
    q = _rope32(q2.view(nb, nh * rep, D), *table, pos).double()
    kx = Kd[:, :, :pos + 1].double().repeat_interleave(rep, dim=1)
    vx = Vd[:, :, :pos + 1].double().repeat_interleave(rep, dim=1)
    att = torch.softmax((q.unsqueeze(2) @ kx.transpose(-1, -2)) * SCALE, -1)
    return (att @ vx).squeeze(2).reshape(nb, nh * rep * D)


def _mx_error(q2, k2, v2, cache, table, pos, rep):
    """Max error of the MX kernel against fp64 attention over the cache as
    stored AFTER the call: only the kernel's arithmetic is under test."""
    nh = cache[0].shape[1]
    out = _call(q2, k2, v2, cache, table, pos, rep, nh=nh)
    assert torch.isfinite(out.float()).all()
    ref = _ref64(q2, _deq64(cache[0], cache[1]), _deq64(cache[2], cache[3]),
                 table, pos, rep)
    return (out.double() - ref).abs().max().item()


def _bf16_error(q2, k2, v2, bk, bv, table, pos, rep):
    """The same for the bf16 kernel (ops.decode_attn_step) on bf16 caches."""
    nh = bk.shape[1]
    out = ops.decode_attn_step(q2, k2, v2, bk, bv, *table, _pos_t(pos),
                               nh * rep, nh, SCALE)
    return (out.double() - _ref64(q2, bk, bv, table, pos, rep)) \
        .abs().max().item()


def _bound(err_bf16):
    return min(2.0 * err_bf16, ATOL_CAP)


@pytest.mark.parametrize("pos", POS)
@pytest.mark.parametrize("rep", REPS)
def test_random_numerics(rep, pos):
    Smax = pos + 3
    table = _rope_table(Smax)
    g = torch.Generator().manual_seed(11 + 1000 * rep + pos)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).bfloat16().cuda()
    cache = (torch.zeros(B, HKV, Smax, D, dtype=torch.uint8, device="cuda"),
             torch.zeros(B, HKV, Smax, D // 32, dtype=torch.uint8,
                         device="cuda"),
             torch.zeros(B, HKV, Smax, D, dtype=torch.uint8, device="cuda"),
             torch.zeros(B, HKV, Smax, D // 32, dtype=torch.uint8,
                         device="cuda"))
    if pos:
        ops.mx_kv_store(rnd(B, HKV, pos, D), rnd(B, HKV, pos, D), *cache, 0)
    q2, k2, v2 = rnd(B, HKV * rep * D), rnd(B, HKV * D), rnd(B, HKV * D)
    # the bf16 kernel sees the very values the MX cache holds (e4m3 times a
    # power of two is exact in bf16)
    err_b = _bf16_error(q2, k2, v2, _deq(cache[0], cache[1], torch.bfloat16),
                        _deq(cache[2], cache[3], torch.bfloat16), table, pos,
                        rep)
    err = _mx_error(q2, k2, v2, cache, table, pos, rep)
    print(f"decode_attn_mx rep {rep} pos {pos}: max err {err:.3e}, bf16 "
          f"kernel {err_b:.3e}, bound {_bound(err_b):.3e}")
    assert err <= _bound(err_b), (err, err_b)

    kp, ks, vp, vs = (t.cpu() for t in cache)
    # appended V row: byte-exact
    ep, es = _packed(v2.cpu().float().reshape(B, HKV, D))
    assert torch.equal(vp[:, :, pos], ep) and torch.equal(vs[:, :, pos], es)
    # appended K row: in-kernel RoPE rounding may move a bf16 ulp, so
    # (a) canonical encoding: re-quantizing the dequantized row reproduces
    #     the bytes.  One legitimate exception: a block whose scaled amax lay
    #     in (224, 232) rounds DOWN to the e4m3 value 224, and 224 * 2^e
    #     re-quantizes as 448 * 2^(e-1): other bytes, the same values.  Such
    #     a block must have payload amax 224 and dequantize identically.
    kq, ke = unpack_mx(kp[:, :, pos], ks[:, :, pos], FMT)
    kd = dequantize_mx(kq, ke, dtype=torch.float32)
    rp, rs = _packed(kd)
    same = (rs == ks[:, :, pos])
    amax224 = kq.reshape(B, HKV, D // 32, 32).abs().amax(-1) == 224
    assert (same | amax224).all()
    assert torch.equal(dequantize_mx(*unpack_mx(rp, rs, FMT),
                                     dtype=torch.float32), kd)
    same_e = same.repeat_interleave(32, dim=-1)
    assert torch.equal(rp[same_e], kp[:, :, pos][same_e])
    # (b) one e4m3 ulp (normal) or one subnormal step from the fp32 row
    k_ref = _rope32(k2.view(B, HKV, D), *table, pos).cpu()
    step = torch.exp2(ke - 9).repeat_interleave(32, dim=-1)
    assert ((kd - k_ref).abs() <= k_ref.abs() / 8 + step).all()


# ---------------------------------------------------------------------------
# 4. mx_kv_store
# ---------------------------------------------------------------------------

def _sentinel_cache(nb, nh, Smax, d=D):
    mk = lambda w: torch.full((nb, nh, Smax, w), 0xAB, dtype=torch.uint8,
                              device="cuda")
    return mk(d), mk(d // 32), mk(d), mk(d // 32)


@pytest.mark.parametrize("layout", ["bshd_view", "batch_slice"])
@pytest.mark.parametrize("pos,S", [(0, 1), (0, 33), (5, 1), (5, 33)])
def test_mx_kv_store(pos, S, layout):
    nb, nh, Smax = 2, 3, 40
    g = torch.Generator().manual_seed(pos + 10 * S)
    mag = torch.exp2(torch.randint(-8, 9, (2 * nb, S, nh, D // 32, 1),
                                   generator=g).float())
    src = (torch.randn(2 * nb, S, nh, D // 32, 32, generator=g) * mag) \
        .reshape(2 * nb, S, nh, D).bfloat16().cuda()
    src_v = src.flip(-1).contiguous()
    if layout == "bshd_view":      # what the models hand in
        k, v = src[:nb].transpose(1, 2), src_v[:nb].transpose(1, 2)
    else:                          # every other batch entry of a BHSD tensor
        k = src.transpose(1, 2).contiguous()[::2]
        v = src_v.transpose(1, 2).contiguous()[::2]
    assert k.shape == (nb, nh, S, D) and (S == 1 or not k.is_contiguous())
    cache = _sentinel_cache(nb, nh, Smax)
    ops.mx_kv_store(k, v, *cache, pos)
    for x, buf, sbuf in ((k, cache[0], cache[1]), (v, cache[2], cache[3])):
        ep, es = _packed(x.cpu().float())
        assert torch.equal(buf[:, :, pos:pos + S].cpu(), ep)
        assert torch.equal(sbuf[:, :, pos:pos + S].cpu(), es)
        for t in (buf, sbuf):
            assert (t[:, :, :pos] == 0xAB).all()
            assert (t[:, :, pos + S:] == 0xAB).all()


def test_mx_kv_store_contract():
    nb, nh, Smax, S = 2, 2, 8, 3
    cache = _sentinel_cache(nb, nh, Smax)
    k = torch.randn(nb, nh, S, D, device="cuda").bfloat16()
    with pytest.raises(ValueError):                  # rows past the cache
        ops.mx_kv_store(k, k, *cache, Smax - S + 1)
    with pytest.raises(ValueError):
        ops.mx_kv_store(k, k, *cache, -1)
    with pytest.raises(ValueError):                  # D % 32 != 0
        k48 = torch.randn(nb, nh, S, 48, device="cuda").bfloat16()
        ops.mx_kv_store(k48, k48, *_sentinel_cache(nb, nh, Smax, 48), 0)
    with pytest.raises(ValueError):                  # non-dense last dim
        wide = torch.randn(nb, nh, S, 2 * D, device="cuda").bfloat16()
        ops.mx_kv_store(wide[..., ::2], k, *cache, 0)
    with pytest.raises(ValueError):                  # wrong dtypes
        ops.mx_kv_store(k.float(), k, *cache, 0)
    with pytest.raises(ValueError):
        ops.mx_kv_store(k, k, cache[0].view(torch.int8), *cache[1:], 0)
    with pytest.raises(ValueError):                  # scales of another shape
        ops.mx_kv_store(k, k, cache[0], cache[1][..., :2], *cache[2:], 0)
    torch.cuda.synchronize()
    for t in cache:                                  # nothing was launched
        assert (t == 0xAB).all()


# ---------------------------------------------------------------------------
# 5. edge blocks
# ---------------------------------------------------------------------------

def test_edge_blocks():
    """An all-zero K row, an all-zero V block, a K block whose amax is the
    bf16 maximum (q is zero on that block's dims and their RoPE partners, so
    the score stays finite), a V block with one tiny element: finite, and
    inside the bound of test_random_numerics."""
    rep, pos = 2, 17
    Smax = pos + 3
    table = _rope_table(Smax)
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).bfloat16()
    k, v = rnd(B, HKV, pos, D), rnd(B, HKV, pos, D)
    k[:, :, 3] = 0
    v[:, :, 5, 32:64] = 0
    k[:, :, 7, 0:32] = 0
    k[:, :, 7, 13] = torch.finfo(torch.bfloat16).max
    v[:, :, 9, 96:128] = 0
    v[:, :, 9, 100] = 1e-30
    q = rnd(B, HKV * rep, D)
    q[..., 0:32] = 0
    q[..., 64:96] = 0
    k2, v2 = rnd(B, HKV, D), rnd(B, HKV, D)
    k2[..., 32:64] = 0
    k2[..., 96:128] = 0           # the RoPE partners: the block stays zero
    v2[:, 0] = 0
    cache = tuple(torch.zeros_like(t) for t in _sentinel_cache(B, HKV, Smax))
    ops.mx_kv_store(k.cuda(), v.cuda(), *cache, 0)
    q2, k2, v2 = (t.reshape(B, -1).cuda() for t in (q, k2, v2))
    # the yardstick: the bf16 kernel on the unquantized rows (the bf16
    # maximum quantizes to 256 * 2^120 = 2^128, which the stored format
    # holds but a bf16 copy of the cache would not)
    pad = lambda t: torch.cat(   # noqa: E731
        [t, torch.zeros(B, HKV, Smax - pos, D, dtype=t.dtype)], 2).cuda()
    err_b = _bf16_error(q2, k2, v2, pad(k), pad(v), table, pos, rep)
    err = _mx_error(q2, k2, v2, cache, table, pos, rep)
    print(f"edge blocks: max err {err:.3e}, bf16 kernel {err_b:.3e}")
    assert err <= _bound(err_b), (err, err_b)
    # the zero block of the appended K row and the zero V row
    assert not cache[0][:, :, pos, 32:64].any()
    assert not cache[2][:, 0, pos].any()


# ---------------------------------------------------------------------------
# 6. determinism and graph capture
# ---------------------------------------------------------------------------

def _random_setup(rep, pos, Smax, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: (torch.randn(*s, generator=g) * 0.5).bfloat16().cuda()
    cache = tuple(torch.zeros_like(t) for t in _sentinel_cache(B, HKV, Smax))
    ops.mx_kv_store(rnd(B, HKV, pos, D), rnd(B, HKV, pos, D), *cache, 0)
    return cache, rnd


def test_deterministic():
    rep, pos = 4, 65
    cache, rnd = _random_setup(rep, pos, pos + 3, 21)
    q2, k2, v2 = rnd(B, HKV * rep * D), rnd(B, HKV * D), rnd(B, HKV * D)
    c1 = tuple(t.clone() for t in cache)
    c2 = tuple(t.clone() for t in cache)
    table = _rope_table(pos + 3)
    o1 = _call(q2, k2, v2, c1, table, pos, rep)
    o2 = _call(q2, k2, v2, c2, table, pos, rep)
    assert torch.equal(o1, o2)
    for a, b in zip(c1, c2):
        assert torch.equal(a, b)


def test_graph_replay_matches_eager():
    rep, pos0, steps = 4, 30, 4
    Smax = pos0 + steps + 2
    cache, rnd = _random_setup(rep, pos0, Smax, 22)
    cos, sin = _rope_table(Smax)
    ins = [(rnd(B, HKV * rep * D), rnd(B, HKV * D), rnd(B, HKV * D))
           for _ in range(steps)]
    eager_cache = tuple(t.clone() for t in cache)
    eager = [ops.decode_attn_mx_step(*ins[i], *eager_cache, cos, sin,
                                     _pos_t(pos0 + i), HKV * rep, HKV, SCALE)
             for i in range(steps)]

    q_s, k_s, v_s = (t.clone() for t in ins[0])
    pos_t = _pos_t(pos0)
    warm = tuple(t.clone() for t in cache)   # warm-up touches a copy only
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.decode_attn_mx_step(q_s, k_s, v_s, *warm, cos, sin, pos_t,
                                HKV * rep, HKV, SCALE)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_s = ops.decode_attn_mx_step(q_s, k_s, v_s, *cache, cos, sin,
                                        pos_t, HKV * rep, HKV, SCALE)
    for i in range(steps):
        for dst, src in zip((q_s, k_s, v_s), ins[i]):
            dst.copy_(src)
        graph.replay()
        assert torch.equal(out_s, eager[i]), i
        pos_t += 1
    for a, b in zip(cache, eager_cache):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------
# 7. guards
# ---------------------------------------------------------------------------

def test_guards():
    rep, pos, Smax = 2, 4, 8
    cos, sin = _rope_table(Smax)
    mx = tuple(torch.zeros_like(t) for t in _sentinel_cache(B, HKV, Smax))
    bf = torch.zeros(B, HKV, Smax, D, dtype=torch.bfloat16, device="cuda")
    q2 = torch.zeros(B, HKV * rep * D, dtype=torch.bfloat16, device="cuda")
    kv = torch.zeros(B, HKV * D, dtype=torch.bfloat16, device="cuda")
    args = (cos, sin, _pos_t(pos), HKV * rep, HKV, SCALE)
    with pytest.raises(ValueError):      # uint8 caches into the bf16 kernel
        ops.decode_attn_step(q2, kv, kv, mx[0], mx[2], *args)
    with pytest.raises(ValueError):      # bf16 caches into the MX kernel
        ops.decode_attn_mx_step(q2, kv, kv, bf, mx[1], bf, mx[3], *args)
    with pytest.raises(ValueError):
        ops.decode_attn_mx_step(q2.float(), kv, kv, *mx, *args)
    with pytest.raises(ValueError):      # RoPE table shorter than the cache
        ops.decode_attn_mx_step(q2, kv, kv, *mx, cos[:Smax - 1],
                                sin[:Smax - 1], *args[2:])
    with pytest.raises(ValueError):      # int32 position
        ops.decode_attn_mx_step(q2, kv, kv, *mx, cos, sin,
                                _pos_t(pos).int(), *args[3:])
    with pytest.raises(ValueError):      # GQA rep 3
        ops.decode_attn_mx_step(
            torch.zeros(B, HKV * 3 * D, dtype=torch.bfloat16, device="cuda"),
            kv, kv, *mx, cos, sin, _pos_t(pos), HKV * 3, HKV, SCALE)
    torch.cuda.synchronize()
    for t in mx:
        assert not t.any()


def test_guards_bf16():
    """decode_attn_step makes the same checks as the MX wrapper: each of
    these raises ValueError and launches nothing."""
    rep, pos, Smax = 2, 4, 8
    cos, sin = _rope_table(Smax)
    kc = torch.zeros(B, HKV, Smax, D, dtype=torch.bfloat16, device="cuda")
    vc = torch.zeros_like(kc)
    q2 = torch.ones(B, HKV * rep * D, dtype=torch.bfloat16, device="cuda")
    kv = torch.ones(B, HKV * D, dtype=torch.bfloat16, device="cuda")
    wide = torch.ones(B, 2 * HKV * D, dtype=torch.bfloat16, device="cuda")
    tail = (HKV * rep, HKV, SCALE)
    with pytest.raises(ValueError):      # GQA rep 3
        ops.decode_attn_step(
            torch.ones(B, HKV * 3 * D, dtype=torch.bfloat16, device="cuda"),
            kv, kv, kc, vc, cos, sin, _pos_t(pos), HKV * 3, HKV, SCALE)
    with pytest.raises(ValueError):      # q2 of the wrong width
        ops.decode_attn_step(q2[:, :-D], kv, kv, kc, vc, cos, sin,
                             _pos_t(pos), *tail)
    with pytest.raises(ValueError):      # fp32 q2
        ops.decode_attn_step(q2.float(), kv, kv, kc, vc, cos, sin,
                             _pos_t(pos), *tail)
    with pytest.raises(ValueError):      # k2, v2 of different row strides
        ops.decode_attn_step(q2, wide[:, :HKV * D], kv, kc, vc, cos, sin,
                             _pos_t(pos), *tail)
    with pytest.raises(ValueError):      # RoPE table shorter than the cache
        ops.decode_attn_step(q2, kv, kv, kc, vc, cos[:Smax - 1],
                             sin[:Smax - 1], _pos_t(pos), *tail)
    with pytest.raises(ValueError):      # int32 position
        ops.decode_attn_step(q2, kv, kv, kc, vc, cos, sin,
                             _pos_t(pos).int(), *tail)
    torch.cuda.synchronize()
    assert not kc.any() and not vc.any()     # nothing was appended


# ---------------------------------------------------------------------------
# 8. end to end
# ---------------------------------------------------------------------------

def test_generate_mxfp8_graph_matches_eager(monkeypatch):
    import torch.distributed as dist
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29553")
        dist.init_process_group("nccl", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg = get_config("test-d128")
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    torch.manual_seed(0)
    with torch.device("cuda"):
        model = LlamaForCausalLM(cfg)
    torch.set_default_dtype(prev)
    model.eval()

    calls = {"mx": 0, "bf16": 0}
    real_mx, real_bf16 = ops.decode_attn_mx_step, ops.decode_attn_step

    def count_mx(*a, **kw):
        calls["mx"] += 1
        return real_mx(*a, **kw)

    def count_bf16(*a, **kw):
        calls["bf16"] += 1
        return real_bf16(*a, **kw)

    monkeypatch.setattr(ops, "decode_attn_mx_step", count_mx)
    monkeypatch.setattr(ops, "decode_attn_step", count_bf16)
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (2, 33), device="cuda")
    new = 9
    out_eager = generate(model, x, max_new_tokens=new, use_cuda_graph=False,
                         kv_format="mxfp8")
    # eager: one call per layer per decode step, none on the bf16 kernel
    assert calls == {"mx": cfg.num_hidden_layers * (new - 1), "bf16": 0}
    out_graph = generate(model, x, max_new_tokens=new, use_cuda_graph=True,
                         kv_format="mxfp8")
    # a captured run calls the kernel from Python only while warming up
    # (twice) and capturing (once); an eager fallback would add new - 1 more
    assert calls == {"mx": cfg.num_hidden_layers * (new - 1 + 3), "bf16": 0}
    assert torch.equal(out_eager, out_graph), (out_eager, out_graph)
