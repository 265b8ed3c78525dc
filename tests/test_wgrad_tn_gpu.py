"""GPU checks for the K-contiguous weight gradient (NXDA_WGRAD_TN): the
dual-output SwiGLU backward (ops/csrc/swiglu.hip ``swiglu_bwd_t``), the
four-matrix transpose with by-value descriptors (ops/csrc/transpose.hip
``transpose_bf16_multi``) and the layer wiring.

Every kernel check is bit equality: ``dx`` against the plain ``swiglu_bwd``
kernel, ``dxt`` against ``dx.t().contiguous()``, a transpose against
``.t().contiguous()``.  Destinations sit inside guarded buffers whose
sentinel elements must not change.  The SwiGLU shapes are the smallest that
reach each edge of its 64 x 64 tiling under the multiple-of-8 contract."""

import ctypes
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops

GUARD = 64      # sentinel elements on each side of a destination
FILL = 0x7B7B


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    from neuronx_distributed_amd.ops import build

    build.build()
    assert ops.swiglu_bwd_t_available(), ops._LIB_ERR
    assert ops.transpose_multi_available(), ops._LIB_ERR


def _bits(rows, cols, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-32768, 32767, (rows, cols), dtype=torch.int16,
                         device="cuda", generator=g).view(torch.bfloat16)


def _guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.int16,
                     device="cuda").view(torch.bfloat16)
    return buf, buf[GUARD:GUARD + numel]


def _guards_intact(buf, numel):
    raw = buf.view(torch.int16)
    return bool((raw[:GUARD] == FILL).all()
                and (raw[GUARD + numel:] == FILL).all())


def _old_swiglu_bwd(x, dy):
    N, twoI = x.shape
    dx = torch.empty_like(x)
    ops._require_lib().swiglu_bwd(
        ops._ptr(x), ops._ptr(dy), ops._ptr(dx), ctypes.c_long(N),
        ctypes.c_int(twoI // 2), ops._stream())
    return dx


@pytest.mark.parametrize("N,I", [(64, 64), (8, 8), (72, 40), (200, 328),
                                 (136, 11008)])
def test_swiglu_bwd_dual_exact_and_guarded(N, I):
    g = torch.Generator(device="cuda").manual_seed(N * 7 + I)
    x = (torch.randn(N, 2 * I, device="cuda", generator=g) * 2).bfloat16()
    dy = torch.randn(N, I, device="cuda", generator=g).bfloat16()
    ref = _old_swiglu_bwd(x, dy)
    bdx, dx = _guarded(N * 2 * I)
    bdt, dxt = _guarded(N * 2 * I)
    ops.swiglu_bwd_t(x, dy, dx=dx.view(N, 2 * I), dxt=dxt.view(2 * I, N))
    torch.cuda.synchronize()
    got = dx.view(N, 2 * I).view(torch.int16)
    assert torch.equal(got, ref.view(torch.int16))
    assert torch.equal(dxt.view(2 * I, N).view(torch.int16),
                       got.t().contiguous())
    assert _guards_intact(bdx, N * 2 * I) and _guards_intact(bdt, N * 2 * I)


def test_swiglu_bwd_dual_rejects_outside_contract():
    x = torch.zeros(12, 32, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):          # N % 8
        ops.swiglu_bwd_t(x, x[:, :16].contiguous())
    x = torch.zeros(16, 24, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):          # I % 8
        ops.swiglu_bwd_t(x, x[:, :12].contiguous())
    x = torch.zeros(16, 32, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(ValueError):          # dy strided
        ops.swiglu_bwd_t(x, x[:, :16])


def _multi_sources():
    wide = _bits(200, 400, seed=11)
    return [_bits(72, 136, seed=1), wide[:, 64:64 + 264], _bits(8, 8, seed=3),
            _bits(136, 64, seed=4)]


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_transpose_multi_exact_and_guarded(n):
    xs = _multi_sources()[:n]
    assert n < 2 or (xs[1].stride(0) == 400 and not xs[1].is_contiguous())
    bufs = [_guarded(x.numel()) for x in xs]
    outs = ops.transpose_multi(
        xs, [d.view(x.shape[1], x.shape[0]) for x, (_, d) in zip(xs, bufs)])
    torch.cuda.synchronize()
    for x, (buf, _), o in zip(xs, bufs, outs):
        assert o.shape == (x.shape[1], x.shape[0])
        assert torch.equal(o.view(torch.int16),
                           x.view(torch.int16).t().contiguous())
        assert _guards_intact(buf, x.numel())
    fresh = ops.transpose_multi(xs)
    for x, o in zip(xs, fresh):
        assert torch.equal(o.view(torch.int16),
                           x.view(torch.int16).t().contiguous())


def test_transpose_multi_rejects_before_launch():
    good = _bits(8, 8, seed=0)
    bg, dg = _guarded(64)
    for bad in (_bits(12, 8, seed=0),               # R % 8
                _bits(8, 16, seed=0)[:, :12],       # C % 8
                _bits(8, 24, seed=0)[:, 4:20],      # misaligned base
                _bits(8, 8, seed=0).float()):
        with pytest.raises(ValueError):
            ops.transpose_multi([good, bad],
                                [dg.view(8, 8),
                                 torch.empty(bad.shape[1], bad.shape[0],
                                             dtype=bad.dtype, device="cuda")])
    with pytest.raises(ValueError):
        ops.transpose_multi([good] * 5)
    with pytest.raises(ValueError):
        ops.transpose_multi([])
    torch.cuda.synchronize()
    # nothing was launched: the good matrix's destination is untouched
    assert bool((bg.view(torch.int16) == FILL).all())


def _ints(*shape, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-4, 5, shape, device="cuda", generator=g).bfloat16()


def _layer_weight_grads(make, x, gouts, on):
    from neuronx_distributed_amd.parallel import layers

    os.environ["NXDA_WGRAD_TN"] = "1" if on else "0"
    layers._WGRAD_TN_MIN_NUMEL = 1
    layers._WGRAD_TN_MIN_M = 1
    calls = []
    orig = ops.transpose_multi

    def counted(xs, outs=None):
        calls.append(len(list(xs)))
        return orig(xs, outs)

    ops.transpose_multi = counted
    try:
        layer = make()
        out = layer(x)
        outs = out if isinstance(out, tuple) else (out,)
        torch.autograd.backward(outs, gouts[:len(outs)])
        torch.cuda.synchronize()
    finally:
        ops.transpose_multi = orig
        layers._WGRAD_TN_MIN_NUMEL = 4096 * 4096
        layers._WGRAD_TN_MIN_M = 16384
        os.environ.pop("NXDA_WGRAD_TN", None)
    assert ops._WGRAD_HANDOFF[0] is None
    return [p.grad.clone() for p in layer.parameters()], calls


def _one_hot_rows(T, width, lo, hi, seed):
    """(1, T, width) with ONE nonzero integer in [lo, hi] per token."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    idx = torch.randint(0, width, (T, 1), device="cuda", generator=g)
    val = torch.randint(lo, hi + 1, (T, 1), device="cuda", generator=g)
    val = torch.where(val == 0, torch.ones_like(val), val)
    out = torch.zeros(T, width, device="cuda")
    return out.scatter_(1, idx, val.float()).bfloat16().unsqueeze(0)


def test_layers_weight_grads_bit_equal_with_and_without_tn():
    """LlamaMLP and LlamaAttention's QKV linear, hidden 256 / intermediate
    512, 264 tokens, the thresholds patched down, integer data, so that every
    fp32 partial sum of a weight gradient is exact and the two summation
    orders must give the same bits.

    QKV is linear: dense integers in [-4, 4].  The MLP has SwiGLU between
    its GEMMs, so its data is chosen to keep dx integer too: one nonzero per
    token in x (3 or 4) and in the upstream gradient, gate weights in
    [6, 9] (gate >= 18, where the fp32 sigmoid is exactly 1, so dgate =
    dy * up and dup = dy * gate), up and down weights in [-4, 4]: |dx| <=
    16 * 36, and a weight-gradient sum stays below 2^20."""
    import torch.distributed as dist

    from neuronx_distributed_amd.models.llama import (LlamaAttention,
                                                      LlamaMLP, get_config)
    from neuronx_distributed_amd.parallel import parallel_state as ps

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29791")
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(tensor_model_parallel_size=1)
    H, I, T = 256, 512, 264
    cfg = get_config("tiny", hidden_size=H, intermediate_size=I,
                     num_attention_heads=2, num_key_value_heads=2)

    def mlp():
        m = LlamaMLP(cfg).cuda().bfloat16()
        g = torch.Generator(device="cuda").manual_seed(5)
        with torch.no_grad():
            w = m.gate_up_proj.weight
            w[:I] = torch.randint(6, 10, (I, H), device="cuda",
                                  generator=g).bfloat16()
            w[I:] = _ints(I, H, seed=6)
            m.down_proj.weight.copy_(_ints(H, I, seed=7))
        return m

    x = _one_hot_rows(T, H, 3, 4, seed=1)
    g = [_one_hot_rows(T, H, -4, 4, seed=2)]
    off, c0 = _layer_weight_grads(mlp, x, g, on=False)
    on, c1 = _layer_weight_grads(mlp, x, g, on=True)
    # gate_up: X^T alone is built, dx^T came from SwiGLU's backward;
    # down_proj has opted out
    assert c0 == [] and c1 == [1], (c0, c1)
    assert all(bool(a.any()) for a in off)
    for a, b in zip(off, on):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))

    def qkv():
        m = LlamaAttention(cfg).cuda().bfloat16().qkv_proj
        with torch.no_grad():
            for i, p in enumerate(m.parameters()):
                p.copy_(_ints(*p.shape, seed=100 + i))
        return m

    x = _ints(1, T, H, seed=1)
    g = [_ints(1, T, H, seed=s) for s in (3, 4, 5)]
    off, c0 = _layer_weight_grads(qkv, x, g, on=False)
    on, c1 = _layer_weight_grads(qkv, x, g, on=True)
    assert c0 == [] and c1 == [4], (c0, c1)  # X^T, gq^T, gk^T, gv^T at once
    assert all(bool(a.any()) for a in off)
    for a, b in zip(off, on):
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))
