"""GPU checks for the tiled bf16 transpose (ops/csrc/transpose.hip).

A transpose is a permutation, so every check is exact equality with
``x.t().contiguous()`` on distinct-enough random bits; the destination sits
inside a larger guarded buffer and the bytes around it must not change.
Shapes: one chunk (8, 8), one full tile (64, 64), edge tiles in both
dimensions (72, 136), many tiles (256, 4096), a column slice of a wider
buffer (source row stride > C), and three different matrices in one batched
launch."""

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops

GUARD = 512  # elements on each side of a destination
FILL = 0x7B7B


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    from neuronx_distributed_amd.ops import build

    build.build()
    assert ops.transpose_available(), ops._LIB_ERR


def _bits(rows, cols, seed):
    """Random 16-bit patterns viewed as bf16 (compared as int16, so NaN
    patterns are fine)."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(-32768, 32767, (rows, cols), dtype=torch.int16,
                         device="cuda", generator=g).view(torch.bfloat16)


def _guarded(numel):
    buf = torch.full((numel + 2 * GUARD,), FILL, dtype=torch.int16,
                     device="cuda").view(torch.bfloat16)
    return buf, buf[GUARD:GUARD + numel]


def _check(buf, x):
    R, C = x.shape
    raw = buf.view(torch.int16)
    got = raw[GUARD:GUARD + R * C].view(C, R)
    assert torch.equal(got, x.view(torch.int16).t().contiguous())
    assert (raw[:GUARD] == FILL).all() and (raw[GUARD + R * C:] == FILL).all()


@pytest.mark.parametrize("R,C", [(8, 8), (64, 64), (72, 136), (256, 4096)])
def test_transpose_exact(R, C):
    x = _bits(R, C, seed=R * 131 + C)
    buf, dst = _guarded(R * C)
    out = ops.transpose(x, out=dst.view(C, R))
    torch.cuda.synchronize()
    assert out.data_ptr() == dst.data_ptr()
    _check(buf, x)
    assert torch.equal(ops.transpose(x).view(torch.int16),
                       x.view(torch.int16).t().contiguous())


def test_transpose_strided_source():
    wide = _bits(4096, 528, seed=7)
    x = wide[:, 128:128 + 264]          # row stride 528 > C = 264
    assert x.stride(0) == 528 and not x.is_contiguous()
    buf, dst = _guarded(x.numel())
    ops.transpose(x, out=dst.view(264, 4096))
    torch.cuda.synchronize()
    _check(buf, x)


def test_transpose_batched_three_shapes():
    wide = _bits(200, 400, seed=11)
    xs = [_bits(72, 136, seed=1), wide[:, 64:64 + 264], _bits(8, 8, seed=3)]
    bufs = [_guarded(x.numel()) for x in xs]
    outs = ops.transpose_batched(
        xs, [d.view(x.shape[1], x.shape[0]) for x, (_, d) in zip(xs, bufs)])
    torch.cuda.synchronize()
    for x, (buf, _), o in zip(xs, bufs, outs):
        _check(buf, x)
        assert o.shape == (x.shape[1], x.shape[0])


def test_transpose_rejects_shapes_outside_contract():
    with pytest.raises(ValueError):
        ops.transpose(_bits(12, 8, seed=0))             # R % 8
    with pytest.raises(ValueError):
        ops.transpose(_bits(8, 16, seed=0)[:, :12])     # C % 8
    with pytest.raises(ValueError):
        ops.transpose(_bits(8, 24, seed=0)[:, 4:20])    # misaligned base
    with pytest.raises(ValueError):
        ops.transpose(_bits(8, 8, seed=0).float())
