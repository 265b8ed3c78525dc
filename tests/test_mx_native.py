"""CPU checks of the stored MX format and the MX linear layers: pack/unpack
bit round trips, the literal byte / nibble layout, the emulated mx_linear,
MXColumnParallel / MXRowParallel over gloo, and quantize.convert with
MX_MAPPING on the tiny llama."""

import pytest
import torch

from neuronx_distributed_amd.quantization import microscaling as mx
from neuronx_distributed_amd.quantization.microscaling import (
    dequantize_mx, mx_linear, pack_mx, quantize_mx, unpack_mx)

FMTS = ("fp8_e4m3", "fp4_e2m1")


def _bits(t):
    return t.contiguous().view(torch.int32)


def _edge_blocks(fmt):
    """(q, scales) as quantize_mx would return them, covering every fp4
    code, negative zero, an all-zero block and scales at both clamps."""
    grid = mx._FP4_GRID
    codes = torch.cat([grid, -grid])          # 16 values, -0.0 included
    assert torch.signbit(codes[8]) and codes[8] == 0
    if fmt == "fp4_e2m1":
        b0 = torch.cat([codes, codes.flip(0)])
    else:
        b0 = torch.cat([codes, torch.tensor(
            [448.0, -448.0, 2.0 ** -9, -2.0 ** -9, 2.0 ** -6, 240.0, 0.875,
             -0.0, 1.125, -13.0, 52.0, 0.001953125 * 3, 416.0, -7.0, 30.0,
             0.0])])
    q = torch.stack([b0, torch.zeros(32), b0.flip(0), -b0]).reshape(1, 128)
    q = torch.cat([q, q.flip(1)])             # (2, 128)
    s = torch.tensor([[-127.0, -127.0, 127.0, 0.0], [3.0, 127.0, -127.0,
                                                     -5.0]])
    return q, s


@pytest.mark.parametrize("fmt", FMTS)
def test_pack_unpack_bit_roundtrip_edges(fmt):
    q, s = _edge_blocks(fmt)
    p, sb = pack_mx(q, s, fmt)
    assert p.dtype == torch.uint8 and sb.dtype == torch.uint8
    assert p.shape == (2, 128 if fmt == "fp8_e4m3" else 64)
    assert sb.shape == (2, 4)
    assert int(sb.min()) == 0 and int(sb.max()) == 254
    q2, s2 = unpack_mx(p, sb, fmt)
    assert q2.dtype == q.dtype and s2.dtype == s.dtype
    assert torch.equal(_bits(q2), _bits(q))   # -0.0 survives
    assert torch.equal(s2, s)


@pytest.mark.parametrize("fmt", FMTS)
def test_pack_unpack_roundtrip_quantized(fmt):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 96, generator=g) * \
        torch.logspace(-4, 4, 15).reshape(3, 5, 1)
    x[0, 0, :32] = 0
    x[1, 2, 40] = -0.0
    q, s = quantize_mx(x, fmt)
    p, sb = pack_mx(q, s, fmt)
    q2, s2 = unpack_mx(p, sb, fmt)
    assert torch.equal(_bits(q2), _bits(q))
    assert torch.equal(s2, s)
    assert torch.equal(dequantize_mx(q2, s2, dtype=torch.float32),
                       dequantize_mx(q, s, dtype=torch.float32))


def test_payload_layout_literal_bytes():
    # fp8: one e4m3fn byte per element
    q = torch.zeros(1, 32)
    q[0, :8] = torch.tensor([1.0, -1.0, 448.0, 0.5, -0.0, 2.0 ** -9, 1.5,
                             -3.0])
    p, sb = pack_mx(q, torch.tensor([[-2.0]]), "fp8_e4m3")
    assert p[0, :8].tolist() == [0x38, 0xB8, 0x7E, 0x30, 0x80, 0x01, 0x3C,
                                 0xC4]
    assert p[0, 8:].tolist() == [0] * 24
    assert sb.tolist() == [[125]]
    # fp4: element 2i low nibble, 2i+1 high nibble; sign bit 3, grid index
    q = torch.zeros(1, 32)
    q[0, :8] = torch.tensor([0.5, 1.0, -6.0, 0.0, -0.0, 3.0, 1.5, -4.0])
    p, sb = pack_mx(q, torch.tensor([[127.0]]), "fp4_e2m1")
    assert p.shape == (1, 16)
    assert p[0, :4].tolist() == [0x21, 0x0F, 0x58, 0xE3]
    assert p[0, 4:].tolist() == [0] * 12
    assert sb.tolist() == [[254]]
    # scale bytes: emulation scale + 127
    _, sb = pack_mx(torch.zeros(1, 96), torch.tensor([[-127.0, 0.0, 9.0]]),
                    "fp8_e4m3")
    assert sb.tolist() == [[0, 127, 136]]
    # and back
    qq, ss = unpack_mx(torch.tensor([[0x21, 0x0F, 0x58, 0xE3] + [0] * 12],
                                    dtype=torch.uint8),
                       torch.tensor([[254]], dtype=torch.uint8), "fp4_e2m1")
    assert qq[0, :8].tolist() == [0.5, 1.0, -6.0, 0.0, -0.0, 3.0, 1.5, -4.0]
    assert torch.signbit(qq[0, 4]) and not torch.signbit(qq[0, 3])
    assert ss.tolist() == [[127.0]]


def test_pack_rejects_other_formats():
    with pytest.raises(ValueError):
        pack_mx(torch.zeros(1, 32), torch.zeros(1, 1), "fp8_e5m2")
    with pytest.raises(ValueError):
        mx_linear(torch.zeros(1, 32), torch.zeros(1, 32, dtype=torch.uint8),
                  torch.zeros(1, 1, dtype=torch.uint8), "fp6_e2m3")


@pytest.mark.parametrize("fmt", FMTS)
def test_cpu_mx_linear_is_the_emulation(fmt):
    """mx_linear on CPU == explicit quantize/dequantize/matmul, and its
    error against the dense fp64 product is the MX error itself: bounded by
    the error of the same dequantized operands multiplied in fp64, plus the
    bf16 output rounding (2^-9 relative per element) and the fp32
    accumulation (K * 2^-24), together below 2^-8."""
    g = torch.Generator().manual_seed(1)
    M, N, K = 17, 48, 256
    x = torch.randn(M, K, generator=g).bfloat16()
    w = torch.randn(N, K, generator=g) * 0.05
    bias = torch.randn(N, generator=g)
    wq, ws = quantize_mx(w, fmt)
    wp, wsb = pack_mx(wq, ws, fmt)

    xq, xs = quantize_mx(x, "fp8_e4m3")
    xd = dequantize_mx(xq, xs, dtype=torch.float32)
    wd = dequantize_mx(wq, ws, dtype=torch.float32)
    explicit = xd @ wd.t()
    assert torch.equal(mx_linear(x.float(), wp, wsb, fmt), explicit)
    assert torch.equal(mx_linear(x.float(), wp, wsb, fmt, bias=bias),
                       explicit + bias)
    y = mx_linear(x, wp, wsb, fmt)
    assert y.dtype == torch.bfloat16
    assert torch.equal(y, explicit.bfloat16())
    # leading dims are kept
    y3 = mx_linear(x.reshape(1, M, K), wp, wsb, fmt)
    assert y3.shape == (1, M, N) and torch.equal(y3[0], y)

    dense = x.double() @ w.double().t()
    emu64 = xd.double() @ wd.double().t()
    e_emul = ((emu64 - dense).norm() / dense.norm()).item()
    e_y = ((y.double() - dense).norm() / dense.norm()).item()
    print(f"{fmt}: rel err of MX operands {e_emul:.4f}, of mx_linear "
          f"{e_y:.4f}")
    assert 0 < e_emul < 0.5
    assert e_y <= e_emul + 2.0 ** -8


# ---------------------------------------------------------------------------
# tensor-parallel layers over gloo
# ---------------------------------------------------------------------------

def _layers_worker(rank, world, fmt):
    import neuronx_distributed_amd.parallel as pl
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import (
        ColumnParallelLinear, RowParallelLinear)
    from neuronx_distributed_amd.quantization import (
        MXColumnParallel, MXConfig, MXRowParallel)

    ps.initialize_model_parallel(tensor_model_parallel_size=world)
    pl.model_parallel_manual_seed(0)
    torch.manual_seed(0)
    cfg = MXConfig(weight_fmt=fmt)
    K, N, M = 128, 64, 9
    g = torch.Generator().manual_seed(5)
    x = torch.randn(M, K, generator=g)
    w_col = torch.randn(N, K, generator=g) * 0.1
    w_row = torch.randn(N, K, generator=g) * 0.1
    b = torch.randn(N, generator=g)

    # column parallel, gather_output: equals mx_linear on the full weight
    col = ColumnParallelLinear(K, N, bias=True, gather_output=True)
    nl = N // world
    with torch.no_grad():
        col.weight.copy_(w_col[rank * nl:(rank + 1) * nl])
        col.bias.copy_(b[rank * nl:(rank + 1) * nl])
    mcol = MXColumnParallel.from_float(col, cfg)
    assert mcol.weight.dtype == torch.uint8 and not mcol.weight.requires_grad
    assert mcol.scale.dtype == torch.uint8 and not mcol.scale.requires_grad
    for attr in ("tensor_model_parallel", "partition_dim"):
        assert getattr(mcol.weight, attr) == getattr(col.weight, attr)
        assert getattr(mcol.scale, attr) == getattr(col.weight, attr)
    full_p, full_s = pack_mx(*quantize_mx(w_col, fmt), fmt)
    assert torch.equal(mcol.weight, full_p[rank * nl:(rank + 1) * nl])
    assert torch.equal(mcol.scale, full_s[rank * nl:(rank + 1) * nl])
    with torch.no_grad():
        out = mcol(x)
    ref = mx_linear(x, full_p, full_s, fmt, bias=b)
    assert out.shape == (M, N)
    assert torch.equal(out, ref)

    # row parallel: K split between 32-blocks -> payload shards are slices
    row = RowParallelLinear(K, N, bias=True, input_is_parallel=False)
    kl = K // world
    with torch.no_grad():
        row.weight.copy_(w_row[:, rank * kl:(rank + 1) * kl])
        row.bias.copy_(b)
    mrow = MXRowParallel.from_float(row, cfg)
    full_p, full_s = pack_mx(*quantize_mx(w_row, fmt), fmt)
    pk = full_p.shape[1] // world
    assert torch.equal(mrow.weight, full_p[:, rank * pk:(rank + 1) * pk])
    assert torch.equal(mrow.scale,
                       full_s[:, rank * (kl // 32):(rank + 1) * (kl // 32)])
    assert mrow.weight.partition_dim == row.weight.partition_dim
    with torch.no_grad():
        out = mrow(x)
    # emulation of the K-split sum: per-shard fp32 products, added in rank
    # order, bias last -- the all-reduce's own order on 2 ranks
    ref = None
    for r in range(world):
        part = mx_linear(x[:, r * kl:(r + 1) * kl],
                         full_p[:, r * pk:(r + 1) * pk].contiguous(),
                         full_s[:, r * (kl // 32):(r + 1) * (kl // 32)]
                         .contiguous(), fmt)
        ref = part if ref is None else ref + part
    ref = ref + b
    assert torch.equal(out, ref)
    # and the split sum is the unsplit product up to fp32 summation order
    whole = mx_linear(x, full_p, full_s, fmt, bias=b)
    assert (out - whole).abs().max() <= 1e-5 * whole.abs().max()
    return True


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_mx_parallel_layers(world, fmt):
    from dist_utils import run_distributed

    assert all(run_distributed(_layers_worker, world_size=world,
                               args=(fmt,)))


def test_from_float_rejects_ragged_k():
    from dist_utils import run_distributed

    assert all(run_distributed(_ragged_worker, world_size=1))


def _ragged_worker(rank, world):
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import ColumnParallelLinear
    from neuronx_distributed_amd.quantization import MXColumnParallel

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    fl = ColumnParallelLinear(48, 16, bias=False)
    with pytest.raises(ValueError, match="48"):
        MXColumnParallel.from_float(fl)
    return True


def _convert_worker(rank, world, fmt):
    import neuronx_distributed_amd.parallel as pl
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.quantization import (
        MX_MAPPING, MXColumnParallel, MXConfig, MXRowParallel, quantize)

    ps.initialize_model_parallel(tensor_model_parallel_size=world)
    pl.model_parallel_manual_seed(0)
    torch.manual_seed(0)
    model = LlamaForCausalLM(get_config("tiny")).eval()
    torch.manual_seed(1)
    ids = torch.randint(0, 256, (1, 16))

    # per-layer MX error on the float model's own activations
    targets = {n: m for n, m in model.named_modules()
               if type(m) in MX_MAPPING}
    seen = {}
    hooks = [m.register_forward_hook(
        lambda mod, inp, out, n=n: seen.__setitem__(n, (inp[0], out)))
        for n, m in targets.items()]
    with torch.no_grad():
        ref_logits = model(ids)
    for h in hooks:
        h.remove()
    assert len(seen) == len(targets) == 7

    cfg = MXConfig(weight_fmt=fmt)
    with torch.no_grad():
        quantize.convert(model, cfg, mapping=MX_MAPPING)
        swapped = {n: m for n, m in model.named_modules()
                   if isinstance(m, (MXColumnParallel, MXRowParallel))}
        assert set(swapped) == set(targets)
        assert not any(type(m) in MX_MAPPING for m in model.modules())
        layer_err = []
        for n, m in swapped.items():
            inp, out = seen[n]
            layer_err.append(((m(inp) - out).norm() / out.norm()).item())
        q_logits = model(ids)
    assert torch.isfinite(q_logits).all()
    rel = ((q_logits - ref_logits).norm() / ref_logits.norm()).item()
    # First order, a relative perturbation e_l at layer l reaches the logits
    # through RMSNorm-ed residual blocks whose relative gain is about one,
    # so the logits move by at most the sum of the per-layer errors.
    bound = sum(layer_err)
    print(f"{fmt}: per-layer rel err {[round(e, 4) for e in layer_err]}, "
          f"logits rel err {rel:.4f}, bound {bound:.4f}")
    assert max(layer_err) < 0.25
    assert rel <= bound
    return True


@pytest.mark.parametrize("fmt", FMTS)
def test_convert_tiny_llama_with_mx_mapping(fmt):
    from dist_utils import run_distributed

    assert all(run_distributed(_convert_worker, world_size=1, args=(fmt,)))
