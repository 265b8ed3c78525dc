"""GPU checks of the skinny MX linear (ops/csrc/mx_skinny.hip): M <= 32 rows,
activation quantized inside the GEMM, K split over the waves of a workgroup
and, on request, over workgroups with a deterministic second-pass reduce.

* exact lane maps (W fragments loaded from global memory, x fragments
  quantized in registers, both reductions) with integer data whose every
  partial sum is exact in fp32,
* random GEMMs against the fp64 product of ``mx_quantize_rows(x)`` and the
  dequantized weight under the bound of tests/test_mx_gemm_gpu.py -- a fused
  quantizer that differed from ``mx_quantize_rows`` by one code or one scale
  step would miss it by orders of magnitude,
* the quantizer's edge blocks, row-strided x, determinism, hipGraph capture,
  no stores past M, the contract, and the dispatch from ``ops.mx_linear``.
"""

import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from neuronx_distributed_amd.quantization.microscaling import (
    dequantize_mx, pack_mx, quantize_mx, unpack_mx, _FP4_GRID)

FMTS = ("fp8_e4m3", "fp4_e2m1")

# The fp32 summation bound B = K * 2^-24 * (sum |a||w| + |bias|) is allowed
# MX_ACC_MARGIN = 4 times over: tests/test_mx_gemm_gpu.py::test_random_gemm
# measured 2.16 * B for one 128-deep block-scaled MFMA on MI355X and took the
# next power of two.  The skinny kernel issues the same instruction and adds
# its partial sums in fp32, so the same yardstick applies unchanged.
MX_ACC_MARGIN = 4.0


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    from neuronx_distributed_amd.ops import build as _build

    _build.build()
    assert ops.is_available(), ops._LIB_ERR
    assert ops.mx_gemm_available()
    assert ops.mx_skinny_available()


def _deq64(payload, scales, fmt):
    q, s = unpack_mx(payload, scales, fmt)
    return dequantize_mx(q.double(), s.double(), dtype=torch.float64)


# ---------------------------------------------------------------------------
# exact maps
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _exact_case(M, N, K, fmt):
    """The operands of test_mx_gemm_gpu._exact_operands: asymmetric integer /
    grid values with a different power-of-two scale per (row, k-block).
    |a| <= 8 * 2^2, |w| <= 8 * 2^2, K <= 640: every partial sum is a
    multiple of 2^-3 below 2^20, exact in fp32.  The activation is handed
    over as bf16, which holds these values exactly; so does e4m3 after the
    in-kernel block scaling (integers up to 8 times a power of two)."""
    m = torch.arange(M).reshape(M, 1)
    n = torch.arange(N).reshape(N, 1)
    k = torch.arange(K).reshape(1, K)
    kb = torch.arange(K // 32).reshape(1, K // 32)
    a = ((3 * m + 5 * k) % 17 - 8).float()
    sa = ((m + 2 * kb) % 4 - 1).float()
    if fmt == "fp8_e4m3":
        w = ((7 * n + 11 * k) % 17 - 8).float()
    else:
        code = (7 * n + 11 * k) % 16
        w = _FP4_GRID[code & 7] * torch.where(code >= 8, -1.0, 1.0)
    sw = ((3 * n + kb) % 4 - 1).float()
    ap, asb = pack_mx(a, sa, "fp8_e4m3")
    wp, wsb = pack_mx(w, sw, fmt)
    a64 = _deq64(ap, asb, "fp8_e4m3")
    x = a64.bfloat16()
    assert torch.equal(x.double(), a64)            # bf16 holds them exactly
    ref = a64 @ _deq64(wp, wsb, fmt).t()
    return x.cuda(), wp.cuda(), wsb.cuda(), ref


@pytest.mark.parametrize("k_splits", [1, 2, 5, 64])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [128, 384, 640])
@pytest.mark.parametrize("N", [16, 48, 272])
@pytest.mark.parametrize("M", [1, 15, 16, 17, 32])
def test_exact_maps(M, N, K, fmt, k_splits):
    x, wp, wsb, ref = _exact_case(M, N, K, fmt)
    assert ref.abs().max() < 2 ** 20 and ref.abs().max() > 0
    out = ops.mx_linear_skinny(x, wp, wsb, fmt, out_dtype=torch.float32,
                               k_splits=k_splits)
    assert out.dtype == torch.float32 and out.shape == (M, N)
    got = out.double().cpu()
    bad = (got != ref).nonzero()
    assert torch.equal(got, ref), (
        f"{len(bad)} of {M * N} wrong, first (m, n) = {bad[:8].tolist()}")


# ---------------------------------------------------------------------------
# random GEMM
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _random_case(M, N, K, fmt, bias_on):
    g = torch.Generator().manual_seed(M + 1000 * N + 7 * K)
    x = torch.randn(M, K, generator=g).bfloat16().cuda()
    w = torch.randn(N, K, generator=g) * 0.1
    bias = (torch.randn(N, generator=g).bfloat16().cuda()
            if bias_on else None)
    wp, wsb = pack_mx(*quantize_mx(w, fmt), fmt)
    wp, wsb = wp.cuda(), wsb.cuda()
    xq, xs = ops.mx_quantize_rows(x)
    xd, wd = _deq64(xq, xs, "fp8_e4m3"), _deq64(wp, wsb, fmt)
    ref = xd @ wd.t()
    absum = xd.abs() @ wd.abs().t()
    if bias_on:
        ref = ref + bias.double()
        absum = absum + bias.double().abs()
    bound = K * 2.0 ** -24 * absum
    return x, wp, wsb, bias, ref, bound


def _check_bound(out, ref, bound, tag):
    err = (out.double() - ref).abs()
    lim = MX_ACC_MARGIN * bound
    if out.dtype == torch.bfloat16:
        lim = lim + 2.0 ** -8 * ref.abs()
    ratio = (err / lim.clamp(min=1e-300)).max().item()
    print(f"{tag}: largest err / allowed = {ratio:.4f}")
    assert torch.isfinite(out).all()
    assert (err <= lim).all(), f"{tag}: err / allowed = {ratio}"


@pytest.mark.parametrize("k_splits", [None, 3])
@pytest.mark.parametrize("out_dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("bias_on", [False, True])
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("K", [128, 384])
@pytest.mark.parametrize("N", [16, 144])
@pytest.mark.parametrize("M", [1, 17, 32])
def test_random_gemm(M, N, K, fmt, bias_on, out_dtype, k_splits):
    """Same reference and bound as test_mx_gemm_gpu.py::test_random_gemm:
    the fp64 product of the operands mx_quantize_rows and the weight payload
    stand for; allowed error MX_ACC_MARGIN * K * 2^-24 * (sum |a||w| +
    |bias|), plus 2^-8 |ref| for a bf16 result."""
    x, wp, wsb, bias, ref, bound = _random_case(M, N, K, fmt, bias_on)
    out = ops.mx_linear_skinny(x, wp, wsb, fmt, bias=bias,
                               out_dtype=out_dtype, k_splits=k_splits)
    assert out.dtype == out_dtype and out.shape == (M, N)
    _check_bound(out, ref, bound,
                 f"M{M} N{N} K{K} {fmt} bias={bias_on} "
                 f"{str(out_dtype)[6:]} splits={k_splits}")


# ---------------------------------------------------------------------------
# the quantizer's edge blocks as activations
# ---------------------------------------------------------------------------

def _edge_rows():
    """The rows of test_mx_gemm_gpu.py::test_quantize_rows_edges."""
    rows = []
    for amax in (448.0, 896.0, 7.0, 1.75 * 2.0 ** -20, 448.0 * 2.0 ** -30,
                 448.0 * 2.0 ** 40, 2.0 ** -126, 450.0, 3.0 * 2.0 ** 100):
        b = torch.linspace(-1, 1, 32) * amax
        b[5] = amax
        b[6] = -amax / 3
        rows.append(b)
    rows.append(torch.zeros(32))
    sub = torch.full((32,), 2.0 ** -130)
    sub[3] = -2.0 ** -133
    rows.append(sub)
    ties = torch.tensor([17.0, 19.0, 21.0, 23.0, 25.0, 27.0, 29.0, 31.0] * 4)
    ties[0] = 448.0
    ties[1] = -0.0
    ties[2] = 2.0 ** -10
    ties[3] = 3 * 2.0 ** -10
    rows.append(ties)
    return torch.cat(rows).reshape(3, 128).bfloat16().cuda()


@pytest.mark.parametrize("fmt", FMTS)
def test_edge_block_activations(fmt):
    x = _edge_rows()
    g = torch.Generator().manual_seed(11)
    w = torch.randn(48, 128, generator=g) * 0.1
    wp, wsb = pack_mx(*quantize_mx(w, fmt), fmt)
    wp, wsb = wp.cuda(), wsb.cuda()
    xq, xs = ops.mx_quantize_rows(x)
    xd, wd = _deq64(xq, xs, "fp8_e4m3"), _deq64(wp, wsb, fmt)
    ref = xd @ wd.t()
    bound = 128 * 2.0 ** -24 * (xd.abs() @ wd.abs().t())
    out = ops.mx_linear_skinny(x, wp, wsb, fmt, out_dtype=torch.float32)
    _check_bound(out, ref, bound, f"edge blocks {fmt}")


# ---------------------------------------------------------------------------
# views, determinism, graphs, stores
# ---------------------------------------------------------------------------

def _small_case(M, N, K, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).bfloat16().cuda()
    w = torch.randn(N, K, generator=g) * 0.1
    bias = torch.randn(N, generator=g).bfloat16().cuda()
    wp, ws = pack_mx(*quantize_mx(w, fmt), fmt)
    return x, wp.cuda(), ws.cuda(), bias


@pytest.mark.parametrize("k_splits", [1, 2])
@pytest.mark.parametrize("M", [1, 17])
def test_row_strided_x(M, k_splits):
    K, N = 384, 48
    x, wp, ws, bias = _small_case(M, N, K, "fp8_e4m3", 5)
    big = torch.zeros(M, K + 64, dtype=torch.bfloat16, device="cuda")
    big[:, :K] = x
    view = big[:, :K]
    assert not view.is_contiguous() or M == 1
    a = ops.mx_linear_skinny(view, wp, ws, "fp8_e4m3", bias=bias,
                             k_splits=k_splits)
    b = ops.mx_linear_skinny(x, wp, ws, "fp8_e4m3", bias=bias,
                             k_splits=k_splits)
    assert torch.equal(a, b) and b.abs().max() > 0


@pytest.mark.parametrize("k_splits", [1, 2])
@pytest.mark.parametrize("fmt", FMTS)
def test_two_calls_bitwise_equal(fmt, k_splits):
    x, wp, ws, bias = _small_case(32, 144, 640, fmt, 7)
    a = ops.mx_linear_skinny(x, wp, ws, fmt, bias=bias,
                             out_dtype=torch.float32, k_splits=k_splits)
    b = ops.mx_linear_skinny(x, wp, ws, fmt, bias=bias,
                             out_dtype=torch.float32, k_splits=k_splits)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert a.abs().max() > 0


def test_graph_capture_replay():
    x, wp, ws, bias = _small_case(4, 48, 384, "fp4_e2m1", 3)

    def run(inp):
        return ops.mx_linear_skinny(inp, wp, ws, "fp4_e2m1", bias=bias,
                                    k_splits=2)

    eager = run(x)
    static_x = torch.zeros_like(x)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(static_x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static_y = run(static_x)
    static_x.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(static_y, eager)
    assert eager.abs().max() > 0


def _c_entry(x, wp, ws, out, work, M, N, K, wfmt, out_fp32, k_splits,
             row_stride=None):
    lib = ops._require_lib()
    return lib.mx_skinny_gemm(
        ops._ptr(x), ctypes.c_long(K if row_stride is None else row_stride),
        ops._ptr(wp), ops._ptr(ws), None, ops._ptr(out),
        ops._ptr(work) if work is not None else None, M, N, K, wfmt,
        out_fp32, k_splits, ops._stream())


@pytest.mark.parametrize("k_splits", [1, 2])
def test_no_stores_past_m(k_splits):
    M, N, K = 17, 48, 384
    x, wp, ws, _ = _small_case(M, N, K, "fp8_e4m3", 9)
    out = torch.full((M + 1, N), 7.0, device="cuda")
    work = torch.full((k_splits * M + 1, N), 7.0, device="cuda")
    assert _c_entry(x, wp, ws, out, work, M, N, K, 0, 1, k_splits) == 0
    torch.cuda.synchronize()
    assert (out[M] == 7.0).all()
    assert (work[k_splits * M] == 7.0).all()
    want = ops.mx_linear_skinny(x, wp, ws, "fp8_e4m3",
                                out_dtype=torch.float32, k_splits=k_splits)
    assert torch.equal(out[:M], want) and want.abs().max() > 0


# ---------------------------------------------------------------------------
# contract
# ---------------------------------------------------------------------------

def _w(N, K, fmt="fp8_e4m3"):
    kp = K // 2 if fmt == "fp4_e2m1" else K
    return (torch.zeros(N, kp, dtype=torch.uint8, device="cuda"),
            torch.full((N, K // 32), 127, dtype=torch.uint8, device="cuda"))


def test_contract_errors():
    x = torch.zeros(4, 128, dtype=torch.bfloat16, device="cuda")
    wp, ws = _w(16, 128)
    # M = 33
    with pytest.raises(ValueError, match="M=33"):
        ops.mx_linear_skinny(torch.zeros(33, 128, dtype=torch.bfloat16,
                                         device="cuda"), wp, ws, "fp8_e4m3")
    # K = 96
    wp96, ws96 = _w(16, 96)
    with pytest.raises(ValueError, match="K=96"):
        ops.mx_linear_skinny(x[:, :96].contiguous(), wp96, ws96, "fp8_e4m3")
    # N = 8
    wp8, ws8 = _w(8, 128)
    with pytest.raises(ValueError, match="N=8"):
        ops.mx_linear_skinny(x, wp8, ws8, "fp8_e4m3")
    # misaligned x
    xraw = torch.zeros(4 * 128 + 8, dtype=torch.bfloat16, device="cuda")
    xmis = xraw[1:1 + 4 * 128].view(4, 128)
    with pytest.raises(ValueError, match="aligned"):
        ops.mx_linear_skinny(xmis, wp, ws, "fp8_e4m3")
    # rows not a 16-byte multiple apart
    xodd = torch.zeros(4, 132, dtype=torch.bfloat16, device="cuda")[:, :128]
    with pytest.raises(ValueError, match="stride"):
        ops.mx_linear_skinny(xodd, wp, ws, "fp8_e4m3")
    # wrong dtypes / formats / mismatched K / bad split count
    with pytest.raises(ValueError):
        ops.mx_linear_skinny(x.float(), wp, ws, "fp8_e4m3")
    with pytest.raises(ValueError):
        ops.mx_linear_skinny(x, wp, ws, "fp8_e5m2")
    with pytest.raises(ValueError):
        ops.mx_linear_skinny(x, wp, ws, "fp4_e2m1")  # payload means K = 256
    with pytest.raises(ValueError):
        ops.mx_linear_skinny(x, wp, ws, "fp8_e4m3", k_splits=0)
    # the launcher itself refuses (buffers are big enough for K = 128)
    out = torch.full((4, 16), 7.0, device="cuda")
    work = torch.full((4, 16), 7.0, device="cuda")

    def launch(M, N, K, wfmt, k_splits=1, row_stride=None, wk=work):
        return _c_entry(x, wp, ws, out, wk, M, N, K, wfmt, 1, k_splits,
                        row_stride)

    assert launch(4, 16, 96, 0) != 0
    assert launch(4, 8, 128, 0) != 0
    assert launch(0, 16, 128, 0) != 0
    assert launch(33, 16, 128, 0) != 0
    assert launch(4, 16, 128, 2) != 0
    assert launch(4, 16, 128, 0, k_splits=0) != 0
    assert launch(4, 16, 128, 0, row_stride=64) != 0
    assert launch(4, 16, 128, 0, row_stride=132) != 0
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (work == 7.0).all()   # nothing ran
    assert launch(4, 16, 128, 0, k_splits=64) == 0      # clamped to 1
    torch.cuda.synchronize()
    assert (out == 0.0).all() and (work == 7.0).all()


# ---------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("fmt", FMTS)
def test_dispatch(fmt, monkeypatch):
    x, wp, ws, bias = _small_case(4, 144, 384, fmt, 13)
    monkeypatch.delenv("NXDA_MX_SKINNY", raising=False)
    skinny = ops.mx_linear_skinny(x, wp, ws, fmt, bias=bias)
    assert torch.equal(ops.mx_linear(x, wp, ws, fmt, bias=bias), skinny)
    # leading dims are flattened on the way in and restored on the way out
    y3 = ops.mx_linear(x.reshape(2, 2, 384), wp, ws, fmt, bias=bias)
    assert y3.shape == (2, 2, 144) and torch.equal(y3.reshape(4, 144), skinny)
    # switched off: quantize + the 128x128 tile, exactly
    monkeypatch.setenv("NXDA_MX_SKINNY", "0")
    xq, xs = ops.mx_quantize_rows(x)
    tile = ops.mx_gemm_packed(xq, xs, wp, ws, fmt, bias=bias)
    assert torch.equal(ops.mx_linear(x, wp, ws, fmt, bias=bias), tile)
    # the two paths are roundings of the same sum
    assert (skinny.float() - tile.float()).abs().max() <= \
        2.0 ** -6 * tile.float().abs().max()


@pytest.mark.parametrize("fmt", FMTS)
def test_mx_column_parallel_decode(fmt):
    import os
    import torch.distributed as dist
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import ColumnParallelLinear
    from neuronx_distributed_amd.quantization import (MXColumnParallel,
                                                      MXConfig)

    if not dist.is_initialized():
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29547")
        dist.init_process_group("nccl", rank=0, world_size=1)
    if not ps.model_parallel_is_initialized():
        ps.initialize_model_parallel(tensor_model_parallel_size=1)
    torch.manual_seed(0)
    K, N = 256, 144
    fl = ColumnParallelLinear(K, N, bias=True, gather_output=False,
                              dtype=torch.bfloat16)
    with torch.no_grad():
        fl.bias.copy_(torch.randn(N))
    ml = MXColumnParallel.from_float(fl, MXConfig(weight_fmt=fmt))
    x = torch.randn(4, 1, K).bfloat16()
    with torch.no_grad():
        gpu = ml.cuda()(x.cuda())
    assert gpu.is_cuda and gpu.dtype == torch.bfloat16
    assert gpu.shape == (4, 1, N)
    xq, xs = quantize_mx(x, "fp8_e4m3")
    xd = dequantize_mx(xq.double(), xs.double(), dtype=torch.float64)
    wd = _deq64(ml.weight.cpu(), ml.scale.cpu(), fmt)
    b = fl.bias.detach().cpu().double()
    ref = xd @ wd.t() + b
    bound = MX_ACC_MARGIN * K * 2.0 ** -24 * \
        (xd.abs() @ wd.abs().t() + b.abs()) + 2.0 ** -8 * ref.abs()
    assert ((gpu.cpu().double() - ref).abs() <= bound).all()
