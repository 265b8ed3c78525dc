"""MX linear microbench: the native block-scaled MFMA GEMM
(ops.mx_gemm_packed, fp8 and fp4 weights) against torch.matmul in bf16 on
the dequantized weight and torch._scaled_mm fp8, with mx_quantize_rows
timed separately.  Random operands; device-event timing after warm-up;
TFLOP/s = 2*M*N*K / time.

Usage (GPU box):  python tests/bench_mx_gemm.py [--iters 20]
"""

import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=20)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "bench_mx_gemm needs a GPU"
assert ops.mx_gemm_available(), "build neuronx_distributed_amd.ops first"

dev = "cuda"
shapes = [
    ("square_4k", 4096, 4096, 4096),
    ("mlp_up", 4096, 11008, 4096),
    ("mlp_down", 4096, 4096, 11008),
    ("decode_4k", 32, 4096, 4096),
    ("decode_up", 32, 11008, 4096),
    ("decode_down", 32, 4096, 11008),
]


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = torch.cuda.Event(True)
    t1 = torch.cuda.Event(True)
    t0.record()
    for _ in range(args.iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / args.iters


def rand_u8(*shape, hi=256):
    return torch.randint(0, hi, shape, dtype=torch.uint8, device=dev)


print(f"{'shape':12s} {'M':>5s} {'N':>6s} {'K':>6s} | {'bf16':>8s} "
      f"{'scaled_mm':>9s} {'mx_fp8':>8s} {'mx_fp4':>8s}  TF | "
      f"{'quant us':>8s} | fp8/bf16 fp4/bf16 (GEMM only; +quant)")
for name, m, n, k in shapes:
    x = torch.randn(m, k, dtype=torch.bfloat16, device=dev)
    w = torch.randn(n, k, dtype=torch.bfloat16, device=dev) * 0.05
    flops = 2.0 * m * n * k

    t_bf16 = timed(lambda: x @ w.t())

    x8 = x.to(torch.float8_e4m3fn)
    w8 = w.to(torch.float8_e4m3fn)
    one = torch.ones((), device=dev)
    try:
        t_smm = timed(lambda: torch._scaled_mm(
            x8, w8.t(), scale_a=one, scale_b=one, out_dtype=torch.bfloat16))
    except Exception as e:  # report, do not hide
        print(f"  _scaled_mm failed at {name}: {e}")
        t_smm = float("nan")

    t_q = timed(lambda: ops.mx_quantize_rows(x))
    xq, xs = ops.mx_quantize_rows(x)
    # random payloads: finite e4m3 bytes (no 0x7F/0xFF NaN), scales near 1
    w8p = (rand_u8(n, k, hi=0x7F) | (rand_u8(n, k, hi=2) << 7))
    w4p = rand_u8(n, k // 2)
    ws = rand_u8(n, k // 32, hi=4) + 120
    t_mx8 = timed(lambda: ops.mx_gemm_packed(xq, xs, w8p, ws, "fp8_e4m3"))
    t_mx4 = timed(lambda: ops.mx_gemm_packed(xq, xs, w4p, ws, "fp4_e2m1"))

    def tf(ms):
        return flops / (ms * 1e-3) / 1e12

    print(f"{name:12s} {m:5d} {n:6d} {k:6d} | {tf(t_bf16):8.1f} "
          f"{tf(t_smm):9.1f} {tf(t_mx8):8.1f} {tf(t_mx4):8.1f}     | "
          f"{t_q * 1e3:8.1f} | {t_bf16 / t_mx8:8.2f} {t_bf16 / t_mx4:8.2f} "
          f"({t_bf16 / (t_mx8 + t_q):.2f}, {t_bf16 / (t_mx4 + t_q):.2f})")
    print(f"    ms: bf16 {t_bf16:.4f} scaled_mm {t_smm:.4f} mx_fp8 "
          f"{t_mx8:.4f} mx_fp4 {t_mx4:.4f} quant {t_q:.4f}")
