"""Microbench for the pieces of the K-contiguous weight gradient at the
llama2-7b training shapes (M = 32768 tokens):

  swiglu_bwd   the plain kernel  vs  the dual-output kernel (dx and dx^T)
               vs  the plain kernel + ops.transpose(dx), 32768 x 22016
  transpose    X^T, gq^T, gk^T, gv^T (32768 x 4096 each) in one
               ops.transpose_multi launch  vs  four ops.transpose launches,
               and ops.transpose_batched (device table) for the host cost

Usage (GPU box):  python tests/bench_wgrad_tn.py [--iters N]
"""

import argparse
import ctypes
import os
import sys
import time

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
from neuronx_distributed_amd import ops  # noqa: E402

assert ops.swiglu_bwd_t_available() and ops.transpose_multi_available()
dev = "cuda"
bf = torch.bfloat16
M, H, I = 32768, 4096, 11008


def timed(fn, iters=args.iters):
    """(device ms per call, host ms per call spent enqueueing)."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    h0 = time.perf_counter()
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    host = (time.perf_counter() - h0) * 1e3 / iters
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters, host


print(f"== swiglu_bwd {M} x {2 * I} -> dx, dx^T")
x = torch.randn(M, 2 * I, dtype=bf, device=dev)
dy = torch.randn(M, I, dtype=bf, device=dev)
dx = torch.empty_like(x)
dxt = torch.empty(2 * I, M, dtype=bf, device=dev)
lib = ops._require_lib()


def old():
    lib.swiglu_bwd(ops._ptr(x), ops._ptr(dy), ops._ptr(dx), ctypes.c_long(M),
                   ctypes.c_int(I), ops._stream())


unit = 2.0 * M * I / 1e9   # GB of one (M, I) bf16 matrix
ms_old, _ = timed(old)
ms_dual, _ = timed(lambda: ops.swiglu_bwd_t(x, dy, dx=dx, dxt=dxt))
ms_tr, _ = timed(lambda: ops.transpose(dx, out=dxt))
print(f"plain           {ms_old:7.3f} ms {5 * unit / ms_old * 1e3:7.0f} GB/s"
      f" (3 read + 2 written)")
print(f"dual            {ms_dual:7.3f} ms {7 * unit / ms_dual * 1e3:7.0f} "
      f"GB/s (3 read + 4 written)")
print(f"plain+transpose {ms_old + ms_tr:7.3f} ms (transpose {ms_tr:.3f})")
print(f"dual - plain    {ms_dual - ms_old:7.3f} ms against a transpose of "
      f"{ms_tr:.3f} ms")
ref = torch.empty_like(dx)
lib.swiglu_bwd(ops._ptr(x), ops._ptr(dy), ops._ptr(ref), ctypes.c_long(M),
               ctypes.c_int(I), ops._stream())
ops.swiglu_bwd_t(x, dy, dx=dx, dxt=dxt)
print("dx bit-identical:", torch.equal(dx.view(torch.int16),
                                       ref.view(torch.int16)),
      " dxt == dx^T:", torch.equal(dxt, dx.t()))
del x, dy, dx, dxt, ref

print(f"== four {M} x {H} transposes")
xs = [torch.randn(M, H, dtype=bf, device=dev) for _ in range(4)]
outs = [torch.empty(H, M, dtype=bf, device=dev) for _ in range(4)]


def four():
    for a, o in zip(xs, outs):
        ops.transpose(a, out=o)


gb = 4 * 4.0 * M * H / 1e9
for name, fn in (("4 x transpose", four),
                 ("transpose_multi", lambda: ops.transpose_multi(xs, outs)),
                 ("transpose_batched", lambda: ops.transpose_batched(xs,
                                                                     outs))):
    ms, host = timed(fn)
    print(f"{name:18s} {ms:7.3f} ms {gb / ms * 1e3:7.0f} GB/s   host "
          f"{host:6.3f} ms per call")
