"""GEMM layout microbench for the llama2-7b backward at M = 32768 tokens
(seq 4096 x microbatch 8): what the K-contiguous (TN) form buys for dgrad and
wgrad, and what the transposes that produce it cost.

  transpose   ops.transpose GB/s (read + write) next to swiglu_fwd's
  dgrad       dY @ W (NN, W strided along the contraction)  vs
              F.linear(dY, W^T) (TN; W^T is cached per optimizer step)
  wgrad       dY^T @ X (NT, both strided)  vs
              transpose(dY) + transpose(X) + F.linear(dY^T, X^T)

Usage (GPU box):  python tests/bench_gemm_layout.py [--iters N]
Reads the shipped TunableOp table like tests/bench_gemm.py.
"""

import argparse
import os

import torch
import torch.nn.functional as F

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=10)
args = ap.parse_args()

table = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                     "profiles", "tunableop_gfx950.csv")
if os.path.exists(table) and os.environ.get("NXDA_TUNABLEOP", "1") == "1":
    torch.cuda.tunable.set_filename(table, insert_device_ordinal=False)
    torch.cuda.tunable.tuning_enable(False)
    torch.cuda.tunable.enable(True)

import sys  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))
from neuronx_distributed_amd import ops  # noqa: E402

assert ops.transpose_available()
dev = "cuda"
bf = torch.bfloat16
M, H, I = 32768, 4096, 11008


def timed(fn, iters=args.iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def rnd(r, c):
    return torch.randn(r, c, dtype=bf, device=dev)


print("== transpose (bytes = read + write)")
for R, C in [(M, H), (M, I), (M, 2 * I), (2 * I, H), (H, H), (H, I)]:
    x = rnd(R, C)
    out = torch.empty(C, R, dtype=bf, device=dev)
    ms = timed(lambda: ops.transpose(x, out=out))
    ms_t = timed(lambda: out.copy_(x.t()))
    gb = 4.0 * R * C / 1e9
    print(f"transpose {R:6d}x{C:6d}  {ms:7.3f} ms {gb / ms * 1e3:7.0f} GB/s"
          f"   (torch copy_ of x.t(): {ms_t:7.3f} ms)")
    del x, out
x = rnd(M, 2 * I)
ms = timed(lambda: ops.swiglu(x))
print(f"swiglu_fwd {M}x{2 * I} -> {I}: {ms:7.3f} ms "
      f"{6.0 * M * I / 1e9 / ms * 1e3:7.0f} GB/s")
del x

print("== dgrad: dY (M, out) @ W (out, in)")
for name, out_f, in_f in [("4096^2", H, H), ("gate_up", 2 * I, H),
                          ("down", H, I)]:
    dy, w = rnd(M, out_f), rnd(out_f, in_f)
    w_t = ops.transpose(w)
    nn_ms = timed(lambda: dy.matmul(w))
    tn_ms = timed(lambda: F.linear(dy, w_t))
    tf = 2.0 * M * out_f * in_f / 1e9
    print(f"dgrad {name:8s} NN {nn_ms:7.3f} ms {tf / nn_ms:6.0f} TF | "
          f"TN {tn_ms:7.3f} ms {tf / tn_ms:6.0f} TF | ratio "
          f"{tn_ms / nn_ms:5.3f}")
    del dy, w, w_t

print("== wgrad: dY^T (out, M) @ X (M, in)")
for name, out_f, in_f in [("4096^2", H, H), ("gate_up", 2 * I, H),
                          ("down", H, I)]:
    dy, x = rnd(M, out_f), rnd(M, in_f)
    dy_t = torch.empty(out_f, M, dtype=bf, device=dev)
    x_t = torch.empty(in_f, M, dtype=bf, device=dev)
    nt_ms = timed(lambda: dy.t().matmul(x))
    tdy_ms = timed(lambda: ops.transpose(dy, out=dy_t))
    tx_ms = timed(lambda: ops.transpose(x, out=x_t))
    tn_ms = timed(lambda: F.linear(dy_t, x_t))
    tf = 2.0 * M * out_f * in_f / 1e9
    total = tdy_ms + tx_ms + tn_ms
    print(f"wgrad {name:8s} NT {nt_ms:7.3f} ms {tf / nt_ms:6.0f} TF | "
          f"T(dY) {tdy_ms:6.3f} T(X) {tx_ms:6.3f} TN {tn_ms:7.3f} ms "
          f"{tf / tn_ms:6.0f} TF | T+T+TN {total:7.3f} ms ratio "
          f"{total / nt_ms:5.3f} (X^T shared by q,k,v: "
          f"{(tdy_ms + tx_ms / 3 + tn_ms) / nt_ms:5.3f})")
    del dy, x, dy_t, x_t
