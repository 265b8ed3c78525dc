"""Decode-attention microbench, MXFP8 cache against bf16 cache: the fused MX
kernel (ops.decode_attn_mx_step) and the bf16 kernel (ops.decode_attn_step)
at the llama3-8b decode shape (B 32, Hq 32, Hkv 8, D 128) over a range of
positions.

Device time per call: each kernel is captured ``--iters`` times into one
hipGraph and the graph is replayed between two device events.  Call i uses
cache set i % copies, one set per "layer", enough sets to exceed the 256 MiB
Infinity Cache (``--cold-bytes``), as the layers of a model do.  The two
graphs are replayed in turn, ``--rounds`` times; the table gives the median
and the spread (min..max).  Cache GB/s = bytes of rows [0, pos) of K and V
(payload + scales for MX) / time; the byte ratio is 132 / 256 = 0.516 by
construction.

Every position runs in a child process of its own under ``--limit`` seconds;
the first child that fails or runs out of time ends the run.

Usage (GPU box):  python tests/bench_decode_attn_mx.py [--pos 1024 4096 16384]
"""

import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pos", type=int, nargs="+", default=[1024, 4096, 16384])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--iters", type=int, default=32)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--cold-bytes", type=int, default=640 << 20)
ap.add_argument("--limit", type=int, default=240,
                help="seconds per position (one child process each)")
ap.add_argument("--child", type=int, default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

if args.child is None:
    for pos in args.pos:
        cmd = [sys.executable, os.path.abspath(__file__), "--child", str(pos),
               "--batch", str(args.batch), "--hq", str(args.hq),
               "--hkv", str(args.hkv), "--iters", str(args.iters),
               "--rounds", str(args.rounds),
               "--cold-bytes", str(args.cold_bytes)]
        try:
            rc = subprocess.run(cmd, timeout=args.limit).returncode
        except subprocess.TimeoutExpired:
            sys.exit(f"pos {pos}: no result within {args.limit} s; stopping")
        if rc != 0:
            sys.exit(f"pos {pos}: child exited with {rc}; stopping")
    sys.exit(0)

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "bench_decode_attn_mx needs a GPU"
assert ops.decode_attn_available() and ops.decode_attn_mx_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
D = 128
B, Hq, Hkv, pos = args.batch, args.hq, args.hkv, args.child
Smax = pos + 8
scale = D ** -0.5
row_bf16 = 2 * D * 2                 # K + V bytes per cached row
row_mx = 2 * (D + D // 32)
rows = B * Hkv * pos                 # rows streamed per call


def copies(set_bytes):
    return max(1, min(args.iters, -(-args.cold_bytes // set_bytes)))


def capture(fns):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for f in fns:
            f()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for i in range(args.iters):
            fns[i % len(fns)]()
    g.replay()
    torch.cuda.synchronize()
    return g


def measure(graphs):
    out = {k: [] for k in graphs}
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    for _ in range(args.rounds):
        for k, g in graphs.items():
            t0.record()
            g.replay()
            t1.record()
            torch.cuda.synchronize()
            out[k].append(t0.elapsed_time(t1) * 1e3 / args.iters)
    return out


torch.manual_seed(0)
cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
q2 = torch.randn(B, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
k2 = torch.randn(B, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
v2 = torch.randn(B, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
pos_t = torch.tensor([pos], dtype=torch.int64, device=dev)

n_bf16 = copies(B * Hkv * Smax * row_bf16)
n_mx = copies(B * Hkv * Smax * row_mx)
bf16_sets, mx_sets = [], []
for i in range(max(n_bf16, n_mx)):
    k = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev) * 0.5
    v = torch.randn(B, Hkv, Smax, D, dtype=torch.bfloat16, device=dev) * 0.5
    if i < n_mx:   # the MX sets hold the same rows, quantized natively
        c = tuple(torch.zeros(B, Hkv, Smax, w, dtype=torch.uint8, device=dev)
                  for w in (D, D // 32, D, D // 32))
        ops.mx_kv_store(k, v, *c, 0)
        mx_sets.append(c)
    if i < n_bf16:
        bf16_sets.append((k, v))
    del k, v

graphs = {
    "bf16": capture([lambda c=c: ops.decode_attn_step(
        q2, k2, v2, c[0], c[1], cos, sin, pos_t, Hq, Hkv, scale)
        for c in bf16_sets]),
    "mxfp8": capture([lambda c=c: ops.decode_attn_mx_step(
        q2, k2, v2, *c, cos, sin, pos_t, Hq, Hkv, scale) for c in mx_sets]),
}
t = measure(graphs)
med = {a: statistics.median(v) for a, v in t.items()}
print(f"pos {pos}  B {B} Hq {Hq} Hkv {Hkv}: {args.iters} calls per graph, "
      f"{args.rounds} rounds, cache sets bf16 {n_bf16} / mxfp8 {n_mx}; "
      f"us per call, median (min..max)")
for a, nbytes in (("bf16", rows * row_bf16), ("mxfp8", rows * row_mx)):
    print(f"    {a:6s} {med[a]:8.1f} ({min(t[a]):7.1f}..{max(t[a]):7.1f})   "
          f"cache {nbytes / 1e6:7.1f} MB  {nbytes / med[a] / 1e3:6.0f} GB/s")
print(f"    bf16 / mxfp8 time: {med['bf16'] / med['mxfp8']:.2f}x   bf16 "
      f"spread {100 * (max(t['bf16']) - min(t['bf16'])) / med['bf16']:.1f}% "
      f"of its median", flush=True)
