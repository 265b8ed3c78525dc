"""MX decode microbench: the skinny MX linear (ops.mx_linear_skinny, fused
activation quantization, fp8 and fp4 weights) against the path it replaces
(ops.mx_quantize_rows + ops.mx_gemm_packed, the 128x128 tile) and against
torch.matmul in bf16, at M in {1, 8, 32} on three decode projections.

Device time per call: every path is captured ``--iters`` times into one
hipGraph and the graph is replayed between two device events, so the host's
per-call cost is not in the figure (a kernel boundary is).  The paths are
replayed in turn, ``--rounds`` times; the table gives the median and the
spread (min..max) over the rounds.  By default each captured call reads a
different copy of the weight, enough copies to exceed the 256 MiB Infinity
Cache, as consecutive layers of a model do; ``--warm`` reuses one copy.
GB/s = (weight payload + scale bytes) / time.

Usage (GPU box):  python tests/bench_mx_decode.py [--iters 40] [--rounds 7]
"""

import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                ".."))

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=40)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--warm", action="store_true",
                help="one weight copy (cache-resident) instead of a rotation")
ap.add_argument("--cold-bytes", type=int, default=640 << 20)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "bench_mx_decode needs a GPU"
assert ops.mx_gemm_available() and ops.mx_skinny_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
shapes = [("4096x4096", 4096, 4096), ("11008x4096", 11008, 4096),
          ("4096x11008", 4096, 11008 // 128 * 128)]
Ms = (1, 8, 32)


def rand_u8(*shape, hi=256):
    return torch.randint(0, hi, shape, dtype=torch.uint8, device=dev)


def copies(nbytes):
    if args.warm:
        return 1
    return min(args.iters, -(-args.cold_bytes // nbytes))


def capture(fns):
    """One graph of --iters calls, call i on weight copy i % len(fns)."""
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
    """{name: [us per call, one per round]}, the graphs replayed in turn."""
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


def fmt_us(v):
    return f"{statistics.median(v):6.1f} ({min(v):5.1f}..{max(v):5.1f})"


print(f"weights: {'one warm copy' if args.warm else 'rotating cold copies'}; "
      f"{args.iters} calls per graph, {args.rounds} rounds; us per call, "
      f"median (min..max)")
for name, n, k in shapes:
    nb16 = n * k * 2
    nb8 = n * k + n * k // 32
    nb4 = n * k // 2 + n * k // 32
    wb = [torch.randn(n, k, dtype=torch.bfloat16, device=dev) * 0.05
          for _ in range(copies(nb16))]
    # random payloads: finite e4m3 bytes (no 0x7F/0xFF NaN), scales near 1
    w8 = [(rand_u8(n, k, hi=0x7F) | (rand_u8(n, k, hi=2) << 7),
           rand_u8(n, k // 32, hi=4) + 120) for _ in range(copies(nb8))]
    w4 = [(rand_u8(n, k // 2), rand_u8(n, k // 32, hi=4) + 120)
          for _ in range(copies(nb4))]
    for m in Ms:
        x = torch.randn(m, k, dtype=torch.bfloat16, device=dev)
        xq, xs = ops.mx_quantize_rows(x)

        def tile(w, f):
            q, s = ops.mx_quantize_rows(x)
            return ops.mx_gemm_packed(q, s, w[0], w[1], f)

        graphs = {
            "bf16": capture([lambda w=w: x @ w.t() for w in wb]),
            "quant": capture([lambda: ops.mx_quantize_rows(x)]),
            "tile8": capture([lambda w=w: tile(w, "fp8_e4m3") for w in w8]),
            "tile4": capture([lambda w=w: tile(w, "fp4_e2m1") for w in w4]),
            "skinny8": capture([lambda w=w: ops.mx_linear_skinny(
                x, w[0], w[1], "fp8_e4m3") for w in w8]),
            "skinny4": capture([lambda w=w: ops.mx_linear_skinny(
                x, w[0], w[1], "fp4_e2m1") for w in w4]),
        }
        t = measure(graphs)
        med = {a: statistics.median(v) for a, v in t.items()}
        ks = ops.mx_skinny_splits(m, n, k, "fp4_e2m1")
        print(f"{name} M={m} (k_splits {ks})")
        for a in graphs:
            print(f"    {a:8s} {fmt_us(t[a])}")
        print(f"    skinny vs quant+tile: fp8 {med['tile8'] / med['skinny8']:.2f}x"
              f"  fp4 {med['tile4'] / med['skinny4']:.2f}x"
              f"   (worst case over rounds: fp8 "
              f"{min(t['tile8']) / max(t['skinny8']):.2f}x  fp4 "
              f"{min(t['tile4']) / max(t['skinny4']):.2f}x)")
        print(f"    bf16 / skinny: fp8 {med['bf16'] / med['skinny8']:.2f}x  "
              f"fp4 {med['bf16'] / med['skinny4']:.2f}x")
        print(f"    weight GB/s: bf16 {nb16 / med['bf16'] / 1e3:.0f}  "
              f"skinny fp8 {nb8 / med['skinny8'] / 1e3:.0f}  "
              f"skinny fp4 {nb4 / med['skinny4'] / 1e3:.0f}")
        del graphs
    del wb, w8, w4
    torch.cuda.empty_cache()
