"""Paged decode attention microbench: ops.paged_attn_step over a page pool
behind a shuffled block table against ops.decode_attn_step(ragged=True) over
the dense cache that holds the same rows, at the llama3-8b decode shape
(B 32, Hq 32, Hkv 8, D 128).

  same      all positions ``--pos`` (1024): the cost of the indirection.
            paged_attn.hip is built without packed fp32 arithmetic
            (ops/build.py), decode_attn.hip with it, so the library's dense
            kernel differs from the paged one in its row math too.  With
            ``--dense-lib`` a third variant runs the dense kernel of a
            library built from decode_attn.hip alone with paged_attn.hip's
            flags: paged against that one is the page walk and nothing else.
  spread    positions evenly spread over ``--spread`` (64..2048), both
            kernels at those positions, and the bytes of a pool that holds
            ceil((pos_b + 1) / 16) pages per sequence against the dense cache
            of max(pos_b) + 1 rows per sequence.

Every variant is captured ``--iters`` times into one hipGraph, call i on
cache set i % sets (enough sets to exceed the Infinity Cache), and the graphs
of a group are replayed in turn ``--rounds`` times between device events;
median and min..max of the rounds are reported, us per call.

One process.  Usage (GPU box):
    timeout 600 python tests/bench_paged_attn.py [--dense-lib PATH]
"""

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--dense-lib", default=None)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--pos", type=int, default=1024)
ap.add_argument("--spread", type=int, nargs=2, default=[64, 2048])
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--iters", type=int, default=24)
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402

assert torch.cuda.is_available(), "bench_paged_attn needs a GPU"
assert ops.paged_attn_available() and ops.ragged_attn_available(), \
    "build neuronx_distributed_amd.ops first"

dense_lib = ctypes.CDLL(args.dense_lib) if args.dense_lib else None
dev = "cuda"
D, PAGE = 128, 16
B, Hq, Hkv = args.batch, args.hq, args.hkv
scale = D ** -0.5


def timed(fn):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3      # us


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


def run_group(title, variants):
    graphs = {n: capture(fns) for n, fns in variants.items()}
    times = {n: [] for n in graphs}
    for _ in range(args.rounds):
        for n, g in graphs.items():
            times[n].append(timed(g.replay) / args.iters)
    res = {n: (statistics.median(v), min(v), max(v)) for n, v in times.items()}
    print(f"  {title}")
    for n, (med, lo, hi) in res.items():
        print(f"    {n:22s} {med:8.1f} us  ({lo:.1f}..{hi:.1f})")
    return res


def bench(title, pos_t):
    """Both kernels at the (B,) positions ``pos_t`` over the same rows."""
    pps = -(-(int(pos_t.max()) + 1) // PAGE)
    Smax, n_pages = pps * PAGE, B * pps
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    q = torch.randn(B, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
    k = torch.randn(B, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    v = torch.randn(B, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    paged, dense, dense_same = [], [], []
    _, st = ops._decode_attn_check("bench", False, q, k, v, cos, sin, pos_t,
                                   B, Hq, Hkv, Smax, q.device, ragged=True)
    for _ in range(args.sets):
        table = torch.randperm(n_pages, device=dev).int().view(B, pps)
        pools = tuple(torch.randn(n_pages, Hkv, PAGE, D, dtype=torch.bfloat16,
                                  device=dev) * 0.5 for _ in range(2))
        rows = tuple(p[table.long()].transpose(1, 2).reshape(B, Hkv, Smax, D)
                     .contiguous() for p in pools)
        paged.append(lambda c=pools, t=table: ops.paged_attn_step(
            q, k, v, *c, t, cos, sin, pos_t, Hq, Hkv, scale))
        dense.append(lambda c=rows: ops.decode_attn_step(
            q, k, v, *c, cos, sin, pos_t, Hq, Hkv, scale, ragged=True))
        if dense_lib is not None:
            dense_same.append(lambda c=rows: ops._decode_attn_launch(
                dense_lib.decode_attn_ragged, False,
                (q, k, v, *c, cos, sin, pos_t), B, 1, Hq, Hkv, Smax, scale,
                st))
    a, b = paged[0](), dense[0]()
    torch.cuda.synchronize()
    print(f"{title}  B {B} Hq {Hq} Hkv {Hkv}, {pps} pages per sequence "
          f"({args.sets} cache sets); outputs differ by at most "
          f"{(a.float() - b.float()).abs().max().item():.2e}", flush=True)
    variants = {"dense ragged": dense, "paged": paged}
    if dense_same:
        same = dense_same[0]()
        torch.cuda.synchronize()
        print(f"  paged equals the same-flags dense output bit for bit: "
              f"{torch.equal(a, same)}")
        variants["dense, paged's flags"] = dense_same
    r = run_group("us per call", variants)
    for n in variants:
        if n != "paged":
            med, lo_, hi_ = r[n]
            print(f"    paged / {n} {r['paged'][0] / med:.3f}  (its spread "
                  f"{hi_ - lo_:.1f} us)", flush=True)
    return Smax


torch.manual_seed(0)
bench(f"all positions {args.pos}", torch.full((B,), args.pos, device=dev))
torch.cuda.empty_cache()
lo, hi = args.spread
spread = torch.linspace(lo, hi, B, device=dev).round().long()
Smax = bench(f"positions spread over [{lo}, {hi}]", spread)
row_bytes = Hkv * D * 2 * 2               # K and V, bf16
pool_rows = int((torch.div(spread + PAGE, PAGE, rounding_mode="floor")
                 * PAGE).sum())
print(f"  cache bytes per layer: pool {pool_rows * row_bytes / 2**20:.1f} "
      f"MiB, dense {B * Smax * row_bytes / 2**20:.1f} MiB "
      f"({pool_rows / (B * Smax):.3f})")
