"""Paged MXFP8 chunk attention microbench: ops.paged_chunk_attn_mx_step
(T = 2, 5, 8 new tokens per sequence) over MXFP8 page pools behind an
interleaved block table, at the llama3-8b decode shape (B 32, Hq 32, Hkv 8,
D 128), against

  chain   what LlamaAttention._cached_step did for this call before the
          kernel existed: the torch chain on PagedMXKVCache.gather() (a
          quantizing scatter of the new rows, a dequantized dense copy of K
          and V, batched GEMMs, softmax), run through that method with the
          kernel reported unavailable.  The one comparison the route depends
          on;
  bf16    ops.paged_chunk_attn_step over bf16 pools that hold the dequantized
          values behind the same table: the price of the dequantizing stage
          against half the bytes;
  dense   ops.chunk_attn_mx_step(ragged=True) over a dense MXFP8 cache that
          holds the same bytes: the price of the indirection.

Method of tests/bench_paged_chunk_attn.py: two position sets (all sequences
at ``--pos``, and positions spread over ``--spread``); every variant captured
``--iters`` times into one hipGraph, call i on cache set i % sets (enough
sets to exceed the Infinity Cache), after a warm-up on a side stream; the
graphs of a group replayed in turn ``--rounds`` times between device events;
the whole measurement ``--runs`` (2) times on fresh data, medians (min..max)
side by side, us per call.

One process.  Usage (GPU box):
    timeout 900 python tests/bench_paged_chunk_attn_mx.py
"""

import argparse
import os
import statistics
import sys
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--tokens", type=int, nargs="+", default=[2, 5, 8])
ap.add_argument("--pos", type=int, default=1024)
ap.add_argument("--spread", type=int, nargs=2, default=[64, 2048])
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--iters", type=int, default=12)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--runs", type=int, default=2)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402
from neuronx_distributed_amd.inference.kv_cache import (  # noqa: E402
    PagedMXKVCache, PagePool)
from neuronx_distributed_amd.models.llama import LlamaAttention  # noqa: E402
from neuronx_distributed_amd.quantization.microscaling import (  # noqa: E402
    dequantize_mx, pack_mx, quantize_mx, unpack_mx)

assert torch.cuda.is_available(), "bench_paged_chunk_attn_mx needs a GPU"
assert ops.paged_chunk_attn_mx_available() \
    and ops.paged_chunk_attn_available() and ops.ragged_attn_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
D, PAGE, FMT = 128, 16, "fp8_e4m3"
B, Hq, Hkv = args.batch, args.hq, args.hkv
scale = D ** -0.5
# LlamaAttention._cached_step without the projections around it
attn = types.SimpleNamespace(num_heads_local=Hq, num_kv_local=Hkv, head_dim=D,
                             sliding_window=None, o_proj=lambda x: x)


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


def run_group(variants):
    graphs = {n: capture(fns) for n, fns in variants.items()}
    times = {n: [] for n in graphs}
    for _ in range(args.rounds):
        for n, g in graphs.items():
            times[n].append(timed(g.replay) / args.iters)
    return {n: (statistics.median(v), min(v), max(v))
            for n, v in times.items()}


def chain(q, k, v, cache, cos, sin, pos_t):
    real = ops.paged_chunk_attn_mx_available
    ops.paged_chunk_attn_mx_available = lambda: False
    try:
        return LlamaAttention._cached_step(
            attn, q.view(B, -1, Hq, D), k.view(B, -1, Hkv, D),
            v.view(B, -1, Hkv, D), cos, sin, pos_t, cache, False)
    finally:
        ops.paged_chunk_attn_mx_available = real


def bench(T, pos_t):
    """The four variants at the (B,) positions ``pos_t`` over the same
    rows: {name: (median, min, max)} us."""
    pps = -(-(int(pos_t.max()) + T) // PAGE)
    Smax, n_pages = pps * PAGE, B * pps
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    q = torch.randn(B, T, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
    k = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    v = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    paged, bf16, dense, chained = [], [], [], []
    for _ in range(args.sets):
        # page j of every sequence before page j + 1 of any, the sequences
        # in a new order each time: no two pages of a sequence are adjacent
        pool = PagePool(n_pages, B, pps, dev)
        for j in range(pps):
            for b in torch.randperm(B).tolist():
                pool.allocate(b, (j + 1) * PAGE)
        cache = PagedMXKVCache(pool, Hkv, D, device=dev)
        table = pool.block_table
        pools = (cache.k_pages, cache.k_scale_pages, cache.v_pages,
                 cache.v_scale_pages)
        for pay, scl in (pools[:2], pools[2:]):
            x = torch.randn(pay.shape, device=dev) * 0.5
            for dst, t in zip((pay, scl), pack_mx(*quantize_mx(x, FMT), FMT)):
                dst.copy_(t)
        # the same values in bf16 pools, the same bytes in a dense cache
        bf = [dequantize_mx(*unpack_mx(pay, scl, FMT), dtype=torch.bfloat16)
              for pay, scl in (pools[:2], pools[2:])]
        rows = [t[table.long()].transpose(1, 2).reshape(
            B, Hkv, Smax, t.shape[-1]).contiguous() for t in pools]
        paged.append(lambda c=pools, t=table: ops.paged_chunk_attn_mx_step(
            q, k, v, *c, t, cos, sin, pos_t, Hq, Hkv, scale))
        bf16.append(lambda c=bf, t=table: ops.paged_chunk_attn_step(
            q, k, v, *c, t, cos, sin, pos_t, Hq, Hkv, scale))
        dense.append(lambda c=rows: ops.chunk_attn_mx_step(
            q, k, v, *c, cos, sin, pos_t, Hq, Hkv, scale, ragged=True))
        chained.append(lambda c=cache: chain(q, k, v, c, cos, sin, pos_t))
    a, b, c = paged[0](), dense[0](), chained[0]()
    torch.cuda.synchronize()
    diff = [(a.float() - x.float()).abs().max().item() for x in (b, c)]
    res = run_group({"chain": chained, "bf16": bf16, "dense": dense,
                     "paged": paged})
    return res, diff, pps


def report(title, pos_fn):
    print(title, flush=True)
    for T in args.tokens:
        runs, diffs = [], []
        for _ in range(args.runs):
            res, diff, pps = bench(T, pos_fn(T))
            runs.append(res)
            diffs.append(diff)
            torch.cuda.empty_cache()
        print(f"  T {T}, {pps} pages per sequence; paged differs from dense "
              f"by at most {max(d[0] for d in diffs):.2e}, from the chain by "
              f"{max(d[1] for d in diffs):.2e}")
        for n in ("chain", "bf16", "dense", "paged"):
            cells = "   ".join(f"{r[n][0]:8.1f} us ({r[n][1]:.1f}..{r[n][2]:.1f})"
                              for r in runs)
            print(f"    {n:6s} {cells}")
        for n in ("chain", "bf16", "dense"):
            cells = "   ".join(f"{r['paged'][0] / r[n][0]:.3f}" for r in runs)
            print(f"    paged / {n:6s} {cells}", flush=True)


torch.manual_seed(0)
report(f"all positions {args.pos}  B {B} Hq {Hq} Hkv {Hkv} ({args.sets} "
       f"cache sets, {args.runs} runs side by side)",
       lambda T: torch.full((B,), args.pos, device=dev))
lo, hi = args.spread
report(f"positions spread over [{lo}, {hi}]",
       lambda T: torch.linspace(lo, hi - T, B, device=dev).round().long())
T = max(args.tokens)
spread = torch.linspace(lo, hi - T, B).round().long()
row_bytes = Hkv * (D + D // 32) * 2        # K and V, payload + scales
pool_rows = int((-(-(spread + T) // PAGE) * PAGE).sum())
dense_rows = B * -(-(int(spread.max()) + T) // PAGE) * PAGE
print(f"  cache bytes per layer (T {T}): pool {pool_rows * row_bytes / 2**20:.1f}"
      f" MiB, dense {dense_rows * row_bytes / 2**20:.1f} MiB "
      f"({pool_rows / dense_rows:.3f})")
