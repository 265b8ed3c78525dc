"""Paged MXFP8 decode attention microbench: ops.paged_attn_mx_step over MXFP8
page pools behind a shuffled block table, at the llama3-8b decode shape
(B 32, Hq 32, Hkv 8, D 128), against

  (a) ops.paged_attn_step on bf16 pools that hold the dequantized values
      (almost twice the bytes),
  (b) ops.decode_attn_mx_step(ragged=True) on the dense MX cache that holds
      the same rows (built with other compiler flags, ops/build.py: the cost
      of the page walk alone is not isolated here),
  (c) the torch chain on PagedMXKVCache: update() + gather() + attention,

with all positions ``--pos`` (1024) and with positions spread over
``--spread`` (64..2048), and the pool bytes against the bf16 pools and the
dense MX cache.

The kernels are captured ``--iters`` times into one hipGraph each, call i on
cache set i % sets (enough sets to exceed the Infinity Cache), and the graphs
are replayed in turn ``--rounds`` times between device events; (c) runs
eagerly on one set, 3 calls per round.  Median and min..max of the rounds, us
per call.

One process.  Usage (GPU box):
    timeout 600 python tests/bench_paged_attn_mx.py
"""

import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
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
from neuronx_distributed_amd.inference.kv_cache import (  # noqa: E402
    PagedMXKVCache, PagePool)
from neuronx_distributed_amd.quantization.microscaling import (  # noqa: E402
    dequantize_mx, unpack_mx)

assert torch.cuda.is_available(), "bench_paged_attn_mx needs a GPU"
assert ops.paged_attn_mx_available() and ops.paged_attn_available() \
    and ops.ragged_attn_available(), "build neuronx_distributed_amd.ops first"

dev = "cuda"
D, PAGE = 128, 16
B, Hq, Hkv = args.batch, args.hq, args.hkv
rep, scale = Hq // Hkv, D ** -0.5
C_CALLS = 3


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


def chain(cache, q, k, v, cos, sin, pos_t):
    """LlamaAttention._cached_step's torch chain on a PagedMXKVCache."""
    c, s = cos[pos_t].view(B, 1, 1, D // 2), sin[pos_t].view(B, 1, 1, D // 2)

    def rope(x):
        x0, x1 = x[..., :D // 2].float(), x[..., D // 2:].float()
        return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s], -1).bfloat16()

    qg = rope(q.view(B, Hkv, rep, D))
    K, V = cache.update(rope(k.view(B, Hkv, 1, D)), v.view(B, Hkv, 1, D),
                        pos_t)
    sc = (qg @ K.transpose(-1, -2)).float() * scale
    idx = torch.arange(K.shape[2], device=dev).view(1, 1, 1, -1)
    sc = sc.masked_fill(idx > pos_t.view(B, 1, 1, 1), float("-inf"))
    return (torch.softmax(sc, -1).bfloat16() @ V).reshape(B, Hq * D)


def bench(title, pos_t):
    pps = -(-(int(pos_t.max()) + 1) // PAGE)
    Smax, n_pages = pps * PAGE, B * pps
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    q, k, v = (torch.randn(B, n * D, dtype=torch.bfloat16, device=dev) * 0.5
               for n in (Hq, Hkv, Hkv))
    mx, bf, dense = [], [], []
    for i in range(args.sets):
        table = torch.randperm(n_pages, device=dev).int().view(B, pps)
        pools = tuple(t for _ in range(2) for t in ops.mx_quantize_rows(
            torch.randn(n_pages, Hkv, PAGE, D, dtype=torch.bfloat16,
                        device=dev) * 0.5))
        bf_pools = tuple(dequantize_mx(*unpack_mx(p, s, "fp8_e4m3"))
                         for p, s in (pools[:2], pools[2:]))
        rows = tuple(t[table.long()].transpose(1, 2)
                     .reshape(B, Hkv, Smax, t.shape[-1]).contiguous()
                     for t in pools)
        mx.append(lambda c=pools, t=table: ops.paged_attn_mx_step(
            q, k, v, *c, t, cos, sin, pos_t, Hq, Hkv, scale))
        bf.append(lambda c=bf_pools, t=table: ops.paged_attn_step(
            q, k, v, *c, t, cos, sin, pos_t, Hq, Hkv, scale))
        dense.append(lambda c=rows: ops.decode_attn_mx_step(
            q, k, v, *c, cos, sin, pos_t, Hq, Hkv, scale, ragged=True))
        if i == 0:
            pool = PagePool(n_pages, B, pps, dev)
            pool.block_table.copy_(table)
            cache = PagedMXKVCache(pool, Hkv, D, torch.bfloat16, dev)
            for dst, src in zip((cache.k_pages, cache.k_scale_pages,
                                 cache.v_pages, cache.v_scale_pages), pools):
                dst.copy_(src)
    o = [f[0]().float() for f in (mx, bf, dense)]
    o.append(chain(cache, q, k, v, cos, sin, pos_t).float())
    torch.cuda.synchronize()
    print(f"{title}  B {B} Hq {Hq} Hkv {Hkv}, {pps} pages per sequence "
          f"({args.sets} cache sets); paged mx differs from (a) by "
          f"{(o[0] - o[1]).abs().max().item():.2e}, from (b) by "
          f"{(o[0] - o[2]).abs().max().item():.2e}, from (c) by "
          f"{(o[0] - o[3]).abs().max().item():.2e}", flush=True)
    graphs = {"paged mx": capture(mx), "(a) paged bf16": capture(bf),
              "(b) dense mx": capture(dense)}
    times = {n: [] for n in list(graphs) + ["(c) torch chain"]}
    for _ in range(args.rounds):
        for n, g in graphs.items():
            times[n].append(timed(g.replay) / args.iters)
        times["(c) torch chain"].append(timed(lambda: [
            chain(cache, q, k, v, cos, sin, pos_t)
            for _ in range(C_CALLS)]) / C_CALLS)
    med = {}
    for n, t in times.items():
        med[n] = statistics.median(t)
        print(f"    {n:18s} {med[n]:9.1f} us  ({min(t):.1f}..{max(t):.1f})")
    for n in list(times)[1:]:
        print(f"    paged mx / {n} {med['paged mx'] / med[n]:.3f}", flush=True)
    return Smax


torch.manual_seed(0)
bench(f"all positions {args.pos}", torch.full((B,), args.pos, device=dev))
torch.cuda.empty_cache()
lo, hi = args.spread
spread = torch.linspace(lo, hi, B, device=dev).round().long()
Smax = bench(f"positions spread over [{lo}, {hi}]", spread)
pool_rows = int((torch.div(spread + PAGE, PAGE, rounding_mode="floor")
                 * PAGE).sum())
mx_row, bf_row = Hkv * (D + D // 32) * 2, Hkv * D * 2 * 2     # K and V
print(f"  cache bytes per layer: mx pool {pool_rows * mx_row / 2**20:.1f} "
      f"MiB, bf16 pool {pool_rows * bf_row / 2**20:.1f} MiB "
      f"({mx_row / bf_row:.3f}), dense mx cache "
      f"{B * Smax * mx_row / 2**20:.1f} MiB "
      f"({pool_rows / (B * Smax):.3f})")
