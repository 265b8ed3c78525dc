"""Paged prefill attention over MXFP8 pages, microbench:
ops.paged_prefill_attn_mx_step at the shapes of bench_paged_prefill_attn.py
(chunks of 512 and 2048 new tokens per sequence over prefixes of 0, 4096 and
16384 rows, and one ragged case with n[b] from 1 to T; llama3-8b per GPU:
B 4, Hq 32, Hkv 8, D 128) over MXFP8 pools behind an interleaved block table,
against

  chain   what serves this call without the kernel: the torch chain of
          LlamaAttention._cached_step on PagedMXKVCache.gather() (a scatter of
          the quantized rows, a dequantized dense copy of K and V, batched
          GEMMs over the whole table, a (B, Hq, T, 16 * pages_per_seq) fp32
          score tensor), run through that method with the kernel reported
          unavailable;
  bf16    ops.paged_prefill_attn_step on bf16 pools that hold the dequantized
          values behind the same table: the cost of the dequantizing stage.

Every variant is warmed up, then timed ``--iters`` calls at a time between
device events, the variants in turn, ``--rounds`` times; medians (min..max)
in us per call, and TFLOP/s from the causal FLOP count of the shapes:
4 * Hq * D * sum_b sum_{t < n_b} (pos_b + t + 1).

One process.  Usage (GPU box):
    timeout 900 python tests/bench_paged_prefill_attn_mx.py
"""

import argparse
import os
import statistics
import sys
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=4)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--tokens", type=int, nargs="+", default=[512, 2048])
ap.add_argument("--prefix", type=int, nargs="+", default=[0, 4096, 16384])
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--chain-iters", type=int, default=2)
ap.add_argument("--no-chain", action="store_true")
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402
from neuronx_distributed_amd.inference.kv_cache import (  # noqa: E402
    PagedMXKVCache, PagePool)
from neuronx_distributed_amd.models.llama import LlamaAttention  # noqa: E402
from neuronx_distributed_amd.quantization.microscaling import (  # noqa: E402
    dequantize_mx, unpack_mx)

assert torch.cuda.is_available(), "bench_paged_prefill_attn_mx needs a GPU"
assert ops.paged_prefill_attn_mx_available() \
    and ops.paged_prefill_attn_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
D, PAGE = 128, 16
B, Hq, Hkv = args.batch, args.hq, args.hkv
scale = D ** -0.5
# LlamaAttention._cached_step without the projections around it
attn = types.SimpleNamespace(num_heads_local=Hq, num_kv_local=Hkv, head_dim=D,
                             sliding_window=None, o_proj=lambda x: x)


def timed(fn, iters):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(iters):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters      # us


def run_group(variants):
    """{name: (fn, iters)} -> {name: (median, min, max)} us, the variants in
    turn every round."""
    for fn, _ in variants.values():
        fn()
    torch.cuda.synchronize()
    times = {n: [] for n in variants}
    for _ in range(args.rounds):
        for n, (fn, iters) in variants.items():
            times[n].append(timed(fn, iters))
    return {n: (statistics.median(v), min(v), max(v))
            for n, v in times.items()}


def chain(q, k, v, cache, cos, sin, pos_t, lens):
    real = ops.paged_prefill_attn_mx_available
    ops.paged_prefill_attn_mx_available = lambda: False
    try:
        return LlamaAttention._cached_step(
            attn, q.view(B, -1, Hq, D), k.view(B, -1, Hkv, D),
            v.view(B, -1, Hkv, D), cos, sin, pos_t, cache, False, lens)
    finally:
        ops.paged_prefill_attn_mx_available = real


def bench(T, prefix, lens=None):
    pps = -(-(prefix + T) // PAGE)
    cos, sin = ops.precompute_rope_freqs(pps * PAGE, D, device=dev)
    q = torch.randn(B, T, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
    k = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    v = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    # page j of every sequence before page j + 1 of any, the sequences in a
    # new order each time: no two pages of a sequence are adjacent
    pool = PagePool(B * pps, B, pps, dev)
    for j in range(pps):
        for b in torch.randperm(B).tolist():
            pool.allocate(b, (j + 1) * PAGE)
    cache = PagedMXKVCache(pool, Hkv, D, device=dev)
    mx = (cache.k_pages, cache.k_scale_pages, cache.v_pages,
          cache.v_scale_pages)
    rows = lambda: torch.randn(B, Hkv, pps * PAGE, D,  # noqa: E731
                               dtype=torch.bfloat16, device=dev) * 0.5
    ops.paged_mx_kv_store(rows(), rows(), *mx, pool.block_table, 0)
    # bf16 pools of the dequantized values
    bf = [dequantize_mx(*unpack_mx(p, s, "fp8_e4m3"), dtype=torch.bfloat16)
          for p, s in (mx[:2], mx[2:])]
    pos_t = torch.full((B,), prefix, dtype=torch.int64, device=dev)
    ns = [T] * B if lens is None else lens.tolist()
    flops = 4 * Hq * D * sum(n * prefix + n * (n + 1) // 2 for n in ns)
    tail = (pool.block_table, cos, sin, pos_t, Hq, Hkv, scale, lens)
    variants = {"mx": (lambda: ops.paged_prefill_attn_mx_step(
        q, k, v, *mx, *tail), args.iters)}
    if not args.no_chain:
        variants["chain"] = (lambda: chain(q, k, v, cache, cos, sin, pos_t,
                                           lens), args.chain_iters)
    variants["bf16"] = (lambda: ops.paged_prefill_attn_step(
        q, k, v, *bf, *tail), args.iters)
    diff = ""
    if "chain" in variants:
        a, c = variants["mx"][0](), variants["chain"][0]()
        diff = f"; mx differs from the chain by at most " \
               f"{(a.float() - c.float()).abs().max().item():.2e}"
        del a, c
    res = run_group(variants)
    ragged = "" if lens is None else f" ragged n {min(ns)}..{max(ns)}"
    print(f"T {T} prefix {prefix}{ragged}: {flops / 1e12:.3f} TFLOP{diff}")
    for n, (med, lo, hi) in res.items():
        print(f"    {n:6s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  "
              f"{flops / med / 1e6:7.1f} TFLOP/s", flush=True)
    for n in res:
        if n != "mx":
            print(f"    mx / {n:6s} {res['mx'][0] / res[n][0]:.3f}",
                  flush=True)
    del cache, mx, bf
    torch.cuda.empty_cache()


torch.manual_seed(0)
print(f"B {B} Hq {Hq} Hkv {Hkv} D {D}, {args.rounds} rounds of {args.iters} "
      f"calls ({args.chain_iters} for the chain)", flush=True)
for T in args.tokens:
    for prefix in args.prefix:
        bench(T, prefix)
T = max(args.tokens)
bench(T, 4096, torch.linspace(1, T, B, device=dev).round().long())
