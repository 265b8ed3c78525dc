"""Paged prefill attention microbench: ops.paged_prefill_attn_step (chunks of
512 and 2048 new tokens per sequence over prefixes of 0, 4096 and 16384 rows,
and one ragged case with n[b] from 1 to T) over a page pool behind an
interleaved block table, at the llama3-8b shape per GPU (B 4, Hq 32, Hkv 8,
D 128), against

  chain   what serves this call without the kernel: the torch chain of
          LlamaAttention._cached_step on PagedKVCache.gather() (scatter of
          the new rows, a dense copy of K and V, batched GEMMs over the whole
          table, a (B, Hq, T, 16 * pages_per_seq) fp32 score tensor), run
          through that method with the kernel reported unavailable;
  flash   prefix 0 only: ops.flash_attn on dense tensors of the same length,
          the project's best case for this arithmetic (no RoPE, no table).

Every variant is warmed up, then timed ``--iters`` calls at a time between
device events, the variants in turn, ``--rounds`` times; medians (min..max)
in us per call, and TFLOP/s from the causal FLOP count of the shapes:
4 * Hq * D * sum_b sum_{t < n_b} (pos_b + t + 1).

One process.  Usage (GPU box):
    timeout 900 python tests/bench_paged_prefill_attn.py
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
    PagedKVCache, PagePool)
from neuronx_distributed_amd.models.llama import LlamaAttention  # noqa: E402

assert torch.cuda.is_available(), "bench_paged_prefill_attn needs a GPU"
assert ops.paged_prefill_attn_available() and ops.flash_attn_available(), \
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
    real = ops.paged_prefill_attn_available
    ops.paged_prefill_attn_available = lambda: False
    try:
        return LlamaAttention._cached_step(
            attn, q.view(B, -1, Hq, D), k.view(B, -1, Hkv, D),
            v.view(B, -1, Hkv, D), cos, sin, pos_t, cache, False, lens)
    finally:
        ops.paged_prefill_attn_available = real


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
    cache = PagedKVCache(pool, Hkv, D, device=dev)
    for t in (cache.k_pages, cache.v_pages):
        t.copy_(torch.randn_like(t) * 0.5)
    pos_t = torch.full((B,), prefix, dtype=torch.int64, device=dev)
    ns = [T] * B if lens is None else lens.tolist()
    flops = 4 * Hq * D * sum(n * prefix + n * (n + 1) // 2 for n in ns)
    variants = {"paged": (lambda: ops.paged_prefill_attn_step(
        q, k, v, cache.k_pages, cache.v_pages, pool.block_table, cos, sin,
        pos_t, Hq, Hkv, scale, lens), args.iters)}
    if not args.no_chain:
        variants["chain"] = (lambda: chain(q, k, v, cache, cos, sin, pos_t,
                                           lens), args.chain_iters)
    if prefix == 0 and lens is None:
        q4 = q.view(B, T, Hq, D).transpose(1, 2).contiguous()
        k4 = k.view(B, T, Hkv, D).transpose(1, 2).contiguous()
        v4 = v.view(B, T, Hkv, D).transpose(1, 2).contiguous()
        variants["flash"] = (lambda: ops.flash_attn(q4, k4, v4, causal=True),
                             args.iters)
    diff = ""
    if "chain" in variants:
        a, c = variants["paged"][0](), variants["chain"][0]()
        diff = f"; paged differs from the chain by at most " \
               f"{(a.float() - c.float()).abs().max().item():.2e}"
        del a, c
    res = run_group(variants)
    ragged = "" if lens is None else f" ragged n {min(ns)}..{max(ns)}"
    print(f"T {T} prefix {prefix}{ragged}: {flops / 1e12:.3f} TFLOP{diff}")
    for n, (med, lo, hi) in res.items():
        print(f"    {n:6s} {med:10.1f} us ({lo:.1f}..{hi:.1f})  "
              f"{flops / med / 1e6:7.1f} TFLOP/s", flush=True)
    for n in res:
        if n != "paged":
            print(f"    paged / {n:6s} {res['paged'][0] / res[n][0]:.3f}",
                  flush=True)
    torch.cuda.empty_cache()


torch.manual_seed(0)
print(f"B {B} Hq {Hq} Hkv {Hkv} D {D}, {args.rounds} rounds of {args.iters} "
      f"calls ({args.chain_iters} for the chain)", flush=True)
for T in args.tokens:
    for prefix in args.prefix:
        bench(T, prefix)
T = max(args.tokens)
bench(T, 4096, torch.linspace(1, T, B, device=dev).round().long())
