"""Per-sequence-position decode attention microbench: the ``ragged=True``
entries of the four fused decode kernels (ops.decode_attn_step,
decode_attn_mx_step, chunk_attn_step, chunk_attn_mx_step) against their
uniform entries, at the llama3-8b shape (B 32, Hq 32, Hkv 8, D 128,
Smax 4096, T 5 for the chunk kernels).

  indirection  all positions 1024: the uniform entry, the ragged entry and,
               with ``--parent-lib``, the uniform entry of a libnxd_ops.so
               built from the parent commit.  Expected: all equal.
  spread       positions evenly spread over [64, 2048], ragged, against the
               uniform entry at 2048 (every row padded to the longest) and at
               the mean position (the same bytes, equal splits).

Every variant is captured ``--iters`` times into one hipGraph, call i on
cache set i % sets (enough sets to exceed the Infinity Cache), and the graphs
of a group are replayed in turn ``--rounds`` times between device events;
median and min..max of the rounds are reported, us per call.

One process.  Usage (GPU box):
    timeout 600 python tests/bench_ragged_attn.py [--parent-lib PATH]
"""

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--smax", type=int, default=4096)
ap.add_argument("--tokens", type=int, default=5)
ap.add_argument("--pos", type=int, default=1024)
ap.add_argument("--spread", type=int, nargs=2, default=[64, 2048])
ap.add_argument("--sets", type=int, default=6)
ap.add_argument("--iters", type=int, default=24)
ap.add_argument("--rounds", type=int, default=9)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402
from neuronx_distributed_amd.inference.kv_cache import (  # noqa: E402
    KVCache, MXKVCache)

assert torch.cuda.is_available(), "bench_ragged_attn needs a GPU"
assert ops.ragged_attn_available(), "build neuronx_distributed_amd.ops first"
parent = ctypes.CDLL(args.parent_lib) if args.parent_lib else None

dev = "cuda"
D = 128
B, Hq, Hkv, T, Smax = args.batch, args.hq, args.hkv, args.tokens, args.smax
scale = D ** -0.5
KERNELS = (("decode_attn", "bf16", 1), ("decode_attn_mx", "mxfp8", 1),
           ("chunk_attn", "bf16", T), ("chunk_attn_mx", "mxfp8", T))


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


def make_sets(fmt):
    """Caches with every row written: any position finds real rows."""
    cls = KVCache if fmt == "bf16" else MXKVCache
    sets = []
    for _ in range(args.sets):
        c = cls(B, Hkv, Smax, D, torch.bfloat16, dev)
        for h in range(Hkv):     # head by head: a small transient
            k = torch.randn(B, 1, Smax, D, dtype=torch.bfloat16, device=dev)
            one = cls(B, 1, Smax, D, torch.bfloat16, dev)
            one.update(k * 0.5, k.flip(2) * 0.5, 0)
            for n in ("k", "v", "k_scale", "v_scale"):
                if hasattr(c, n):
                    getattr(c, n)[:, h:h + 1] = getattr(one, n)
        sets.append((c.k, c.v) if fmt == "bf16"
                    else (c.k, c.k_scale, c.v, c.v_scale))
    return sets


def run_group(title, variants):
    """variants: name -> list of per-set callables.  Returns name -> (median,
    min, max) us per call."""
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


def bench(name, fmt, t):
    torch.manual_seed(0)
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    shp = (B,) if t == 1 else (B, t)
    q = torch.randn(*shp, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
    k = torch.randn(*shp, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    v = torch.randn(*shp, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    sets = make_sets(fmt)
    step = getattr(ops, name + "_step")
    lo, hi = args.spread
    spread = torch.linspace(lo, hi, B, device=dev).round().long()
    mean = int(spread.float().mean().round())

    def one(p):
        return torch.tensor([p], dtype=torch.int64, device=dev)

    def uniform(p):
        pt = one(p)
        return [lambda c=c: step(q, k, v, *c, cos, sin, pt, Hq, Hkv, scale)
                for c in sets]

    def ragged(pt):
        return [lambda c=c: step(q, k, v, *c, cos, sin, pt, Hq, Hkv, scale,
                                 ragged=True) for c in sets]

    def parent_uniform(p):
        pt = one(p)
        _, st = ops._decode_attn_check(name, t > 1, q, k, v, cos, sin, pt, B,
                                       Hq, Hkv, Smax, q.device)
        fn = getattr(parent, name)
        return [lambda c=c: ops._decode_attn_launch(
            fn, t > 1, (q, k, v, *c, cos, sin, pt), B, t, Hq, Hkv, Smax,
            scale, st) for c in sets]

    print(f"{name}  B {B} Hq {Hq} Hkv {Hkv} T {t} Smax {Smax}  "
          f"({args.sets} cache sets)", flush=True)
    same = {"uniform": uniform(args.pos),
            "ragged": ragged(torch.full((B,), args.pos, device=dev))}
    if parent is not None:
        same = {"parent uniform": parent_uniform(args.pos), **same}
    r = run_group(f"all positions {args.pos}", same)
    if parent is not None:
        p_med, p_lo, p_hi = r["parent uniform"]
        bound = p_med + (p_hi - p_lo)
        for n in ("uniform", "ragged"):
            print(f"    {n} / parent {r[n][0] / p_med:.3f}  (bound: parent "
                  f"median + its spread = {bound:.1f} us: "
                  f"{'inside' if r[n][0] <= bound else 'OUTSIDE'})")
    r = run_group(f"positions spread over [{lo}, {hi}] (mean {mean})",
                  {"ragged spread": ragged(spread),
                   f"uniform at {hi}": uniform(hi),
                   f"uniform at {mean}": uniform(mean)})
    print(f"    ragged / uniform at {hi} (padded) "
          f"{r['ragged spread'][0] / r[f'uniform at {hi}'][0]:.3f}   "
          f"ragged / uniform at {mean} (ideal) "
          f"{r['ragged spread'][0] / r[f'uniform at {mean}'][0]:.3f}",
          flush=True)


for kern in KERNELS:
    bench(*kern)
    torch.cuda.empty_cache()
