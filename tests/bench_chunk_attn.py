"""Multi-token decode attention microbench: the fused chunk step
(ops.chunk_attn_step / ops.chunk_attn_mx_step, T new tokens in one call)
against what it replaces, at the llama3-8b verify shape (B 32, Hq 32, Hkv 8,
D 128, T 5) for the bf16 and the MXFP8 cache.

Per position and format, us per call:

  chunk   the fused chunk step
  rect    the int-position path: cache.update(k, v, pos) + flash_attn_func
          with Sq != Sk ("rectangular attention" over the prefix; RoPE not
          included, which favours it)
  seq     T single-token fused decode steps in sequence
  floor   bytes of K + V rows [0, pos) read once / the copy bandwidth
          measured in the same run (a large device-to-device copy, read +
          written bytes over time)

chunk and seq are captured ``--iters`` times into one hipGraph each and
replayed between two device events; call i uses cache set i % copies, enough
sets to exceed the Infinity Cache (``--cold-bytes``).  rect allocates by
position and is timed eagerly between events over the same sets.  The graphs
are replayed in turn ``--rounds`` times; medians are reported.

One process, all positions.  Usage (GPU box):
    timeout 600 python tests/bench_chunk_attn.py [--pos 1024 4096]
"""

import argparse
import os
import statistics
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pos", type=int, nargs="+", default=[1024, 4096])
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--hq", type=int, default=32)
ap.add_argument("--hkv", type=int, default=8)
ap.add_argument("--tokens", type=int, default=5)
ap.add_argument("--iters", type=int, default=16)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--cold-bytes", type=int, default=640 << 20)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402
from neuronx_distributed_amd.inference.kv_cache import (  # noqa: E402
    KVCache, MXKVCache)
from neuronx_distributed_amd.kernels.flash_attn import (  # noqa: E402
    flash_attn_func)

assert torch.cuda.is_available(), "bench_chunk_attn needs a GPU"
assert ops.chunk_attn_available() and ops.chunk_attn_mx_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
D = 128
B, Hq, Hkv, T = args.batch, args.hq, args.hkv, args.tokens
scale = D ** -0.5
ROW = {"bf16": 2 * D * 2, "mxfp8": 2 * (D + D // 32)}  # K + V bytes per row


def timed(fn, n=1):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / n      # us


def copy_bandwidth():
    src = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    dst.copy_(src)
    us = statistics.median(timed(lambda: dst.copy_(src)) for _ in range(7))
    return 2 * src.numel() / us / 1e3         # GB/s, read + written


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


def make_cache(fmt, Smax, k, v):
    cls = KVCache if fmt == "bf16" else MXKVCache
    c = cls(B, Hkv, Smax, D, torch.bfloat16, dev)
    c.update(k, v, 0)
    return c


def buffers(fmt, c):
    return (c.k, c.v) if fmt == "bf16" else (c.k, c.k_scale, c.v, c.v_scale)


def bench(fmt, pos, gbps):
    Smax = pos + 8
    torch.manual_seed(0)
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    q3 = torch.randn(B, T, Hq * D, dtype=torch.bfloat16, device=dev) * 0.5
    k3 = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    v3 = torch.randn(B, T, Hkv * D, dtype=torch.bfloat16, device=dev) * 0.5
    pos_t = torch.tensor([pos], dtype=torch.int64, device=dev)
    pos_ts = [torch.tensor([pos + t], dtype=torch.int64, device=dev)
              for t in range(T)]
    n = max(1, min(args.iters, -(-args.cold_bytes // (B * Hkv * Smax
                                                      * ROW[fmt]))))
    sets = []
    for _ in range(n):
        k = torch.randn(B, Hkv, pos, D, dtype=torch.bfloat16, device=dev) * 0.5
        v = torch.randn(B, Hkv, pos, D, dtype=torch.bfloat16, device=dev) * 0.5
        sets.append(make_cache(fmt, Smax, k, v))
        del k, v
    step = ops.chunk_attn_step if fmt == "bf16" else ops.chunk_attn_mx_step
    one = ops.decode_attn_step if fmt == "bf16" else ops.decode_attn_mx_step

    def seq(c):
        for t in range(T):
            one(q3[:, t], k3[:, t], v3[:, t], *buffers(fmt, c), cos, sin,
                pos_ts[t], Hq, Hkv, scale)

    qh = q3.view(B, T, Hq, D).transpose(1, 2)
    kh = k3.view(B, T, Hkv, D).transpose(1, 2)
    vh = v3.view(B, T, Hkv, D).transpose(1, 2)

    def rect(c):
        K, V = c.update(kh, vh, pos)
        return flash_attn_func(qh, K, V, causal=True)

    graphs = {
        "chunk": capture([lambda c=c: step(q3, k3, v3, *buffers(fmt, c), cos,
                                           sin, pos_t, Hq, Hkv, scale)
                          for c in sets]),
        "seq": capture([lambda c=c: seq(c) for c in sets]),
    }
    times = {"chunk": [], "seq": [], "rect": []}
    rect(sets[0])
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(timed(g.replay) / args.iters)
        us = 0.0
        for i in range(args.iters):
            us += timed(lambda: rect(sets[i % n]))
        times["rect"].append(us / args.iters)
    med = {a: statistics.median(v) for a, v in times.items()}
    nbytes = B * Hkv * pos * ROW[fmt]
    floor = nbytes / gbps / 1e3
    print(f"{fmt:6s} pos {pos:5d}  B {B} Hq {Hq} Hkv {Hkv} T {T}  "
          f"({n} cache sets, {nbytes / 1e6:.0f} MB of rows)")
    for a in ("chunk", "rect", "seq"):
        print(f"    {a:6s} {med[a]:9.1f} us  ({min(times[a]):.1f}.."
              f"{max(times[a]):.1f})")
    print(f"    floor  {floor:9.1f} us   rect / chunk {med['rect'] / med['chunk']:.2f}x"
          f"   seq / chunk {med['seq'] / med['chunk']:.2f}x   chunk / floor "
          f"{med['chunk'] / floor:.2f}x", flush=True)


gbps = copy_bandwidth()
print(f"copy bandwidth {gbps:.0f} GB/s (1 GiB device copy, read + written)",
      flush=True)
for pos in args.pos:
    for fmt in ("bf16", "mxfp8"):
        bench(fmt, pos, gbps)
        torch.cuda.empty_cache()
