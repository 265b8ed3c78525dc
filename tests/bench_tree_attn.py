"""Tree-masked decode attention microbench: ops.tree_attn_step (T tree nodes
verified in one call) against the eager tree chain it replaces
(LlamaAttention._tree_step with the kernel switched off) and against
ops.chunk_attn_step at the same T <= 8, which does the same work without the
tree mask; and ops.tree_kv_commit against the torch index-copy of
KVCache.commit_path.  B 32, D 128; Hq 32 / Hkv 8 with T 8 and 16, and
Hq 32 / Hkv 4 (rep 8) with T 8; position 1024 for the batch, and positions
spread evenly over [64, 1024] per sequence.

tree, chunk and commit are captured ``--iters`` times into one hipGraph each
over enough cache sets to exceed the Infinity Cache and replayed between two
device events; the eager chain allocates and is timed eagerly over the same
sets.  Medians of ``--rounds`` rounds.  Run it twice and take the medians of
the two runs.

Usage (GPU box):  timeout 600 python tests/bench_tree_attn.py
"""

import argparse
import os
import statistics
import sys
import types

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--pos", type=int, default=1024)
ap.add_argument("--batch", type=int, default=32)
ap.add_argument("--iters", type=int, default=16)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--cold-bytes", type=int, default=640 << 20)
args = ap.parse_args()

import torch  # noqa: E402

from neuronx_distributed_amd import ops  # noqa: E402
from neuronx_distributed_amd.inference.kv_cache import KVCache  # noqa: E402
from neuronx_distributed_amd.models.llama import LlamaAttention  # noqa: E402
from neuronx_distributed_amd.utils.medusa_utils import (  # noqa: E402
    generate_medusa_buffers, medusa_tree_topology)

assert torch.cuda.is_available(), "bench_tree_attn needs a GPU"
assert ops.tree_attn_available() and ops.chunk_attn_available(), \
    "build neuronx_distributed_amd.ops first"

dev = "cuda"
D = 128
B = args.batch
scale = D ** -0.5
TREES = {
    8: [[0], [1], [0, 0], [0, 1], [1, 0], [0, 0, 0], [1, 0, 0]],
    16: [[0], [1], [2], [0, 0], [0, 1], [1, 0], [1, 1], [2, 0], [0, 0, 0],
         [0, 0, 1], [0, 1, 0], [1, 0, 0], [0, 0, 0, 0], [0, 0, 0, 1],
         [1, 0, 0, 0]],
}


def timed(fn, n=1):
    t0, t1 = torch.cuda.Event(True), torch.cuda.Event(True)
    t0.record()
    for _ in range(n):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / n      # us


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


def bench(Hq, Hkv, T, spread):
    pos = args.pos
    Smax = pos + T
    buf = generate_medusa_buffers(TREES[T], device=dev)
    tree = medusa_tree_topology(buf["medusa_attn_mask"], device=dev)
    path = buf["retrieve_indices"][-1:].to(torch.int32).expand(B, -1) \
        .contiguous()
    torch.manual_seed(0)
    cos, sin = ops.precompute_rope_freqs(Smax, D, device=dev)
    rnd = lambda *s: torch.randn(*s, dtype=torch.bfloat16,  # noqa: E731
                                 device=dev) * 0.5
    q3, k3, v3 = rnd(B, T, Hq * D), rnd(B, T, Hkv * D), rnd(B, T, Hkv * D)
    if spread:
        pos_t = torch.linspace(64, pos, B, device=dev).long()
    else:
        pos_t = torch.tensor([pos], dtype=torch.int64, device=dev)
    n = max(1, min(args.iters,
                   -(-args.cold_bytes // (B * Hkv * Smax * 4 * D))))
    sets = []
    for _ in range(n):
        c = KVCache(B, Hkv, Smax, D, torch.bfloat16, dev)
        c.k.copy_(rnd(B, Hkv, Smax, D))
        c.v.copy_(rnd(B, Hkv, Smax, D))
        sets.append(c)
    me = types.SimpleNamespace(num_heads_local=Hq, num_kv_local=Hkv,
                               head_dim=D, sliding_window=None,
                               o_proj=lambda x: x)
    q4, k4, v4 = (q3.view(B, T, Hq, D), k3.view(B, T, Hkv, D),
                  v3.view(B, T, Hkv, D))
    real_avail = ops.tree_attn_available

    def eager(c):
        ops.tree_attn_available = lambda: False
        try:
            LlamaAttention._tree_step(me, q4, k4, v4, cos, sin, pos_t, c,
                                      False, tree)
        finally:
            ops.tree_attn_available = real_avail

    def eager_commit(c):
        ops.tree_attn_available = lambda: False
        try:
            c.commit_path(pos_t, path)
        finally:
            ops.tree_attn_available = real_avail

    graphs = {
        "tree": capture([lambda c=c: ops.tree_attn_step(
            q3, k3, v3, c.k, c.v, cos, sin, pos_t, *tree, Hq, Hkv, scale,
            ragged=spread) for c in sets]),
        "commit": capture([lambda c=c: ops.tree_kv_commit(
            c.k, c.v, pos_t, path, ragged=spread) for c in sets]),
    }
    if T <= 8:
        graphs["chunk"] = capture([lambda c=c: ops.chunk_attn_step(
            q3, k3, v3, c.k, c.v, cos, sin, pos_t, Hq, Hkv, scale,
            ragged=spread) for c in sets])
    times = {a: [] for a in (*graphs, "eager", "index")}
    eager(sets[0])
    eager_commit(sets[0])
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, g in graphs.items():
            times[name].append(timed(g.replay) / args.iters)
        for name, fn in (("eager", eager), ("index", eager_commit)):
            us = sum(timed(lambda: fn(sets[i % n]))
                     for i in range(args.iters))
            times[name].append(us / args.iters)
    med = {a: statistics.median(v) for a, v in times.items()}
    print(f"Hq {Hq} Hkv {Hkv} T {T} B {B} pos "
          f"{'64..' if spread else ''}{pos}  ({n} cache sets)")
    for a in times:
        print(f"    {a:6s} {med[a]:9.1f} us  ({min(times[a]):.1f}.."
              f"{max(times[a]):.1f})")
    line = f"    eager / tree {med['eager'] / med['tree']:.2f}x"
    if "chunk" in med:
        line += f"   tree / chunk {med['tree'] / med['chunk']:.3f}x"
    print(line + f"   index / commit {med['index'] / med['commit']:.2f}x",
          flush=True)


for spread in (False, True):
    for Hq, Hkv, T in ((32, 8, 8), (32, 8, 16), (32, 4, 8)):
        bench(Hq, Hkv, T, spread)
        torch.cuda.empty_cache()
