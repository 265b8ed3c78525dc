#!/usr/bin/env python3
"""Speculative decoding demo: draft-and-verify (a small draft model) and
Medusa heads, both exactly matching target-only greedy decoding.

  python examples/inference/run_speculative.py            # CPU demo
  torchrun --nproc-per-node 1 examples/inference/run_speculative.py
"""

import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)),
                                "..", ".."))

import torch
import torch.distributed as dist


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="test-d128")
    p.add_argument("--draft-layers", type=int, default=1)
    p.add_argument("--batch", type=int, default=2)
    p.add_argument("--prompt-len", type=int, default=64)
    p.add_argument("--new-tokens", type=int, default=64)
    p.add_argument("--spec-len", type=int, default=4)
    p.add_argument("--fused-verify", action="store_true",
                   help="verify chunks through the fused multi-token decode "
                        "attention (device position) instead of rectangular "
                        "attention over the prefix")
    p.add_argument("--per-sequence", action="store_true",
                   help="accept per sequence (one device position per "
                        "sequence) instead of what the whole batch agrees on")
    p.add_argument("--draft-from-target", action="store_true",
                   help="copy the target's embeddings, first --draft-layers "
                        "layers, final norm and head into the draft: without "
                        "a trained pair, a draft that agrees with the target "
                        "often enough for acceptance rates to mean something")
    p.add_argument("--repeats", type=int, default=1,
                   help="time draft-verify this many times (after one "
                        "untimed run when > 1) and report the median and "
                        "the min..max")
    p.add_argument("--no-assert", action="store_true",
                   help="report how many rows differ from target-only greedy "
                        "decoding instead of stopping (in bf16 a near-tie "
                        "may flip a token between a chunk forward and a "
                        "one-token forward)")
    args = p.parse_args()

    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29791")
    os.environ.setdefault("NXDA_FAST_INIT", "1")
    on_gpu = torch.cuda.is_available()
    dist.init_process_group("nccl" if on_gpu else "gloo",
                            rank=int(os.environ.get("RANK", "0")),
                            world_size=int(os.environ.get("WORLD_SIZE", "1")))

    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.models import get_config, LlamaForCausalLM
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.inference.speculation import (
        medusa_generate, speculative_generate)
    from neuronx_distributed_amd.utils.medusa_utils import MedusaHead

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    device = torch.device("cuda") if on_gpu else torch.device("cpu")
    dtype = torch.bfloat16 if on_gpu else torch.float32
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    torch.manual_seed(0)
    cfg = get_config(args.model)
    with torch.device(device):
        target = LlamaForCausalLM(cfg).eval()
        draft = LlamaForCausalLM(
            get_config(args.model,
                       num_hidden_layers=args.draft_layers)).eval()
        heads = torch.nn.ModuleList(
            [MedusaHead(cfg.hidden_size, cfg.vocab_size)
             for _ in range(args.spec_len)])
    torch.set_default_dtype(prev)
    if args.draft_from_target:
        t_state = target.state_dict()
        draft.load_state_dict({k: t_state[k] for k in draft.state_dict()})

    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (args.batch, args.prompt_len),
                      device=device)

    t0 = time.perf_counter()
    ref = generate(target, x, max_new_tokens=args.new_tokens)
    t_ref = time.perf_counter() - t0

    def same(out, what):
        """Rows of ``out`` that differ from target-only decoding."""
        n_diff = int((out != ref).any(dim=1).sum())
        assert args.no_assert or n_diff == 0, f"{what} output diverged"
        return n_diff

    times = []
    for i in range(args.repeats + (args.repeats > 1)):
        t0 = time.perf_counter()
        out, rate = speculative_generate(target, draft, x,
                                         max_new_tokens=args.new_tokens,
                                         spec_len=args.spec_len,
                                         fused_verify=args.fused_verify,
                                         per_sequence=args.per_sequence)
        if on_gpu:  # the timing ends when the device is done
            torch.cuda.synchronize()
        if i > 0 or args.repeats == 1:
            times.append(time.perf_counter() - t0)
    t_spec = sorted(times)[len(times) // 2]
    diff = same(out, "speculative")

    t0 = time.perf_counter()
    out_m, rate_m = medusa_generate(target, heads, x,
                                    max_new_tokens=args.new_tokens,
                                    fused_verify=args.fused_verify)
    t_med = time.perf_counter() - t0
    diff_m = same(out_m, "medusa")

    n_tok = args.batch * args.new_tokens
    print(f"target-only: {t_ref:.3f}s | draft-verify: {t_spec:.3f}s "
          f"[{min(times):.3f}..{max(times):.3f}, {len(times)} runs] "
          f"(acceptance {rate:.3f}, {n_tok / t_spec:.0f} tokens/s"
          f"{', per sequence' if args.per_sequence else ''}) | "
          f"medusa: {t_med:.3f}s (acceptance {rate_m:.2f}) — "
          + ("outputs identical" if diff == diff_m == 0 else
             f"rows differing from target-only: draft-verify {diff}, "
             f"medusa {diff_m} of {args.batch}"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
