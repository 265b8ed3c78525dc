#!/usr/bin/env python3
"""Inference benchmark — BASELINE.json config #5 shape: Llama-3 8B GQA
KV-cache decode, batch 32 (TP = num GPUs; synthetic prompts, random-init
weights).  Reports prefill throughput and steady-state decode tokens/s.

Not the driver's headline bench (that is bench.py); run manually:
    python bench_infer.py [--model llama3-8b] [--batch 32] [--new 64]
N GPUs: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
    --master-addr 127.0.0.1 bench_infer.py
"""

import argparse
import json
import os
import sys
import time

import torch
import torch.distributed as dist


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--model", default="llama3-8b")
    p.add_argument("--batch", type=int, default=32)
    p.add_argument("--prompt", type=int, default=1024)
    p.add_argument("--new", type=int, default=64)
    p.add_argument("--quantize", default=None, choices=[None, "fp8"],
                   help="W8A8 fp8-quantize the Column/RowParallel linears "
                        "(gate_up/down/o/lm_head) before serving: halves "
                        "their weight reads on the memory-bound decode")
    p.add_argument("--block", type=int, default=1,
                   help="decode steps captured per hipGraph (greedy "
                        "feedback inside the graph); measured ~4%% slower "
                        "than per-step replay at b32 on MI355X, kept for "
                        "multi-token stepping API coverage")
    p.add_argument("--kv-format", default="bf16", choices=["bf16", "mxfp8"],
                   help="KV-cache storage: the model dtype, or MXFP8 (e4m3 "
                        "+ e8m0 block scales, 0.516 of the bytes) read by "
                        "the fused MX decode-attention kernel")
    args = p.parse_args()
    kv_format = None if args.kv_format == "bf16" else args.kv_format

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29779")
    os.environ.setdefault("NXDA_FAST_INIT", "1")

    on_gpu = torch.cuda.is_available()
    if on_gpu:
        torch.cuda.set_device(local_rank)
        try:
            tun = os.environ.get(
                "NXDA_TUNABLEOP_FILE",
                os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "profiles", "tunableop_gfx950.csv"))
            if os.environ.get("NXDA_TUNE", "0") == "1":
                # tuning run: search hipBLASLt algos for this run's GEMM
                # shapes, write the selections (GraphDecoder detects tuning
                # mode and decodes eagerly so every shape gets tuned)
                torch.cuda.tunable.set_filename(
                    os.environ.get("NXDA_TUNE_OUT", "tunableop_out.csv"),
                    insert_device_ordinal=False)
                torch.cuda.tunable.tuning_enable(True)
                torch.cuda.tunable.enable(True)
            elif os.path.exists(tun) and \
                    os.environ.get("NXDA_TUNABLEOP", "1") == "1":
                torch.cuda.tunable.set_filename(tun,
                                                insert_device_ordinal=False)
                torch.cuda.tunable.tuning_enable(False)
                torch.cuda.tunable.enable(True)
        except Exception:
            pass
    dist.init_process_group("nccl" if on_gpu else "gloo", rank=rank,
                            world_size=world)

    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.models import get_config, LlamaForCausalLM
    from neuronx_distributed_amd.inference.generation import generate

    ps.initialize_model_parallel(tensor_model_parallel_size=world)
    cfg = get_config(args.model,
                     max_position_embeddings=args.prompt + args.new + 64)
    device = torch.device("cuda", local_rank) if on_gpu else "cpu"
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    torch.manual_seed(0)
    with torch.device(device):
        model = LlamaForCausalLM(cfg)
    torch.set_default_dtype(prev)
    model.eval()

    if args.quantize == "fp8":
        from neuronx_distributed_amd.quantization import quantize
        from neuronx_distributed_amd.quantization.quantization_config import (
            QuantizationConfig, QuantizedDtype)

        quantize.convert(model, QuantizationConfig(
            quantized_dtype=QuantizedDtype.F8E4M3,
            quantize_activation=True))

    from neuronx_distributed_amd.inference.decode_graph import GraphDecoder
    from neuronx_distributed_amd.inference.kv_cache import build_kv_caches
    from neuronx_distributed_amd.utils.sampling import Sampler

    x = torch.randint(0, cfg.vocab_size, (args.batch, args.prompt),
                      device=device)
    # warmup (library init, graph pool)
    generate(model, x[:, : min(128, args.prompt)], max_new_tokens=4)
    if on_gpu:
        torch.cuda.synchronize()
    dist.barrier()

    tp = world
    kv_mult = max(1, tp // cfg.num_key_value_heads)
    n_kv_local = cfg.num_key_value_heads * kv_mult // tp
    caches = build_kv_caches(cfg.num_hidden_layers, args.batch, n_kv_local,
                             args.prompt + args.new, cfg.head_dim,
                             device=device, kv_format=kv_format)
    sampler = Sampler(do_sample=False)

    t0 = time.perf_counter()
    with torch.no_grad():
        logits = model(x, kv_caches=caches, pos_offset=0)
    if on_gpu:
        torch.cuda.synchronize()
    prefill_s = time.perf_counter() - t0

    next_tok = sampler(logits[:, -1, :])
    blk = max(1, args.block) if on_gpu else 1
    dec = GraphDecoder(model, caches, start_pos=args.prompt,
                       batch=args.batch, device=x.device,
                       steps_per_capture=blk) if on_gpu else None
    if dec is not None:
        dec.capture_block()  # untimed (one-off per shape bucket)
        # one settle replay, then rewind the position for the timed region
        if blk > 1:
            toks = dec.step_block(next_tok)
            dec.pos_t -= blk
        else:
            dec.step(next_tok)

    t0 = time.perf_counter()
    if blk > 1:
        n_calls = max(1, (args.new - 1) // blk)
        for _ in range(n_calls):
            toks = dec.step_block(next_tok)
            next_tok = toks[:, -1]
        steps = n_calls * blk
    else:
        steps = max(1, args.new - 1)
        for _ in range(steps):
            logits = dec.step(next_tok) if dec is not None else None
            next_tok = sampler(logits[:, -1, :])
    if on_gpu:
        torch.cuda.synchronize()
    decode_s = time.perf_counter() - t0

    if rank == 0:
        print(json.dumps({
            "metric": "decode tokens/s, GQA KV-cache generation",
            "model": args.model, "n_gpus": world, "batch": args.batch,
            "prompt_len": args.prompt, "new_tokens": args.new,
            "prefill_s": round(prefill_s, 4),
            "prefill_tokens_per_s": round(args.batch * args.prompt /
                                          prefill_s, 1),
            "decode_ms_per_step": round(decode_s / steps * 1000, 3),
            "decode_tokens_per_s": round(args.batch * steps / decode_s, 1),
            "dtype": "bf16" if not args.quantize else "bf16+w8a8-fp8", "data": "synthetic",
            **({"kv_format": kv_format} if kv_format else {}),
        }), flush=True)
        if on_gpu:
            print(f"kv_format={args.kv_format} peak_memory_gb="
                  f"{torch.cuda.max_memory_allocated() / 1e9:.2f}",
                  file=sys.stderr, flush=True)
    if on_gpu and os.environ.get("NXDA_TUNE", "0") == "1" and \
            hasattr(torch.cuda.tunable, "write_file"):
        torch.cuda.tunable.write_file()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
