#!/usr/bin/env python3
"""Flagship training benchmark: Llama-2-7B bf16 pretraining step, TP=N,
seq 4096, ZeRO-1 AdamW — the BASELINE.json headline metric
(tokens/sec whole job).

Single GPU:     python bench.py --steps 8 --warmup 3
N GPUs (driver): python -m torch.distributed.run --nnodes=1 --nproc-per-node N
                 --master-addr 127.0.0.1 bench.py --gpus N --steps K --warmup W

--dump-outputs DIR writes the last timed step's loss and a fixed sample of
the updated weights as .npy files; inputs and initial weights are seeded, so
the same arguments give the same inputs in every run.  --full is reserved
for measurements beyond the headline figure.
"""

import argparse
import json
import os
import time

import torch
import torch.distributed as dist


def parse_args():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=8)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--model", type=str, default="llama2-7b")
    p.add_argument("--seq", type=int, default=4096)
    p.add_argument("--batch", type=int, default=0,
                   help="global batch per step (default: n_gpus)")
    p.add_argument("--tp", type=int, default=0, help="TP degree (default: world)")
    p.add_argument("--pp", type=int, default=1)
    p.add_argument("--sequence-parallel", action="store_true")
    p.add_argument("--no-sequence-parallel", action="store_true",
                   help="disable the TP>1 default of sequence parallelism")
    p.add_argument("--layers", type=int, default=0,
                   help="override layer count (debug only; overridden runs "
                        "are marked invalid in the output)")
    p.add_argument("--microbatch", type=int, default=8)
    p.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                   help="after the timed steps, write what the last timed "
                        "step produced (loss, a seeded sample of the updated "
                        "weights) as DIR/<name>.npy")
    p.add_argument("--full", action="store_true",
                   help="also run the measurements beyond the headline "
                        "figure (none at present: the plain run is the "
                        "whole benchmark)")
    return p.parse_args()


def dump_outputs(out_dir, loss, params, suffix="", per_param=4096):
    """Write the last timed step's results as float32 .npy files: the loss
    the step returned and the weights it left behind.  The weights are a
    fixed sample - the same ``per_param`` seeded positions of every
    parameter tensor in every run - so two builds compare element for
    element (a few MB for Llama-2-7B)."""
    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, f"loss{suffix}.npy"),
            loss.detach().float().cpu().numpy().reshape(1))
    gen = torch.Generator().manual_seed(2024)
    sample = []
    for p in params:
        flat = p.detach().reshape(-1)
        idx = torch.randint(0, flat.numel(), (min(per_param, flat.numel()),),
                            generator=gen)
        sample.append(flat[idx.to(flat.device)].float().cpu())
    np.save(os.path.join(out_dir, f"params_sample{suffix}.npy"),
            torch.cat(sample).numpy())


def main():
    args = parse_args()
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", str(args.gpus)))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29777")

    # synthetic random-init bench: shard-local fast init (skips the
    # TP-invariant master-weight protocol, irrelevant for synthetic data)
    os.environ.setdefault("NXDA_FAST_INIT", "1")

    on_gpu = torch.cuda.is_available()
    if on_gpu:
        torch.cuda.set_device(local_rank)
        try:
            # pre-tuned hipBLASLt/rocBLAS GEMM selections (profiles/, gfx950);
            # tuning itself stays off - unknown shapes use defaults
            tun = os.environ.get(
                "NXDA_TUNABLEOP_FILE",
                os.path.join(os.path.dirname(os.path.abspath(__file__)),
                             "profiles", "tunableop_gfx950.csv"))
            if os.environ.get("NXDA_TUNE", "0") == "1":
                # tuning run: search hipBLASLt algos for this run's GEMM
                # shapes and write the selections (NXDA_TUNE_OUT)
                torch.cuda.tunable.set_filename(
                    os.environ.get("NXDA_TUNE_OUT", "tunableop_out.csv"),
                    insert_device_ordinal=False)
                torch.cuda.tunable.tuning_enable(True)
                torch.cuda.tunable.enable(True)
            elif os.path.exists(tun) and \
                    os.environ.get("NXDA_TUNABLEOP", "1") == "1":
                torch.cuda.tunable.set_filename(tun, insert_device_ordinal=False)
                torch.cuda.tunable.tuning_enable(False)
                torch.cuda.tunable.enable(True)
        except Exception:
            pass
    backend = "nccl" if on_gpu else "gloo"
    if not dist.is_initialized():
        dist.init_process_group(backend, rank=rank, world_size=world)

    import neuronx_distributed_amd as nxd
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.models import get_config, LlamaForCausalLM
    from neuronx_distributed_amd.optimizer import NeuronZero1Optimizer

    tp = args.tp or (world // args.pp)
    ps.initialize_model_parallel(tensor_model_parallel_size=tp,
                                 pipeline_model_parallel_size=args.pp)
    nxd.parallel.model_parallel_manual_seed(1234)

    # SP is on by default for TP>1: same math (reduce-scatter+all-gather ==
    # all-reduce volume) but the norms/elementwise shard tp-ways.
    # (PP runs without SP: the FX pipeline partition traces the dense
    # activation layout.)
    use_sp = (args.sequence_parallel or tp > 1) and \
        not args.no_sequence_parallel and args.seq % max(tp, 1) == 0 and \
        args.pp == 1
    overrides = {"sequence_parallel_enabled": use_sp,
                 "max_position_embeddings": max(args.seq, 4096)}
    if args.layers:
        overrides["num_hidden_layers"] = args.layers
    cfg = get_config(args.model, **overrides)

    device = torch.device("cuda", local_rank) if on_gpu else torch.device("cpu")
    dtype = torch.bfloat16
    torch.manual_seed(1234)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    with torch.device(device):
        model = LlamaForCausalLM(cfg)
    torch.set_default_dtype(prev)
    model = model.to(device)

    # per-GPU batch 32 amortizes the fixed step costs (optimizer, norms):
    # measured 19.3k (b4) -> 20.5k (b16) -> 21.0k (b32) tokens/s on 1 GPU;
    # at N=8 this is global batch 256 = the BASELINE headline recipe's GBS
    B = args.batch or 32 * max(1, world)
    S = args.seq
    mbs = args.microbatch
    assert B % mbs == 0
    n_micro = B // mbs

    if args.pp > 1:
        # 1F1B pipeline over FX-partitioned stages (BASELINE config #3
        # shape, e.g. --tp 2 --pp 4 on 8 GPUs)
        from neuronx_distributed_amd.pipeline import NxDPPModel
        from neuronx_distributed_amd.models.llama import LlamaDecoderLayer

        model = NxDPPModel(model, transformer_layer_cls=LlamaDecoderLayer,
                           num_microbatches=n_micro,
                           input_names=["input_ids", "labels"])
        params = list(model.local_parameters())
    else:
        params = list(model.parameters())

    opt = NeuronZero1Optimizer(params, torch.optim.AdamW,
                               lr=1.5e-4, betas=(0.9, 0.95), weight_decay=0.1,
                               grad_clipping=True, max_norm=1.0)

    # FRESH synthetic batch every step (pre-generated outside the timed
    # region): no batch is ever repeated, so the loss reflects actual
    # optimization rather than memorizing one batch
    torch.manual_seed(4321)
    n_unique = args.warmup + args.steps
    if args.pp > 1:
        fulls = [torch.randint(0, cfg.vocab_size, (B, S), device=device)
                 for _ in range(n_unique)]
        counter = [0]

        def step():
            full = fulls[counter[0] % n_unique]
            counter[0] += 1
            opt.zero_grad()
            loss = model.run_train(input_ids=full, labels=full)
            opt.step()
            return loss
    else:
        data = [torch.randint(0, cfg.vocab_size, (mbs, S), device=device)
                for _ in range(n_micro * n_unique)]
        counter = [0]

        def step():
            base = (counter[0] % n_unique) * n_micro
            counter[0] += 1
            opt.zero_grad()
            for x in data[base:base + n_micro]:
                loss = model(x, labels=x)
                (loss / n_micro).backward()
            opt.step()
            return loss

    for _ in range(args.warmup):
        step()

    dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        loss = step()
    dist.barrier()
    if on_gpu:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0

    t = torch.tensor([elapsed], dtype=torch.float64, device=device)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    elapsed = t.item()

    if args.dump_outputs:
        # each rank holds its own shard of the weights
        dump_outputs(args.dump_outputs, loss, params,
                     suffix="" if world == 1 else f"_rank{rank}")

    tokens = B * S * args.steps
    ms_per_step = elapsed / args.steps * 1000.0
    value = tokens / elapsed
    if rank == 0:
        result = {
            "metric": "tokens/sec (whole node) Llama-2-7B training, "
                      "TP=num_gpus, seq=4096",
            "value": value,
            "unit": "tokens/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "bf16",
            "data": "synthetic",
            "config": {
                "model": args.model if not args.layers else
                         f"{args.model}-layers{args.layers}-INVALID",
                "global_batch": B,
                "seq_len": S,
                "parallelism": f"tp{tp}" + (f"_pp{args.pp}" if args.pp > 1 else "")
                               + ("_sp" if use_sp else ""),
                "zero1": True,
                "loss": float(loss.item()),
            },
        }
        print(json.dumps(result), flush=True)
    if on_gpu and os.environ.get("NXDA_TUNE", "0") == "1" and \
            hasattr(torch.cuda.tunable, "write_file"):
        torch.cuda.tunable.write_file()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
