"""Autoregressive generation loop (reference examples/inference runner +
utils/sampling): prefill through the flash kernel, decode through the
KV-cache path, sampling over vocab-parallel logits."""

from typing import Optional

import torch

from ..utils.sampling import Sampler
from .kv_cache import build_kv_caches


def check_prompt_lens(prompt_lens, input_ids: torch.Tensor) -> torch.Tensor:
    """``prompt_lens`` ((B,) ints, tensor or list) as a device int64 (B,)
    tensor; every length must lie in [1, S]."""
    B, S = input_ids.shape
    lens = torch.as_tensor(prompt_lens).reshape(-1).to(torch.long)
    if lens.numel() != B or int(lens.min()) < 1 or int(lens.max()) > S:
        raise ValueError(f"prompt_lens {lens.tolist()} must hold {B} lengths "
                         f"in [1, {S}]")
    return lens.to(input_ids.device)


def ragged_output(input_ids: torch.Tensor, lens: torch.Tensor,
                  new_tokens: torch.Tensor, width: int, pad_token_id: int):
    """(B, width): row b holds its prompt in [0, len_b), then its row of
    ``new_tokens`` (B, N) from column len_b, and ``pad_token_id`` elsewhere."""
    B, S = input_ids.shape
    out = input_ids.new_full((B, width), pad_token_id)
    cols = torch.arange(S, device=input_ids.device)
    out[:, :S] = torch.where(cols < lens.view(B, 1), input_ids, out[:, :S])
    idx = lens.view(B, 1) + torch.arange(new_tokens.shape[1],
                                         device=input_ids.device)
    return out.scatter_(1, idx, new_tokens)


def _generate_ragged(model, input_ids, prompt_lens, max_new_tokens, sampler,
                     eos_token_id, use_cuda_graph, kv_format, pad_token_id,
                     n_kv_local, model_dtype):
    """generate() for right-padded prompts of different lengths: one padded
    prefill, then decode with one position per sequence."""
    from .decode_graph import GraphDecoder

    cfg = model.config
    B, S = input_ids.shape
    dev = input_ids.device
    lens = check_prompt_lens(prompt_lens, input_ids)
    if max_new_tokens < 1:
        raise ValueError(f"prompt_lens: max_new_tokens {max_new_tokens} must "
                         f"be at least 1")
    window = getattr(cfg, "sliding_window", None)
    if window is not None and window < S + max_new_tokens:
        raise NotImplementedError(
            "prompt_lens with a sliding window smaller than the sequence: "
            "the rolling cache keeps one position for the whole batch")
    if not getattr(model, "supports_tensor_position", False):
        raise NotImplementedError(
            "prompt_lens needs a model that takes device-tensor positions")
    caches = build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                             S + max_new_tokens, cfg.head_dim,
                             dtype=model_dtype, device=dev,
                             kv_format=kv_format)
    # padding sits to the right: no real token attends it, and the cache rows
    # it leaves at >= len_b are masked until a decode step overwrites them
    logits = model(input_ids, kv_caches=caches, pos_offset=0)
    next_tok = sampler(logits[torch.arange(B, device=dev), lens - 1])
    new = [next_tok]
    if input_ids.is_cuda:
        dec = GraphDecoder(model, caches, start_pos=lens, batch=B, device=dev)
        if use_cuda_graph:
            dec.capture()
        step = dec.step
    else:
        pos = lens.clone()

        def step(tok):
            lg = model(tok.unsqueeze(1), kv_caches=caches, pos_offset=pos)
            pos.add_(1)
            return lg
    for _ in range(max_new_tokens - 1):
        next_tok = sampler(step(next_tok)[:, -1, :])
        new.append(next_tok)
        if eos_token_id >= 0 and bool((next_tok == eos_token_id).all()):
            break
    return ragged_output(input_ids, lens, torch.stack(new, dim=1),
                         S + max_new_tokens, pad_token_id)


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int = 32,
             sampler: Optional[Sampler] = None, eos_token_id: int = -1,
             use_cuda_graph: bool = True, kv_format=None, prompt_lens=None,
             pad_token_id: int = 0):
    """model: LlamaForCausalLM-compatible (vocab-parallel logits out).
    input_ids (B, S) on the model's device; returns (B, S+new).

    ``prompt_lens``: (B,) lengths, 1 <= len_b <= S, of prompts right-padded
    to S.  Row b is then generated from its own length: the result is always
    (B, S + max_new_tokens), row b holding its prompt, its new tokens from
    column len_b and ``pad_token_id`` elsewhere.

    On GPU the per-token decode step is captured in a hipGraph and
    replayed (launch-bound otherwise); pass ``use_cuda_graph=False`` for
    the eager loop.  ``kv_format="mxfp8"`` keeps the KV cache in MXFP8
    (inference.kv_cache.MXKVCache) instead of the model dtype."""
    from ..parallel import parallel_state as ps
    from .decode_graph import GraphDecoder

    sampler = sampler or Sampler(do_sample=False)
    cfg = model.config
    tp = ps.get_tensor_model_parallel_size()
    B, S = input_ids.shape
    kv_mult = max(1, tp // cfg.num_key_value_heads)
    n_kv_local = cfg.num_key_value_heads * kv_mult // tp
    model_dtype = next(model.parameters()).dtype
    if prompt_lens is not None:
        return _generate_ragged(model, input_ids, prompt_lens,
                                max_new_tokens, sampler, eos_token_id,
                                use_cuda_graph, kv_format, pad_token_id,
                                n_kv_local, model_dtype)
    caches = build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                             S + max_new_tokens, cfg.head_dim,
                             dtype=model_dtype, device=input_ids.device,
                             window=getattr(cfg, "sliding_window", None),
                             kv_format=kv_format)

    # prefill (eager, flash kernel)
    logits = model(input_ids, kv_caches=caches, pos_offset=0)
    next_tok = sampler(logits[:, -1, :])
    out = [input_ids, next_tok.unsqueeze(1)]

    if input_ids.is_cuda and getattr(model, "supports_tensor_position",
                                     False):
        dec = GraphDecoder(model, caches, start_pos=S, batch=B,
                           device=input_ids.device)
        if use_cuda_graph:
            dec.capture()
        for _ in range(max_new_tokens - 1):
            logits = dec.step(next_tok)
            next_tok = sampler(logits[:, -1, :])
            out.append(next_tok.unsqueeze(1))
            if eos_token_id >= 0 and bool((next_tok == eos_token_id).all()):
                break
        return torch.cat(out, dim=1)

    # eager decode: tensor positions when supported — the tensor-pos
    # decode step masks by cache position_index(), which RollingKVCache
    # (sliding-window models) requires; int positions assume ordered
    # cache rows
    tensor_pos = getattr(model, "supports_tensor_position", False)
    pos = S
    for _ in range(max_new_tokens - 1):
        step_in = next_tok.unsqueeze(1)
        po = torch.tensor([pos], device=input_ids.device) if tensor_pos \
            else pos
        logits = model(step_in, kv_caches=caches, pos_offset=po)
        next_tok = sampler(logits[:, -1, :])
        out.append(next_tok.unsqueeze(1))
        pos += 1
        if eos_token_id >= 0 and bool((next_tok == eos_token_id).all()):
            break
    return torch.cat(out, dim=1)
