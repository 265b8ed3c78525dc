"""Autoregressive generation loop (reference examples/inference runner +
utils/sampling): prefill through the flash kernel, decode through the
KV-cache path, sampling over vocab-parallel logits."""

from typing import Optional

import torch

from ..utils.sampling import Sampler
from .kv_cache import PAGE_ROWS, PagePool, build_kv_caches

PAGED_FORMATS = ("paged", "paged_mxfp8")   # one position per sequence


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
                     n_kv_local, model_dtype, who="prompt_lens",
                     prefill_chunk=None):
    """generate() for right-padded prompts of different lengths: one padded
    prefill, then decode with one position per sequence.

    ``kv_format="paged"`` or "paged_mxfp8": one PagePool of sum_b
    ceil((len_b + max_new_tokens) / 16) pages, every sequence allocated up front, so the
    table is static while the decode graph replays; the prefill drops the
    padding rows beyond a sequence's pages.  The cache of a sequence then
    ends on a page boundary: the model's RoPE table must cover
    16 * ceil((len_b + max_new_tokens) / 16) rows, up to 15 more than the
    tokens need.

    ``prefill_chunk=N`` (paged formats only): the prompt is prefilled in
    ceil(S / N) forwards of N tokens instead of one of S.  Chunk c runs at
    the per-sequence position min(c N, len_b) with
    chunk_lens = clamp(len_b - c N, 0, N) real tokens, so the padding of a
    short prompt costs nothing once the prompt has ended, and the first new
    token of sequence b comes from the logits row of its last real token, in
    the chunk that holds it.

    ``who``: the argument the caller chose this path with, for messages."""
    from .decode_graph import GraphDecoder

    cfg = model.config
    B, S = input_ids.shape
    dev = input_ids.device
    lens = check_prompt_lens(prompt_lens, input_ids)
    if max_new_tokens < 1:
        raise ValueError(f"{who}: max_new_tokens {max_new_tokens} must "
                         f"be at least 1")
    window = getattr(cfg, "sliding_window", None)
    if window is not None and window < S + max_new_tokens:
        raise NotImplementedError(
            f"{who} with a sliding window smaller than the sequence: "
            f"the rolling cache keeps one position for the whole batch")
    if not getattr(model, "supports_tensor_position", False):
        raise NotImplementedError(
            f"{who} needs a model that takes device-tensor positions")
    pool = None
    if kv_format in PAGED_FORMATS:
        rows = [n + max_new_tokens for n in lens.tolist()]
        pages = [-(-n // PAGE_ROWS) for n in rows]
        pool = PagePool(sum(pages), B, max(pages), dev)
        for b, n in enumerate(rows):
            pool.allocate(b, n)
    caches = build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                             S + max_new_tokens, cfg.head_dim,
                             dtype=model_dtype, device=dev,
                             kv_format=kv_format, page_pool=pool)
    if prefill_chunk is not None:
        next_tok = _prefill_chunked(model, input_ids, lens, caches,
                                    int(prefill_chunk), sampler)
    else:
        # padding sits to the right: no real token attends it, and the cache
        # rows it leaves at >= len_b are masked until a decode step
        # overwrites them
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


def _prefill_chunked(model, input_ids, lens, caches, N, sampler):
    """The prompt in ceil(S / N) forwards of N tokens at per-sequence device
    positions (_generate_ragged); returns the first new token of every
    sequence.  The last chunk is right-padded to N tokens: one static shape
    for every forward."""
    B, S = input_ids.shape
    dev = input_ids.device
    rows = torch.arange(B, device=dev)
    next_tok = None
    for c0 in range(0, S, N):
        ids = input_ids[:, c0:c0 + N]
        if ids.shape[1] < N:
            ids = torch.cat([ids, ids.new_zeros(B, N - ids.shape[1])], dim=1)
        n = (lens - c0).clamp(0, N)
        logits = model(ids, kv_caches=caches, pos_offset=lens.clamp(max=c0),
                       chunk_lens=n)
        # sampled for every sequence (one call, static shapes), kept for those
        # whose last real token lies in this chunk
        tok = sampler(logits[rows, (n - 1).clamp(min=0)])
        here = (lens > c0) & (lens <= c0 + N)
        next_tok = tok if next_tok is None else torch.where(here, tok,
                                                            next_tok)
    return next_tok


@torch.no_grad()
def generate(model, input_ids: torch.Tensor, max_new_tokens: int = 32,
             sampler: Optional[Sampler] = None, eos_token_id: int = -1,
             use_cuda_graph: bool = True, kv_format=None, prompt_lens=None,
             pad_token_id: int = 0, prefill_chunk=None):
    """model: LlamaForCausalLM-compatible (vocab-parallel logits out).
    input_ids (B, S) on the model's device; returns (B, S+new).

    ``prompt_lens``: (B,) lengths, 1 <= len_b <= S, of prompts right-padded
    to S.  Row b is then generated from its own length: the result is always
    (B, S + max_new_tokens), row b holding its prompt, its new tokens from
    column len_b and ``pad_token_id`` elsewhere.

    On GPU the per-token decode step is captured in a hipGraph and
    replayed (launch-bound otherwise); pass ``use_cuda_graph=False`` for
    the eager loop.  ``kv_format="mxfp8"`` keeps the KV cache in MXFP8
    (inference.kv_cache.MXKVCache) instead of the model dtype;
    ``kv_format="paged"`` keeps it in a page pool sized for the sequences'
    own lengths (inference.kv_cache.PagedKVCache) and always returns the
    ``prompt_lens`` layout (without ``prompt_lens``, every length is S).
    ``kv_format="paged_mxfp8"`` is the paged cache with MXFP8 rows inside the
    pages (inference.kv_cache.PagedMXKVCache), sized and laid out the same;
    its one-token decode step is fused (ops.paged_attn_mx_step).
    ``prefill_chunk=N`` (with a paged ``kv_format`` only, N > 8) prefills the
    prompt in chunks of N tokens through the paged prefill kernel
    (ops.paged_prefill_attn_step), which bounds the activation memory of a
    long prompt; None is one prefill of the whole prompt.  On
    ``"paged_mxfp8"`` the chunks go through its MX form
    (ops.paged_prefill_attn_mx_step)."""
    from ..parallel import parallel_state as ps
    from .decode_graph import GraphDecoder

    sampler = sampler or Sampler(do_sample=False)
    cfg = model.config
    tp = ps.get_tensor_model_parallel_size()
    B, S = input_ids.shape
    kv_mult = max(1, tp // cfg.num_key_value_heads)
    n_kv_local = cfg.num_key_value_heads * kv_mult // tp
    model_dtype = next(model.parameters()).dtype
    if prefill_chunk is not None:
        if kv_format not in PAGED_FORMATS:
            raise ValueError(f"prefill_chunk needs kv_format='paged' or "
                             f"'paged_mxfp8', got {kv_format!r}")
        if int(prefill_chunk) <= 8:
            raise ValueError(f"prefill_chunk {prefill_chunk} must exceed 8: "
                             f"shorter chunks are decode steps")
    if prompt_lens is not None or kv_format in PAGED_FORMATS:
        who = "prompt_lens"
        if prompt_lens is None:   # a paged cache has one position per sequence
            prompt_lens, who = [S] * B, f"kv_format={kv_format!r}"
        return _generate_ragged(model, input_ids, prompt_lens,
                                max_new_tokens, sampler, eos_token_id,
                                use_cuda_graph, kv_format, pad_token_id,
                                n_kv_local, model_dtype, who, prefill_chunk)
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
