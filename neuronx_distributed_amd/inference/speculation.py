"""Speculative decoding (draft-and-verify; reference: spec-draft groups in
parallel_state.py:1533 + the NxDI speculation flow).

Greedy acceptance: the draft proposes ``spec_len`` tokens autoregressively;
the target scores the whole chunk in ONE forward and the longest prefix
agreeing with the target's own greedy choices is accepted, plus one bonus
token from the target distribution.  With greedy sampling the output is
IDENTICAL to target-only decoding — only the number of target forwards
changes (that invariant is what the test asserts).

KV-cache bookkeeping: both caches may hold STALE rows beyond the accepted
position after a rejection; every attention path here masks by position
and rewrites rows in place, so stale rows are simply overwritten."""


import torch

from .kv_cache import build_kv_caches


def _greedy(logits: torch.Tensor) -> torch.Tensor:
    return logits.argmax(dim=-1)


def _chunk_pos(pos: int, n_tokens: int, fused: bool, device):
    """The position argument of a multi-token forward at ``pos``: a device
    int64 tensor, which routes attention to the fused chunk step
    (LlamaAttention._cached_step), when ``fused`` and the forward is one that
    step takes (2..8 tokens against a cache that holds rows); else the int."""
    if fused and pos > 0 and 2 <= n_tokens <= 8:
        return torch.tensor([pos], dtype=torch.long, device=device)
    return pos


def _speculative_per_sequence(target, draft, input_ids, max_new_tokens,
                              spec_len, prompt_lens, pad_token_id, caches):
    """speculative_generate(per_sequence=True): every sequence keeps its own
    device position, accepts its own longest agreeing prefix and goes
    inactive (position -1) once it has its ``max_new_tokens``."""
    from .generation import check_prompt_lens, ragged_output

    B, S = input_ids.shape
    dev = input_ids.device
    k = spec_len
    if max_new_tokens < 1:
        raise ValueError(f"per_sequence: max_new_tokens {max_new_tokens} must "
                         f"be at least 1")
    if not 1 <= k <= 7:
        raise ValueError(f"per_sequence speculation verifies spec_len + 1 "
                         f"tokens per device-position forward: spec_len {k} "
                         f"must lie in [1, 7]")
    lens = check_prompt_lens([S] * B if prompt_lens is None else prompt_lens,
                             input_ids)
    t_caches, d_caches = caches
    rows = torch.arange(B, device=dev)

    # both prefill the padded prompt; the draft's logits are unused and its
    # first step rewrites row len_b - 1
    t_logits = target(input_ids, kv_caches=t_caches, pos_offset=0)
    draft(input_ids, kv_caches=d_caches, pos_offset=0)
    tok = _greedy(t_logits[rows, lens - 1])
    d_prev = input_ids[rows, lens - 1]

    # row b's new tokens, written at its own column ``produced``; a round
    # writes k + 1 of which the first j_b + 1 stand, the rest is overwritten
    # by the next round or cut off at max_new_tokens
    new = input_ids.new_full((B, max_new_tokens + k + 1), pad_token_id)
    new[:, 0] = tok
    produced = torch.ones(B, dtype=torch.long, device=dev)
    pos = torch.where(produced < max_new_tokens, lens, -torch.ones_like(lens))
    steps = torch.arange(k + 1, device=dev)
    n_accepted = torch.zeros((), dtype=torch.long, device=dev)
    n_row_rounds = 0

    while True:
        act = pos >= 0
        n_act = int(act.sum())
        if n_act == 0:
            break
        n_row_rounds += n_act

        def at(off):  # an inactive row stays at -1
            return torch.where(act, pos + off, pos)

        # ---- draft proposes k tokens ---------------------------------
        dl = draft(torch.stack([d_prev, tok], 1), kv_caches=d_caches,
                   pos_offset=at(-1))
        proposals = [_greedy(dl[:, -1, :])]
        for i in range(1, k):
            dl = draft(proposals[-1].unsqueeze(1), kv_caches=d_caches,
                       pos_offset=at(i))
            proposals.append(_greedy(dl[:, -1, :]))
        dmat = torch.stack(proposals, dim=1)  # (B, k)

        # ---- target verifies the chunk in one forward ----------------
        chunk = torch.cat([tok.unsqueeze(1), dmat], dim=1)  # (B, k+1)
        tmat = _greedy(target(chunk, kv_caches=t_caches, pos_offset=pos))

        # per row: the longest agreeing prefix j_b; the j_b accepted tokens
        # ARE the target's choices, so the row emits tmat[b, :j_b + 1]
        j = (dmat == tmat[:, :-1]).long().cumprod(dim=1).sum(dim=1)  # (B,)
        idx = produced.view(B, 1) + steps
        idx = torch.where(act.view(B, 1), idx, steps.expand(B, -1))
        new.scatter_(1, idx, torch.where(act.view(B, 1), tmat,
                                         new.gather(1, idx)))
        n_accepted += (j * act).sum()
        d_prev = torch.where(j > 0, dmat.gather(
            1, (j - 1).clamp(min=0).view(B, 1)).view(B), tok)
        tok = tmat.gather(1, j.view(B, 1)).view(B)
        produced = produced + (j + 1) * act
        pos = torch.where(act & (produced < max_new_tokens), pos + j + 1,
                          -torch.ones_like(pos))

    tokens = ragged_output(input_ids, lens, new[:, :max_new_tokens],
                           S + max_new_tokens, pad_token_id)
    rate = int(n_accepted) / max(1, n_row_rounds * spec_len)
    return tokens, rate


@torch.no_grad()
def speculative_generate(target, draft, input_ids: torch.Tensor,
                         max_new_tokens: int = 32, spec_len: int = 4,
                         kv_format=None, fused_verify: bool = False,
                         per_sequence: bool = False, prompt_lens=None,
                         pad_token_id: int = 0):
    """Greedy speculative generation.  target/draft:
    LlamaForCausalLM-compatible; input_ids (B, S).  Returns
    (tokens (B, S+new), acceptance_rate).  ``kv_format``: the cache format
    of both models (build_kv_caches).  ``fused_verify``: run the target's
    verify chunk and the draft's two-token step with a device position, i.e.
    through the fused multi-token decode attention (ops.chunk_attn_step /
    ops.chunk_attn_mx_step on GPU) instead of rectangular attention over the
    prefix; chunks of more than 8 tokens keep the default path.

    ``per_sequence``: acceptance per sequence instead of what the whole batch
    agrees on.  Positions are a device (B,) tensor and every draft step and
    verify chunk is a device-position forward (LlamaAttention._cached_step):
    through the fused ragged kernels with ``fused_verify`` where the model
    can take them, through its eager chain otherwise; spec_len <= 7.  A
    sequence that has its ``max_new_tokens`` goes inactive.  The result is
    laid out as by ``generate(prompt_lens=...)`` and the rate is accepted
    tokens over (active sequence-rounds x spec_len).  ``prompt_lens``
    (per_sequence only): lengths of right-padded prompts, as in generate."""
    if prompt_lens is not None and not per_sequence:
        raise ValueError("prompt_lens needs per_sequence=True")
    B, S = input_ids.shape
    dev = input_ids.device

    def make_caches(model):
        cfg = model.config
        from ..parallel import parallel_state as ps

        tp = ps.get_tensor_model_parallel_size()
        kv_mult = max(1, tp // cfg.num_key_value_heads)
        n_kv_local = cfg.num_key_value_heads * kv_mult // tp
        return build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                               S + max_new_tokens + spec_len + 1,
                               cfg.head_dim, device=input_ids.device,
                               kv_format=kv_format)

    t_caches = make_caches(target)
    d_caches = make_caches(draft)
    if per_sequence:
        from .. import ops

        with ops.ragged_attn_step(fused_verify):
            return _speculative_per_sequence(target, draft, input_ids,
                                             max_new_tokens, spec_len,
                                             prompt_lens, pad_token_id,
                                             (t_caches, d_caches))

    # prefill both; the draft's prefill logits are unused
    t_logits = target(input_ids, kv_caches=t_caches, pos_offset=0)
    if S > 1:
        draft(input_ids[:, :-1], kv_caches=d_caches, pos_offset=0)

    tok = _greedy(t_logits[:, -1, :])  # (B,)
    out = [input_ids, tok.unsqueeze(1)]
    # target cache holds rows [0, S); draft cache rows [0, S-1); the last
    # prompt token goes through the draft with its first proposal step
    pos = S
    d_prev = input_ids[:, -1]
    produced = 1
    n_rounds = 0
    n_accepted = 0

    while produced < max_new_tokens:
        k = min(spec_len, max_new_tokens - produced)
        # ---- draft proposes k tokens ---------------------------------
        proposals = []
        cur = tok
        dl = draft(torch.stack([d_prev, cur], 1), kv_caches=d_caches,
                   pos_offset=_chunk_pos(pos - 1, 2, fused_verify, dev))
        proposals.append(_greedy(dl[:, -1, :]))
        for i in range(1, k):
            dl = draft(proposals[-1].unsqueeze(1), kv_caches=d_caches,
                       pos_offset=pos + i)
            proposals.append(_greedy(dl[:, -1, :]))
        dmat = torch.stack(proposals, dim=1)  # (B, k)

        # ---- target verifies the chunk in one forward ----------------
        chunk = torch.cat([tok.unsqueeze(1), dmat], dim=1)  # (B, k+1)
        tl = target(chunk, kv_caches=t_caches,
                    pos_offset=_chunk_pos(pos, k + 1, fused_verify, dev))
        tmat = _greedy(tl)  # (B, k+1): target choice AFTER each prefix

        # longest agreeing prefix (whole batch must agree to advance a
        # slot; per_sequence=True accepts per row)
        agree = (dmat == tmat[:, :-1]).all(dim=0)  # (k,)
        j = int(agree.cumprod(dim=0).sum().item())

        accepted = [dmat[:, i] for i in range(j)]
        bonus = tmat[:, j]
        for a in accepted:
            out.append(a.unsqueeze(1))
        out.append(bonus.unsqueeze(1))
        produced += j + 1
        n_rounds += 1
        n_accepted += j
        d_prev = dmat[:, j - 1] if j > 0 else tok
        tok = bonus
        pos += j + 1

    tokens = torch.cat(out, dim=1)[:, : S + max_new_tokens]
    rate = n_accepted / max(1, n_rounds * spec_len)
    return tokens, rate


@torch.no_grad()
def medusa_generate(target, medusa_heads, input_ids: torch.Tensor,
                    max_new_tokens: int = 32, kv_format=None,
                    fused_verify: bool = False):
    """Medusa-style speculation: ``medusa_heads`` (iterable of
    utils.medusa_utils.MedusaHead, head i predicting the token at offset
    i+2) propose a chain from the LAST HIDDEN STATE in one shot — no
    autoregressive draft model — and the target verifies the chunk exactly
    like :func:`speculative_generate`.  Greedy output is identical to
    plain generation.  ``fused_verify``: as in :func:`speculative_generate`,
    for the verify chunk."""
    from ..utils.sampling import Sampler

    sampler = Sampler(do_sample=False)
    heads = list(medusa_heads)
    k = len(heads)
    B, S = input_ids.shape

    from ..parallel import parallel_state as ps

    cfg = target.config
    tp = ps.get_tensor_model_parallel_size()
    kv_mult = max(1, tp // cfg.num_key_value_heads)
    n_kv_local = cfg.num_key_value_heads * kv_mult // tp
    caches = build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                             S + max_new_tokens + k + 1, cfg.head_dim,
                             device=input_ids.device, kv_format=kv_format)

    hidden = target.model(input_ids, pos_offset=0, kv_caches=caches)
    tok = sampler(target.lm_head(hidden)[:, -1, :])
    h_last = hidden[:, -1, :]
    out = [input_ids, tok.unsqueeze(1)]
    pos = S
    produced = 1
    n_rounds = 0
    n_accepted = 0

    while produced < max_new_tokens:
        kk = min(k, max_new_tokens - produced)
        props = [sampler(heads[i](h_last)) for i in range(kk)]
        dmat = torch.stack(props, dim=1)  # (B, kk)
        chunk = torch.cat([tok.unsqueeze(1), dmat], dim=1)
        hidden = target.model(
            chunk, kv_caches=caches,
            pos_offset=_chunk_pos(pos, kk + 1, fused_verify,
                                  input_ids.device))
        tl = target.lm_head(hidden)
        tmat = torch.stack([sampler(tl[:, i, :])
                            for i in range(kk + 1)], dim=1)
        agree = (dmat == tmat[:, :-1]).all(dim=0)
        j = int(agree.cumprod(dim=0).sum().item())
        for i in range(j):
            out.append(dmat[:, i].unsqueeze(1))
        out.append(tmat[:, j].unsqueeze(1))
        h_last = hidden[:, j, :]
        tok = tmat[:, j]
        produced += j + 1
        pos += j + 1
        n_rounds += 1
        n_accepted += j

    tokens = torch.cat(out, dim=1)[:, : S + max_new_tokens]
    rate = n_accepted / max(1, n_rounds * k)
    return tokens, rate
