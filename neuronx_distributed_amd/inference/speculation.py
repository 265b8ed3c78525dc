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

from .kv_cache import PAGE_ROWS, PagePool, build_kv_caches


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
    (per_sequence only): lengths of right-padded prompts, as in generate.

    ``kv_format="paged"`` (per_sequence only): each model gets one PagePool
    of sum_b ceil((len_b + max_new_tokens + spec_len + 1) / 16) pages,
    allocated up front.  On GPU the one-token draft steps then run through
    ops.paged_attn_step, the draft's two-token step and the verify chunk
    through ops.paged_chunk_attn_step.  ``kv_format="paged_mxfp8"``: the same
    rules and pools with MXFP8 rows inside the pages, through
    ops.paged_attn_mx_step and ops.paged_chunk_attn_mx_step."""
    if prompt_lens is not None and not per_sequence:
        raise ValueError("prompt_lens needs per_sequence=True")
    paged = kv_format in ("paged", "paged_mxfp8")
    if paged and not per_sequence:
        raise ValueError(f"kv_format={kv_format!r} needs per_sequence=True: "
                         f"a paged cache keeps one position per sequence")
    B, S = input_ids.shape
    dev = input_ids.device
    extra = max_new_tokens + spec_len + 1   # rows beyond a prompt

    def make_caches(model):
        cfg = model.config
        from ..parallel import parallel_state as ps

        tp = ps.get_tensor_model_parallel_size()
        kv_mult = max(1, tp // cfg.num_key_value_heads)
        n_kv_local = cfg.num_key_value_heads * kv_mult // tp
        pool = None
        if paged:
            # as generate(): every sequence allocated up front, so the table
            # is static; stale rows of a rejected chunk stay inside it
            from .generation import check_prompt_lens

            lens = check_prompt_lens(
                [S] * B if prompt_lens is None else prompt_lens, input_ids)
            rows = [n + extra for n in lens.tolist()]
            pages = [-(-n // PAGE_ROWS) for n in rows]
            pool = PagePool(sum(pages), B, max(pages), dev)
            for b, n in enumerate(rows):
                pool.allocate(b, n)
        return build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                               S + extra, cfg.head_dim, device=dev,
                               kv_format=kv_format, page_pool=pool)

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


def _medusa_tree(target, heads, input_ids, max_new_tokens, medusa_choices,
                 caches):
    """medusa_generate(medusa_choices=...): every round verifies the whole
    candidate tree in ONE forward at per-sequence device positions, each
    sequence accepts its own longest root path, and the accepted rows are
    packed down in every layer's cache (KVCache.commit_path)."""
    from ..utils.medusa_utils import (generate_medusa_buffers,
                                      medusa_tree_topology)

    B, S = input_ids.shape
    dev = input_ids.device
    buf = generate_medusa_buffers(medusa_choices, device=dev)
    tree = medusa_tree_topology(buf["medusa_attn_mask"], device=dev)
    tree_indices, retrieve = buf["tree_indices"], buf["retrieve_indices"]
    P, L = retrieve.shape                      # root paths, depth + 1
    max_k = max(p[-1] for p in medusa_choices) + 1
    if L - 1 > len(heads):
        raise ValueError(f"a choice tree of depth {L - 1} needs as many "
                         f"heads, got {len(heads)}")
    if max_new_tokens < 1:
        raise ValueError(f"max_new_tokens {max_new_tokens} must be at least 1")
    node = retrieve.clamp(min=0)               # (P, L)
    parent = torch.cat([node[:, :1], node[:, :-1]], dim=1)
    steps = torch.arange(L, device=dev)

    hidden = target.model(input_ids, pos_offset=0, kv_caches=caches)
    tok = _greedy(target.lm_head(hidden[:, -1:, :])[:, 0])
    h_last = hidden[:, -1, :]
    new = input_ids.new_zeros((B, max_new_tokens + L))
    new[:, 0] = tok
    produced = torch.ones(B, dtype=torch.long, device=dev)
    pos = torch.where(produced < max_new_tokens, torch.full_like(produced, S),
                      -torch.ones_like(produced))
    n_accepted = torch.zeros((), dtype=torch.long, device=dev)
    n_row_rounds = 0

    while True:
        act = pos >= 0
        n_act = int(act.sum())
        if n_act == 0:
            break
        n_row_rounds += n_act
        # 1. the T candidates: the last token, then each head's top-k
        topk = [heads[i](h_last).topk(max_k, dim=-1).indices
                for i in range(L - 1)]
        cand = torch.cat([tok.unsqueeze(1)] + topk, dim=1)[:, tree_indices]
        # 2., 3. one tree forward; the target's greedy token at every node
        hidden = target.model(cand, pos_offset=pos, kv_caches=caches,
                              tree=tree)
        tgt = _greedy(target.lm_head(hidden))  # (B, T)
        # 4. per sequence the longest root path on which every node's token
        # is the target's token at its parent
        ok = (cand[:, node] == tgt[:, parent]) & (retrieve >= 0)  # (B, P, L)
        ok[:, :, 0] = True
        n_ok = ok.long().cumprod(dim=2).sum(dim=2) - 1            # (B, P)
        j, best = n_ok.max(dim=1)                                 # (B,)
        path = torch.where(steps.view(1, L) <= j.view(B, 1), node[best],
                           -torch.ones_like(node[best]))          # (B, L)
        # 5. the accepted rows move to pos + 1 .. pos + j
        for c in caches:
            c.commit_path(pos, path)
        # 6., 7. the path's target tokens are the output; the last one and
        # its hidden state start the next round
        emit = tgt.gather(1, path.clamp(min=0))                   # (B, L)
        idx = torch.where(act.view(B, 1), produced.view(B, 1) + steps,
                          steps.expand(B, -1))
        new.scatter_(1, idx, torch.where(act.view(B, 1), emit,
                                         new.gather(1, idx)))
        last = node[best].gather(1, j.view(B, 1))                 # (B, 1)
        tok = tgt.gather(1, last).view(B)
        h_last = hidden.gather(
            1, last.view(B, 1, 1).expand(B, 1, hidden.shape[-1]))[:, 0]
        n_accepted += (j * act).sum()
        produced = produced + (j + 1) * act
        pos = torch.where(act & (produced < max_new_tokens), pos + j + 1,
                          -torch.ones_like(pos))

    tokens = torch.cat([input_ids, new[:, :max_new_tokens]], dim=1)
    return tokens, int(n_accepted) / max(1, n_row_rounds * (L - 1))


@torch.no_grad()
def medusa_generate(target, medusa_heads, input_ids: torch.Tensor,
                    max_new_tokens: int = 32, kv_format=None,
                    fused_verify: bool = False, medusa_choices=None):
    """Medusa-style speculation: ``medusa_heads`` (iterable of
    utils.medusa_utils.MedusaHead, head i predicting the token at offset
    i+2) propose a chain from the LAST HIDDEN STATE in one shot — no
    autoregressive draft model — and the target verifies the chunk exactly
    like :func:`speculative_generate`.  Greedy output is identical to
    plain generation.  ``fused_verify``: as in :func:`speculative_generate`,
    for the verify chunk.

    ``medusa_choices``: a choice tree as taken by
    utils.medusa_utils.generate_medusa_buffers, at most 15 entries.  Head i
    then proposes its top-k tokens and the whole tree of candidates is
    verified in one forward per round (LlamaAttention._tree_step), each
    sequence accepting its own longest path.  Tree mode works on the plain
    cache only and always at device positions, so ``fused_verify`` has no
    say in it: the fused kernel runs wherever the tree step can take it."""
    from ..utils.sampling import Sampler

    sampler = Sampler(do_sample=False)
    heads = list(medusa_heads)
    k = len(heads)
    B, S = input_ids.shape
    if medusa_choices is not None:
        if kv_format is not None:
            raise ValueError(f"medusa_choices needs the plain cache, not "
                             f"kv_format={kv_format!r}")
        k = len(medusa_choices)   # T - 1 spare rows for the last round

    from ..parallel import parallel_state as ps

    cfg = target.config
    tp = ps.get_tensor_model_parallel_size()
    kv_mult = max(1, tp // cfg.num_key_value_heads)
    n_kv_local = cfg.num_key_value_heads * kv_mult // tp
    caches = build_kv_caches(cfg.num_hidden_layers, B, n_kv_local,
                             S + max_new_tokens + k + 1, cfg.head_dim,
                             device=input_ids.device, kv_format=kv_format,
                             **({} if medusa_choices is None else
                                {"dtype": next(target.parameters()).dtype}))
    if medusa_choices is not None:
        return _medusa_tree(target, heads, input_ids, max_new_tokens,
                            medusa_choices, caches)

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
