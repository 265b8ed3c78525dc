"""Medusa tree verification on the CPU in fp32: the eager tree chain of
LlamaAttention._tree_step (the reference of the fused kernel of
test_tree_attn_gpu.py), KVCache.commit_path and
medusa_generate(medusa_choices=...)."""

import pytest
import torch

from dist_utils import run_distributed

CHOICES = [[0], [1], [0, 0], [0, 1], [1, 0], [0, 0, 0], [1, 0, 0]]  # 8 nodes


def _model(seed=0):
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    cfg = get_config("tiny")
    torch.manual_seed(seed)
    return cfg, LlamaForCausalLM(cfg).eval()


def _tree_worker(rank, world, ragged):
    from neuronx_distributed_amd.inference.kv_cache import build_kv_caches
    from neuronx_distributed_amd.utils.medusa_utils import (
        generate_medusa_buffers, medusa_tree_topology)

    cfg, model = _model()
    mask = generate_medusa_buffers(CHOICES)["medusa_attn_mask"]
    tree = medusa_tree_topology(mask)
    assert tree[1].tolist() == [0, 1, 1, 2, 2, 2, 3, 3]
    B, P, T = 2, 7, mask.shape[0]
    pos = [P, P - 2] if ragged else [P, P]
    torch.manual_seed(1)
    x = torch.randint(0, cfg.vocab_size, (B, P))
    nodes = torch.randint(0, cfg.vocab_size, (B, T))
    with torch.no_grad():
        caches = build_kv_caches(cfg.num_hidden_layers, B,
                                 cfg.num_key_value_heads, P + T + 3,
                                 cfg.head_dim, dtype=torch.float32,
                                 device="cpu")
        model(x, kv_caches=caches, pos_offset=0)
        pos_t = torch.tensor(pos if ragged else pos[:1])
        got = model(nodes, kv_caches=caches, pos_offset=pos_t, tree=tree)
        for b in range(B):
            for i in range(T):
                path = mask[i].nonzero().view(-1)
                seq = torch.cat([x[b, :pos[b]], nodes[b, path]]).view(1, -1)
                want = model(seq)[0, -1]
                assert torch.allclose(got[b, i], want, atol=1e-5, rtol=1e-5), \
                    (b, i, (got[b, i] - want).abs().max())
        with pytest.raises(ValueError):
            model(nodes, kv_caches=caches, pos_offset=pos_t, tree=tree,
                  chunk_lens=torch.tensor([T, T]))
    return True


@pytest.mark.parametrize("ragged", [False, True])
def test_tree_chain_equals_path_forwards(ragged):
    run_distributed(_tree_worker, world_size=1, args=(ragged,))


def test_topology_rejects_a_non_tree():
    from neuronx_distributed_amd.utils.medusa_utils import (
        medusa_tree_topology)

    bad = torch.eye(4, dtype=torch.bool)
    bad[:, 0] = True
    bad[3, 1] = bad[3, 2] = True     # two parents
    with pytest.raises(ValueError):
        medusa_tree_topology(bad)
    with pytest.raises(ValueError):
        medusa_tree_topology(torch.ones(17, 17, dtype=torch.bool).tril())


@pytest.mark.parametrize("paths,pos", [
    ([[0, 3, 5, 7], [0, 2, -1, -1]], [4, 9]),      # overlap; -1 padding
    ([[0, 1, 4, 6], [0, 3, 5, 7]], [6]),           # one shared position
    ([[0, 16, 3, -5], [0, 3, 5, 7]], [4, -1]),     # bad entries; inactive
    ([[0, 3, 5, 7], [0, 3, 5, 7]], [11, 10]),      # row 18 is past the cache
])
def test_commit_path_equals_loop(paths, pos):
    from neuronx_distributed_amd.inference.kv_cache import KVCache

    B, H, Smax, D = 2, 2, 18, 16
    c = KVCache(B, H, Smax, D, dtype=torch.float32, device="cpu")
    torch.manual_seed(0)
    c.k.normal_()
    c.v.normal_()
    src_k, src_v = c.k.clone(), c.v.clone()
    want_k, want_v = c.k.clone(), c.v.clone()
    c.commit_path(torch.tensor(pos), torch.tensor(paths))
    for b in range(B):
        p = pos[b % len(pos)]
        for d, node in enumerate(paths[b]):
            if d >= 1 and 0 <= node < 16 and p >= 0 \
                    and p + max(node, d) < Smax:
                want_k[b, :, p + d] = src_k[b, :, p + node]
                want_v[b, :, p + d] = src_v[b, :, p + node]
    assert torch.equal(c.k, want_k) and torch.equal(c.v, want_v)
    assert not torch.equal(c.k, src_k)


def _oracle_heads(target, ref, n_heads):
    """Heads that find the position of h_last in the greedy continuation
    ``ref`` and propose its tokens: head 0 right at top-1 on even positions
    and at top-2 on odd ones, the deeper heads right for sequence 0 and wrong
    for sequence 1."""
    hid = target.model(ref)                       # (B, N, H)
    V = target.config.vocab_size

    def head(i):
        def f(h):
            p = (hid - h.unsqueeze(1)).norm(dim=-1).argmin(dim=1)   # (B,)
            nxt = ref.gather(1, (p + 2 + i).clamp(max=ref.shape[1] - 1)
                             .view(-1, 1)).view(-1)
            wrong = (nxt + 1) % V
            swap = (p % 2 == 1) if i == 0 else torch.tensor(
                [False, True], device=h.device)
            logits = torch.zeros(h.shape[0], V, device=h.device)
            logits.scatter_(1, torch.where(swap, wrong, nxt).view(-1, 1), 2.0)
            logits.scatter_(1, torch.where(swap, nxt, wrong).view(-1, 1), 1.0)
            return logits
        return f
    return [head(i) for i in range(n_heads)]


def _medusa_worker(rank, world):
    from neuronx_distributed_amd.inference.generation import generate
    from neuronx_distributed_amd.inference.speculation import medusa_generate

    cfg, target = _model()
    torch.manual_seed(3)
    x = torch.randint(0, cfg.vocab_size, (2, 9))
    with torch.no_grad():
        ref = generate(target, x, max_new_tokens=16)
        heads = _oracle_heads(target, ref, 3)
        out, rate = medusa_generate(target, heads, x, max_new_tokens=14,
                                    medusa_choices=CHOICES)
        assert torch.equal(out, ref[:, :out.shape[1]]), (out, ref)
        assert out.shape == (2, 9 + 14)
        # sequence 0 accepts up to three tokens a round, sequence 1 at most
        # one: the rate lies strictly between
        assert 1 / 3 < rate < 1.0, rate
        with pytest.raises(ValueError):
            medusa_generate(target, heads, x, max_new_tokens=4,
                            medusa_choices=CHOICES, kv_format="mxfp8")
    return True


def test_medusa_tree_equals_greedy():
    run_distributed(_medusa_worker, world_size=1)
