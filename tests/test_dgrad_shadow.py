"""dgrad as a K-contiguous product on W^T (parallel/layers.py
``dgrad_weight_t``): gradients, freshness of W^T, checkpoints, and the
weight-value generation that the remaining weight-derived caches key on.

Runs on CPU tensors through the composed ``ops.transpose`` fallback (so it
also runs where a GPU is present).  The size threshold is lowered by
patching ``layers._DGRAD_SHADOW_MIN_NUMEL`` so the tiny layers are eligible.

W^T is built from the weight at every backward and never cached, so the
checks below take a forward and backward DIRECTLY after each kind of write
(optimizer step, a fused-step stub writing ``flat_param`` with no
``_version`` moving, ``weight.data.mul_()``, an in-place op on the
parameter, the optimizer's ``load_state_dict``) and compare the W^T that
the backward used, at the moment of use, with the weight transposed.
"""

import copy
import os

import torch

from dist_utils import run_distributed

TOKENS, HIDDEN, HEADS, KV_HEADS, HEAD_DIM = 48, 64, 4, 2, 16


def _env(shadow: bool):
    from neuronx_distributed_amd.parallel import layers

    os.environ["NXDA_DGRAD_SHADOW"] = "1" if shadow else "0"
    layers._DGRAD_SHADOW_MIN_NUMEL = 1


def _grads(layer, x, gouts):
    """One backward with fixed upstream gradients; returns (grad_input,
    [grad_weight...]) and clears the parameter grads."""
    xi = x.clone().requires_grad_(True)
    out = layer(xi)
    outs = out if isinstance(out, tuple) else (out,)
    loss = sum((o.float() * g.float()).sum() for o, g in zip(outs, gouts))
    loss.backward()
    gws = [p.grad.clone() for p in layer.parameters()]
    for p in layer.parameters():
        p.grad = None
    return xi.grad.clone(), gws


def _gradient_worker(rank, world):
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import (
        ColumnParallelLinear, RowParallelLinear)
    from neuronx_distributed_amd.parallel.qkv_linear import (
        GQAQKVColumnParallelLinear)

    from neuronx_distributed_amd import ops

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    bf = torch.bfloat16
    torch.manual_seed(0)
    built, orig_tr = [], ops.transpose

    def tr(x, out=None):
        built.append(1)
        return orig_tr(x, out=out)

    ops.transpose = tr
    layers = {
        "column": ColumnParallelLinear(HIDDEN, 2 * HIDDEN, bias=False,
                                       gather_output=False, dtype=bf),
        "row": RowParallelLinear(2 * HIDDEN, HIDDEN, bias=False,
                                 input_is_parallel=True, dtype=bf),
        "qkv": GQAQKVColumnParallelLinear(
            HIDDEN, [HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM], bias=False,
            gather_output=False, dtype=bf, head_dim=HEAD_DIM),
    }
    report = {}
    for name, layer in layers.items():
        ws = [p.detach() for p in layer.parameters()]
        x = torch.randn(TOKENS, ws[0].shape[1]).to(bf)
        gouts = [torch.randn(TOKENS, w.shape[0]).to(bf) for w in ws]
        # float64 reference on the same bf16 inputs
        ref_gi = sum(g.double() @ w.double() for g, w in zip(gouts, ws))
        ref_gw = [g.double().t() @ x.double() for g in gouts]

        dev = {}
        for shadow in (False, True):
            _env(shadow)
            built.clear()
            gi, gws = _grads(layer, x, gouts)
            assert len(built) == (len(ws) if shadow else 0), (name, built)
            dev[shadow] = (
                (gi.double() - ref_gi).abs().max().item(),
                max((a.double() - b).abs().max().item()
                    for a, b in zip(gws, ref_gw)))
        report[name] = dev
        print(f"{name}: grad_input dev off {dev[False][0]:.4g} on "
              f"{dev[True][0]:.4g}; grad_weight dev off {dev[False][1]:.4g} "
              f"on {dev[True][1]:.4g}")
        # both are fp32-accumulate, bf16-round: only the order differs
        assert dev[False][0] > 0 and dev[False][1] > 0
        assert dev[True][0] <= 2 * dev[False][0], (name, dev)
        assert dev[True][1] <= 2 * dev[False][1], (name, dev)
    return report


def test_gradients_match_float64_with_and_without_shadow():
    run_distributed(_gradient_worker, world_size=1)


def _staleness_worker(rank, world):
    import torch.nn as nn

    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.optimizer import NeuronZero1Optimizer
    from neuronx_distributed_amd.parallel import layers, qkv_linear
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    _env(True)
    bf = torch.bfloat16
    torch.manual_seed(0)

    class Tiny(nn.Module):
        def __init__(self):
            super().__init__()
            self.qkv = qkv_linear.GQAQKVColumnParallelLinear(
                HIDDEN, [HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM], bias=False,
                gather_output=False, dtype=bf, head_dim=HEAD_DIM)
            self.up = layers.ColumnParallelLinear(
                HIDDEN, 2 * HIDDEN, bias=False, gather_output=False, dtype=bf)
            self.down = layers.RowParallelLinear(
                2 * HIDDEN, HIDDEN, bias=False, input_is_parallel=True,
                dtype=bf)

        def forward(self, x):
            q, k, v = self.qkv(x)
            h = q + torch.cat([k, v], dim=-1)
            return self.down(torch.tanh(self.up(h)))

    model = Tiny()
    n_weights = len(list(model.parameters()))
    opt = NeuronZero1Optimizer(model.parameters(), torch.optim.AdamW,
                               lr=1e-1, weight_decay=0.0)
    saved = copy.deepcopy(opt.state_dict())
    w0 = [p.detach().clone() for p in model.parameters()]

    # record every shadow at the moment a backward uses it
    uses, builds = [], []
    orig_get, orig_tr = layers.dgrad_weight_t, ops.transpose

    def get(weight):
        w_t = orig_get(weight)
        assert w_t is not None
        uses.append(torch.equal(w_t, weight.detach().t()))
        return w_t

    def tr(x, out=None):
        builds.append(1)
        return orig_tr(x, out=out)

    layers.dgrad_weight_t = qkv_linear.dgrad_weight_t = get
    ops.transpose = tr

    def fwd_bwd(expect_builds=n_weights):
        uses.clear()
        builds.clear()
        x = torch.randn(TOKENS, HIDDEN).to(bf).requires_grad_(True)
        model(x).float().pow(2).mean().backward()
        assert len(uses) == n_weights and all(uses), uses
        assert len(builds) == expect_builds, (len(builds), expect_builds)

    def moved():
        return [not torch.equal(p.detach(), w) for p, w in
                zip(model.parameters(), w0)]

    opt.zero_grad()
    fwd_bwd()
    fwd_bwd()               # second microbatch of the window

    opt.step()              # unfused path (CPU)
    assert all(moved())
    fwd_bwd()

    # fused-path shape: the update goes through flat_param, no parameter's
    # _version moves
    versions = [p._version for p in model.parameters()]

    def fused_stub(clip):
        for b in opt.buckets:
            b.flat_param[b.shard_lo:b.shard_hi].mul_(0.5)

    opt._use_fused = lambda: True
    opt._fused_step = fused_stub
    before = [p.detach().clone() for p in model.parameters()]
    keys = [layers._weight_cache_key(p) for p in model.parameters()]
    opt.step()
    del opt._use_fused, opt._fused_step
    assert versions == [p._version for p in model.parameters()]
    assert all(not torch.equal(p.detach(), b) for p, b in
               zip(model.parameters(), before))
    fwd_bwd()
    # ... and the generation did, for the caches that key on it
    assert all(k != layers._weight_cache_key(p)
               for k, p in zip(keys, model.parameters()))

    # eager write through .data: no version counter moves at all; the very
    # next backward must still see the new values
    before = [p.detach().clone() for p in model.parameters()]
    for p in model.parameters():
        p.data.mul_(-2.0)
    assert versions == [p._version for p in model.parameters()]
    assert all(not torch.equal(p.detach(), b) for p, b in
               zip(model.parameters(), before))
    fwd_bwd()

    # in-place op on the parameter itself
    with torch.no_grad():
        model.up.weight.mul_(0.5)
    fwd_bwd()

    keys = [layers._weight_cache_key(p) for p in model.parameters()]
    opt.load_state_dict(saved)
    assert not any(moved())
    fwd_bwd()
    assert all(k != layers._weight_cache_key(p)
               for k, p in zip(keys, model.parameters()))

    # checkpoints: nothing is attached to the parameters or the module
    names = {n for n, _ in model.named_parameters()}
    assert names == {"qkv.weight_q", "qkv.weight_k", "qkv.weight_v",
                     "up.weight", "down.weight"}
    sd = model.state_dict()
    assert set(sd) == names
    for k, v in sd.items():
        assert v.shape == dict(model.named_parameters())[k].shape
    assert set(dict(model.named_buffers())) == set()
    for p in model.parameters():
        assert not [a for a in vars(p) if "shadow" in a or "dgrad" in a]
    return True


def test_weight_t_never_stale_and_never_in_checkpoints():
    run_distributed(_staleness_worker, world_size=1)


def _switch_worker(rank, world):
    from neuronx_distributed_amd.parallel import layers
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    bf = torch.bfloat16
    w = torch.nn.Parameter(torch.randn(64, 128).to(bf))
    os.environ.pop("NXDA_DGRAD_SHADOW", None)
    assert layers._DGRAD_SHADOW_MIN_NUMEL == 4096 * 4096
    with torch.no_grad():
        assert layers.dgrad_weight_t(w) is None      # below 4096 x 4096
        layers._DGRAD_SHADOW_MIN_NUMEL = 1
        assert torch.equal(layers.dgrad_weight_t(w), w.detach().t())
        os.environ["NXDA_DGRAD_SHADOW"] = "0"
        assert layers.dgrad_weight_t(w) is None
        os.environ["NXDA_DGRAD_SHADOW"] = "1"
        w.dgrad_shadow = False                       # lm_head opt-out
        assert layers.dgrad_weight_t(w) is None
        del w.dgrad_shadow
        assert layers.dgrad_weight_t(w.float()) is None
        assert layers.dgrad_weight_t(w[:, :56]) is None  # strided rows
        assert layers.dgrad_weight_t(w[:60]) is None     # 60 % 8
    assert layers.dgrad_weight_t(w) is None          # double backward
    return True


def test_shadow_eligibility_and_switch():
    run_distributed(_switch_worker, world_size=1)


def _lm_head_worker(rank, world):
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import layers
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    for tie in (False, True):
        m = LlamaForCausalLM(get_config("tiny", tie_word_embeddings=tie))
        x = torch.randint(0, 256, (1, 8))
        m(x, labels=x).backward()
        assert m.lm_head.dgrad_shadow is False
        assert m.lm_head.weight.dgrad_shadow is False
        layers._DGRAD_SHADOW_MIN_NUMEL = 1
        with torch.no_grad():
            assert layers.dgrad_weight_t(m.lm_head.weight) is None
        layers._DGRAD_SHADOW_MIN_NUMEL = 4096 * 4096
    return True


def test_lm_head_is_excluded():
    run_distributed(_lm_head_worker, world_size=1)


def _fused_qkv_cache_worker(rank, world):
    """The inference-side concatenated QKV weight keys on the generation
    too: an optimizer write through flat_param must rebuild it."""
    from neuronx_distributed_amd.optimizer import NeuronZero1Optimizer
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.qkv_linear import (
        GQAQKVColumnParallelLinear)

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    qkv = GQAQKVColumnParallelLinear(
        HIDDEN, [HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM], bias=False,
        gather_output=False, head_dim=HEAD_DIM)
    opt = NeuronZero1Optimizer(qkv.parameters(), torch.optim.AdamW, lr=1e-1)
    wcat, _ = qkv._fused_qkv_weight()
    assert qkv._fused_qkv_weight()[0] is wcat
    for b in opt.buckets:       # what the fused AdamW kernel does
        b.flat_param[b.shard_lo:b.shard_hi].mul_(0.5)
    opt._all_gather_params(copy_master=False)
    wcat2, _ = qkv._fused_qkv_weight()
    assert torch.equal(wcat2, torch.cat([qkv.weight_q, qkv.weight_k,
                                         qkv.weight_v]).detach())
    assert not torch.equal(wcat2, wcat)
    return True


def test_fused_qkv_cache_sees_raw_pointer_updates():
    run_distributed(_fused_qkv_cache_worker, world_size=1)
