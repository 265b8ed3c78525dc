"""Weight gradients as K-contiguous products (parallel/layers.py
``wgrad_tn``, NXDA_WGRAD_TN): exact gradients, the single X^T of the QKV
backward, the dx^T hand-off from SwiGLU's backward, the opt-outs, and the
whole model.

Runs on CPU tensors through the composed ``ops.transpose`` fallback.  The
size thresholds are lowered by patching ``layers._WGRAD_TN_MIN_NUMEL`` and
``layers._WGRAD_TN_MIN_M`` so the tiny layers are eligible.

Exactness: inputs, weights and upstream gradients are integers in [-4, 4]
stored as bf16, 48 tokens, hidden 64.  A weight-gradient element is a sum of
48 products of at most 16, so every fp32 partial sum is exact in any order
and the two forms must agree bit for bit with the fp32 product rounded to
bf16.
"""

import os

import torch

from dist_utils import run_distributed

TOKENS, HIDDEN, HEADS, KV_HEADS, HEAD_DIM = 48, 64, 4, 2, 16
bf = torch.bfloat16


def _knob(on: bool, low_thresholds: bool = True):
    from neuronx_distributed_amd.parallel import layers

    os.environ["NXDA_WGRAD_TN"] = "1" if on else "0"
    layers._WGRAD_TN_MIN_NUMEL = 1 if low_thresholds else 4096 * 4096
    layers._WGRAD_TN_MIN_M = 1 if low_thresholds else 16384


def _ints(*shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).to(bf)


class _Count:
    """Counts ops.transpose_multi calls (matrices per call)."""

    def __enter__(self):
        from neuronx_distributed_amd import ops

        self.ops, self.orig, self.calls = ops, ops.transpose_multi, []

        def counted(xs, outs=None):
            xs = list(xs)
            self.calls.append(len(xs))
            return self.orig(xs, outs)

        ops.transpose_multi = counted
        return self

    def __exit__(self, *exc):
        self.ops.transpose_multi = self.orig


def _backward(layer, x, gouts):
    xi = x.clone().requires_grad_(True)
    out = layer(xi)
    outs = out if isinstance(out, tuple) else (out,)
    torch.autograd.backward(outs, list(gouts))
    grads = {n: p.grad.clone() for n, p in layer.named_parameters()}
    for p in layer.parameters():
        p.grad = None
    return xi.grad.clone(), grads


def _exact_worker(rank, world):
    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import (
        ColumnParallelLinear, RowParallelLinear)
    from neuronx_distributed_amd.parallel.qkv_linear import (
        GQAQKVColumnParallelLinear)

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    layers = {
        "column": ColumnParallelLinear(HIDDEN, 2 * HIDDEN, bias=True,
                                       gather_output=False, stride=2,
                                       dtype=bf),
        "row": RowParallelLinear(2 * HIDDEN, HIDDEN, bias=True,
                                 input_is_parallel=True, dtype=bf),
        "qkv": GQAQKVColumnParallelLinear(
            HIDDEN, [HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM], bias=True,
            gather_output=False, dtype=bf, head_dim=HEAD_DIM),
    }
    for li, (name, layer) in enumerate(layers.items()):
        with torch.no_grad():
            for i, p in enumerate(layer.parameters()):
                p.copy_(_ints(*p.shape, seed=10 * li + i))
        ws = [p.detach() for n, p in layer.named_parameters()
              if n.startswith("weight")]
        x = _ints(TOKENS, ws[0].shape[1], seed=100 + li)
        gouts = [_ints(TOKENS, w.shape[0], seed=200 + 10 * li + i)
                 for i, w in enumerate(ws)]
        res = {}
        for on in (False, True):
            _knob(on)
            with _Count() as c:
                res[on] = _backward(layer, x, gouts)
            assert bool(c.calls) == on, (name, on, c.calls)
            assert ops._WGRAD_HANDOFF[0] is None
        (gi0, g0), (gi1, g1) = res[False], res[True]
        assert torch.equal(gi0, gi1), name
        assert set(g0) == set(g1)
        for n in g0:
            assert torch.equal(g0[n], g1[n]), (name, n)
        # the fp32 product rounded to bf16
        wnames = [n for n in g0 if n.startswith("weight")]
        bnames = [n for n in g0 if n.startswith("bias")]
        assert len(wnames) == len(ws) == len(bnames)
        for n, g in zip(wnames, gouts):
            ref = (g.float().t() @ x.float()).to(bf)
            assert torch.equal(g1[n], ref), (name, n)
        for n, g in zip(bnames, gouts):
            assert torch.equal(g1[n], g.float().sum(0).to(bf)), (name, n)
        if len(ws) == 1:
            # (the QKV input gradient is a sum of three separately rounded
            # products, as before this path existed: on == off above)
            ref = (gouts[0].float() @ ws[0].float()).to(bf)
            assert torch.equal(gi1, ref), name
    return True


def test_exact_gradients_knob_on_and_off():
    run_distributed(_exact_worker, world_size=1)


def _shared_xt_worker(rank, world):
    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.qkv_linear import (
        GQAQKVColumnParallelLinear)

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    _knob(True)
    qkv = GQAQKVColumnParallelLinear(
        HIDDEN, [HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM], bias=False,
        gather_output=False, dtype=bf, head_dim=HEAD_DIM)
    x = _ints(TOKENS, HIDDEN, seed=1)
    gouts = [_ints(TOKENS, n, seed=2 + i) for i, n in
             enumerate((HEADS * HEAD_DIM, KV_HEADS * HEAD_DIM,
                        KV_HEADS * HEAD_DIM))]
    singles, orig_tr = [], ops.transpose

    def tr(t, out=None):
        singles.append(tuple(t.shape))
        return orig_tr(t, out=out)

    seen = []
    orig_multi = ops.transpose_multi

    def multi(xs, outs=None):
        xs = list(xs)
        seen.append([tuple(t.shape) for t in xs])
        # the composed fallback goes through ops.transpose: call the
        # original so that `singles` counts only direct calls
        return [orig_tr(t) for t in xs]

    ops.transpose, ops.transpose_multi = tr, multi
    try:
        _backward(qkv, x, gouts)
    finally:
        ops.transpose, ops.transpose_multi = orig_tr, orig_multi
    # ONE launch: X^T once, then gq^T, gk^T, gv^T; nothing else transposes
    # an activation (the dgrad's W^T stays below its own size threshold)
    assert seen == [[(TOKENS, HIDDEN), (TOKENS, HEADS * HEAD_DIM),
                     (TOKENS, KV_HEADS * HEAD_DIM),
                     (TOKENS, KV_HEADS * HEAD_DIM)]], seen
    assert singles == [], singles
    return True


def test_qkv_backward_builds_one_x_t():
    run_distributed(_shared_xt_worker, world_size=1)


def _handoff_worker(rank, world):
    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.parallel import parallel_state as ps
    from neuronx_distributed_amd.parallel.layers import ColumnParallelLinear

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    I = HIDDEN
    gate_up = ColumnParallelLinear(HIDDEN, 2 * I, bias=False,
                                   gather_output=False, stride=2, dtype=bf)
    # data that keeps dx integer, so that the checks below are bit equality:
    # one nonzero (3 or 4) per token in x, gate weights in [6, 9] (gate >=
    # 18, where the fp32 sigmoid rounds to exactly 1: dgate = dy * up, dup =
    # dy * gate), up weights and dy in [-4, 4]
    g = torch.Generator().manual_seed(0)
    x = torch.zeros(TOKENS, HIDDEN).scatter_(
        1, torch.randint(0, HIDDEN, (TOKENS, 1), generator=g),
        torch.randint(3, 5, (TOKENS, 1), generator=g).float()).to(bf)
    with torch.no_grad():
        gate_up.weight[:I] = _ints(I, HIDDEN, seed=1, lo=6, hi=9)
        gate_up.weight[I:] = _ints(I, HIDDEN, seed=2)
    gy = _ints(TOKENS, I, seed=3)

    def run(on, between=None, hook=None):
        """gate_up -> [between] -> swiglu; returns (grad_weight, transposes
        per transpose_multi call)."""
        _knob(on)
        y = gate_up(x)
        if hook is not None:
            y.register_hook(hook)
        if between is not None:
            y = between(y)
        out = ops.swiglu(y, wgrad_dxt=True)
        with _Count() as c:
            out.backward(gy)
        g = gate_up.weight.grad.clone()
        gate_up.weight.grad = None
        assert ops._WGRAD_HANDOFF[0] is None    # empty after every backward
        return g, c.calls

    def check(between=None, hook=None, used=None):
        ref, c0 = run(False, between, hook)
        got, c1 = run(True, between, hook)
        assert c0 == [] and bool(ref.any())
        assert torch.equal(got, ref)
        if used is not None:
            # a consumed hand-off leaves only X^T to build
            assert c1 == ([1] if used else [2]), (c1, used)
        return got

    base = check(used=True)                                  # matching
    check(hook=lambda g: g * 2, used=False)                  # rewritten
    check(hook=lambda g: g.clone(), used=False)              # copied
    doubled = check(hook=lambda g: (g.mul_(2), None)[1], used=False)
    assert torch.equal(doubled.float(), 2 * base.float())    # edited in place
    # a clone between the nodes in the forward: autograd hands the clone's
    # backward whatever tensor it got; used or not, the gradient is right
    assert torch.equal(check(between=lambda y: y.clone()), base)

    # a stale entry: a SwiGLU backward whose input is no linear's output
    # leaves its dx^T in the slot ...
    _knob(True)
    leaf = _ints(TOKENS, 2 * I, seed=4).requires_grad_(True)
    ops.swiglu(leaf, wgrad_dxt=True).backward(gy)
    assert ops._WGRAD_HANDOFF[0] is not None
    stale = ops._WGRAD_HANDOFF[0][2]
    # ... and the next microbatch never sees it: a plain linear backward
    # with a gradient of the very same shape drops it
    go = _ints(TOKENS, 2 * I, seed=5)
    with _Count() as c:
        gate_up(x).backward(go)
    assert c.calls == [2] and ops._WGRAD_HANDOFF[0] is None
    assert torch.equal(gate_up.weight.grad,
                       (go.float().t() @ x.float()).to(bf))
    gate_up.weight.grad = None
    assert not torch.equal(stale.float(), go.float().t())
    # ... nor does a full second microbatch after a stale entry
    ops.swiglu(leaf, wgrad_dxt=True).backward(gy)
    assert ops._WGRAD_HANDOFF[0] is not None
    assert torch.equal(check(used=True), base)
    return True


def test_handoff_slot():
    run_distributed(_handoff_worker, world_size=1)


def _optout_worker(rank, world):
    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.parallel import layers
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    x = _ints(TOKENS, HIDDEN, seed=1)
    go = [_ints(TOKENS, 2 * HIDDEN, seed=2)]

    def calls(layer, create_graph=False):
        with _Count() as c:
            if create_graph:
                xi = x.clone().requires_grad_(True)
                (gw,) = torch.autograd.grad(layer(xi), layer.weight, go[0],
                                            create_graph=True)
                assert gw.requires_grad     # still differentiable
            else:
                _backward(layer, x, go)
        return c.calls

    def col(**kw):
        return layers.ColumnParallelLinear(HIDDEN, 2 * HIDDEN, bias=False,
                                           gather_output=False, dtype=bf,
                                           **kw)

    _knob(True)
    assert calls(col()) == [2]
    assert calls(col(), create_graph=True) == []         # double backward
    out = col(wgrad_tn=False)
    assert calls(out) == [] and out.weight.wgrad_tn is False
    row = layers.RowParallelLinear(2 * HIDDEN, HIDDEN, bias=False,
                                   input_is_parallel=True, dtype=bf,
                                   wgrad_tn=False)
    with _Count() as c:
        _backward(row, go[0], [x])
    assert c.calls == [] and row.weight.wgrad_tn is False
    _knob(False)
    assert calls(col()) == []                            # NXDA_WGRAD_TN=0
    _knob(True, low_thresholds=False)
    assert calls(col()) == []                            # the size gate
    os.environ.pop("NXDA_WGRAD_TN", None)                # default is on
    assert layers._wgrad_tn_enabled()
    w = torch.nn.Parameter(torch.zeros(64, 128, dtype=bf))
    a, b = torch.zeros(48, 64, dtype=bf), torch.zeros(48, 128, dtype=bf)
    with torch.no_grad():
        assert not layers.wgrad_tn_eligible(w, a, b)     # sizes
        _knob(True)
        assert layers.wgrad_tn_eligible(w, a, b)
        assert not layers.wgrad_tn_eligible(w.float(), a, b)
        assert not layers.wgrad_tn_eligible(w, a.float(), b)
        assert not layers.wgrad_tn_eligible(w, a[:44], b[:44])   # 44 % 8
        assert not layers.wgrad_tn_eligible(w, a[:, :60], b)     # 60 % 8
        assert layers.wgrad_tn_eligible(w, a[:, :56], b)   # strided rows ok
        layers._WGRAD_TN_MIN_M = 64
        assert not layers.wgrad_tn_eligible(w, a, b)     # too few tokens
    _knob(True)
    assert not layers.wgrad_tn_eligible(w, a, b)         # grad mode
    # the model's opt-outs
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config

    m = LlamaForCausalLM(get_config("tiny"))
    ids = torch.randint(0, 256, (1, 8))
    m(ids, labels=ids).backward()
    assert m.lm_head.weight.wgrad_tn is False
    for layer in m.model.layers:
        assert layer.mlp.down_proj.weight.wgrad_tn is False
        assert getattr(layer.mlp.gate_up_proj.weight, "wgrad_tn", True)
        assert getattr(layer.self_attn.o_proj.weight, "wgrad_tn", True)
    assert ops._WGRAD_HANDOFF[0] is None
    return True


def test_opt_outs_size_gate_and_double_backward():
    run_distributed(_optout_worker, world_size=1)


def _model_worker(rank, world):
    """Tiny Llama, fused-norm training path, random data, one forward and
    backward with the knob off and on.  There is no exact-integer variant of
    this case: RMSNorm, softmax and the SwiGLU sigmoid leave no integer
    activations in a whole transformer, so bit equality is checked per layer
    (above, and for LlamaMLP / QKV on the GPU) and the model against the
    tolerance measured here."""
    from neuronx_distributed_amd import ops
    from neuronx_distributed_amd.models import LlamaForCausalLM, get_config
    from neuronx_distributed_amd.parallel import layers, qkv_linear
    from neuronx_distributed_amd.parallel import parallel_state as ps

    ps.initialize_model_parallel(tensor_model_parallel_size=1)
    os.environ["NXDA_FUSED_NORM_FORCE"] = "1"
    torch.manual_seed(0)
    model = LlamaForCausalLM(get_config("tiny")).to(bf)
    ids = torch.randint(0, 256, (2, 24))         # 48 tokens

    # the operands of every K-contiguous wgrad of the run, to measure what
    # the order of the reference product is worth on exactly these numbers
    seen, orig = [], layers.wgrad_tn

    def spy(go2d, in2d, go_t=None, in_t=None):
        seen.append((go2d.detach().clone(), in2d.detach().clone()))
        return orig(go2d, in2d, go_t=go_t, in_t=in_t)

    grads = {}
    for on in (False, True):
        _knob(on)
        layers.wgrad_tn = qkv_linear.wgrad_tn = spy
        try:
            with _Count() as c:
                model(ids, labels=ids).backward()
        finally:
            layers.wgrad_tn = qkv_linear.wgrad_tn = orig
        grads[on] = {n: p.grad.clone() for n, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        assert ops._WGRAD_HANDOFF[0] is None
        n_layers = len(model.model.layers)
        # per layer: gate_up (X^T; dx^T handed over), o (2), QKV (4)
        assert sorted(c.calls) == (sorted([1, 2, 4] * n_layers) if on
                                   else []), c.calls
    assert len(seen) == 5 * len(model.model.layers)
    # tolerance: the fp32 product in its two orders, plus one bf16 rounding
    # of the result (an fp32 difference can move the bf16 rounding by an ulp)
    d32 = 0.0
    for go, x in seen:
        nt = go.float().t() @ x.float()
        tn = torch.nn.functional.linear(go.float().t().contiguous(),
                                        x.float().t().contiguous())
        d32 = max(d32, (nt - tn).abs().max().item())
    print(f"fp32 NT vs TN max abs difference over {len(seen)} products: "
          f"{d32:.3g}")
    worst = 0.0
    for n, g0 in grads[False].items():
        g0, g1 = g0.float(), grads[True][n].float()
        assert torch.isfinite(g1).all() and g0.abs().max() > 0, n
        diff = (g1 - g0).abs()
        worst = max(worst, diff.max().item())
        assert diff.le(d32 + 2.0 ** -7 * g0.abs()).all(), (n, diff.max())
    print(f"largest gradient difference knob on vs off: {worst:.3g}")
    return True


def test_full_model_gradients_within_reference_order_tolerance():
    run_distributed(_model_worker, world_size=1)
