"""Megatron-style tensor-parallel NN layers, MI355X-native.

API parity with the reference's ``parallel_layers/layers.py`` (1,604 LoC):
``ColumnParallelLinear`` (:561), ``RowParallelLinear`` (:815),
``ParallelEmbedding`` (:186), ``LinearWithAsyncCommunication`` (:434-504),
deterministic CPU master-weight init (:111-164), ``preshard_hook`` protocol
(:411,770,1015).

MI355X design notes:
* GEMMs go to hipBLASLt via ``F.linear``; the hot fused ops (RMSNorm, RoPE,
  flash attention, cross entropy) are hand-written HIP kernels in
  ``neuronx_distributed_amd.ops``.
* The backward grad-input all-reduce is issued async on RCCL and overlapped
  with the weight-grad GEMM (reference layers_utils.py:91-103) — eager mode
  gives us real overlap, no compiler needed.
* Sequence parallelism: forward all-gathers the (S/tp,B,H) activation along
  dim 0 before the GEMM and backward reduce-scatters the grad, matching
  reference semantics (layers.py:597,856; layers_utils.py:44-140).
"""

import math
import os
from typing import Callable, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.distributed as dist

from . import comm
from . import parallel_state as ps
from .mappings import (
    copy_to_tensor_model_parallel_region,
    gather_from_tensor_model_parallel_region,
    reduce_from_tensor_model_parallel_region,
    reduce_scatter_to_sequence_parallel_region,
    gather_from_sequence_parallel_region,
    scatter_to_tensor_model_parallel_region,
)
from .random import get_rng_state_tracker
from .utils import (
    create_local_weight,
    divide,
    set_tensor_model_parallel_attributes,
    cast_if_autocast_enabled,
)

_PARAMETER_INIT_SEED = 424242


def _init_normal(std):
    def init_(tensor):
        return nn.init.normal_(tensor, mean=0.0, std=std)

    return init_


def default_init_method(tensor):
    return nn.init.kaiming_uniform_(tensor, a=math.sqrt(5))


def _initialize_affine_weight(
    weight: torch.Tensor,
    out_features: int,
    in_features: int,
    per_partition_size: int,
    partition_dim: int,
    init_method: Callable,
    stride: int = 1,
    return_master_weight: bool = False,
    dtype: Optional[torch.dtype] = None,
):
    """Deterministic TP-degree-invariant init (reference layers.py:111-164):
    build the FULL master weight on CPU fp32 with a fixed per-layer seed,
    then slice this rank's shard.  Identical math at any TP degree."""
    world = ps.get_tensor_model_parallel_size()
    set_tensor_model_parallel_attributes(weight, world > 1, partition_dim, stride,
                                         world)
    if ps.is_aot_mode():
        return None  # AOT tracing skips weight init (reference layers.py:138-140)

    if os.environ.get("NXDA_FAST_INIT", "0") == "1":
        # bench/synthetic mode: init the SHARD directly (per-rank RNG, not
        # TP-degree-invariant) — skips the full master-weight materialization
        with torch.no_grad():
            tmp = torch.empty(weight.shape, dtype=torch.float32,
                              device=weight.device)
            init_method(tmp)
            weight.data.copy_(tmp.to(weight.dtype))
        return None

    master = torch.empty(out_features, in_features, dtype=torch.float32,
                         device="cpu", requires_grad=False)
    init_method(master)
    if dtype is not None:
        master = master.to(dtype)
    if world == 1:
        with torch.no_grad():
            weight.data.copy_(master.to(weight.dtype))
        return master if return_master_weight else None
    with torch.no_grad():
        shard = create_local_weight(master, partition_dim, per_partition_size,
                                    stride)
        weight.data.copy_(shard.to(weight.dtype))
    return master if return_master_weight else None


# ---------------------------------------------------------------------------
# Fused forward/backward with async TP communication
# ---------------------------------------------------------------------------

def _sp_overlapped_linear(input_, weight, bias, tp_info):
    """Ring-pipelined SP forward (NXDA_SP_OVERLAP=1): instead of one
    blocking all-gather followed by one GEMM, the TP ranks rotate their
    sequence chunks around the ring with batched isend/irecv while each
    in-hand chunk is GEMMed — every transfer except the first overlaps
    MFMA work, and on xGMI each hop is a single point-to-point link
    (SURVEY §7 hard-parts: fused SP producer; reference
    layers_utils.py:91-103 async-overlap semantics)."""
    world = tp_info.size
    me = tp_info.rank_in_group(dist.get_rank())
    ranks = tp_info.ranks_of(dist.get_rank())
    nxt = ranks[(me + 1) % world]
    prv = ranks[(me - 1) % world]
    S = input_.shape[0]
    src = input_.contiguous()
    cur = src
    recv_buf = torch.empty_like(src)
    # src is SAVED for backward — it may be sent from but never received
    # into, so the rotation uses a second scratch buffer in its place
    spare = torch.empty_like(src)
    out = torch.empty((world * S,) + tuple(input_.shape[1:-1])
                      + (weight.shape[0],),
                      dtype=input_.dtype, device=input_.device)
    for t in range(world):
        owner = (me - t) % world
        works = []
        if t < world - 1:
            ops_ = [dist.P2POp(dist.isend, cur, nxt, group=tp_info.group),
                    dist.P2POp(dist.irecv, recv_buf, prv,
                               group=tp_info.group)]
            works = dist.batch_isend_irecv(ops_)
        out[owner * S:(owner + 1) * S] = F.linear(cur, weight)
        for w in works:
            w.wait()
        if t < world - 1:
            nxt_recv = spare if cur is src else cur
            cur = recv_buf
            recv_buf = nxt_recv
    if bias is not None:
        out = out + bias
    return out


class _RPLOverlappedLinearRS(torch.autograd.Function):
    """RowParallel forward GEMM with the SP reduce-scatter CHUNKED as a
    consumer: the partial output for destination rank c is GEMMed then
    reduced (async) toward c while the next chunk's GEMM runs — the
    reduce-scatter hides under MFMA instead of trailing it (SURVEY §7
    hard-parts: fused SP consumer)."""

    @staticmethod
    def forward(ctx, input_parallel, weight):
        tp_info = ps.get_group_info("tp")
        world = tp_info.size
        me = tp_info.rank_in_group(dist.get_rank())
        ranks = tp_info.ranks_of(dist.get_rank())
        ctx.save_for_backward(input_parallel, weight)
        x = input_parallel.contiguous()
        assert x.shape[0] % world == 0
        Sc = x.shape[0] // world
        handles = []
        chunks = []
        mine = None
        for c in range(world):
            y = F.linear(x[c * Sc:(c + 1) * Sc], weight)
            chunks.append(y)  # keep alive until the reduce drains
            handles.append(dist.reduce(y, dst=ranks[c],
                                       group=tp_info.group, async_op=True))
            if c == me:
                mine = y
        for h in handles:
            h.wait()
        return mine.clone()

    @staticmethod
    def backward(ctx, grad_output):
        input_parallel, weight = ctx.saved_tensors
        tp_info = ps.get_group_info("tp")
        g = comm.all_gather(grad_output.contiguous(), dim=0, group=tp_info)
        grad_input = _dgrad(g, weight)
        go2d = g.reshape(-1, g.shape[-1])
        in2d = input_parallel.reshape(-1, input_parallel.shape[-1])
        grad_weight = go2d.t().matmul(in2d)
        return grad_input, grad_weight


def _fp8_forward_enabled() -> bool:
    return os.environ.get("NXDA_FP8_LINEAR", "0") == "1"


def _fp8_eligible(x: torch.Tensor, w: torch.Tensor) -> bool:
    """fp8 pays ONLY on wide column GEMMs on this hipBLASLt build
    (measured at the training shapes, M=32k: gate_up N=22016/K=4096 runs
    2.2 PF fp8 vs 1.5 bf16; square/row shapes LOSE to the rowwise-scale
    epilogue — profiles/README.md round-2 fp8 notes)."""
    return (x.is_cuda and x.dtype == torch.bfloat16
            and w.dtype == torch.bfloat16
            and x.shape[-1] % 16 == 0 and w.shape[0] % 16 == 0
            and w.shape[0] >= 2 * w.shape[1]
            and x.numel() // x.shape[-1] >= 2048)


# Generation of the parameter VALUES, for caches of tensors derived from a
# weight (fp8 quantization, the fused inference QKV weight).
# ``weight._version`` alone misses the fused optimizer, which updates
# ``flat_param`` through raw pointers: NeuronZero1Optimizer bumps the
# generation in ``_all_gather_params``, the one place where it leaves the
# parameters final (step, load_state_dict, DCP restore).  A write through
# ``weight.data`` moves neither counter (``.data`` is an alias with a
# version counter of its own): code that edits weights that way and relies on
# such a cache calls ``bump_weight_generation()``.
_WEIGHT_GENERATION = [0]


def bump_weight_generation() -> int:
    """Invalidate every cached tensor derived from a weight."""
    _WEIGHT_GENERATION[0] += 1
    return _WEIGHT_GENERATION[0]


def weight_generation() -> int:
    return _WEIGHT_GENERATION[0]


def _weight_cache_key(weight: torch.Tensor):
    return (weight.data_ptr(), weight._version, _WEIGHT_GENERATION[0])


def _fp8_quantized_weight(weight: torch.Tensor):
    """Per-channel e4m3 weight quantization, cached per weight VERSION and
    value generation so the n_micro forward calls of one optimizer step
    quantize once."""
    from ..quantization.quantization_config import (QuantizationConfig,
                                                    QuantizedDtype)
    from ..quantization.quantization_utils import quantize_symmetric

    key = _weight_cache_key(weight)
    cache = getattr(weight, "_fp8_cache", None)
    if cache is None or cache[0] != key:
        cfg = QuantizationConfig(quantized_dtype=QuantizedDtype.F8E4M3,
                                 quantize_activation=True)
        with torch.no_grad():
            qw, ws = quantize_symmetric(weight.detach(), cfg)
        cache = (key, qw, ws)
        weight._fp8_cache = cache
    return cache[1], cache[2]


def _forward_gemm(total_input: torch.Tensor, weight: torch.Tensor, bias):
    """The forward GEMM of the parallel linears.  NXDA_FP8_LINEAR=1 runs
    the wide (gate_up-class) forward GEMMs on the gfx950 fp8 MFMA pipe:
    per-channel e4m3 weight scales (quantized once per optimizer step via
    the version cache) + dynamic per-token activation scales through
    torch._scaled_mm.  The BACKWARD stays bf16 on the saved tensors — only
    the forward activations carry fp8 quantization error, like
    transformer-engine's default training recipe."""
    if _fp8_forward_enabled() and _fp8_eligible(total_input, weight):
        from ..quantization.quantization_utils import fp8_scaled_linear

        qw, ws = _fp8_quantized_weight(weight)
        with torch.no_grad():
            out = fp8_scaled_linear(total_input, qw, ws, total_input.dtype)
        if bias is not None:
            out = out + bias
        return out
    return F.linear(total_input, weight, bias)


def _dgrad_shadow_enabled() -> bool:
    return os.environ.get("NXDA_DGRAD_SHADOW", "1") == "1"


# The transposes cost ~0.1 ms per 4096x4096 weight per backward against a
# GEMM of ~1 ms: below this size the dgrad stays on the strided weight.
_DGRAD_SHADOW_MIN_NUMEL = 4096 * 4096


def _dgrad_shadow_eligible(weight: torch.Tensor) -> bool:
    """Weights whose dgrad runs on W^T: the big GEMMs only (out*in >=
    4096x4096), shapes inside the transpose kernel's contract; a weight opts
    out with ``weight.dgrad_shadow = False`` (the vocabulary projections)."""
    return (weight.dim() == 2 and weight.dtype == torch.bfloat16
            and weight.is_contiguous()
            and weight.numel() >= _DGRAD_SHADOW_MIN_NUMEL
            and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0
            and getattr(weight, "dgrad_shadow", True))


def dgrad_weight_t(weight: torch.Tensor) -> Optional[torch.Tensor]:
    """W^T (in, out) contiguous for the dgrad of ``y = x W^T``, or None when
    the weight keeps the strided form.

    ``dY @ W`` walks W along its strided dimension (hipBLASLt NN class);
    ``F.linear(dY, W^T)`` is the same product with both operands contiguous
    along the contraction (TN class, the forward's), and the library stops
    re-staging W through LDS in every tile.

    W^T is built by ``ops.transpose`` from the weight AS IT IS at this
    backward and dropped after it: nothing is cached, so no write to the
    weight (optimizer kernels on raw pointers, ``weight.data.mul_()``, which
    no version counter sees) can leave a stale copy behind, and nothing is
    attached to the parameter or reaches a checkpoint.  The price is one
    transpose per weight per microbatch (~0.4 % of the Llama-2-7B step, an
    eighth of what the TN product saves; profiles/README.md)."""
    if torch.is_grad_enabled():  # double backward differentiates through W
        return None
    if not (_dgrad_shadow_enabled() and _dgrad_shadow_eligible(weight)):
        return None
    from .. import ops as _ops

    return _ops.transpose(weight.detach())


def _dgrad(grad_output: torch.Tensor, weight: torch.Tensor) -> torch.Tensor:
    """grad_input = grad_output @ W, as a K-contiguous product if eligible."""
    w_t = dgrad_weight_t(weight)
    if w_t is None:
        return grad_output.matmul(weight)
    return F.linear(grad_output, w_t)


def _wgrad_tn_enabled() -> bool:
    return os.environ.get("NXDA_WGRAD_TN", "1") == "1"


# Same floor as the dgrad: the 4096x4096 class and up.
_WGRAD_TN_MIN_NUMEL = 4096 * 4096
# The contraction runs over the tokens.  The K-contiguous form was measured
# at M = 32768 only (profiles/README.md); shorter contractions keep dY^T @ X.
_WGRAD_TN_MIN_M = 16384


def wgrad_tn_weight_eligible(weight: torch.Tensor) -> bool:
    """Weights whose gradient may run K-contiguous: bf16, out*in >=
    4096x4096, both sizes inside the transpose contract; a weight opts out
    with ``weight.wgrad_tn = False`` (down_proj, lm_head)."""
    return (weight.dim() == 2 and weight.dtype == torch.bfloat16
            and weight.numel() >= _WGRAD_TN_MIN_NUMEL
            and weight.shape[0] % 8 == 0 and weight.shape[1] % 8 == 0
            and getattr(weight, "wgrad_tn", True))


def _wgrad_tn_operand_ok(t: torch.Tensor) -> bool:
    """A (tokens, features) operand that ``ops.transpose`` takes: bf16,
    dense rows with a 16-byte-multiple stride and base, tokens >= the
    threshold; on the GPU the native transpose must be there, on the CPU the
    composed fallback stands in for it."""
    if t.dim() != 2 or t.dtype != torch.bfloat16:
        return False
    M, C = t.shape
    if M < _WGRAD_TN_MIN_M or M % 8 or C % 8 or t.stride(1) != 1 \
            or t.stride(0) < C or t.stride(0) % 8 or t.data_ptr() % 16:
        return False
    if t.is_cuda:
        from .. import ops as _ops

        return _ops.transpose_multi_available()
    return True


def wgrad_tn_eligible(weight: torch.Tensor, go2d: torch.Tensor,
                      in2d: torch.Tensor) -> bool:
    """True when ``grad_weight = go2d^T @ in2d`` runs as ``wgrad_tn``."""
    if torch.is_grad_enabled():  # double backward differentiates through it
        return False
    return (_wgrad_tn_enabled() and wgrad_tn_weight_eligible(weight)
            and go2d.device == in2d.device
            and _wgrad_tn_operand_ok(go2d) and _wgrad_tn_operand_ok(in2d))


def wgrad_tn_wants_dxt(x: torch.Tensor) -> bool:
    """Asked by SwiGLU's backward (x = its saved input, the output of the
    gate_up linear): would that linear's wgrad take a dx^T right now?"""
    if not _wgrad_tn_enabled() or x.dtype != torch.bfloat16 \
            or not x.is_contiguous() or x.dim() < 2:
        return False
    C = x.shape[-1]
    M = x.numel() // max(C, 1)
    if M < _WGRAD_TN_MIN_M or M % 8 or C % 16 or x.data_ptr() % 16:
        return False
    if x.is_cuda:
        from .. import ops as _ops

        return (_ops.swiglu_bwd_t_available()
                and _ops.transpose_multi_available())
    return True


def wgrad_tn(go2d: torch.Tensor, in2d: torch.Tensor,
             go_t: Optional[torch.Tensor] = None,
             in_t: Optional[torch.Tensor] = None) -> torch.Tensor:
    """grad_weight (out, in) = go2d^T @ in2d as a K-contiguous product.

    ``go2d.t().matmul(in2d)`` walks both operands along their strided
    dimension (hipBLASLt NT class, a depth-32 tile that re-stages both
    through LDS).  ``F.linear(go_t, in_t)`` with go_t (out, M) and in_t
    (in, M) contiguous is the same product in the forward's TN class.
    Whichever transpose was not handed in is built here, both in one launch
    (``ops.transpose_multi``), and dropped with the call."""
    from .. import ops as _ops

    todo = [t for t, have in ((go2d, go_t), (in2d, in_t)) if have is None]
    if todo:
        built = _ops.transpose_multi(todo)
        if go_t is None:
            go_t = built.pop(0)
        if in_t is None:
            in_t = built.pop(0)
    return F.linear(go_t, in_t)


class LinearWithAsyncCommunication(torch.autograd.Function):
    """F.linear with TP/SP collectives placed for overlap.

    Reference: layers.py:434-504 + layers_utils.py:44-140.  Backward issues
    the grad-input all-reduce (TP) or reduce-scatter (SP) asynchronously and
    overlaps it with the weight-grad GEMM.
    """

    @staticmethod
    def forward(ctx, input_, weight, bias, async_grad_allreduce,
                sequence_parallel_enabled, save_for_backward=True):
        ctx.use_bias = bias is not None
        ctx.async_grad_allreduce = async_grad_allreduce
        ctx.sequence_parallel_enabled = sequence_parallel_enabled
        ctx.compute_weight_gradient = weight.requires_grad

        if sequence_parallel_enabled:
            tp_info = ps.get_group_info("tp")
            if os.environ.get("NXDA_SP_OVERLAP", "0") == "1" and \
                    tp_info.size > 1 and not ps.is_aot_mode():
                output = _sp_overlapped_linear(input_, weight, bias, tp_info)
                if save_for_backward:
                    if ctx.compute_weight_gradient:
                        ctx.save_for_backward(input_, weight)
                    else:
                        ctx.save_for_backward(weight)
                return output
            total_input = comm.all_gather(input_, dim=0, group=tp_info)
        else:
            total_input = input_

        output = _forward_gemm(total_input, weight, bias)

        if save_for_backward:
            if ctx.compute_weight_gradient:
                ctx.save_for_backward(input_, weight)
            else:
                ctx.save_for_backward(weight)
        return output

    @staticmethod
    def backward(ctx, grad_output):
        if ctx.compute_weight_gradient:
            input_, weight = ctx.saved_tensors
        else:
            (weight,) = ctx.saved_tensors
            input_ = None

        tp_info = ps.get_group_info("tp")
        handle = None

        # dx^T left by a SwiGLU backward for exactly this grad_output, or
        # None; taking it empties the slot whatever this backward does next
        from .. import ops as _ops

        go_t = _ops.wgrad_handoff_take(grad_output)
        grad_output = grad_output.contiguous()
        grad_input = _dgrad(grad_output, weight)

        if ctx.sequence_parallel_enabled and ctx.compute_weight_gradient:
            # re-gather the saved sharded input for the weight-grad GEMM
            total_input = comm.all_gather(input_, dim=0, group=tp_info)
        else:
            total_input = input_

        if ctx.sequence_parallel_enabled:
            # reduce-scatter grad_input along seq dim, async over the
            # weight-grad GEMM below
            world = tp_info.size
            if world > 1 and not ps.is_aot_mode():
                gi = grad_input.contiguous()
                sub_shape = (gi.shape[0] // world,) + tuple(gi.shape[1:])
                grad_input_out = torch.empty(sub_shape, dtype=gi.dtype,
                                             device=gi.device)
                if comm._backend_is_gloo(tp_info.group):
                    dist.all_reduce(gi, group=tp_info.group)
                    rank = tp_info.rank_in_group(dist.get_rank())
                    grad_input_out.copy_(gi[rank * sub_shape[0]:(rank + 1) * sub_shape[0]])
                else:
                    handle = dist.reduce_scatter_tensor(
                        grad_input_out, gi, group=tp_info.group, async_op=True)
                grad_input = grad_input_out
        elif ctx.async_grad_allreduce:
            handle = comm.all_reduce(grad_input, group=tp_info, async_op=True)

        grad_weight = grad_bias = None
        if ctx.compute_weight_gradient:
            go2d = grad_output.reshape(-1, grad_output.shape[-1])
            in2d = total_input.reshape(-1, total_input.shape[-1])
            if wgrad_tn_eligible(weight, go2d, in2d):
                grad_weight = wgrad_tn(go2d, in2d, go_t=go_t)
            else:
                grad_weight = go2d.t().matmul(in2d)
            go_t = None  # 1.4 GB at gate_up: gone once its GEMM is issued
            if ctx.use_bias:
                grad_bias = go2d.sum(dim=0)
        elif ctx.use_bias:
            grad_bias = grad_output.reshape(-1, grad_output.shape[-1]).sum(dim=0)

        if handle is not None:
            handle.wait()
        return grad_input, grad_weight, grad_bias, None, None, None


def linear_with_async_allreduce(input_, weight, bias=None,
                                async_grad_allreduce=False,
                                sequence_parallel_enabled=False):
    from .. import ops as _ops

    if _ops.use_skinny_linear(input_, weight, sequence_parallel_enabled):
        # decode fast path: M <= 32 tokens, inference — the split-K
        # weight-streaming HIP kernel instead of hipBLASLt skinny kernels
        flat = input_.reshape(-1, input_.shape[-1]).contiguous()
        out = _ops.skinny_linear(flat, weight)
        if bias is not None:
            out = out + bias
        return out.reshape(*input_.shape[:-1], weight.shape[0])
    args = cast_if_autocast_enabled(input_, weight, bias)
    with torch.amp.autocast("cuda", enabled=False):
        return LinearWithAsyncCommunication.apply(
            *args, async_grad_allreduce, sequence_parallel_enabled)


class BaseParallelLinear(nn.Module):
    def reset_parameters(self):
        """Re-run the deterministic TP-invariant init (meta-device
        materialization path, utils/model_utils.reinit_model)."""
        spec = getattr(self, "_reset_spec", None)
        if spec is None:
            return
        out_f, in_f, per_part, pdim, stride, init_method, dtype = spec
        _initialize_affine_weight(self.weight, out_f, in_f, per_part,
                                  partition_dim=pdim, init_method=init_method,
                                  stride=stride, dtype=dtype)
        if getattr(self, "bias", None) is not None:
            with torch.no_grad():
                self.bias.zero_()

    def _init_weight(self, weight, init_method):
        if getattr(weight, "device", torch.device("cpu")).type == "meta":
            return
        with get_rng_state_tracker().fork():
            init_method(weight)

    def preshard_hook(self, model_state_dict: dict, prefix: str) -> None:
        """Slice a full checkpoint weight into this rank's shard in-place
        (reference layers.py:411,770,1015 — part of the sharded-checkpoint
        contract)."""
        name = prefix.rsplit(".", 1)[0] if prefix.endswith("weight") else prefix
        for pname, param in self.named_parameters():
            key = f"{name}.{pname}" if not prefix.endswith(pname) else prefix
            if key not in model_state_dict:
                continue
            full = model_state_dict[key]
            pdim = getattr(param, "partition_dim", -1)
            if pdim < 0 or not getattr(param, "tensor_model_parallel", False):
                continue
            if full.shape[pdim] == param.shape[pdim]:
                continue  # already sharded
            model_state_dict[key] = create_local_weight(
                full, pdim, param.shape[pdim], getattr(param, "partition_stride", 1))


class ColumnParallelLinear(BaseParallelLinear):
    """Y = XW^T + b with W sharded along the output dim (reference
    layers.py:561).  ``gather_output`` all-gathers the (.., out/tp) shards;
    ``sequence_parallel_enabled`` all-gathers the seq-sharded input in fwd
    and reduce-scatters its grad in bwd."""

    def __init__(self, input_size, output_size, bias=True, gather_output=True,
                 dtype=None, device=None, init_method=None, stride=1,
                 sequence_parallel_enabled=False, keep_master_weight=False,
                 skip_bias_add=False, dgrad_shadow=True, wgrad_tn=True):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.gather_output = gather_output
        # False: the dgrad stays on the strided weight (vocabulary
        # projections: no gain at 32000x4096, profiles/README.md)
        self.dgrad_shadow = dgrad_shadow
        # False: the wgrad stays dY^T @ X (wgrad_tn_weight_eligible)
        self.wgrad_tn = wgrad_tn
        self.sequence_parallel_enabled = sequence_parallel_enabled
        self.skip_bias_add = skip_bias_add
        self.stride = stride
        world = ps.get_tensor_model_parallel_size()
        self.output_size_per_partition = divide(output_size, world)
        dtype = dtype or torch.get_default_dtype()
        self.dtype = dtype
        init_method = init_method or default_init_method

        self.weight = nn.Parameter(
            torch.empty(self.output_size_per_partition, input_size, dtype=dtype,
                        device=device))
        self._reset_spec = (output_size, input_size,
                            self.output_size_per_partition, 0, stride,
                            init_method, dtype)
        self.master_weight = _initialize_affine_weight(
            self.weight, output_size, input_size, self.output_size_per_partition,
            partition_dim=0, init_method=init_method, stride=stride,
            return_master_weight=keep_master_weight, dtype=dtype)

        if bias:
            self.bias = nn.Parameter(
                torch.zeros(self.output_size_per_partition, dtype=dtype,
                            device=device))
            set_tensor_model_parallel_attributes(self.bias, world > 1, 0, stride,
                                                 world)
        else:
            self.register_parameter("bias", None)

        self.async_tensor_model_parallel_allreduce = (
            not sequence_parallel_enabled and world > 1)

    def forward(self, input_):
        if self.async_tensor_model_parallel_allreduce or self.sequence_parallel_enabled:
            input_parallel = input_
        else:
            input_parallel = copy_to_tensor_model_parallel_region(input_)

        bias = self.bias if not self.skip_bias_add else None
        if not self.dgrad_shadow:
            # marked here, not at construction: weight tying replaces the
            # Parameter object after __init__
            self.weight.dgrad_shadow = False
        if not self.wgrad_tn:
            self.weight.wgrad_tn = False
        output_parallel = linear_with_async_allreduce(
            input_parallel, self.weight, bias,
            async_grad_allreduce=self.async_tensor_model_parallel_allreduce,
            sequence_parallel_enabled=self.sequence_parallel_enabled)

        if self.gather_output:
            output = gather_from_tensor_model_parallel_region(output_parallel)
        else:
            output = output_parallel
        if self.skip_bias_add:
            return output, self.bias
        return output


class RowParallelLinear(BaseParallelLinear):
    """Y = XW^T + b with W sharded along the input dim (reference
    layers.py:815).  Output is all-reduced over TP, or reduce-scattered
    along seq when ``sequence_parallel_enabled``."""

    def __init__(self, input_size, output_size, bias=True,
                 input_is_parallel=True, dtype=None, device=None,
                 init_method=None, stride=1, sequence_parallel_enabled=False,
                 keep_master_weight=False, skip_bias_add=False,
                 reduce_output=True, wgrad_tn=True):
        super().__init__()
        self.input_size = input_size
        self.output_size = output_size
        self.input_is_parallel = input_is_parallel
        # False: the wgrad stays dY^T @ X (wgrad_tn_weight_eligible)
        self.wgrad_tn = wgrad_tn
        self.sequence_parallel_enabled = sequence_parallel_enabled
        self.skip_bias_add = skip_bias_add
        self.reduce_output = reduce_output
        world = ps.get_tensor_model_parallel_size()
        self.input_size_per_partition = divide(input_size, world)
        dtype = dtype or torch.get_default_dtype()
        self.dtype = dtype
        init_method = init_method or default_init_method

        self.weight = nn.Parameter(
            torch.empty(output_size, self.input_size_per_partition, dtype=dtype,
                        device=device))
        self._reset_spec = (output_size, input_size,
                            self.input_size_per_partition, 1, stride,
                            init_method, dtype)
        self.master_weight = _initialize_affine_weight(
            self.weight, output_size, input_size, self.input_size_per_partition,
            partition_dim=1, init_method=init_method, stride=stride,
            return_master_weight=keep_master_weight, dtype=dtype)

        if bias:
            self.bias = nn.Parameter(torch.zeros(output_size, dtype=dtype,
                                                 device=device))
        else:
            self.register_parameter("bias", None)

    def forward(self, input_):
        if self.input_is_parallel:
            input_parallel = input_
        else:
            input_parallel = scatter_to_tensor_model_parallel_region(input_)

        if (self.sequence_parallel_enabled and self.reduce_output
                and os.environ.get("NXDA_SP_OVERLAP", "0") == "1"
                and ps.get_tensor_model_parallel_size() > 1
                and not ps.is_aot_mode()
                and not isinstance(input_parallel, torch.fx.Proxy)):
            return self._forward_sp_overlapped(input_parallel)

        if not self.wgrad_tn:
            self.weight.wgrad_tn = False
        output_parallel = linear_with_async_allreduce(
            input_parallel, self.weight, None,
            async_grad_allreduce=False, sequence_parallel_enabled=False)

        if not self.reduce_output:
            output = output_parallel
        elif self.sequence_parallel_enabled:
            output = reduce_scatter_to_sequence_parallel_region(output_parallel,
                                                                seq_dim=0)
        else:
            output = reduce_from_tensor_model_parallel_region(output_parallel)

        if self.skip_bias_add:
            return output, self.bias
        if self.bias is not None:
            output = output + self.bias
        return output

    def _forward_sp_overlapped(self, input_parallel):
        output = _RPLOverlappedLinearRS.apply(input_parallel, self.weight)

        if self.skip_bias_add:
            return output, self.bias
        if self.bias is not None:
            output = output + self.bias
        return output


class ParallelEmbedding(BaseParallelLinear):
    """Embedding sharded over TP (reference layers.py:186,334-431).

    Default: VOCAB-dim shard — out-of-shard ids are masked to 0, looked
    up locally, masked out, and the partial embeddings all-reduced (or
    reduce-scattered along seq when sequence-parallel).
    ``shard_along_embedding=True``: EMBEDDING-dim shard — every rank
    holds the full vocab over H/tp columns; the local lookup is
    all-gathered along the last dim."""

    def __init__(self, num_embeddings, embedding_dim, init_method=None,
                 dtype=None, device=None, padding_idx=None,
                 sequence_parallel_enabled=False, shard_along_embedding=False,
                 pad=False):
        super().__init__()
        self.num_embeddings = num_embeddings
        self.embedding_dim = embedding_dim
        self.padding_idx = padding_idx
        self.sequence_parallel_enabled = sequence_parallel_enabled
        self.shard_along_embedding = shard_along_embedding
        world = ps.get_tensor_model_parallel_size()
        tp_rank = ps.get_tensor_model_parallel_rank()
        dtype = dtype or torch.get_default_dtype()
        init_method = init_method or _init_normal(1.0)

        if shard_along_embedding:
            self.embedding_dim_per_partition = divide(embedding_dim, world)
            self.num_embeddings_per_partition = num_embeddings
            self.start_index = 0
            self.end_index = num_embeddings
            self.weight = nn.Parameter(
                torch.empty(num_embeddings, self.embedding_dim_per_partition,
                            dtype=dtype, device=device))
            self._reset_spec = (num_embeddings, embedding_dim,
                                self.embedding_dim_per_partition, 1, 1,
                                init_method, dtype)
            _initialize_affine_weight(
                self.weight, num_embeddings, embedding_dim,
                self.embedding_dim_per_partition, partition_dim=1,
                init_method=init_method, dtype=dtype)
            return
        self.num_embeddings_per_partition = divide(num_embeddings, world)
        self.start_index = tp_rank * self.num_embeddings_per_partition
        self.end_index = self.start_index + self.num_embeddings_per_partition

        self.weight = nn.Parameter(
            torch.empty(self.num_embeddings_per_partition, embedding_dim,
                        dtype=dtype, device=device))
        self._reset_spec = (num_embeddings, embedding_dim,
                            self.num_embeddings_per_partition, 0, 1,
                            init_method, dtype)
        _initialize_affine_weight(
            self.weight, num_embeddings, embedding_dim,
            self.num_embeddings_per_partition, partition_dim=0,
            init_method=init_method, dtype=dtype)

    def forward(self, input_):
        world = ps.get_tensor_model_parallel_size()
        if self.shard_along_embedding:
            local = F.embedding(input_, self.weight,
                                padding_idx=self.padding_idx)
            if world == 1:
                return local
            return gather_from_tensor_model_parallel_region(local)
        if world > 1:
            input_mask = (input_ >= self.start_index) & (input_ < self.end_index)
            masked_input = (input_ - self.start_index) * input_mask
            output_parallel = F.embedding(masked_input, self.weight,
                                          padding_idx=self.padding_idx)
            output_parallel = output_parallel * input_mask.unsqueeze(-1).to(
                output_parallel.dtype)
        else:
            output_parallel = F.embedding(input_, self.weight,
                                          padding_idx=self.padding_idx)
        if world == 1:
            return output_parallel
        if self.sequence_parallel_enabled:
            # (B,S,H) -> transpose handled by caller convention: we use seq
            # dim 0 layout (S,B,H) for SP, matching the reference.
            return reduce_scatter_to_sequence_parallel_region(output_parallel,
                                                              seq_dim=0)
        return reduce_from_tensor_model_parallel_region(output_parallel)


class SPMDRank(nn.Module):
    """Holds this rank's id as a tensor so AOT-traced graphs can be rank
    polymorphic (reference layers.py:1543-1602)."""

    def __init__(self, world_size: int):
        super().__init__()
        self.world_size = world_size
        rank = ps.get_tensor_model_parallel_rank() if ps.model_parallel_is_initialized() else 0
        self.rank = nn.Parameter(torch.tensor([rank], dtype=torch.int32),
                                 requires_grad=False)

    def get_rank(self) -> torch.Tensor:
        return self.rank
