"""Llama-2/3 model family on the MI355X parallel layers.

The model-zoo equivalent of the reference's
``examples/training/llama/modeling_llama_nxd.py`` (ParallelEmbedding +
GQAQKVColumnParallelLinear + Row/ColumnParallel MLP + parallel CE), built
MI355X-first:

* hot ops (RMSNorm, RoPE, SwiGLU, flash attention) are HIP kernels
  (``neuronx_distributed_amd.ops``), everything GEMM-shaped is hipBLASLt
  via F.linear;
* gate/up projections are ONE fused stride-2 ColumnParallel GEMM;
* layout is (B,S,H); with sequence parallelism the activations between TP
  regions are (S/tp,B,H) (seq dim 0), matching the reference's SP design.
"""

import math
import os
from dataclasses import dataclass, field
from typing import Optional

import torch
import torch.nn as nn

from .. import ops
from ..parallel import parallel_state as ps
from ..parallel.layers import (
    ColumnParallelLinear,
    RowParallelLinear,
    ParallelEmbedding,
    wgrad_tn_weight_eligible,
)
from ..parallel.qkv_linear import GQAQKVColumnParallelLinear
from ..parallel.loss_functions import parallel_cross_entropy

# fx.wrap patches name lookups in THIS module's globals (the defining
# module's wrap does not cover imported references) so the pipeline tracer
# treats the collective-bearing loss as a leaf call
torch.fx.wrap("parallel_cross_entropy")
from ..parallel.mappings import (
    scatter_to_sequence_parallel_region,
    gather_from_sequence_parallel_region,
)
from ..kernels.flash_attn import flash_attn_func


@dataclass
class LlamaConfig:
    hidden_size: int = 4096
    intermediate_size: int = 11008
    num_hidden_layers: int = 32
    num_attention_heads: int = 32
    num_key_value_heads: int = 32
    vocab_size: int = 32000
    max_position_embeddings: int = 4096
    rope_theta: float = 10000.0
    rms_norm_eps: float = 1e-5
    initializer_range: float = 0.02
    sequence_parallel_enabled: bool = False
    tie_word_embeddings: bool = False
    # set by pad_llama_config: padded head counts keep the ORIGINAL head
    # size (hidden_size // original_num_heads)
    head_dim_override: Optional[int] = None
    # Mistral-style sliding-window attention (None = full causal).
    # Training AND inference run on the windowed MFMA flash kernels
    # (band-limited fwd/dkdv/dq); window >= seq short-circuits to plain
    # causal.
    sliding_window: Optional[int] = None
    # Qwen-2 style QKV bias
    attention_bias: bool = False
    # llama-3.1 style long-context RoPE scaling dict (rope_type
    # "llama3": factor / low_freq_factor / high_freq_factor /
    # original_max_position_embeddings), or {"rope_type": "linear", ...}
    rope_scaling: Optional[dict] = None
    # >0: compute lm_head+CE in this many sequence chunks under
    # checkpointing (caps logits memory; utils/chunked_loss.py)
    loss_chunks: int = 0

    @property
    def head_dim(self):
        if self.head_dim_override is not None:
            return self.head_dim_override
        return self.hidden_size // self.num_attention_heads


CONFIGS = {
    "llama2-7b": LlamaConfig(),
    "llama2-13b": LlamaConfig(hidden_size=5120, intermediate_size=13824,
                              num_hidden_layers=40, num_attention_heads=40,
                              num_key_value_heads=40),
    "llama2-70b": LlamaConfig(hidden_size=8192, intermediate_size=28672,
                              num_hidden_layers=80, num_attention_heads=64,
                              num_key_value_heads=8),
    "llama3-8b": LlamaConfig(hidden_size=4096, intermediate_size=14336,
                             num_hidden_layers=32, num_attention_heads=32,
                             num_key_value_heads=8, vocab_size=128256,
                             rope_theta=500000.0,
                             max_position_embeddings=8192),
    "mistral-7b": LlamaConfig(hidden_size=4096, intermediate_size=14336,
                              num_hidden_layers=32, num_attention_heads=32,
                              num_key_value_heads=8, vocab_size=32000,
                              sliding_window=4096,
                              max_position_embeddings=8192),
    "qwen2-7b": LlamaConfig(hidden_size=3584, intermediate_size=18944,
                            num_hidden_layers=28, num_attention_heads=28,
                            num_key_value_heads=4, vocab_size=152064,
                            rope_theta=1e6, attention_bias=True,
                            max_position_embeddings=8192),
    "llama3.1-8b": LlamaConfig(hidden_size=4096, intermediate_size=14336,
                               num_hidden_layers=32, num_attention_heads=32,
                               num_key_value_heads=8, vocab_size=128256,
                               rope_theta=500000.0,
                               max_position_embeddings=131072,
                               rope_scaling={
                                   "rope_type": "llama3", "factor": 8.0,
                                   "low_freq_factor": 1.0,
                                   "high_freq_factor": 4.0,
                                   "original_max_position_embeddings": 8192,
                               }),
    "llama3-70b": LlamaConfig(hidden_size=8192, intermediate_size=28672,
                              num_hidden_layers=80, num_attention_heads=64,
                              num_key_value_heads=8, vocab_size=128256,
                              rope_theta=500000.0,
                              max_position_embeddings=8192),
    "test-d128": LlamaConfig(hidden_size=512, intermediate_size=1024,
                             num_hidden_layers=2, num_attention_heads=4,
                             num_key_value_heads=2, vocab_size=1024,
                             max_position_embeddings=512),
    "tiny": LlamaConfig(hidden_size=64, intermediate_size=128,
                        num_hidden_layers=2, num_attention_heads=4,
                        num_key_value_heads=2, vocab_size=256,
                        max_position_embeddings=128, rms_norm_eps=1e-5),
}


def get_config(name: str, **overrides) -> LlamaConfig:
    import dataclasses

    cfg = dataclasses.replace(CONFIGS[name], **overrides)
    return cfg


class RMSNorm(nn.Module):
    """Reference modules/rms_norm.py parity; HIP-fused on GPU."""

    def __init__(self, hidden_size, eps=1e-6, sequence_parallel_enabled=False):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(hidden_size))
        self.variance_epsilon = eps
        self.sequence_parallel_enabled = sequence_parallel_enabled
        self.weight.sequence_parallel_enabled = sequence_parallel_enabled

    def reset_parameters(self):
        with torch.no_grad():
            self.weight.fill_(1.0)

    def forward(self, x):
        return ops.rmsnorm(x, self.weight, self.variance_epsilon)


def _init_method(std):
    def f(t):
        return nn.init.normal_(t, mean=0.0, std=std)

    return f


class LlamaAttention(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        tp = ps.get_tensor_model_parallel_size()
        self.head_dim = config.head_dim
        # shared by the MoE/other families whose configs lack the field
        self.sliding_window = getattr(config, "sliding_window", None)
        kv_mult = max(1, tp // config.num_key_value_heads)
        self.kv_mult = kv_mult
        self.num_heads_local = config.num_attention_heads // tp
        self.num_kv_local = config.num_key_value_heads * kv_mult // tp
        sp = config.sequence_parallel_enabled

        self.qkv_proj = GQAQKVColumnParallelLinear(
            config.hidden_size,
            [config.num_attention_heads * self.head_dim,
             config.num_key_value_heads * self.head_dim],
            bias=getattr(config, "attention_bias", False),
            gather_output=False,
            num_attention_heads=config.num_attention_heads,
            num_key_value_heads=config.num_key_value_heads,
            head_dim=self.head_dim, kv_size_multiplier=kv_mult,
            sequence_parallel_enabled=sp,
            init_method=_init_method(config.initializer_range))
        self.o_proj = RowParallelLinear(
            config.num_attention_heads * self.head_dim, config.hidden_size,
            bias=False, input_is_parallel=True, sequence_parallel_enabled=sp,
            init_method=_init_method(config.initializer_range))

    def forward(self, hidden, cos, sin, pos_offset=0, kv_cache=None):
        sp = self.config.sequence_parallel_enabled
        q, k, v = self.qkv_proj(hidden)
        if sp:
            # (S,B,*) -> (B,S,*)
            q, k, v = (t.transpose(0, 1) for t in (q, k, v))
        B, S = q.shape[0], q.shape[1]
        q = q.reshape(B, S, self.num_heads_local, self.head_dim)
        k = k.reshape(B, S, self.num_kv_local, self.head_dim)
        v = v.reshape(B, S, self.num_kv_local, self.head_dim)
        if isinstance(pos_offset, torch.Tensor):
            # hipGraph-capturable decode: device-tensor position, S == 1
            # (or a chunk of 2..8 tokens: speculative verification),
            # full-cache masked attention (no dynamic shapes)
            if not 1 <= S <= 8:
                raise ValueError(
                    f"a device-tensor position takes 1..8 tokens per "
                    f"forward, got {S}; use an int position for a longer "
                    f"chunk")
            return self._cached_step(q, k, v, cos, sin, pos_offset, kv_cache,
                                     sp)
        q, k = ops.apply_rotary_pos_emb(q, k, cos, sin, pos_offset)

        # (B,S,h,D) -> (B,h,S,D)
        q = q.transpose(1, 2)
        k = k.transpose(1, 2)
        v = v.transpose(1, 2)
        if kv_cache is not None:
            k, v = kv_cache.update(k, v, pos_offset)
        if kv_cache is None and not isinstance(pos_offset, torch.Tensor) \
                and ps.get_context_model_parallel_size() > 1:
            # context parallelism: q/k/v are this rank's contiguous S/cp
            # slice (utils.batch_utils); K/V ring-rotate over the CP group
            from ..kernels.ring_attn import ring_attn_func

            out = ring_attn_func(q, k, v, causal=True,
                                 window=self.sliding_window)
        else:
            out = flash_attn_func(q, k, v, causal=True,
                                  window=self.sliding_window)
        out = out.transpose(1, 2).reshape(B, S, -1)
        if sp:
            out = out.transpose(0, 1)
        return self.o_proj(out)

    def _cached_step(self, q, k, v, cos, sin, pos_t, kv_cache, sp):
        """S = 1..8 new tokens at the device position ``pos_t`` (shape (1,)):
        token t is roped at pos + t, written to cache row pos + t and attends
        rows [0, pos + t].  Everything derives from the device tensor, so the
        whole step can be captured in a hipGraph and replayed with only
        memory updates between steps.

        On GPU with D=128 the whole chain (RoPE + cache append +
        flash-decode + GQA) is fused HIP, chosen by S and the cache's type:
        ops.decode_attn_step / ops.chunk_attn_step for a plain bf16 KVCache,
        ops.decode_attn_mx_step / ops.chunk_attn_mx_step for an MXKVCache.
        Any other cache, and the CPU and odd shapes, take the torch chain
        below (the reference).

        ``pos_t`` with B > 1 elements is one position per sequence (the
        ragged step): sequence b's tokens sit at pos_t[b] + t and attend its
        own rows.  It is fused under the same conditions where
        ops.ragged_attn_enabled().  A sequence with pos_t[b] < 0 or
        pos_t[b] + S beyond the cache is inactive: its cache rows stay and
        its attention output is zero on both paths."""
        from ..inference.kv_cache import KVCache, MXKVCache

        B, S = q.shape[0], q.shape[1]
        ragged = B > 1 and pos_t.numel() == B
        if not ragged and pos_t.numel() != 1:
            raise ValueError(
                f"a device-tensor position holds one element, or one per "
                f"sequence ({B}), got {tuple(pos_t.shape)}")
        rep = self.num_heads_local // self.num_kv_local
        scale = 1.0 / math.sqrt(self.head_dim)
        mx = type(kv_cache) is MXKVCache
        fusable = (q.is_cuda and self.head_dim == 128 and rep in (1, 2, 4, 8)
                   and q.dtype == torch.bfloat16
                   and self.sliding_window is None
                   and (mx or (type(kv_cache) is KVCache
                               and kv_cache.k.dtype == torch.bfloat16))
                   and kv_cache.k.is_cuda)
        if fusable:  # ops.* looked up per call: the tests patch them
            if S == 1:
                fusable = (ops.decode_attn_mx_available() if mx
                           else ops.decode_attn_available())
                step = ops.decode_attn_mx_step if mx else ops.decode_attn_step
            else:
                fusable = (ops.chunk_attn_mx_available() if mx
                           else ops.chunk_attn_available())
                step = ops.chunk_attn_mx_step if mx else ops.chunk_attn_step
            if ragged:
                fusable = fusable and ops.ragged_attn_enabled()
        if fusable:
            if S == 1:
                def _flat(t):
                    # (B,1,h,D) -> (B, h*D) as a VIEW even for fused-QKV
                    # slices (batch stride may exceed h*D; decode_attn takes
                    # strides)
                    t = t.squeeze(1)
                    f = t.reshape(B, -1)
                    return f if f.stride(1) == 1 \
                        else t.contiguous().view(B, -1)
            else:
                def _flat(t):
                    # (B,S,h,D) -> (B,S,h*D) as a VIEW of a fused-QKV slice
                    # where its strides allow (the kernels take row strides)
                    f = t.reshape(B, S, -1)
                    ok = (f.stride(2) == 1 and f.stride(1) >= f.shape[2]
                          and f.stride(0) % 8 == 0 and f.stride(1) % 8 == 0
                          and f.data_ptr() % 16 == 0)
                    return f if ok else f.contiguous()

            qf, kf, vf = _flat(q), _flat(k), _flat(v)
            if S > 1 and kf.stride() != vf.stride():
                kf, vf = kf.contiguous(), vf.contiguous()
            bufs = (kv_cache.k, kv_cache.k_scale, kv_cache.v,
                    kv_cache.v_scale) if mx else (kv_cache.k, kv_cache.v)
            if ragged:
                out = step(qf, kf, vf, *bufs, cos, sin,
                           pos_t.reshape(B).contiguous(),
                           self.num_heads_local, self.num_kv_local, scale,
                           ragged=True)
            else:
                out = step(qf, kf, vf, *bufs, cos, sin, pos_t.reshape(1),
                           self.num_heads_local, self.num_kv_local, scale)
            if S == 1:
                out = out.unsqueeze(1)  # (B, 1, H*D)
            if sp:
                out = out.transpose(0, 1)
            return self.o_proj(out)
        half = self.head_dim // 2
        if ragged:
            if hasattr(kv_cache, "position_index"):
                raise NotImplementedError(
                    "per-sequence positions need a plain cache, not a "
                    "rolling one")
            Smax = kv_cache.k.shape[2]
            pos_b = pos_t.reshape(B, 1)
            active = (pos_b >= 0) & (pos_b + S <= Smax)       # (B, 1)
            tpos = pos_b + torch.arange(S, device=q.device)   # (B, S)
            if cos.shape[0] < Smax:
                raise ValueError(
                    f"the RoPE table ({cos.shape[0]} rows) must cover the "
                    f"cache ({Smax} rows)")
            # an inactive sequence ropes at row 0; its output is zeroed below
            rows = torch.where(active, tpos, 0).reshape(-1)
            c = cos.index_select(0, rows).view(B, S, 1, half)
            s = sin.index_select(0, rows).view(B, S, 1, half)
            tq = tpos.view(B, 1, 1, S, 1)   # against (B,Hkv,rep,S,Smax)
        else:
            tpos = pos_t.reshape(1) + torch.arange(S, device=q.device)  # (S,)
            c = cos.index_select(0, tpos).view(1, S, 1, half)
            s = sin.index_select(0, tpos).view(1, S, 1, half)
            tq = tpos.view(S, 1)

        def rope(x):
            x0 = x[..., :half].float()
            x1 = x[..., half:].float()
            return torch.cat([x0 * c - x1 * s, x1 * c + x0 * s],
                             dim=-1).to(x.dtype)

        q = rope(q).transpose(1, 2)  # (B,h,S,D)
        k = rope(k).transpose(1, 2)
        v = v.transpose(1, 2)
        K, V = kv_cache.update(k, v, pos_t)  # FULL (B,Hkv,Smax,D) buffers
        if K.dtype != q.dtype:  # a cache kept in another dtype than the model
            K, V = K.to(q.dtype), V.to(q.dtype)
        Smax = K.shape[2]
        # bf16 batched GEMM against the cache (fp32 accumulation inside the
        # GEMM; casting K/V to fp32 would re-materialize the whole cache
        # every step): (B,Hkv,rep*S,D) -> (B,Hkv,rep,S,Smax)
        qg = q.reshape(B, self.num_kv_local, rep * S, self.head_dim)
        scores = (qg @ K.transpose(-1, -2)).float() * scale
        scores = scores.view(B, self.num_kv_local, rep, S, Smax)
        if hasattr(kv_cache, "position_index"):
            # rolling window cache (S == 1, its update refuses more): slots
            # carry their GLOBAL position, -1 = unwritten
            idx = kv_cache.position_index().view(1, Smax)
            invalid = (idx > tq) | (idx < 0)  # (S, Smax)
        else:
            idx = torch.arange(Smax, device=q.device).view(1, Smax)
            invalid = idx > tq
        if self.sliding_window is not None:
            invalid = invalid | (idx <= tq - self.sliding_window)
        if ragged:
            # an inactive sequence at a negative position would mask every
            # row: let it see row 0, its output is zeroed anyway
            invalid = invalid & ~((idx == 0) & ~active.view(B, 1, 1, 1, 1))
        scores = scores.masked_fill(invalid, float("-inf"))
        probs = torch.softmax(scores, dim=-1).to(q.dtype)
        out = probs.view(B, self.num_kv_local, rep * S, Smax) @ V
        out = out.view(B, self.num_heads_local, S, self.head_dim)
        out = out.transpose(1, 2).reshape(B, S, -1)
        if ragged:
            # exact zeros, whatever the stale rows of the sequence hold
            out = torch.where(active.view(B, 1, 1), out, 0)
        if sp:
            out = out.transpose(0, 1)
        return self.o_proj(out)


class LlamaMLP(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        sp = config.sequence_parallel_enabled
        # fused [gate; up] stride-2 column-parallel GEMM
        self.gate_up_proj = ColumnParallelLinear(
            config.hidden_size, 2 * config.intermediate_size, bias=False,
            gather_output=False, stride=2, sequence_parallel_enabled=sp,
            init_method=_init_method(config.initializer_range))
        # wgrad_tn=False: at M = 32768 the K-contiguous wgrad of the
        # 4096 x 11008 output LOSES (transposes 0.114 + 0.298 + TN 2.871 =
        # 3.284 ms against NT 3.074 ms, ratio 1.068; profiles/README.md)
        self.down_proj = RowParallelLinear(
            config.intermediate_size, config.hidden_size, bias=False,
            input_is_parallel=True, sequence_parallel_enabled=sp,
            wgrad_tn=False,
            init_method=_init_method(config.initializer_range))

    def forward(self, x):
        # the SwiGLU backward holds dx in registers: it also writes dx^T for
        # the gate_up weight gradient when that one runs K-contiguous
        # (a wrapped gate_up_proj, LoRA or quantized, keeps the plain kernel)
        gu = self.gate_up_proj
        return self.down_proj(ops.swiglu(
            gu(x), wgrad_dxt=(type(gu) is ColumnParallelLinear
                              and wgrad_tn_weight_eligible(gu.weight))))


def fused_norm_train_ok(config, hidden, training=True) -> bool:
    """Gate for the fused residual+RMSNorm TRAINING path.  True when the
    fused autograd op applies: training under grad, bf16 CUDA rows with
    H % 8 == 0 and the kernel built.  NXDA_FUSED_NORM=0 disables;
    NXDA_FUSED_NORM_FORCE=1 bypasses the cuda/bf16/kernel checks so CPU
    tests can exercise the fused wiring via the op's composed fallback."""
    if isinstance(hidden, torch.fx.Proxy):
        return False
    if not training or not torch.is_grad_enabled():
        return False
    if os.environ.get("NXDA_FUSED_NORM", "1") != "1":
        return False
    if config.hidden_size % 8 != 0:
        return False
    if os.environ.get("NXDA_FUSED_NORM_FORCE", "0") == "1":
        return True
    return (hidden.is_cuda and hidden.dtype == torch.bfloat16
            and ops.add_rmsnorm_train_available())


class LlamaDecoderLayer(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        sp = config.sequence_parallel_enabled
        self.self_attn = LlamaAttention(config)
        self.mlp = LlamaMLP(config)
        self.input_layernorm = RMSNorm(config.hidden_size, config.rms_norm_eps,
                                       sequence_parallel_enabled=sp)
        self.post_attention_layernorm = RMSNorm(
            config.hidden_size, config.rms_norm_eps,
            sequence_parallel_enabled=sp)

    def forward(self, hidden, cos, sin, pos_offset=0, kv_cache=None):
        h = hidden + self.self_attn(self.input_layernorm(hidden), cos, sin,
                                    pos_offset, kv_cache)
        return h + self.mlp(self.post_attention_layernorm(h))

    def forward_fused(self, residual, delta, cos, sin, pos_offset, kv_cache):
        """Inference path carrying (residual, delta) so every residual-add
        fuses into the next RMSNorm (ops.add_rmsnorm): 2 elementwise kernels
        per layer instead of 4.  hidden == residual + delta."""
        if delta is None:
            normed = self.input_layernorm(residual)
        else:
            residual, normed = ops.add_rmsnorm(
                residual, delta, self.input_layernorm.weight,
                self.input_layernorm.variance_epsilon)
        attn_out = self.self_attn(normed, cos, sin, pos_offset, kv_cache)
        residual, normed2 = ops.add_rmsnorm(
            residual, attn_out, self.post_attention_layernorm.weight,
            self.post_attention_layernorm.variance_epsilon)
        return residual, self.mlp(normed2)

    def forward_fused_train(self, residual, delta, cos, sin, pos_offset=0):
        """Training twin of ``forward_fused``: the residual add fuses into
        the next RMSNorm through the autograd op (ops.add_rmsnorm_train),
        whose backward folds the residual fork's pass-through gradient
        into the RMSNorm backward kernel — each residual site costs one
        kernel per direction instead of norm + eager add."""
        if delta is None:
            normed = self.input_layernorm(residual)
        else:
            residual, normed = ops.add_rmsnorm_train(
                delta, residual, self.input_layernorm.weight,
                self.input_layernorm.variance_epsilon)
        attn_out = self.self_attn(normed, cos, sin, pos_offset, None)
        residual, normed2 = ops.add_rmsnorm_train(
            attn_out, residual, self.post_attention_layernorm.weight,
            self.post_attention_layernorm.variance_epsilon)
        return residual, self.mlp(normed2)


class LlamaModel(nn.Module):
    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.embed_tokens = ParallelEmbedding(
            config.vocab_size, config.hidden_size,
            init_method=_init_method(config.initializer_range),
            sequence_parallel_enabled=False)
        self.layers = nn.ModuleList(
            LlamaDecoderLayer(config) for _ in range(config.num_hidden_layers))
        self.norm = RMSNorm(config.hidden_size, config.rms_norm_eps,
                            sequence_parallel_enabled=config.sequence_parallel_enabled)
        cos, sin = ops.precompute_rope_freqs(
            config.max_position_embeddings, config.head_dim,
            config.rope_theta,
            rope_scaling=getattr(config, "rope_scaling", None))
        self.register_buffer("rope_cos", cos, persistent=False)
        self.register_buffer("rope_sin", sin, persistent=False)

    def reset_parameters(self):
        # meta materialization clobbers non-persistent buffers: recompute
        cos, sin = ops.precompute_rope_freqs(
            self.config.max_position_embeddings, self.config.head_dim,
            self.config.rope_theta, device=self.rope_cos.device,
            rope_scaling=getattr(self.config, "rope_scaling", None))
        with torch.no_grad():
            self.rope_cos.copy_(cos)
            self.rope_sin.copy_(sin)

    def forward(self, input_ids, pos_offset=0, kv_caches=None):
        hidden = self.embed_tokens(input_ids)  # (B,S,H)
        if self.config.sequence_parallel_enabled:
            hidden = hidden.transpose(0, 1).contiguous()  # (S,B,H)
            hidden = scatter_to_sequence_parallel_region(hidden, seq_dim=0)
        if (not isinstance(hidden, torch.fx.Proxy)
                and not self.training and not torch.is_grad_enabled()
                and hidden.is_cuda and hidden.dtype == torch.bfloat16
                and not self.config.sequence_parallel_enabled
                and self.config.hidden_size % 8 == 0
                and ops.add_rmsnorm_available()
                and all(hasattr(l, "forward_fused")
                        for l in self.layers)):
            # fused residual+norm inference path (2 elementwise kernels per
            # layer instead of 4; decode steps are kernel-count-bound)
            residual, delta = hidden, None
            for i, layer in enumerate(self.layers):
                kc = kv_caches[i] if kv_caches is not None else None
                residual, delta = layer.forward_fused(
                    residual, delta, self.rope_cos, self.rope_sin,
                    pos_offset, kc)
            _, hidden = ops.add_rmsnorm(residual, delta, self.norm.weight,
                                        self.norm.variance_epsilon)
            return hidden
        if fused_norm_train_ok(self.config, hidden, self.training) \
                and kv_caches is None \
                and all(hasattr(l, "forward_fused_train")
                        and not l._forward_hooks
                        and not l._forward_pre_hooks
                        for l in self.layers):
            # fused residual+norm TRAINING path (autograd twin of the
            # inference path above; NXDA_FUSED_NORM=0 reverts).  Works
            # under SP too: the adds/norms are per-row ops on the local
            # seq shard, and the RMSNorm weights keep their
            # sequence_parallel_enabled PARAM attribute for the SP grad
            # all-reduce regardless of which op computes the grad.
            residual, delta = hidden, None
            for layer in self.layers:
                residual, delta = layer.forward_fused_train(
                    residual, delta, self.rope_cos, self.rope_sin,
                    pos_offset)
            _, hidden = ops.add_rmsnorm_train(delta, residual,
                                              self.norm.weight,
                                              self.norm.variance_epsilon)
        else:
            for i, layer in enumerate(self.layers):
                kc = kv_caches[i] if kv_caches is not None else None
                hidden = layer(hidden, self.rope_cos, self.rope_sin,
                               pos_offset, kc)
            hidden = self.norm(hidden)
        if self.config.sequence_parallel_enabled:
            hidden = gather_from_sequence_parallel_region(
                hidden, seq_dim=0, to_model_parallel=True)
            hidden = hidden.transpose(0, 1)  # (B,S,H)
        return hidden


class LlamaForCausalLM(nn.Module):
    # decode path accepts a device-tensor position (hipGraph decode engine)
    supports_tensor_position = True

    def __init__(self, config: LlamaConfig):
        super().__init__()
        self.config = config
        self.model = LlamaModel(config)
        self.lm_head = ColumnParallelLinear(
            config.hidden_size, config.vocab_size, bias=False,
            gather_output=False, dgrad_shadow=False, wgrad_tn=False,
            init_method=_init_method(config.initializer_range))
        if config.tie_word_embeddings:
            self.lm_head.weight = self.model.embed_tokens.weight

    def forward(self, input_ids, labels=None, pos_offset=0, kv_caches=None):
        hidden = self.model(input_ids, pos_offset, kv_caches)
        if labels is not None and self.config.loss_chunks > 0:
            from ..utils.chunked_loss import chunked_lm_loss

            return chunked_lm_loss(hidden, self.lm_head, labels,
                                   num_chunks=self.config.loss_chunks)
        logits = self.lm_head(hidden)  # (B,S,V/tp)
        if labels is None:
            return logits
        shift = labels[:, 1:].contiguous()
        loss = parallel_cross_entropy(logits[:, :-1, :].contiguous(), shift)
        valid = (shift != -100).sum().clamp(min=1)
        return loss.sum() / valid
