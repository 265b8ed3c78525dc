"""Hand-written CDNA4 HIP kernels — python wrappers + autograd.

The native library (``libnxd_ops.so``, built in-tree by ``ops/build.py``)
replaces the reference's NKI kernels: RMSNorm, RoPE,
SwiGLU, flash attention, fused AdamW.  On a GPU box the HIP path is
MANDATORY — if the library is missing, GPU calls raise instead of silently
falling back to eager torch.  CPU tensors use plain-torch reference
implementations (the numerics baseline the GPU kernels are tested against).
"""

import contextlib
import contextvars
import ctypes
import math
import os
from typing import Optional

import torch

_LIB = None
_LIB_ERR = None


def _load():
    global _LIB, _LIB_ERR
    if _LIB is not None or _LIB_ERR is not None:
        return _LIB
    from .build import LIB

    if not os.path.exists(LIB):
        _LIB_ERR = f"{LIB} not built — run neuronx_distributed_amd.ops.build"
        return None
    try:
        lib = ctypes.CDLL(LIB)
    except OSError as e:  # pragma: no cover
        _LIB_ERR = str(e)
        return None
    _LIB = lib
    return _LIB


def is_available() -> bool:
    return _load() is not None


def _require_lib():
    lib = _load()
    if lib is None:
        raise RuntimeError(
            f"nxd_ops HIP library unavailable on a GPU tensor: {_LIB_ERR}. "
            "The MI355X-native kernels are mandatory on GPU — build with "
            "python -m neuronx_distributed_amd.ops.build")
    return lib


def _stream() -> ctypes.c_void_p:
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: torch.Tensor) -> ctypes.c_void_p:
    return ctypes.c_void_p(t.data_ptr())


# ---------------------------------------------------------------------------
# RMSNorm
# ---------------------------------------------------------------------------

class _RMSNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, eps):
        ctx.eps = eps
        if x.is_cuda and x.dtype == torch.bfloat16 and x.shape[-1] % 8 == 0:
            lib = _require_lib()
            x2 = x.contiguous()
            rows = x2.numel() // x2.shape[-1]
            out = torch.empty_like(x2)
            rstd = torch.empty(rows, dtype=torch.float32, device=x.device)
            lib.rmsnorm_fwd(_ptr(x2), _ptr(weight.contiguous()), _ptr(out),
                            _ptr(rstd), ctypes.c_int(rows),
                            ctypes.c_int(x2.shape[-1]), ctypes.c_float(eps),
                            _stream())
            ctx.save_for_backward(x2, weight, rstd)
            return out
        # CPU reference (fp32 math like the kernel)
        xf = x.float()
        rstd = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
        ctx.save_for_backward(x, weight, rstd.squeeze(-1).reshape(-1))
        return (xf * rstd * weight.float()).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        x, weight, rstd = ctx.saved_tensors
        H = x.shape[-1]
        if x.is_cuda and x.dtype == torch.bfloat16 and H % 8 == 0:
            lib = _require_lib()
            dy2 = dy.contiguous()
            rows = x.numel() // H
            dx = torch.empty_like(x)
            dw32 = torch.zeros(H, dtype=torch.float32, device=x.device)
            lib.rmsnorm_bwd(_ptr(x), _ptr(weight.contiguous()), _ptr(dy2),
                            _ptr(rstd), _ptr(dx), _ptr(dw32),
                            ctypes.c_int(rows), ctypes.c_int(H), _stream())
            return dx, dw32.to(weight.dtype), None
        xf = x.float()
        dyf = dy.float()
        wf = weight.float()
        r = rstd.reshape(x.shape[:-1]).unsqueeze(-1).to(torch.float32)
        dot = (dyf * wf * xf).sum(-1, keepdim=True)
        dx = r * wf * dyf - r.pow(3) / H * xf * dot
        dw = (dyf * xf * r).reshape(-1, H).sum(0)
        return dx.to(x.dtype), dw.to(weight.dtype), None


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float = 1e-6):
    return _RMSNormFn.apply(x, weight, eps)


def add_rmsnorm_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "add_rmsnorm_fwd")


def add_rmsnorm(residual: torch.Tensor, delta: torch.Tensor,
                weight: torch.Tensor, eps: float = 1e-6):
    """Fused ``res_out = residual + delta; normed = rmsnorm(res_out)*w``
    (inference only, no autograd).  bf16 GPU rows; H % 8 == 0."""
    lib = _require_lib()
    H = residual.shape[-1]
    rows = residual.numel() // H
    r = residual.contiguous()
    d = delta.contiguous()
    res_out = torch.empty_like(r)
    normed = torch.empty_like(r)
    lib.add_rmsnorm_fwd(_ptr(r), _ptr(d), _ptr(weight.contiguous()),
                        _ptr(res_out), _ptr(normed), rows, H,
                        ctypes.c_float(eps), _stream())
    return res_out, normed


class _AddRMSNormFn(torch.autograd.Function):
    """Training fused residual-add + RMSNorm: (delta, res) -> (h, normed)
    with h = bf16(delta + res), normed = rmsnorm(h) * w.  The backward
    folds the residual fork's pass-through gradient dh into the RMSNorm
    backward pass (``rmsnorm_bwd_add``), so the fused site costs one
    kernel in each direction instead of norm + a 3-pass eager add
    (CUDAFunctor_add was ~2%% of the training step)."""

    @staticmethod
    def forward(ctx, delta, res, weight, eps):
        ctx.eps = eps
        if delta.is_cuda and delta.dtype == torch.bfloat16 \
                and delta.shape[-1] % 8 == 0:
            lib = _require_lib()
            H = delta.shape[-1]
            rows = delta.numel() // H
            dc, rc = delta.contiguous(), res.contiguous()
            h = torch.empty_like(dc)
            normed = torch.empty_like(dc)
            rstd = torch.empty(rows, dtype=torch.float32,
                               device=delta.device)
            lib.add_rmsnorm_fwd_train(_ptr(rc), _ptr(dc),
                                      _ptr(weight.contiguous()), _ptr(h),
                                      _ptr(normed), _ptr(rstd), rows, H,
                                      ctypes.c_float(eps), _stream())
            ctx.save_for_backward(h, weight, rstd)
            return h, normed
        # composed reference (fp32 math, norm stats on the rounded sum —
        # matches the kernel and an unfused bf16 add -> rmsnorm chain)
        h = (delta.float() + res.float()).to(delta.dtype)
        hf = h.float()
        rstd = torch.rsqrt(hf.pow(2).mean(-1, keepdim=True) + eps)
        ctx.save_for_backward(h, weight, rstd.squeeze(-1).reshape(-1))
        return h, (hf * rstd * weight.float()).to(delta.dtype)

    @staticmethod
    def backward(ctx, dh, dnormed):
        h, weight, rstd = ctx.saved_tensors
        H = h.shape[-1]
        if dnormed is None:
            # normed output unused: the op reduces to the residual add —
            # grads pass straight through, no weight grad
            return dh, dh, None, None
        if h.is_cuda and h.dtype == torch.bfloat16 and H % 8 == 0:
            lib = _require_lib()
            rows = h.numel() // H
            dy = dnormed.contiguous()
            dx = torch.empty_like(h)
            dw32 = torch.zeros(H, dtype=torch.float32, device=h.device)
            if dh is None:
                lib.rmsnorm_bwd(_ptr(h), _ptr(weight.contiguous()),
                                _ptr(dy), _ptr(rstd), _ptr(dx), _ptr(dw32),
                                rows, H, _stream())
            else:
                lib.rmsnorm_bwd_add(_ptr(h), _ptr(weight.contiguous()),
                                    _ptr(dy), _ptr(rstd),
                                    _ptr(dh.contiguous()), _ptr(dx),
                                    _ptr(dw32), rows, H, _stream())
            return dx, dx, dw32.to(weight.dtype), None
        hf = h.float()
        dyf = dnormed.float()
        wf = weight.float()
        r = rstd.reshape(h.shape[:-1]).unsqueeze(-1).to(torch.float32)
        dot = (dyf * wf * hf).sum(-1, keepdim=True)
        dx = r * wf * dyf - r.pow(3) / H * hf * dot
        if dh is not None:
            dx = dx + dh.float()
        dw = (dyf * hf * r).reshape(-1, H).sum(0)
        dxc = dx.to(h.dtype)
        return dxc, dxc, dw.to(weight.dtype), None


def add_rmsnorm_train(delta: torch.Tensor, res: torch.Tensor,
                      weight: torch.Tensor, eps: float = 1e-6):
    """Autograd fused ``h = delta + res; normed = rmsnorm(h) * w`` —
    returns (h, normed); d delta == d res == rmsnorm_bwd + dh (fused)."""
    return _AddRMSNormFn.apply(delta, res, weight, eps)


def add_rmsnorm_train_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "add_rmsnorm_fwd_train")


# ---------------------------------------------------------------------------
# RoPE (neox rotate-half), in-place on clones
# ---------------------------------------------------------------------------

def _rope_torch(x, cos, sin, sign=1.0):
    # x (B,S,h,D); cos/sin (S, D/2) f32
    half = x.shape[-1] // 2
    x0 = x[..., :half].float()
    x1 = x[..., half:].float()
    c = cos.view(1, cos.shape[0], 1, half)
    s = sin.view(1, sin.shape[0], 1, half) * sign
    o0 = x0 * c - x1 * s
    o1 = x1 * c + x0 * s
    return torch.cat([o0, o1], dim=-1).to(x.dtype)


class _RoPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, cos, sin, pos_offset):
        # bounds-check HERE: an out-of-range position would be an
        # out-of-bounds global read inside the HIP kernel (GPU fault)
        S = q.shape[1]
        off = int(pos_offset) if not isinstance(pos_offset, torch.Tensor) \
            else 0  # device-tensor positions are decode-path (S == 1)
        if off + S > cos.shape[0]:
            raise ValueError(
                f"RoPE table too short: seq {off}+{S} > table "
                f"{cos.shape[0]} (raise max_position_embeddings)")
        ctx.pos_offset = pos_offset
        ctx.save_for_backward(cos, sin)
        if q.is_cuda and q.dtype == torch.bfloat16:
            lib = _require_lib()
            B, S, Hq, D = q.shape
            Hk = k.shape[2]
            qc, kc = q.contiguous(), k.contiguous()
            qo = torch.empty_like(qc)
            ko = torch.empty_like(kc)
            lib.rope_fwd(_ptr(qc), _ptr(kc), _ptr(qo), _ptr(ko), _ptr(cos),
                         _ptr(sin),
                         ctypes.c_int(B), ctypes.c_int(S), ctypes.c_int(Hq),
                         ctypes.c_int(Hk), ctypes.c_int(D),
                         ctypes.c_int(pos_offset), ctypes.c_int(0), _stream())
            return qo, ko
        S = q.shape[1]
        c = cos[pos_offset:pos_offset + S]
        s = sin[pos_offset:pos_offset + S]
        return _rope_torch(q, c, s), _rope_torch(k, c, s)

    @staticmethod
    def backward(ctx, dq, dk):
        cos, sin = ctx.saved_tensors
        off = ctx.pos_offset
        if dq.is_cuda and dq.dtype == torch.bfloat16:
            lib = _require_lib()
            B, S, Hq, D = dq.shape
            Hk = dk.shape[2]
            dqc, dkc = dq.contiguous(), dk.contiguous()
            dqo = torch.empty_like(dqc)
            dko = torch.empty_like(dkc)
            lib.rope_fwd(_ptr(dqc), _ptr(dkc), _ptr(dqo), _ptr(dko),
                         _ptr(cos), _ptr(sin),
                         ctypes.c_int(B), ctypes.c_int(S), ctypes.c_int(Hq),
                         ctypes.c_int(Hk), ctypes.c_int(D), ctypes.c_int(off),
                         ctypes.c_int(1), _stream())
            return dqo, dko, None, None, None
        S = dq.shape[1]
        c = cos[off:off + S]
        s = sin[off:off + S]
        return (_rope_torch(dq, c, s, -1.0), _rope_torch(dk, c, s, -1.0),
                None, None, None)


def apply_rotary_pos_emb(q, k, cos, sin, pos_offset: int = 0):
    """q (B,S,Hq,D), k (B,S,Hk,D); cos/sin (S_max, D/2) fp32 tables."""
    return _RoPEFn.apply(q, k, cos, sin, pos_offset)


def _llama3_scale_freqs(inv_freqs: torch.Tensor, scaling: dict):
    """Llama-3.1 long-context frequency scaling (reference
    attention/utils.py apply_scaling): high-frequency components (short
    wavelength vs the original context) pass through, low-frequency ones
    divide by ``factor``, the band between interpolates smoothly."""
    import math as _math

    factor = float(scaling["factor"])
    lo = float(scaling.get("low_freq_factor", 1.0))
    hi = float(scaling.get("high_freq_factor", 4.0))
    orig = float(scaling.get("original_max_position_embeddings", 8192))
    wavelen = 2 * _math.pi / inv_freqs
    smooth = ((orig / wavelen - lo) / (hi - lo)).clamp(0.0, 1.0)
    blended = (1.0 - smooth) * inv_freqs / factor + smooth * inv_freqs
    return torch.where(wavelen < orig / hi, inv_freqs,
                       torch.where(wavelen > orig / lo, inv_freqs / factor,
                                   blended))


def precompute_rope_freqs(seq_len: int, dim: int, theta: float = 10000.0,
                          device=None, rope_scaling: dict = None):
    """cos/sin tables (S, D/2) fp32 (reference attention/utils.py
    precompute_freqs_cis; ``rope_scaling`` with rope_type \"llama3\"
    applies the 3.1 long-context wavelength interpolation)."""
    inv = 1.0 / (theta ** (torch.arange(0, dim, 2, device=device,
                                        dtype=torch.float32) / dim))
    if rope_scaling:
        rt = rope_scaling.get("rope_type", rope_scaling.get("type",
                                                            "llama3"))
        if rt == "llama3":
            inv = _llama3_scale_freqs(inv, rope_scaling)
        elif rt == "linear":
            inv = inv / float(rope_scaling["factor"])
        else:
            raise NotImplementedError(f"rope_scaling type {rt!r}")
    t = torch.arange(seq_len, device=device, dtype=torch.float32)
    freqs = torch.outer(t, inv)
    return freqs.cos(), freqs.sin()


def apply_rotary_polar_compatible(query, key, freqs):
    """Meta-llama INTERLEAVED rotary (reference attention/utils.py:50
    apply_rotary_polar_compatible): dims pair as (2i, 2i+1) complex
    components — used for Meta-format checkpoints, whereas the model
    stack and HIP kernel use the HF neox rotate-half pairing.
    query/key (B, S, H, D); freqs (S, D/2) fp32 angles."""
    if freqs.dtype != torch.float32:
        raise ValueError("freqs must be fp32 for accuracy")
    phase = torch.polar(torch.ones_like(freqs), freqs)  # e^{i*theta}
    phase = phase.view(1, freqs.shape[0], 1, freqs.shape[1])

    def rot(x):
        xc = torch.view_as_complex(
            x.float().reshape(*x.shape[:-1], x.shape[-1] // 2, 2))
        return torch.view_as_real(xc * phase).reshape(x.shape).to(x.dtype)

    return rot(query), rot(key)


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------

# One-slot hand-off of dx^T from SwiGLU's backward to the weight-gradient
# GEMM of the linear that produced its input (parallel/layers.py wgrad_tn).
# Autograd has no channel for a second gradient, so the slot is keyed by the
# dx tensor itself: its data pointer, shape, strides and ``_version``.  The
# slot keeps dx alive, so the pointer cannot be handed out again while the
# entry exists; every linear backward takes (and thereby empties) the slot
# first, so an entry lives only between two neighbouring backward nodes.
_WGRAD_HANDOFF = [None]


def wgrad_handoff_put(dx: torch.Tensor, dxt: torch.Tensor) -> None:
    _WGRAD_HANDOFF[0] = (dx, dx._version, dxt)


def wgrad_handoff_take(grad_output: Optional[torch.Tensor] = None):
    """Empty the slot; return its dx^T iff ``grad_output`` is the very dx it
    was filled with, unmodified (same memory, shape, strides, version).
    Anything else (a hook that replaced or edited the gradient, a copy)
    returns None and the entry is dropped."""
    entry, _WGRAD_HANDOFF[0] = _WGRAD_HANDOFF[0], None
    if entry is None or grad_output is None:
        return None
    dx, version, dxt = entry
    if (grad_output.data_ptr() == dx.data_ptr()
            and grad_output.shape == dx.shape
            and grad_output.stride() == dx.stride()
            and grad_output.dtype == dx.dtype
            and grad_output._version == version
            and dx._version == version):
        return dxt
    return None


def swiglu_bwd_t_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "swiglu_bwd_t")


def swiglu_bwd_t(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor = None,
                 dxt: torch.Tensor = None):
    """SwiGLU backward with two outputs: dx (like x) bit-identical to the
    plain backward kernel, and dxt (2I, N) = dx^T contiguous, written by one
    tiled kernel (csrc/swiglu.hip).  x (..., 2I), dy (..., I) contiguous
    bf16 GPU tensors; N (rows) and I multiples of 8."""
    lib = _require_lib()
    twoI = x.shape[-1]
    I = twoI // 2
    N = x.numel() // max(twoI, 1)
    if not (x.is_cuda and x.dtype == torch.bfloat16 and x.is_contiguous()
            and dy.is_cuda and dy.dtype == torch.bfloat16
            and dy.is_contiguous() and dy.numel() == N * I
            and twoI == 2 * I and N > 0 and I > 0 and N % 8 == 0
            and I % 8 == 0):
        raise ValueError(f"swiglu_bwd_t: x {tuple(x.shape)} / dy "
                         f"{tuple(dy.shape)} outside the kernel contract "
                         f"(contiguous bf16 on the GPU, rows and I "
                         f"multiples of 8)")
    if dx is None:
        dx = torch.empty_like(x)
    if dxt is None:
        dxt = torch.empty(twoI, N, dtype=x.dtype, device=x.device)
    for name, t, shape in (("dx", dx, tuple(x.shape)),
                           ("dxt", dxt, (twoI, N))):
        if t.dtype != x.dtype or t.device != x.device or \
                tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"swiglu_bwd_t: {name} must be a contiguous "
                             f"{shape} bf16 tensor on {x.device}")
    rc = lib.swiglu_bwd_t(_ptr(x), _ptr(dy), _ptr(dx), _ptr(dxt),
                          ctypes.c_long(N), ctypes.c_long(I), _stream())
    if rc != 0:
        raise ValueError(f"swiglu_bwd_t rejected N={N}, I={I} (16-byte "
                         f"aligned pointers required)")
    return dx, dxt


class _SwiGLUFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, wgrad_dxt=False):
        ctx.wgrad_dxt = bool(wgrad_dxt)
        ctx.save_for_backward(x)
        I = x.shape[-1] // 2
        if x.is_cuda and x.dtype == torch.bfloat16 and I % 8 == 0:
            lib = _require_lib()
            x2 = x.contiguous()
            N = x2.numel() // x2.shape[-1]
            out = torch.empty(x2.shape[:-1] + (I,), dtype=x2.dtype,
                              device=x2.device)
            lib.swiglu_fwd(_ptr(x2), _ptr(out), ctypes.c_long(N),
                           ctypes.c_int(I), _stream())
            return out
        g, u = x[..., :I].float(), x[..., I:].float()
        return (torch.nn.functional.silu(g) * u).to(x.dtype)

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        I = x.shape[-1] // 2
        # dx^T for the producer's K-contiguous weight gradient: only when the
        # caller asked for it and that wgrad would take it right now
        want_t = False
        if ctx.wgrad_dxt and not torch.is_grad_enabled():
            from ..parallel.layers import wgrad_tn_wants_dxt

            want_t = wgrad_tn_wants_dxt(x)
        if x.is_cuda and x.dtype == torch.bfloat16 and I % 8 == 0:
            lib = _require_lib()
            dy2 = dy.contiguous()
            N = x.numel() // x.shape[-1]
            if want_t:
                dx, dxt = swiglu_bwd_t(x, dy2)
                wgrad_handoff_put(dx, dxt)
                return dx, None
            dx = torch.empty_like(x)
            lib.swiglu_bwd(_ptr(x), _ptr(dy2), _ptr(dx), ctypes.c_long(N),
                           ctypes.c_int(I), _stream())
            return dx, None
        g, u = x[..., :I].float(), x[..., I:].float()
        dyf = dy.float()
        sig = torch.sigmoid(g)
        s = g * sig
        dg = dyf * u * (sig + s * (1 - sig))
        du = dyf * s
        dx = torch.cat([dg, du], dim=-1).to(x.dtype)
        if want_t:  # composed stand-in for the dual-output kernel
            wgrad_handoff_put(dx, transpose(dx.reshape(-1, dx.shape[-1])))
        return dx, None


def swiglu(x: torch.Tensor, wgrad_dxt: bool = False) -> torch.Tensor:
    """x = [gate; up] on the last dim -> silu(gate)*up.

    ``wgrad_dxt``: x is the output of a linear whose weight gradient may run
    K-contiguous (``parallel.layers.wgrad_tn``); the backward then also
    writes dx^T and hands it to that wgrad instead of leaving it to
    transpose dx again."""
    return _SwiGLUFn.apply(x, wgrad_dxt)


# ---------------------------------------------------------------------------
# Flash attention (MFMA kernel in csrc/flash_attn.hip)
# ---------------------------------------------------------------------------

def flash_attn_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "flash_attn_fwd")


def _fa_ok_layout(t) -> bool:
    """The flash kernels take any (batch, head, seq) strides with a DENSE
    last dim — transpose views of BSHD activations go in with no copy."""
    return t.stride(3) == 1


def _fa_strides(*tensors):
    vals = []
    for t in tensors:
        vals += [t.stride(0), t.stride(1), t.stride(2)]
    arr = (ctypes.c_long * len(vals))(*vals)
    return arr


def _fa_alloc_like(t):
    """Allocate an empty tensor with t's LAYOUT (so a BSHD-view input
    produces a BSHD-view output and the downstream reshape stays a view)."""
    B, H, S, D = t.shape
    if t.stride(1) == D and t.stride(2) == H * D:  # BSHD transpose view
        return torch.empty(B, S, H, D, dtype=t.dtype,
                           device=t.device).permute(0, 2, 1, 3)
    return torch.empty_like(t, memory_format=torch.contiguous_format)


class _FlashAttnFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, causal, scale, window=0):
        lib = _require_lib()
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        assert D == 128, "flash kernel supports D=128"
        assert q.dtype == torch.bfloat16
        if not _fa_ok_layout(q):
            q = q.contiguous()
        if not _fa_ok_layout(k):
            k = k.contiguous()
        if not _fa_ok_layout(v):
            v = v.contiguous()
        out = _fa_alloc_like(q)
        lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        lib.flash_attn_fwd_strided(
            _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(lse),
            ctypes.c_int(B), ctypes.c_int(Hq), ctypes.c_int(Hkv),
            ctypes.c_int(S), ctypes.c_float(scale),
            ctypes.c_int(1 if causal else 0), ctypes.c_int(window or 0),
            _fa_strides(q, k, v, out), _stream())
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.causal = causal
        ctx.scale = scale
        ctx.window = window or 0
        return out

    @staticmethod
    def backward(ctx, dout):
        q, k, v, out, lse = ctx.saved_tensors
        lib = _require_lib()
        if not hasattr(lib, "flash_attn_bwd"):
            raise RuntimeError("flash_attn_bwd kernel not built")
        B, Hq, S, D = q.shape
        Hkv = k.shape[1]
        if not _fa_ok_layout(dout):
            dout = dout.contiguous()
        delta = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
        # grads are allocated in their producer's LAYOUT so autograd's
        # accumulation into BSHD views stays copy-free
        dq = _fa_alloc_like(q)
        # dk/dv are written bf16 PER Q-HEAD (B,Hq,S,D); GQA replicas are
        # reduced here (each replica covers distinct Q heads -> SUM)
        if Hq == Hkv:
            # no reduction: write dk/dv straight in k's/v's layout, so a
            # BSHD-view k/v gets BSHD grads and the consumers' .contiguous()
            # stays a no-op (the kernels take the strides)
            dk_pq = _fa_alloc_like(k)
            dv_pq = _fa_alloc_like(v)
        else:
            # the .view(B, Hkv, rep, S, D) reduction needs contiguous BHSD
            dk_pq = torch.empty(B, Hq, S, D, dtype=q.dtype, device=q.device)
            dv_pq = torch.empty(B, Hq, S, D, dtype=q.dtype, device=q.device)
        lib.flash_attn_bwd_strided(
            _ptr(q), _ptr(k), _ptr(v), _ptr(out), _ptr(dout),
            _ptr(lse), _ptr(delta), _ptr(dq), _ptr(dk_pq), _ptr(dv_pq),
            ctypes.c_int(B), ctypes.c_int(Hq), ctypes.c_int(Hkv),
            ctypes.c_int(S), ctypes.c_float(ctx.scale),
            ctypes.c_int(1 if ctx.causal else 0),
            ctypes.c_int(getattr(ctx, "window", 0)),
            _fa_strides(q, k, v, out, dout, dq, dk_pq, dv_pq), _stream())
        rep = Hq // Hkv
        if rep > 1:
            dk = dk_pq.view(B, Hkv, rep, S, D).float().sum(2).to(q.dtype)
            dv = dv_pq.view(B, Hkv, rep, S, D).float().sum(2).to(q.dtype)
        else:
            dk = dk_pq
            dv = dv_pq
        return dq, dk, dv, None, None, None


def flash_attn(q, k, v, causal=True, softmax_scale=None, window=0):
    """q (B,Hq,S,D=128), k/v (B,Hkv,S,D) bf16 on GPU.  window > 0:
    sliding-window causal (Mistral), fwd AND bwd on the MFMA kernels."""
    scale = softmax_scale or 1.0 / math.sqrt(q.shape[-1])
    return _FlashAttnFn.apply(q, k, v, causal, scale, window)


def flash_attn_window_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "flash_attn_fwd_window")


def flash_attn_windowed(q, k, v, window: int, softmax_scale=None):
    """Sliding-window causal flash attention (inference/no-grad): q row i
    attends kv rows [i-window+1, i].  q (B,Hq,S,128), k/v (B,Hkv,S,128)
    bf16; out-of-band tiles are skipped entirely (Mistral-style)."""
    lib = _require_lib()
    B, Hq, S, D = q.shape
    Hkv = k.shape[1]
    assert D == 128 and q.dtype == torch.bfloat16
    scale = softmax_scale or 1.0 / math.sqrt(D)
    q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    out = torch.empty_like(q)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    lib.flash_attn_fwd_window(_ptr(q), _ptr(k), _ptr(v), _ptr(out),
                              _ptr(lse), ctypes.c_int(B), ctypes.c_int(Hq),
                              ctypes.c_int(Hkv), ctypes.c_int(S),
                              ctypes.c_float(scale), ctypes.c_int(window),
                              _stream())
    return out


# ---------------------------------------------------------------------------
# Fused AdamW (ZeRO-1 master-shard update; csrc/adamw.hip)
# ---------------------------------------------------------------------------

def adamw_step(master: torch.Tensor, m: torch.Tensor, v: torch.Tensor,
               grad_bf16: torch.Tensor, param_bf16: torch.Tensor,
               clip: Optional[torch.Tensor], lr: float, beta1: float,
               beta2: float, eps: float, weight_decay: float, step: int):
    """One fused pass: bf16 grad -> fp32 m/v/master update -> bf16 param."""
    lib = _require_lib()
    n = master.numel()
    assert m.numel() == n and v.numel() == n and grad_bf16.numel() == n
    assert grad_bf16.dtype == torch.bfloat16 and param_bf16.dtype == torch.bfloat16
    inv_bc1 = 1.0 / (1.0 - beta1 ** step)
    inv_bc2 = 1.0 / (1.0 - beta2 ** step)
    lib.adamw_step(ctypes.c_long(n), _ptr(master), _ptr(m), _ptr(v),
                   _ptr(grad_bf16), _ptr(param_bf16),
                   _ptr(clip) if clip is not None else None,
                   ctypes.c_float(lr), ctypes.c_float(beta1),
                   ctypes.c_float(beta2), ctypes.c_float(eps),
                   ctypes.c_float(weight_decay), ctypes.c_float(inv_bc1),
                   ctypes.c_float(inv_bc2), _stream())


# ---------------------------------------------------------------------------
# bf16 2-D transpose (csrc/transpose.hip)
# ---------------------------------------------------------------------------

def transpose_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "transpose_bf16")


def _transpose_tiles(lib, who: str, x: torch.Tensor, out: torch.Tensor):
    """Validate one (source, destination) pair against the kernel contract;
    returns its tile count.  Raises before anything is launched."""
    if x.dim() != 2 or x.dtype != torch.bfloat16 or not x.is_cuda:
        raise ValueError(f"{who}: source must be a 2-D bf16 GPU tensor, got "
                         f"{tuple(x.shape)} {x.dtype} on {x.device}")
    R, C = x.shape
    rs = x.stride(0) if R > 1 else max(C, 8)
    if x.stride(1) != 1 and C > 1:
        raise ValueError(f"{who}: source rows must be dense, strides "
                         f"{x.stride()}")
    if out.dtype != x.dtype or out.device != x.device or \
            tuple(out.shape) != (C, R) or not out.is_contiguous():
        raise ValueError(f"{who}: destination must be a contiguous "
                         f"{(C, R)} bf16 tensor on {x.device}, got "
                         f"{tuple(out.shape)} strides {out.stride()}")
    lib.transpose_bf16_tiles.restype = ctypes.c_long
    tiles = lib.transpose_bf16_tiles(ctypes.c_long(R), ctypes.c_long(C),
                                     ctypes.c_long(rs))
    if tiles < 0 or x.data_ptr() % 16 or out.data_ptr() % 16:
        raise ValueError(f"{who}: shape {(R, C)} row stride {rs} outside the "
                         f"kernel contract (R, C, stride multiples of 8, "
                         f"16-byte aligned)")
    return tiles, rs


def transpose(x: torch.Tensor, out: Optional[torch.Tensor] = None):
    """x (R, C) -> (C, R) contiguous.  bf16 GPU tensors go through the tiled
    LDS kernel: rows may be strided (a column slice of a wider buffer), R, C
    and the row stride are multiples of 8.  ``out`` reuses a destination.
    Anything on the CPU is the composed torch transpose."""
    if x.dim() != 2:
        raise ValueError(f"transpose: 2-D input expected, got {tuple(x.shape)}")
    if out is None:
        out = torch.empty(x.shape[1], x.shape[0], dtype=x.dtype,
                          device=x.device)
    if not x.is_cuda:
        out.copy_(x.t())
        return out
    lib = _require_lib()
    _, rs = _transpose_tiles(lib, "transpose", x, out)
    rc = lib.transpose_bf16(_ptr(x), _ptr(out), ctypes.c_long(rs),
                            ctypes.c_long(x.shape[0]),
                            ctypes.c_long(x.shape[1]), _stream())
    if rc != 0:
        raise ValueError(f"transpose rejected shape {tuple(x.shape)}")
    return out


TRANSPOSE_MULTI_MAX = 4  # csrc/transpose.hip TR_MULTI_MAX


def transpose_multi(xs, outs=None):
    """Transpose one to four 2-D matrices (different shapes allowed) in ONE
    launch whose descriptors are kernel arguments: no device table and no
    host-to-device copy, unlike :func:`transpose_batched`.  Same contract
    per matrix as :func:`transpose`; everything is validated before the
    launch.  Returns the list of (C, R) results."""
    xs = list(xs)
    if not 1 <= len(xs) <= TRANSPOSE_MULTI_MAX:
        raise ValueError(f"transpose_multi: 1 to {TRANSPOSE_MULTI_MAX} "
                         f"matrices, got {len(xs)}")
    if outs is None:
        outs = [torch.empty(x.shape[1], x.shape[0], dtype=x.dtype,
                            device=x.device) if x.dim() == 2 else None
                for x in xs]
    outs = list(outs)
    if len(outs) != len(xs):
        raise ValueError("transpose_multi: one destination per source")
    if not xs[0].is_cuda:
        for x, o in zip(xs, outs):
            transpose(x, o)
        return outs
    lib = _require_lib()
    n = len(xs)
    strides = []
    for x, o in zip(xs, outs):
        if o is None or x.device != xs[0].device:
            raise ValueError("transpose_multi: 2-D sources on one device")
        _, rs = _transpose_tiles(lib, "transpose_multi", x, o)
        strides.append(rs)
    rc = lib.transpose_bf16_multi(
        (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs]),
        (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs]),
        (ctypes.c_long * n)(*strides),
        (ctypes.c_long * n)(*[x.shape[0] for x in xs]),
        (ctypes.c_long * n)(*[x.shape[1] for x in xs]),
        ctypes.c_int(n), _stream())
    if rc != 0:
        raise ValueError(f"transpose_multi rejected {n} matrices")
    return outs


def transpose_multi_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "transpose_bf16_multi")


def transpose_batched(xs, outs=None):
    """Transpose many 2-D matrices (different shapes allowed) in ONE launch
    driven by a device descriptor table; same contract per matrix as
    :func:`transpose`.  Returns the list of (C, R) results."""
    xs = list(xs)
    if outs is None:
        outs = [torch.empty(x.shape[1], x.shape[0], dtype=x.dtype,
                            device=x.device) for x in xs]
    outs = list(outs)
    if len(outs) != len(xs):
        raise ValueError("transpose_batched: one destination per source")
    if not xs:
        return outs
    if not xs[0].is_cuda:
        for x, o in zip(xs, outs):
            transpose(x, o)
        return outs
    lib = _require_lib()
    rows, first = [], 0
    for x, o in zip(xs, outs):
        if x.device != xs[0].device:
            raise ValueError("transpose_batched: all sources on one device")
        tiles, rs = _transpose_tiles(lib, "transpose_batched", x, o)
        rows.append([x.data_ptr(), o.data_ptr(), rs, x.shape[0], x.shape[1],
                     first])
        first += tiles
    desc = torch.tensor(rows, dtype=torch.int64).to(xs[0].device)
    rc = lib.transpose_bf16_batched(_ptr(desc), len(rows),
                                    ctypes.c_long(first), _stream())
    if rc != 0:
        raise ValueError(f"transpose_batched rejected {len(rows)} matrices, "
                         f"{first} tiles")
    # desc was allocated on the launch's own stream, so the caching
    # allocator cannot hand it out again before the kernel has read it
    return outs


# ---------------------------------------------------------------------------
# Fused MoE decode (K9 parity; csrc/moe_decode.hip)
# ---------------------------------------------------------------------------

_MOE_MB = 16


def moe_decode_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "moe_decode_glu")


def moe_decode_glu(hidden: torch.Tensor, gate_up_w: torch.Tensor,
                   down_w: torch.Tensor, expert_affinities: torch.Tensor,
                   expert_index: torch.Tensor) -> torch.Tensor:
    """Fused decode MoE (inference): hidden (T,H) bf16, gate_up_w
    (E,H,2I) fused [gate|up], down_w (E,I,H), affinities (T,E) float,
    expert_index (T,k) long -> (T,H) bf16 (TP-partial, like ExpertMLPs).

    Slots (token, expert hit) are grouped per expert into blocks of 16 so
    each block streams its expert's weights once; gather, SwiGLU, affinity
    scaling and the scatter-add all happen inside the two kernels."""
    lib = _require_lib()
    T, H = hidden.shape
    E, _, twoI = gate_up_w.shape
    I = twoI // 2
    assert H % 64 == 0 and I % 64 == 0, (H, I)
    k = expert_index.shape[1]
    dev = hidden.device

    flat_e = expert_index.reshape(-1)
    order = torch.argsort(flat_e, stable=True)
    sorted_e = flat_e[order].to(torch.long)
    sorted_tok = (order // k).to(torch.int32)

    counts = torch.bincount(flat_e, minlength=E)
    blocks_per_e = (counts + _MOE_MB - 1) // _MOE_MB
    nb = int(blocks_per_e.sum().item())
    if nb == 0:
        return hidden.new_zeros(T, H)
    blockbase = torch.cumsum(torch.nn.functional.pad(blocks_per_e, (1, 0)),
                             0)  # (E+1,)
    countbase = torch.cumsum(torch.nn.functional.pad(counts, (1, 0)), 0)

    within = torch.arange(T * k, device=dev) - countbase[sorted_e]
    padded_idx = (blockbase[sorted_e] + within // _MOE_MB) * _MOE_MB + \
        within % _MOE_MB

    slot_token = torch.zeros(nb * _MOE_MB, dtype=torch.int32, device=dev)
    slot_token[padded_idx] = sorted_tok
    aff = torch.zeros(nb * _MOE_MB, dtype=torch.float32, device=dev)
    aff[padded_idx] = expert_affinities.float()[
        sorted_tok.long(), sorted_e]

    block_expert = torch.repeat_interleave(
        torch.arange(E, device=dev), blocks_per_e).to(torch.int32)
    bi = torch.arange(nb, device=dev)
    block_ord = bi - blockbase[block_expert.long()]
    block_len = torch.clamp(counts[block_expert.long()] -
                            _MOE_MB * block_ord, 0, _MOE_MB).to(torch.int32)

    act = torch.empty(nb * _MOE_MB, I, dtype=torch.bfloat16, device=dev)
    out = torch.zeros(T, H, dtype=torch.float32, device=dev)
    hidden = hidden.contiguous()
    gate_up_w = gate_up_w.contiguous()
    down_w = down_w.contiguous()
    lib.moe_decode_glu(_ptr(hidden), _ptr(gate_up_w), _ptr(down_w),
                       _ptr(slot_token), _ptr(block_expert), _ptr(block_len),
                       _ptr(aff), _ptr(act), _ptr(out), nb, H, I, _stream())
    return out.to(hidden.dtype)


# ---------------------------------------------------------------------------
# Skinny-M decode GEMM (csrc/skinny_gemm.hip)
# ---------------------------------------------------------------------------

def skinny_gemm_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "skinny_gemm")


def skinny_linear(x2: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x2 (M<=32, K) bf16 @ w (N, K)^T -> (M, N) bf16 via the split-K
    weight-streaming kernel (decode shapes run ~10x hipBLASLt's skinny
    kernels; see profiles/README.md)."""
    lib = _require_lib()
    M, K = x2.shape
    N = w.shape[0]
    out = torch.zeros(M, N, dtype=torch.float32, device=x2.device)
    lib.skinny_gemm(_ptr(x2), _ptr(w), _ptr(out), M, N, K, _stream())
    return out.to(torch.bfloat16)


def use_skinny_linear(inp: torch.Tensor, weight: torch.Tensor,
                      sequence_parallel_enabled: bool = False) -> bool:
    """Gate for the decode GEMM fast path (opt-in via NXDA_SKINNY_GEMM=1):
    measured on MI355X, hipBLASLt's skinny kernels already run the decode
    shapes at 1.8-6.6 TB/s — this kernel is kept for shapes/layouts where
    the library falls over, not as the default."""
    if os.environ.get("NXDA_SKINNY_GEMM", "0") != "1":
        return False
    return (not torch.is_grad_enabled() and not sequence_parallel_enabled
            and inp.is_cuda and inp.dtype == torch.bfloat16
            and weight.dtype == torch.bfloat16
            and inp.numel() // inp.shape[-1] <= 32
            and weight.shape[-1] % 8 == 0 and inp.shape[-1] == weight.shape[-1]
            and skinny_gemm_available())


# ---------------------------------------------------------------------------
# Fused decode attention (csrc/decode_attn.hip)
# ---------------------------------------------------------------------------

def decode_attn_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "decode_attn")


_DA_D = 128     # head dim of the fused decode kernels
_DA_SPLIT = 4   # DA_SPLIT of csrc/decode_attn_common.h
_CA_TMIN, _CA_TMAX = 2, 8   # CA_TMIN / CA_TMAX of csrc/chunk_attn.hip


def ragged_attn_available() -> bool:
    """The per-sequence-position entries of all four fused decode kernels
    (``ragged=True`` of the ``*_step`` functions below)."""
    lib = _load()
    return lib is not None and all(
        hasattr(lib, n) for n in ("decode_attn_ragged", "decode_attn_mx_ragged",
                                  "chunk_attn_ragged", "chunk_attn_mx_ragged"))


# a context variable: the choice holds for the calling thread (or task) only
_RAGGED_STEP = contextvars.ContextVar("nxd_ragged_attn_step", default=True)


def ragged_attn_enabled() -> bool:
    """Whether a model should take the ragged entries where it can:
    :func:`ragged_attn_available`, unless the caller is inside
    ``ragged_attn_step(False)``."""
    return _RAGGED_STEP.get() and ragged_attn_available()


@contextlib.contextmanager
def ragged_attn_step(enabled: bool):
    """Within the block, and for the calling thread only, models with
    per-sequence positions take the fused ragged step (``enabled``) or their
    eager chain (not ``enabled``); the ``*_step`` functions themselves are not
    affected."""
    token = _RAGGED_STEP.set(bool(enabled))
    try:
        yield
    finally:
        _RAGGED_STEP.reset(token)


def _ragged_entry(lib, name):
    """The ``_ragged`` sibling of the C entry ``name``."""
    if not ragged_attn_available():
        raise RuntimeError(f"nxd_ops library has no {name}_ragged — rebuild")
    return getattr(lib, name + "_ragged")


def _decode_attn_check(who, chunk, q, k, v, cos, sin, pos_t, B, Hq, Hkv, Smax,
                       dev, ragged=False):
    """Everything but the cache, for the four fused decode kernels: 2-D
    q2/k2/v2 (one token) or, with ``chunk``, 3-D q3/k3/v3 (T = 2..8 tokens).
    Returns T and the strides to launch with.  One token: the (q, kv) row
    strides, the dense widths when B = 1; 2-byte alignment.  A chunk: the
    element strides (q batch, q token, kv batch, kv token), multiples of 8,
    and 16-byte pointers.  ``pos_t``: one int64, or with ``ragged`` a
    contiguous (B,) of them."""
    D = _DA_D
    if Hkv < 1 or Hq % Hkv or Hq // Hkv not in (1, 2, 4, 8):
        raise ValueError(f"{who}: Hq={Hq}, Hkv={Hkv} outside the kernel "
                         f"contract (GQA rep 1/2/4/8)")
    if chunk and (q.dim() != 3 or not _CA_TMIN <= q.shape[1] <= _CA_TMAX):
        raise ValueError(f"{who}: q3 {tuple(q.shape)} must be (B, T, Hq*128) "
                         f"with {_CA_TMIN} <= T <= {_CA_TMAX}")
    T = q.shape[1] if chunk else 1
    if Smax < T:
        raise ValueError(f"{who}: a cache of {Smax} rows cannot take {T} "
                         f"tokens")
    n, align = (3, 16) if chunk else (2, 2)
    for name, t, width in ((f"q{n}", q, Hq * D), (f"k{n}", k, Hkv * D),
                           (f"v{n}", v, Hkv * D)):
        shape = (B, T, width) if chunk else (B, width)
        ok = t.dtype == torch.bfloat16 and t.device == dev \
            and tuple(t.shape) == shape and t.stride(-1) == 1 \
            and t.data_ptr() % align == 0
        if ok and chunk:
            ok = t.stride(1) >= width and not (t.stride(0) % 8
                                               or t.stride(1) % 8)
        elif ok:
            ok = B == 1 or t.stride(0) >= width
        if not ok:
            raise ValueError(f"{who}: {name} must be a {align}-byte aligned "
                             f"bf16 {shape} tensor on {dev} with a dense "
                             f"last dim and row strides that hold a row, got "
                             f"{t.dtype} {tuple(t.shape)} strides "
                             f"{t.stride()} on {t.device}")
    if k.stride() != v.stride() and (chunk or B > 1):
        raise ValueError(f"{who}: k{n} and v{n} must share their strides, "
                         f"got {k.stride()} and {v.stride()}")
    for name, t in (("cos", cos), ("sin", sin)):
        _mx_check_dense(f"{who}: {name}", t, torch.float32)
        if t.device != dev or t.dim() != 2 or t.shape[1] != D // 2 \
                or t.shape[0] < Smax or (chunk and t.data_ptr() % 16):
            raise ValueError(f"{who}: {name} {tuple(t.shape)} on {t.device} "
                             f"must be (>= {Smax}, {D // 2}) on {dev}: the "
                             f"RoPE table covers the cache")
    if ragged:
        if pos_t.dtype != torch.int64 or pos_t.device != dev \
                or tuple(pos_t.shape) != (B,) or not pos_t.is_contiguous():
            raise ValueError(f"{who}: a ragged pos_t must be a contiguous "
                             f"int64 ({B},) tensor on {dev}, got "
                             f"{pos_t.dtype} {tuple(pos_t.shape)} strides "
                             f"{pos_t.stride()} on {pos_t.device}")
    elif pos_t.dtype != torch.int64 or pos_t.device != dev \
            or pos_t.numel() != 1:
        raise ValueError(f"{who}: pos_t must be one int64 on {dev}, got "
                         f"{pos_t.dtype} {tuple(pos_t.shape)} on "
                         f"{pos_t.device}")
    if chunk:
        return T, tuple(ctypes.c_long(int(st)) for st in
                        (q.stride(0), q.stride(1), k.stride(0), k.stride(1)))
    if B > 1:
        return T, (int(q.stride(0)), int(k.stride(0)))
    return T, (Hq * D, Hkv * D)


def _decode_attn_check_cache(who, kcache, vcache, Hkv):
    """The two buffers of a bf16 KVCache: contiguous (B, Hkv, Smax, 128) on
    one GPU.  Returns (B, Smax)."""
    for name, t in (("kcache", kcache), ("vcache", vcache)):
        # an MXKVCache's uint8 buffers are half as large: the kernel would
        # run past them
        if t.dtype != torch.bfloat16 or t.dim() != 4 \
                or t.shape[-1] != _DA_D or not t.is_cuda \
                or not t.is_contiguous():
            raise ValueError(f"{who}: {name} must be a contiguous bf16 "
                             f"(B, Hkv, Smax, 128) GPU cache, got {t.dtype} "
                             f"{tuple(t.shape)} on {t.device}")
    if vcache.shape != kcache.shape or vcache.device != kcache.device \
            or kcache.shape[1] != Hkv or min(kcache.shape) < 1:
        raise ValueError(f"{who}: kcache {tuple(kcache.shape)} and vcache "
                         f"{tuple(vcache.shape)} must be one non-empty shape "
                         f"on one GPU with Hkv={Hkv} heads")
    return kcache.shape[0], kcache.shape[2]


def _decode_attn_workspace(B, T, Hq, Hkv, dev, chunk):
    """(part_o, part_ml, out), out (B, T, Hq*128) for a chunk and (B, Hq*128)
    for one token; static shapes from the caching allocator, so the launches
    are hipGraph-capturable."""
    R = Hq // Hkv * T
    part_o = torch.empty(B * Hkv * _DA_SPLIT, R, _DA_D, dtype=torch.float32,
                         device=dev)
    part_ml = torch.empty(B * Hkv * _DA_SPLIT, R, 2, dtype=torch.float32,
                          device=dev)
    out = torch.empty((B, T, Hq * _DA_D) if chunk else (B, Hq * _DA_D),
                      dtype=torch.bfloat16, device=dev)
    return part_o, part_ml, out


def _decode_attn_launch(fn, chunk, tensors, B, T, Hq, Hkv, Smax, scale,
                        strides):
    """The C entry ``fn`` over q, k, v, the cache buffers, cos, sin and pos_t
    (``tensors``) and a fresh workspace; a non-zero return, which launched
    nothing, becomes ValueError."""
    ws = _decode_attn_workspace(B, T, Hq, Hkv, tensors[-1].device, chunk)
    rc = fn(*map(_ptr, tensors + ws), B, *((T,) if chunk else ()), Hq, Hkv,
            Smax, ctypes.c_float(scale), *strides, _stream())
    if rc != 0:
        raise ValueError(f"{fn.__name__} rejected B={B}, T={T}, Hq={Hq}, "
                         f"Hkv={Hkv}, Smax={Smax}, strides "
                         f"{[getattr(st, 'value', st) for st in strides]}")
    return ws[2]


def decode_attn_step(q2: torch.Tensor, k2: torch.Tensor, v2: torch.Tensor,
                     kcache: torch.Tensor, vcache: torch.Tensor,
                     cos: torch.Tensor, sin: torch.Tensor,
                     pos_t: torch.Tensor, Hq: int, Hkv: int,
                     scale: float, *, ragged: bool = False) -> torch.Tensor:
    """One fused decode-attention step: RoPE(q,k) + cache append at the
    device position ``pos_t`` + flash-decode over the cache + GQA.
    q2 (B, Hq*128), k2/v2 (B, Hkv*128) bf16 pre-rope; kcache/vcache
    (B, Hkv, Smax, 128); cos/sin (>= Smax, 64) fp32 -> out (B, Hq*128).

    ``ragged``: ``pos_t`` is a contiguous int64 (B,) tensor, one position
    per sequence.  Sequence b appends at row ``pos_t[b]`` and attends its own
    rows [0, pos_t[b]]; its result is what the call gives for that sequence
    alone.  A sequence with a position outside [0, Smax) is inactive: its
    cache is left alone and its output row is zero.  (All four ``*_step``
    functions take the flag; a chunk of T tokens is inactive unless
    ``0 <= pos_t[b]`` and ``pos_t[b] + T <= Smax``.)

    q2/k2/v2 may be row-strided views (e.g. slices of one fused-QKV GEMM
    output): only the last dim must be dense (stride 1).  A wrong dtype or
    shape raises ValueError and launches nothing."""
    lib = _require_lib()
    who = "decode_attn_step"
    if not decode_attn_available():
        raise RuntimeError("nxd_ops library has no decode_attn — rebuild")
    B, Smax = _decode_attn_check_cache(who, kcache, vcache, Hkv)
    T, st = _decode_attn_check(who, False, q2, k2, v2, cos, sin, pos_t, B, Hq,
                               Hkv, Smax, kcache.device, ragged)
    fn = _ragged_entry(lib, "decode_attn") if ragged else lib.decode_attn
    return _decode_attn_launch(
        fn, False, (q2, k2, v2, kcache, vcache, cos, sin, pos_t),
        B, T, Hq, Hkv, Smax, scale, st)


# ---------------------------------------------------------------------------
# Native MX linear (block-scaled MFMA; csrc/mx_gemm.hip)
# ---------------------------------------------------------------------------

_MX_FMT_CODE = {"fp8_e4m3": 0, "fp4_e2m1": 4}  # the instruction's cbsz/blgp


def mx_gemm_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "mx_gemm")


def _mx_check_dense(name: str, t: torch.Tensor, dtype):
    if not t.is_cuda:
        raise ValueError(f"{name} must be a GPU tensor")
    if t.dtype != dtype:
        raise ValueError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous: shape "
                         f"{tuple(t.shape)} strides {t.stride()}")
    if t.data_ptr() % 16:
        raise ValueError(f"{name} must be 16-byte aligned: shape "
                         f"{tuple(t.shape)} at 0x{t.data_ptr():x}")


def mx_quantize_rows(x: torch.Tensor):
    """bf16 (..., K) -> (e4m3 payload uint8 (..., K), e8m0 scales uint8
    (..., K/32)), bit-identical to ``pack_mx(*quantize_mx(x, "fp8_e4m3"))``.
    Leading dims are flattened; a 2-D input may be a row-strided view with
    a dense last dim."""
    lib = _require_lib()
    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise ValueError(f"mx_quantize_rows: x must be a bf16 GPU tensor, "
                         f"got {x.dtype} on {x.device}")
    K = x.shape[-1] if x.dim() else 0
    if x.dim() < 1 or K < 32 or K % 32 or x.numel() == 0:
        raise ValueError(f"mx_quantize_rows: K must be a positive multiple "
                         f"of 32 and x non-empty, got {tuple(x.shape)}")
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    M = x2.shape[0]
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) < K
                                        or x2.stride(0) % 8)):
        raise ValueError(f"mx_quantize_rows: rows must be dense with a "
                         f"16-byte-multiple stride: shape {tuple(x2.shape)} "
                         f"strides {x2.stride()}")
    if x2.data_ptr() % 16:
        raise ValueError(f"mx_quantize_rows: x must be 16-byte aligned: "
                         f"shape {tuple(x2.shape)} at 0x{x2.data_ptr():x}")
    rs = x2.stride(0) if M > 1 else K
    q = torch.empty(M, K, dtype=torch.uint8, device=x.device)
    s = torch.empty(M, K // 32, dtype=torch.uint8, device=x.device)
    rc = lib.mx_quantize_rows(_ptr(x2), ctypes.c_long(rs), _ptr(q), _ptr(s),
                              M, K, _stream())
    if rc != 0:
        raise ValueError(f"mx_quantize_rows rejected shape {tuple(x2.shape)}"
                         f" row stride {rs}")
    lead = x.shape[:-1]
    return q.reshape(*lead, K), s.reshape(*lead, K // 32)


def _mx_check_weight(who: str, w_payload, w_scales, fmt, bias, out_dtype):
    """Validate the weight side of the kernel contract; returns (N, K,
    fp32 bias or None, out dtype).  Raises before anything is launched."""
    if fmt not in _MX_FMT_CODE:
        raise ValueError(f"{who}: weight format {fmt!r} not supported "
                         f"(one of {tuple(_MX_FMT_CODE)})")
    out_dtype = out_dtype or torch.bfloat16
    if out_dtype not in (torch.bfloat16, torch.float32):
        raise ValueError(f"{who}: out_dtype {out_dtype} not supported")
    _mx_check_dense(f"{who}: w_payload", w_payload, torch.uint8)
    _mx_check_dense(f"{who}: w_scales", w_scales, torch.uint8)
    if w_payload.dim() != 2 or w_scales.dim() != 2:
        raise ValueError(f"{who}: payload {tuple(w_payload.shape)} / "
                         f"scales {tuple(w_scales.shape)} must be 2-D")
    N = w_payload.shape[0]
    K = w_payload.shape[1] * (2 if fmt == "fp4_e2m1" else 1)
    if K < 128 or K % 128 or N < 16 or N % 16:
        raise ValueError(f"{who}: N={N}, K={K} outside the kernel "
                         f"contract (K % 128 == 0, N % 16 == 0)")
    if tuple(w_scales.shape) != (N, K // 32):
        raise ValueError(f"{who}: scales {tuple(w_scales.shape)} do not "
                         f"match payload (N={N}, K={K})")
    bias32 = None
    if bias is not None:
        if bias.numel() != N or not bias.is_cuda:
            raise ValueError(f"{who}: bias {tuple(bias.shape)} does not "
                             f"match N={N}")
        bias32 = bias.detach().reshape(N).float().contiguous()
        _mx_check_dense(f"{who}: bias", bias32, torch.float32)
    return N, K, bias32, out_dtype


def _mx_gemm_launch(lib, a_payload, a_scales, w_payload, w_scales, fmt,
                    bias32, out_dtype, M, N, K):
    out = torch.empty(M, N, dtype=out_dtype, device=a_payload.device)
    rc = lib.mx_gemm(_ptr(a_payload), _ptr(a_scales), _ptr(w_payload),
                     _ptr(w_scales),
                     _ptr(bias32) if bias32 is not None else None,
                     _ptr(out), M, N, K, _MX_FMT_CODE[fmt],
                     1 if out_dtype == torch.float32 else 0, _stream())
    if rc != 0:
        raise ValueError(f"mx_gemm rejected M={M}, N={N}, K={K}, {fmt}")
    return out


def mx_gemm_packed(a_payload: torch.Tensor, a_scales: torch.Tensor,
                   w_payload: torch.Tensor, w_scales: torch.Tensor, fmt: str,
                   bias=None, out_dtype=None):
    """C = A_mx . W_mx^T on the block-scaled MFMA for an already-quantized
    MXFP8 activation: payload (M, K) + scales (M, K/32), both uint8.  Same
    weight contract and checks as :func:`mx_linear`."""
    lib = _require_lib()
    who = "mx_gemm_packed"
    N, K, bias32, out_dtype = _mx_check_weight(who, w_payload, w_scales, fmt,
                                               bias, out_dtype)
    _mx_check_dense(f"{who}: a_payload", a_payload, torch.uint8)
    _mx_check_dense(f"{who}: a_scales", a_scales, torch.uint8)
    M = a_payload.shape[0] if a_payload.dim() == 2 else 0
    if M < 1 or tuple(a_payload.shape) != (M, K) or \
            tuple(a_scales.shape) != (M, K // 32):
        raise ValueError(f"{who}: activation payload "
                         f"{tuple(a_payload.shape)} / scales "
                         f"{tuple(a_scales.shape)} do not match K={K}")
    return _mx_gemm_launch(lib, a_payload, a_scales, w_payload, w_scales,
                           fmt, bias32, out_dtype, M, N, K)


def mx_skinny_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "mx_skinny_gemm")


MX_SKINNY_MAX_M = 32     # csrc/mx_skinny.hip: two 16-row x fragments
_MX_SKINNY_CUS = 256     # workgroups that fill an MI355X once


def _mx_skinny_tile_n(M: int) -> int:
    """n rows per workgroup of mx_skinny.hip: one 16-row W fragment per x
    fragment."""
    return 16 if M <= 16 else 32


def mx_skinny_splits(M: int, N: int, K: int, fmt: str) -> int:
    """Global K-split count of the skinny MX GEMM, in [1, K // 128].

    The four waves of a workgroup already split K among themselves, so a
    global split is added only while the N / tile workgroups leave CUs idle:
    1 when they already give one workgroup per CU, else the smallest count
    that does, capped so every wave of every slice keeps at least one
    128-deep K step (K // 512).  The same rule holds for both formats: the
    partials cost (KS, M, N) fp32 of traffic whatever the weight format."""
    if fmt not in _MX_FMT_CODE:
        raise ValueError(f"mx_skinny_splits: weight format {fmt!r} not "
                         f"supported (one of {tuple(_MX_FMT_CODE)})")
    if not 1 <= M <= MX_SKINNY_MAX_M or N < 16 or N % 16 or K < 128 \
            or K % 128:
        raise ValueError(f"mx_skinny_splits: M={M}, N={N}, K={K} outside "
                         f"the kernel contract (M <= {MX_SKINNY_MAX_M}, "
                         f"K % 128 == 0, N % 16 == 0)")
    tile = _mx_skinny_tile_n(M)
    groups = -(-N // tile)
    if groups >= _MX_SKINNY_CUS:
        return 1
    want = -(-_MX_SKINNY_CUS // groups)
    return max(1, min(want, K // 512, K // 128))


def _mx_skinny_enabled() -> bool:
    """NXDA_MX_SKINNY=0 (read per call) turns the skinny dispatch off;
    unset or any other value leaves it on."""
    return os.environ.get("NXDA_MX_SKINNY", "1").strip() != "0"


def _mx_skinny_gate(x: torch.Tensor, M: int, N: int, K: int, fmt: str
                    ) -> bool:
    """The one place that decides whether ``mx_linear`` takes the skinny
    kernel instead of quantize + the 128x128 tile."""
    return (_mx_skinny_enabled() and x.is_cuda
            and 1 <= M <= MX_SKINNY_MAX_M and mx_skinny_available())


def _mx_check_x(who: str, x: torch.Tensor, K: int):
    """The x checks of mx_quantize_rows; returns (2-D view, M, row stride)."""
    if not x.is_cuda or x.dtype != torch.bfloat16:
        raise ValueError(f"{who}: x must be a bf16 GPU tensor, got "
                         f"{x.dtype} on {x.device}")
    if x.dim() < 1 or x.shape[-1] != K or x.numel() == 0:
        raise ValueError(f"{who}: x {tuple(x.shape)} does not match K={K}")
    x2 = x if x.dim() == 2 else x.reshape(-1, K)
    M = x2.shape[0]
    if x2.stride(1) != 1 or (M > 1 and (x2.stride(0) < K
                                        or x2.stride(0) % 8)):
        raise ValueError(f"{who}: rows must be dense with a "
                         f"16-byte-multiple stride: shape {tuple(x2.shape)} "
                         f"strides {x2.stride()}")
    if x2.data_ptr() % 16:
        raise ValueError(f"{who}: x must be 16-byte aligned: shape "
                         f"{tuple(x2.shape)} at 0x{x2.data_ptr():x}")
    return x2, M, (x2.stride(0) if M > 1 else K)


def _mx_skinny_launch(lib, x2, rs, w_payload, w_scales, fmt, bias32,
                      out_dtype, M, N, K, k_splits):
    KS = min(int(k_splits), K // 128)
    out = torch.empty(M, N, dtype=out_dtype, device=x2.device)
    # cached-alloc tensor with a static shape: hipGraph-capturable
    ws = (torch.empty(KS, M, N, dtype=torch.float32, device=x2.device)
          if KS > 1 else None)
    rc = lib.mx_skinny_gemm(_ptr(x2), ctypes.c_long(rs), _ptr(w_payload),
                            _ptr(w_scales),
                            _ptr(bias32) if bias32 is not None else None,
                            _ptr(out), _ptr(ws) if ws is not None else None,
                            M, N, K, _MX_FMT_CODE[fmt],
                            1 if out_dtype == torch.float32 else 0, KS,
                            _stream())
    if rc != 0:
        raise ValueError(f"mx_skinny_gemm rejected M={M}, N={N}, K={K}, "
                         f"{fmt}, k_splits={KS}")
    return out


def mx_linear_skinny(x: torch.Tensor, w_payload: torch.Tensor,
                     w_scales: torch.Tensor, fmt: str, bias=None,
                     out_dtype=None, k_splits=None):
    """:func:`mx_linear` for at most 32 rows of x (decode) in one fused
    kernel: x is quantized to MXFP8 inside the GEMM (same bytes as
    ``mx_quantize_rows``) and W is streamed once.  Same weight contract as
    ``mx_linear`` and the x contract of ``mx_quantize_rows``, plus M <= 32;
    anything else raises ValueError and launches nothing.  ``k_splits``:
    global K-split count (clamped to K // 128); default
    :func:`mx_skinny_splits`."""
    lib = _require_lib()
    who = "mx_linear_skinny"
    N, K, bias32, out_dtype = _mx_check_weight(who, w_payload, w_scales, fmt,
                                               bias, out_dtype)
    x2, M, rs = _mx_check_x(who, x, K)
    if M > MX_SKINNY_MAX_M:
        raise ValueError(f"{who}: M={M} rows, at most {MX_SKINNY_MAX_M}")
    if k_splits is None:
        k_splits = mx_skinny_splits(M, N, K, fmt)
    elif int(k_splits) < 1:
        raise ValueError(f"{who}: k_splits={k_splits} must be >= 1")
    if not mx_skinny_available():
        raise RuntimeError("nxd_ops library has no mx_skinny_gemm — rebuild")
    out = _mx_skinny_launch(lib, x2, rs, w_payload, w_scales, fmt, bias32,
                            out_dtype, M, N, K, k_splits)
    return out.reshape(*x.shape[:-1], N)


def mx_linear(x: torch.Tensor, w_payload: torch.Tensor,
              w_scales: torch.Tensor, fmt: str, bias=None, out_dtype=None):
    """y = x . W^T on the block-scaled MFMA: x bf16 (..., K) is quantized to
    MXFP8; W is an MX payload (N, K) e4m3 or (N, K/2) e2m1 with e8m0 scales
    (N, K/32) (microscaling.pack_mx).  Up to 32 rows of x (decode) take the
    fused skinny kernel (:func:`mx_linear_skinny`; ``NXDA_MX_SKINNY=0``
    turns that off), more rows ``mx_quantize_rows`` + the 128x128 tile.
    Contract: K % 128 == 0, N % 16 == 0; anything else raises ValueError
    and launches nothing.  out_dtype: bf16 (default) or fp32; the bias is
    added in fp32 before the output rounding."""
    lib = _require_lib()
    N, K, bias32, out_dtype = _mx_check_weight("mx_linear", w_payload,
                                               w_scales, fmt, bias, out_dtype)
    if x.dim() < 1 or x.shape[-1] != K or x.numel() == 0:
        raise ValueError(f"mx_linear: x {tuple(x.shape)} does not match "
                         f"K={K}")
    if _mx_skinny_gate(x, x.numel() // K, N, K, fmt):
        x2, M, rs = _mx_check_x("mx_linear", x, K)
        out = _mx_skinny_launch(lib, x2, rs, w_payload, w_scales, fmt,
                                bias32, out_dtype, M, N, K,
                                mx_skinny_splits(M, N, K, fmt))
        return out.reshape(*x.shape[:-1], N)
    xq, xs = mx_quantize_rows(x)
    M = xq.numel() // K
    out = _mx_gemm_launch(lib, xq.reshape(M, K), xs.reshape(M, K // 32),
                          w_payload, w_scales, fmt, bias32, out_dtype, M, N,
                          K)
    return out.reshape(*x.shape[:-1], N)


# ---------------------------------------------------------------------------
# MXFP8 KV cache: fused decode attention + prefill store
# (csrc/decode_attn_mx.hip)
# ---------------------------------------------------------------------------

def decode_attn_mx_available() -> bool:
    lib = _load()
    return (lib is not None and hasattr(lib, "decode_attn_mx")
            and hasattr(lib, "mx_kv_store"))


def _mxkv_check_cache(who, k_payload, k_scale, v_payload, v_scale):
    """The four buffers of an MXKVCache: dense uint8 (B, Hkv, Smax, D) and
    (B, Hkv, Smax, D/32) on one GPU.  Returns (B, Hkv, Smax, D)."""
    for name, t in (("k_payload", k_payload), ("k_scale", k_scale),
                    ("v_payload", v_payload), ("v_scale", v_scale)):
        _mx_check_dense(f"{who}: {name}", t, torch.uint8)
        if t.dim() != 4 or t.device != k_payload.device:
            raise ValueError(f"{who}: {name} must be 4-D on "
                             f"{k_payload.device}, got {tuple(t.shape)} on "
                             f"{t.device}")
    B, Hkv, Smax, D = k_payload.shape
    if D < 32 or D % 32 or min(B, Hkv, Smax) < 1:
        raise ValueError(f"{who}: payload {tuple(k_payload.shape)} needs "
                         f"D % 32 == 0 and non-empty dims")
    if tuple(v_payload.shape) != (B, Hkv, Smax, D) or \
            tuple(k_scale.shape) != (B, Hkv, Smax, D // 32) or \
            tuple(v_scale.shape) != (B, Hkv, Smax, D // 32):
        raise ValueError(
            f"{who}: v_payload {tuple(v_payload.shape)}, k_scale "
            f"{tuple(k_scale.shape)}, v_scale {tuple(v_scale.shape)} do not "
            f"match k_payload {tuple(k_payload.shape)}")
    return B, Hkv, Smax, D


def decode_attn_mx_step(q2: torch.Tensor, k2: torch.Tensor, v2: torch.Tensor,
                        k_payload: torch.Tensor, k_scale: torch.Tensor,
                        v_payload: torch.Tensor, v_scale: torch.Tensor,
                        cos: torch.Tensor, sin: torch.Tensor,
                        pos_t: torch.Tensor, Hq: int, Hkv: int,
                        scale: float, *, ragged: bool = False
                        ) -> torch.Tensor:
    """:func:`decode_attn_step` over an MXFP8 cache (``MXKVCache`` buffers:
    e4m3 payload (B, Hkv, Smax, 128) + e8m0 scales (B, Hkv, Smax, 4), both
    uint8).  The new K (after RoPE) and V rows are quantized and appended at
    ``pos_t``; their bytes equal ``pack_mx(quantize_mx(row))``, and the
    output attends to the cache as stored, the new row included.  Everything
    is validated here; a wrong dtype or shape raises ValueError and launches
    nothing."""
    lib = _require_lib()
    who = "decode_attn_mx_step"
    if not decode_attn_mx_available():
        raise RuntimeError("nxd_ops library has no decode_attn_mx — rebuild")
    B, Hkv_c, Smax, D = _mxkv_check_cache(who, k_payload, k_scale, v_payload,
                                          v_scale)
    dev = k_payload.device
    if D != _DA_D or Hkv_c != Hkv:
        raise ValueError(f"{who}: cache {tuple(k_payload.shape)} with "
                         f"Hkv={Hkv} outside the kernel contract (D = 128)")
    T, st = _decode_attn_check(who, False, q2, k2, v2, cos, sin, pos_t, B, Hq,
                               Hkv, Smax, dev, ragged)
    fn = _ragged_entry(lib, "decode_attn_mx") if ragged else lib.decode_attn_mx
    return _decode_attn_launch(
        fn, False, (q2, k2, v2, k_payload, k_scale, v_payload, v_scale, cos,
                    sin, pos_t),
        B, T, Hq, Hkv, Smax, scale, st)


def mx_kv_store(k: torch.Tensor, v: torch.Tensor, k_payload: torch.Tensor,
                k_scale: torch.Tensor, v_payload: torch.Tensor,
                v_scale: torch.Tensor, pos: int) -> None:
    """Quantize bf16 k, v (B, Hkv, S, D) to MXFP8 straight into cache rows
    [pos, pos + S) in one launch.  k and v may be any strided views with a
    dense last dim (the models hand in transposes of (B, S, Hkv, D));
    strides must be multiples of 8 elements.  Written bytes equal
    ``pack_mx(*quantize_mx(x, "fp8_e4m3"))``.  Contract violations raise
    ValueError and launch nothing."""
    lib = _require_lib()
    who = "mx_kv_store"
    if not decode_attn_mx_available():
        raise RuntimeError("nxd_ops library has no mx_kv_store — rebuild")
    B, Hkv, Smax, D = _mxkv_check_cache(who, k_payload, k_scale, v_payload,
                                        v_scale)
    dev = k_payload.device
    if k.dim() != 4 or tuple(k.shape[:2]) != (B, Hkv) or k.shape[3] != D \
            or k.shape[2] < 1 or tuple(v.shape) != tuple(k.shape):
        raise ValueError(f"{who}: k {tuple(k.shape)} / v {tuple(v.shape)} do "
                         f"not match the cache {tuple(k_payload.shape)}")
    S = k.shape[2]
    pos = int(pos)
    if pos < 0 or pos + S > Smax:
        raise ValueError(f"{who}: rows [{pos}, {pos + S}) outside the cache "
                         f"of {Smax} rows")
    for name, t in (("k", k), ("v", v)):
        if t.dtype != torch.bfloat16 or t.device != dev:
            raise ValueError(f"{who}: {name} must be bf16 on {dev}, got "
                             f"{t.dtype} on {t.device}")
        if t.stride(3) != 1 or any(st < 0 or st % 8 for st in t.stride()[:3]) \
                or t.data_ptr() % 16:
            raise ValueError(f"{who}: {name} needs a dense last dim, strides "
                             f"that are multiples of 8 and 16-byte "
                             f"alignment, got strides {t.stride()}")
    rc = lib.mx_kv_store(_ptr(k), _ptr(v),
                         (ctypes.c_long * 4)(*k.stride()),
                         (ctypes.c_long * 4)(*v.stride()),
                         _ptr(k_payload), _ptr(k_scale), _ptr(v_payload),
                         _ptr(v_scale), B, Hkv, S, D, Smax,
                         ctypes.c_long(pos), _stream())
    if rc != 0:
        raise ValueError(f"mx_kv_store rejected k {tuple(k.shape)} strides "
                         f"{k.stride()} at pos {pos}, cache "
                         f"{tuple(k_payload.shape)}")


# ---------------------------------------------------------------------------
# Fused multi-token decode attention (csrc/chunk_attn.hip): T = 2..8 new
# tokens against the cache from a device position (speculative verification,
# chunked prefill)
# ---------------------------------------------------------------------------

def chunk_attn_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "chunk_attn")


def chunk_attn_mx_available() -> bool:
    lib = _load()
    return lib is not None and hasattr(lib, "chunk_attn_mx")


def chunk_attn_step(q3: torch.Tensor, k3: torch.Tensor, v3: torch.Tensor,
                    kcache: torch.Tensor, vcache: torch.Tensor,
                    cos: torch.Tensor, sin: torch.Tensor,
                    pos_t: torch.Tensor, Hq: int, Hkv: int,
                    scale: float, *, ragged: bool = False) -> torch.Tensor:
    """The multi-token sibling of :func:`decode_attn_step`: T = 2..8 new
    tokens per sequence.  q3 (B, T, Hq*128), k3/v3 (B, T, Hkv*128) bf16
    pre-rope (row-strided views with a dense last dim are fine);
    kcache/vcache bf16 (B, Hkv, Smax, 128); cos/sin (>= Smax, 64) fp32;
    ``pos_t`` one device int64 (``ragged``: (B,) of them, see
    :func:`decode_attn_step`) -> out (B, T, Hq*128).

    Token t is roped at position pos + t, its K/V row is stored at cache row
    pos + t (rows at or beyond Smax are not written) and it attends cache
    rows [0, pos + t] as stored.  Three launches on the current stream, no
    host sync: hipGraph-capturable.  A wrong dtype or shape raises
    ValueError and launches nothing."""
    lib = _require_lib()
    who = "chunk_attn_step"
    if not chunk_attn_available():
        raise RuntimeError("nxd_ops library has no chunk_attn — rebuild")
    B, Smax = _decode_attn_check_cache(who, kcache, vcache, Hkv)
    T, st = _decode_attn_check(who, True, q3, k3, v3, cos, sin, pos_t, B, Hq,
                               Hkv, Smax, kcache.device, ragged)
    fn = _ragged_entry(lib, "chunk_attn") if ragged else lib.chunk_attn
    return _decode_attn_launch(
        fn, True, (q3, k3, v3, kcache, vcache, cos, sin, pos_t),
        B, T, Hq, Hkv, Smax, scale, st)


def chunk_attn_mx_step(q3: torch.Tensor, k3: torch.Tensor, v3: torch.Tensor,
                       k_payload: torch.Tensor, k_scale: torch.Tensor,
                       v_payload: torch.Tensor, v_scale: torch.Tensor,
                       cos: torch.Tensor, sin: torch.Tensor,
                       pos_t: torch.Tensor, Hq: int, Hkv: int,
                       scale: float, *, ragged: bool = False
                       ) -> torch.Tensor:
    """:func:`chunk_attn_step` over an MXFP8 cache (``MXKVCache`` buffers).
    The T new K (after RoPE) and V rows are stored as
    ``pack_mx(quantize_mx(row))`` and the output attends to the cache as
    stored, the new rows included."""
    lib = _require_lib()
    who = "chunk_attn_mx_step"
    if not chunk_attn_mx_available():
        raise RuntimeError("nxd_ops library has no chunk_attn_mx — rebuild")
    B, Hkv_c, Smax, D = _mxkv_check_cache(who, k_payload, k_scale, v_payload,
                                          v_scale)
    dev = k_payload.device
    if D != _DA_D or Hkv_c != Hkv or not k_payload.is_cuda:
        raise ValueError(f"{who}: cache {tuple(k_payload.shape)} on {dev} "
                         f"with Hkv={Hkv} outside the kernel contract "
                         f"(D = 128, GPU)")
    T, st = _decode_attn_check(who, True, q3, k3, v3, cos, sin, pos_t, B, Hq,
                               Hkv, Smax, dev, ragged)
    fn = _ragged_entry(lib, "chunk_attn_mx") if ragged else lib.chunk_attn_mx
    return _decode_attn_launch(
        fn, True, (q3, k3, v3, k_payload, k_scale, v_payload, v_scale, cos,
                   sin, pos_t),
        B, T, Hq, Hkv, Smax, scale, st)
