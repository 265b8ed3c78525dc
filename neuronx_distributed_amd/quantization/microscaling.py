"""OCP Microscaling (MX) quantization — torch emulation (reference
experimental/quantization/microscaling/mx_torch.py:65-203).

MXFP8/MXFP4: per-32-element blocks share an e8m0 power-of-two scale.  On
CDNA4 this maps natively onto ``v_mfma_scale_*_f8f6f4`` (the ONLY path to
the 5/10 PF low-precision peaks, cdna_hip_programming.md §3/§4); this
module provides the numerics-faithful emulation used for quantized-weight
preparation and accuracy studies."""

from typing import Tuple

import torch

MX_BLOCK = 32

_FMT = {
    "fp8_e4m3": (448.0, torch.float8_e4m3fn),
    "fp8_e5m2": (57344.0, torch.float8_e5m2),
    # fp4 e2m1: emulated via rounding to the 16-value grid
    "fp4_e2m1": (6.0, None),
}

_FP4_GRID = torch.tensor([0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0])


def _round_fp4(x: torch.Tensor) -> torch.Tensor:
    sign = x.sign()
    mag = x.abs().clamp(max=6.0)
    grid = _FP4_GRID.to(x.device)
    idx = torch.bucketize(mag, (grid[1:] + grid[:-1]) / 2)
    return sign * grid[idx]


def quantize_mx(x: torch.Tensor, fmt: str = "fp8_e4m3", axis: int = -1
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Quantize along ``axis`` in blocks of 32 with shared e8m0 scales.
    Returns (q, scales) with x ~= q * 2**scales (q in the element format,
    kept as the emulation dtype)."""
    emax, qdtype = _FMT[fmt]
    x = x.movedim(axis, -1)
    orig = x.shape
    assert orig[-1] % MX_BLOCK == 0
    xb = x.reshape(*orig[:-1], orig[-1] // MX_BLOCK, MX_BLOCK).float()
    amax = xb.abs().amax(dim=-1, keepdim=True).clamp(min=2.0 ** -126)
    # e8m0: power-of-two scale so the block max lands INSIDE the element
    # range (ceil: scaled max in (emax/2, emax], never overflowing e4m3fn's
    # finite-only encoding)
    scales = torch.ceil(torch.log2(amax / emax)).clamp(-127, 127)
    scaled = xb / torch.exp2(scales)
    if fmt == "fp4_e2m1":
        q = _round_fp4(scaled)
    else:
        q = scaled.to(qdtype).float()
    q = q.reshape(orig).movedim(-1, axis)
    return q, scales.squeeze(-1)


def dequantize_mx(q: torch.Tensor, scales: torch.Tensor, axis: int = -1,
                  dtype=torch.bfloat16) -> torch.Tensor:
    x = q.movedim(axis, -1).float()
    orig = x.shape
    xb = x.reshape(*orig[:-1], orig[-1] // MX_BLOCK, MX_BLOCK)
    out = xb * torch.exp2(scales.float()).unsqueeze(-1)
    return out.reshape(orig).movedim(-1, axis).to(dtype)


def mx_matmul(a: torch.Tensor, qb: torch.Tensor, b_scales: torch.Tensor,
              dtype=torch.bfloat16) -> torch.Tensor:
    """a (bf16) @ dequant(qb) — emulation of the scaled-MFMA GEMM."""
    return a.to(dtype) @ dequantize_mx(qb, b_scales, axis=-2, dtype=dtype)


# ---------------------------------------------------------------------------
# Stored MX format + the MX linear (native kernels: ops/csrc/mx_gemm.hip,
# the 128x128 tile, and ops/csrc/mx_skinny.hip, the M <= 32 decode kernel
# that quantizes x inside the GEMM; both read the layout below as stored)
#
# Public layout contract (what checkpoints and the HIP kernel share):
#   fp8_e4m3 payload  uint8 (..., K)    one e4m3fn byte per element
#   fp4_e2m1 payload  uint8 (..., K/2)  element 2i in the LOW nibble, 2i+1 in
#                                       the high nibble; nibble = sign<<3 |
#                                       index into _FP4_GRID
#   scales            uint8 (..., K/32) biased e8m0: byte = scale + 127
#                                       (0..254; 255 never occurs)
# Supported natively: fp8_e4m3 activations x {fp8_e4m3, fp4_e2m1} weights,
# forward only; and the fp8_e4m3 layout as KV-cache storage along head_dim
# (inference/kv_cache.py MXKVCache, ops/csrc/decode_attn_mx.hip).  fp6 / e5m2, backward and grouped (MoE) MX GEMMs are out of
# scope; mx_matmul and moe.blockwise_mm_mx keep their emulation.
# ---------------------------------------------------------------------------

MX_NATIVE_FORMATS = ("fp8_e4m3", "fp4_e2m1")
MX_GEMM_K = 128   # native kernel contract: K % 128 == 0, N % 16 == 0
MX_GEMM_N = 16


def _check_native_fmt(fmt: str):
    if fmt not in MX_NATIVE_FORMATS:
        raise ValueError(f"MX storage format {fmt!r} not supported "
                         f"(one of {MX_NATIVE_FORMATS})")


def pack_mx(q: torch.Tensor, scales: torch.Tensor, fmt: str
            ) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q, scales) of ``quantize_mx(..., axis=-1)`` -> (payload, scales) in
    the stored uint8 layout above."""
    _check_native_fmt(fmt)
    if fmt == "fp8_e4m3":
        payload = q.to(torch.float8_e4m3fn).view(torch.uint8)
    else:
        if q.shape[-1] % 2:
            raise ValueError(f"fp4 payload needs an even K, got {q.shape}")
        idx = torch.bucketize(q.abs().float(), _FP4_GRID.to(q.device))
        code = (idx | (torch.signbit(q).to(idx.dtype) << 3)).to(torch.uint8)
        payload = code[..., 0::2] | (code[..., 1::2] << 4)
    return payload.contiguous(), (scales + 127).to(torch.uint8)


def unpack_mx(payload: torch.Tensor, scales: torch.Tensor, fmt: str
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Inverse of :func:`pack_mx`: bit-identical (q, scales) in the
    emulation dtype (fp32)."""
    _check_native_fmt(fmt)
    if fmt == "fp8_e4m3":
        q = payload.view(torch.float8_e4m3fn).float()
    else:
        code = torch.stack([payload & 0xF, payload >> 4], dim=-1)
        code = code.reshape(*payload.shape[:-1], payload.shape[-1] * 2)
        mag = _FP4_GRID.to(payload.device)[(code & 7).long()]
        q = torch.where((code & 8) != 0, -mag, mag)
    return q, scales.float() - 127.0


def mx_payload_k(payload: torch.Tensor, fmt: str) -> int:
    return payload.shape[-1] * (2 if fmt == "fp4_e2m1" else 1)


def mx_linear_emulated(x: torch.Tensor, w_payload: torch.Tensor,
                       w_scales: torch.Tensor, fmt: str, bias=None,
                       out_dtype=None) -> torch.Tensor:
    """Reference MX linear: x is quantized to MXFP8 per 32-block, both
    operands are dequantized to fp32, multiplied, and cast."""
    wq, ws = unpack_mx(w_payload, w_scales, fmt)
    xq, xs = quantize_mx(x, "fp8_e4m3")
    y = dequantize_mx(xq, xs, dtype=torch.float32) @ \
        dequantize_mx(wq, ws, dtype=torch.float32).t()
    if bias is not None:
        y = y + bias.float()
    return y.to(out_dtype or x.dtype)


def mx_native_shape_ok(x: torch.Tensor, w_payload: torch.Tensor,
                       fmt: str) -> bool:
    """Inside the HIP kernel's contract (bf16 x, K % 128, N % 16)?"""
    K = x.shape[-1]
    return (x.dtype == torch.bfloat16 and x.numel() > 0
            and K % MX_GEMM_K == 0 and w_payload.shape[0] % MX_GEMM_N == 0)


def mx_linear(x: torch.Tensor, w_payload: torch.Tensor,
              w_scales: torch.Tensor, fmt: str, bias=None) -> torch.Tensor:
    """y = x . W^T with W stored in MX format (``pack_mx``) and x quantized
    to MXFP8 on the fly.  Inference only.

    GPU tensors inside the kernel contract run the native block-scaled MFMA
    GEMM (a missing library raises); CPU tensors and shapes outside the
    contract run :func:`mx_linear_emulated`, the numerical reference."""
    _check_native_fmt(fmt)
    if w_payload.dim() != 2 or mx_payload_k(w_payload, fmt) != x.shape[-1]:
        raise ValueError(f"mx_linear: x {tuple(x.shape)} does not match "
                         f"{fmt} payload {tuple(w_payload.shape)}")
    if x.is_cuda and mx_native_shape_ok(x, w_payload, fmt):
        from .. import ops

        return ops.mx_linear(x, w_payload, w_scales, fmt, bias=bias)
    return mx_linear_emulated(x, w_payload, w_scales, fmt, bias=bias)
