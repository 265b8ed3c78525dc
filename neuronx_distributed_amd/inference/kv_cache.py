"""KV cache for GQA decode (reference trace/ StateInitializer-aliased
INPUT_STATE tensors, nxd_model.py:123-139 — here plain device-resident
buffers updated in place, hipGraph-compatible)."""

from typing import List

import torch


class KVCache:
    """One layer's cache: k/v (B, Hkv_local, S_max, D) bf16."""

    def __init__(self, batch: int, n_kv_heads: int, max_seq: int,
                 head_dim: int, dtype=torch.bfloat16, device=None):
        device = device or (torch.device("cuda") if torch.cuda.is_available()
                            else "cpu")
        self.k = torch.zeros(batch, n_kv_heads, max_seq, head_dim,
                             dtype=dtype, device=device)
        self.v = torch.zeros_like(self.k)
        self.max_seq = max_seq

    def update(self, k_new: torch.Tensor, v_new: torch.Tensor, pos):
        """k_new (B,H,S,D) written at [pos:pos+S]; returns views of the
        cache covering [0:pos+S].

        ``pos`` may be a device int64 tensor of shape (1,) (hipGraph
        decode): the write becomes index_copy_ and the FULL buffers are
        returned (attention masks by position — no dynamic shapes).  With
        S > 1 the rows go to ``pos + arange(S)``.

        A tensor of B > 1 positions is one per sequence: the rows go to
        ``(b, :, pos[b] + s)``.  A sequence with ``pos[b] < 0`` or
        ``pos[b] + S > max_seq`` is inactive and keeps its cache rows.  No
        host sync either."""
        if _is_ragged(pos, k_new.shape[0]):
            _ragged_write(pos, (self.k, k_new.to(self.k.dtype)),
                          (self.v, v_new.to(self.v.dtype)))
            return self.k, self.v
        if isinstance(pos, torch.Tensor):
            pos = _chunk_rows(pos, k_new.shape[2])
            self.k.index_copy_(2, pos, k_new.to(self.k.dtype))
            self.v.index_copy_(2, pos, v_new.to(self.v.dtype))
            return self.k, self.v
        S = k_new.shape[2]
        self.k[:, :, pos:pos + S] = k_new
        self.v[:, :, pos:pos + S] = v_new
        return self.k[:, :, :pos + S], self.v[:, :, :pos + S]


def _chunk_rows(pos: torch.Tensor, S: int) -> torch.Tensor:
    """Cache row indices of S new tokens at the device position ``pos``:
    ``pos`` itself for one token, ``pos + arange(S)`` for a chunk."""
    if S == 1:
        return pos
    return pos.reshape(1) + torch.arange(S, device=pos.device)


def _is_ragged(pos, B: int) -> bool:
    """One position per sequence: a tensor of B > 1 elements ((1,) with
    B = 1 means the same in both readings and stays the shared position)."""
    return isinstance(pos, torch.Tensor) and B > 1 and pos.numel() == B


def _ragged_write(pos: torch.Tensor, *pairs) -> None:
    """For each (buf (B,H,Smax,W), new (B,H,S,W)): new[b, :, s] into
    buf[b, :, pos[b] + s] for the active sequences, those with all S rows in
    [0, Smax).  An inactive one scatters back what its (clamped) rows hold,
    so the write has one static shape and no host sync."""
    B, _, S, _ = pairs[0][1].shape
    Smax = pairs[0][0].shape[2]
    pos = pos.reshape(B)
    active = ((pos >= 0) & (pos + S <= Smax)).view(B, 1, 1, 1)
    rows = pos.view(B, 1) + torch.arange(S, device=pos.device)
    rows = rows.clamp(0, Smax - 1).view(B, 1, S, 1)
    for buf, new in pairs:
        idx = rows.expand(B, buf.shape[1], S, buf.shape[3])
        buf.scatter_(2, idx, torch.where(active, new, buf.gather(2, idx)))


KV_FORMATS = (None, "mxfp8")


def build_kv_caches(n_layers: int, batch: int, n_kv_heads_local: int,
                    max_seq: int, head_dim: int, dtype=torch.bfloat16,
                    device=None, window=None, kv_format=None
                    ) -> List[KVCache]:
    """``window``: sliding-window models get RollingKVCache (O(window)
    memory per layer) when the window is smaller than max_seq.

    ``kv_format``: None stores K/V in ``dtype``; "mxfp8" returns
    :class:`MXKVCache` (e4m3 payload + e8m0 block scales, 0.516 of the bf16
    bytes) with ``dtype`` as the compute dtype.  The rolling cache has no
    MX form."""
    if kv_format not in KV_FORMATS:
        raise ValueError(f"kv_format {kv_format!r} not supported (one of "
                         f"{KV_FORMATS})")
    if kv_format == "mxfp8":
        if window is not None and window < max_seq:
            raise NotImplementedError(
                "kv_format='mxfp8' with a sliding window smaller than "
                "max_seq: the rolling cache has no MX form")
        return [MXKVCache(batch, n_kv_heads_local, max_seq, head_dim, dtype,
                          device)
                for _ in range(n_layers)]
    if window is not None and window < max_seq:
        return [RollingKVCache(batch, n_kv_heads_local, int(window),
                               head_dim, dtype, device)
                for _ in range(n_layers)]
    return [KVCache(batch, n_kv_heads_local, max_seq, head_dim, dtype, device)
            for _ in range(n_layers)]


class RollingKVCache(KVCache):
    """Window-bounded cache for sliding-window (Mistral-style) models:
    ``window`` slots addressed ``pos % window``, with ``slot_pos`` (W,)
    int64 tracking each slot's GLOBAL position (-1 = unwritten) so the
    decode step masks by true position while memory stays O(window)
    regardless of context length.  hipGraph-compatible: the tensor-pos
    update is index_copy_ on both the buffers and slot_pos.

    Supported pattern: one-shot prefill from position 0, then per-token
    decode (the serving pattern); chunked prefill at pos > 0 would need
    a rotated gather and raises."""

    def __init__(self, batch: int, n_kv_heads: int, window: int,
                 head_dim: int, dtype=torch.bfloat16, device=None):
        super().__init__(batch, n_kv_heads, window, head_dim, dtype, device)
        self.window = window
        self.slot_pos = torch.full((window,), -1, dtype=torch.long,
                                   device=self.k.device)

    def position_index(self) -> torch.Tensor:
        return self.slot_pos

    def update(self, k_new: torch.Tensor, v_new: torch.Tensor, pos):
        if isinstance(pos, torch.Tensor) and pos.numel() > 1:
            raise NotImplementedError(
                "RollingKVCache keeps one position for the whole batch; "
                "per-sequence positions need a plain cache")
        if isinstance(pos, torch.Tensor):  # decode: one token
            if k_new.shape[2] != 1:
                raise NotImplementedError(
                    "RollingKVCache takes one token per tensor-position "
                    "update; a multi-token chunk needs a plain cache")
            slot = pos % self.window
            self.k.index_copy_(2, slot, k_new.to(self.k.dtype))
            self.v.index_copy_(2, slot, v_new.to(self.v.dtype))
            self.slot_pos.index_copy_(0, slot, pos)
            return self.k, self.v
        S = k_new.shape[2]
        if pos != 0:
            raise NotImplementedError(
                "RollingKVCache supports one-shot prefill from pos 0")
        # keep only the last ``window`` prefill rows (older ones can
        # never be attended again)
        tail = min(S, self.window)
        idx = torch.arange(S - tail, S, device=self.k.device)
        slot = idx % self.window
        self.k.index_copy_(2, slot, k_new[:, :, S - tail:].to(self.k.dtype))
        self.v.index_copy_(2, slot, v_new[:, :, S - tail:].to(self.v.dtype))
        self.slot_pos.index_copy_(0, slot, idx)
        # prefill attention runs over the CURRENT chunk directly (the
        # cache held nothing before position 0)
        return k_new, v_new


class MXKVCache(KVCache):
    """One layer's cache in MXFP8: 0.516 of the bf16 bytes at D = 128.

    ``k``, ``v``: uint8 (B, Hkv, S_max, D), the e4m3 payload; ``k_scale``,
    ``v_scale``: uint8 (B, Hkv, S_max, D/32), biased e8m0.  Blocks of 32 run
    along D; the layout is exactly
    ``pack_mx(*quantize_mx(x, "fp8_e4m3"), "fp8_e4m3")`` of the (..., D)
    rows, which is also what the fused decode kernel
    (ops.decode_attn_mx_step) reads and appends.  ``dtype`` is the compute
    dtype of the dequantized views.

    The cache is the single source of truth: ``update`` returns DEQUANTIZED
    views of what it holds, the rows just written included, so prefill,
    eager decode, chunked verification and the fused kernel all attend to
    the same values.  On every path but the fused kernel that view is a
    transient copy in ``dtype`` of the rows it covers ([0, pos + S) for an
    int ``pos``, the whole buffer for a tensor ``pos``); only the fused
    kernel streams the quantized bytes.

    bf16 GPU tensors are quantized by the native kernels (ops.mx_kv_store
    for an int ``pos``, ops.mx_quantize_rows for a tensor ``pos``); CPU
    tensors and other dtypes go through quantization.microscaling."""

    def __init__(self, batch: int, n_kv_heads: int, max_seq: int,
                 head_dim: int, dtype=torch.bfloat16, device=None):
        if head_dim < 32 or head_dim % 32 != 0:
            raise ValueError(f"MXKVCache: head_dim {head_dim} must be a "
                             f"multiple of the MX block (32)")
        device = device or (torch.device("cuda") if torch.cuda.is_available()
                            else "cpu")
        self.k = torch.zeros(batch, n_kv_heads, max_seq, head_dim,
                             dtype=torch.uint8, device=device)
        self.v = torch.zeros_like(self.k)
        self.k_scale = torch.zeros(batch, n_kv_heads, max_seq, head_dim // 32,
                                   dtype=torch.uint8, device=device)
        self.v_scale = torch.zeros_like(self.k_scale)
        self.max_seq = max_seq
        self.dtype = dtype

    @staticmethod
    def _native(x: torch.Tensor) -> bool:
        return x.is_cuda and x.dtype == torch.bfloat16

    @staticmethod
    def _quantize(x: torch.Tensor):
        """(..., D) -> (payload, scales) uint8 in the stored layout."""
        if MXKVCache._native(x):
            from .. import ops

            return ops.mx_quantize_rows(x.contiguous())
        from ..quantization.microscaling import pack_mx, quantize_mx

        return pack_mx(*quantize_mx(x, "fp8_e4m3"), "fp8_e4m3")

    def _dequantize(self, payload: torch.Tensor, scale: torch.Tensor):
        from ..quantization.microscaling import dequantize_mx, unpack_mx

        return dequantize_mx(*unpack_mx(payload, scale, "fp8_e4m3"),
                             dtype=self.dtype)

    def update(self, k_new: torch.Tensor, v_new: torch.Tensor, pos):
        """Same signature and modes as :meth:`KVCache.update`; the returned
        K, V are dequantized copies in ``dtype`` (class docstring)."""
        if _is_ragged(pos, k_new.shape[0]):
            kq, ks = self._quantize(k_new)
            vq, vs = self._quantize(v_new)
            _ragged_write(pos, (self.k, kq), (self.k_scale, ks),
                          (self.v, vq), (self.v_scale, vs))
            return (self._dequantize(self.k, self.k_scale),
                    self._dequantize(self.v, self.v_scale))
        if isinstance(pos, torch.Tensor):
            pos = _chunk_rows(pos, k_new.shape[2])
            kq, ks = self._quantize(k_new)
            vq, vs = self._quantize(v_new)
            self.k.index_copy_(2, pos, kq)
            self.k_scale.index_copy_(2, pos, ks)
            self.v.index_copy_(2, pos, vq)
            self.v_scale.index_copy_(2, pos, vs)
            return (self._dequantize(self.k, self.k_scale),
                    self._dequantize(self.v, self.v_scale))
        S = k_new.shape[2]
        if self._native(k_new) and self._native(v_new):
            from .. import ops

            ops.mx_kv_store(k_new, v_new, self.k, self.k_scale, self.v,
                            self.v_scale, pos)
        else:
            kq, ks = self._quantize(k_new)
            vq, vs = self._quantize(v_new)
            self.k[:, :, pos:pos + S] = kq
            self.k_scale[:, :, pos:pos + S] = ks
            self.v[:, :, pos:pos + S] = vq
            self.v_scale[:, :, pos:pos + S] = vs
        end = pos + S
        return (self._dequantize(self.k[:, :, :end], self.k_scale[:, :, :end]),
                self._dequantize(self.v[:, :, :end], self.v_scale[:, :, :end]))
