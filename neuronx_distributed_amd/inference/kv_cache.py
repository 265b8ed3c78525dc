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

    def commit_path(self, pos: torch.Tensor, path: torch.Tensor) -> None:
        """After a tree step at the device position ``pos`` (one element, or
        one per sequence): pack the accepted root path down to consecutive
        rows.  ``path`` (B, L) integer, L <= 16: column 0 is the root, then
        the accepted node indices, then -1.  Row ``pos + d`` takes what row
        ``pos + path[b, d]`` held for every d >= 1 with a valid entry; all
        sources are read before any row is written.  Entries that are
        negative, 16 or more, or whose rows fall outside the cache move
        nothing.  No host sync.  ops.tree_kv_commit on a bf16 GPU cache with
        head dim 128, torch index ops otherwise."""
        from .. import ops

        if type(self) is not KVCache:
            raise NotImplementedError(
                f"commit_path needs a plain KVCache, not "
                f"{type(self).__name__}")
        B, _, Smax, D = self.k.shape
        ragged = _is_ragged(pos, B)
        if self.k.is_cuda and self.k.dtype == torch.bfloat16 and D == 128 \
                and ops.tree_attn_available():
            ops.tree_kv_commit(
                self.k, self.v,
                pos.reshape(B).contiguous() if ragged else pos.reshape(1),
                path.to(torch.int32).contiguous(), ragged=ragged)
            return
        L = path.shape[1]
        node = path.long()
        pos_b = pos.reshape(-1, 1).expand(B, 1)
        d = torch.arange(L, device=path.device).view(1, L)
        ok = (d >= 1) & (node >= 0) & (node < 16) & (pos_b >= 0) \
            & (pos_b + torch.maximum(node, d) < Smax)
        # an entry that moves nothing rewrites row pos (clamped) with itself;
        # no valid entry writes there, its d being at least 1
        keep = pos_b.clamp(0, Smax - 1).expand(B, L)
        src = torch.where(ok, pos_b + node, keep).view(B, 1, L, 1)
        dst = torch.where(ok, pos_b + d, keep).view(B, 1, L, 1)
        for buf in (self.k, self.v):
            shape = (B, buf.shape[1], L, D)
            buf.scatter_(2, dst.expand(shape), buf.gather(2, src.expand(shape)))


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


KV_FORMATS = (None, "mxfp8", "paged", "paged_mxfp8")


def build_kv_caches(n_layers: int, batch: int, n_kv_heads_local: int,
                    max_seq: int, head_dim: int, dtype=torch.bfloat16,
                    device=None, window=None, kv_format=None, page_pool=None
                    ) -> List[KVCache]:
    """``window``: sliding-window models get RollingKVCache (O(window)
    memory per layer) when the window is smaller than max_seq.

    ``kv_format``: None stores K/V in ``dtype``; "mxfp8" returns
    :class:`MXKVCache` (e4m3 payload + e8m0 block scales, 0.516 of the bf16
    bytes) with ``dtype`` as the compute dtype.  The rolling cache has no
    MX form.  "paged" returns :class:`PagedKVCache` layers on the
    :class:`PagePool` ``page_pool``, whose table all layers share; it has
    no rolling form either.  "paged_mxfp8" is the same with
    :class:`PagedMXKVCache` layers: MXFP8 rows inside the pages."""
    if kv_format not in KV_FORMATS:
        raise ValueError(f"kv_format {kv_format!r} not supported (one of "
                         f"{KV_FORMATS})")
    if kv_format in ("paged", "paged_mxfp8"):
        if window is not None and window < max_seq:
            raise NotImplementedError(
                f"kv_format={kv_format!r} with a sliding window smaller "
                f"than max_seq: the rolling cache has no paged form")
        if page_pool is None or page_pool.batch != batch:
            raise ValueError(f"kv_format={kv_format!r} needs a page_pool "
                             f"for a batch of {batch}")
        cls = PagedKVCache if kv_format == "paged" else PagedMXKVCache
        return [cls(page_pool, n_kv_heads_local, head_dim, dtype, device)
                for _ in range(n_layers)]
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


PAGE_ROWS = 16   # rows of a page; PG_ROWS of ops/csrc/paged_attn.hip


class PagePool:
    """``num_pages`` pages of PAGE_ROWS cache rows, shared by ``batch``
    sequences of at most ``pages_per_seq`` pages each.

    ``block_table`` int32 (batch, pages_per_seq) on the device is the one
    table all layers' :class:`PagedKVCache` read: entry [b, j] is the pool
    page of rows [16 j, 16 j + 16) of sequence b, -1 = not allocated.  The
    free list lives on the host; ``allocate`` and ``release`` ``copy_`` the
    new table into the same device buffer, so a captured hipGraph sees the
    update."""

    def __init__(self, num_pages: int, batch: int, pages_per_seq: int,
                 device=None):
        if min(num_pages, batch, pages_per_seq) < 1:
            raise ValueError(f"PagePool({num_pages}, {batch}, "
                             f"{pages_per_seq}): sizes must be positive")
        device = device or (torch.device("cuda") if torch.cuda.is_available()
                            else "cpu")
        self.num_pages, self.batch = num_pages, batch
        self.pages_per_seq = pages_per_seq
        self._host = torch.full((batch, pages_per_seq), -1, dtype=torch.int32)
        self.block_table = self._host.to(device)
        self._free = list(range(num_pages - 1, -1, -1))  # page 0 goes first
        self._held = [0] * batch   # pages of each sequence

    @property
    def num_free(self) -> int:
        return len(self._free)

    def allocate(self, b: int, n_rows: int) -> None:
        """Grow sequence ``b`` to cover rows [0, n_rows); raises, changing
        nothing, if the table row or the pool cannot hold them."""
        need = -(-int(n_rows) // PAGE_ROWS)
        if need > self.pages_per_seq:
            raise ValueError(f"{n_rows} rows need {need} pages, a sequence "
                             f"holds at most {self.pages_per_seq}")
        grow = need - self._held[b]
        if grow <= 0:
            return
        if grow > len(self._free):
            raise RuntimeError(f"PagePool out of pages: sequence {b} needs "
                               f"{grow} more, {len(self._free)} of "
                               f"{self.num_pages} are free")
        for j in range(self._held[b], need):
            self._host[b, j] = self._free.pop()
        self._held[b] = need
        self.block_table.copy_(self._host)

    def release(self, b: int) -> None:
        """Return the pages of sequence ``b``; its entries become -1."""
        self._free.extend(reversed(self._host[b, :self._held[b]].tolist()))
        self._host[b] = -1
        self._held[b] = 0
        self.block_table.copy_(self._host)


class PagedKVCache:
    """One layer's K/V in the pages of a :class:`PagePool`: ``k_pages``,
    ``v_pages`` (num_pages, Hkv, PAGE_ROWS, D), addressed through the pool's
    ``block_table``.  A sequence holds only the pages it was allocated, not
    max_seq rows.

    No table entry is trusted, here as in the kernels (ops.paged_attn_step,
    ops.paged_kv_store): a prefill row whose page entry lies outside
    [0, num_pages) is skipped, and a decode write of S rows at ``pos[b]``
    happens only for an ACTIVE sequence (:meth:`active`).

    bf16 GPU tensors with D = 128 are stored by the native kernels; CPU
    tensors and other dtypes go through gather / scatter, the reference."""

    def __init__(self, pool: PagePool, n_kv_heads: int, head_dim: int,
                 dtype=torch.bfloat16, device=None):
        self.pool = pool
        device = device or pool.block_table.device
        # one page more than the pool: where the reference path sends the
        # writes it skips, so that its scatter keeps one static shape
        self._k = torch.zeros(pool.num_pages + 1, n_kv_heads, PAGE_ROWS,
                              head_dim, dtype=dtype, device=device)
        self._v = torch.zeros_like(self._k)
        self.k_pages = self._k[:pool.num_pages]
        self.v_pages = self._v[:pool.num_pages]
        self.max_seq = PAGE_ROWS * pool.pages_per_seq

    def _valid(self) -> torch.Tensor:
        """(B, pages_per_seq): the table entries that name a pool page."""
        t = self.pool.block_table
        return (t >= 0) & (t < self.pool.num_pages)

    def active(self, pos: torch.Tensor, S: int = 1,
               chunk_lens=None) -> torch.Tensor:
        """(B,) bool for S new rows at ``pos`` (B,): all of them inside
        [0, 16 * pages_per_seq) and every table entry up to the page of the
        last one valid.  No host sync.

        ``chunk_lens`` (B,): only the first ``n[b] = chunk_lens[b]`` of the S
        rows are real (chunked prefill).  ``n[b]`` then takes the place of S
        and must lie in [1, S]; ``n[b] = 0`` is inactive."""
        pps = self.pool.pages_per_seq
        pos = pos.reshape(-1, 1)
        n = S if chunk_lens is None else chunk_lens.reshape(-1, 1)
        last = torch.div(pos + n - 1, PAGE_ROWS, rounding_mode="floor")
        beyond = torch.arange(pps, device=pos.device).view(1, pps) > last
        ok = (self._valid() | beyond).all(dim=1)
        if chunk_lens is not None:
            ok = ok & (n[:, 0] >= 1) & (n[:, 0] <= S)
        return ok & (pos[:, 0] >= 0) & ((pos + n)[:, 0] <= self.max_seq)

    def _scatter(self, k_new, v_new, rows, ok) -> None:
        """The reference write: k_new/v_new (B, Hkv, S, D) to rows (B, S) of
        their sequences where ``ok`` (B, S) and the row's page is valid; the
        rest lands in the spare page.  No host sync."""
        pps, n = self.pool.pages_per_seq, self.pool.num_pages
        j = torch.div(rows, PAGE_ROWS, rounding_mode="floor")
        ok = ok & (j >= 0) & (j < pps)
        j = j.clamp(0, pps - 1)
        ok = ok & self._valid().gather(1, j)
        page = torch.where(ok, self.pool.block_table.gather(1, j).long(), n)
        slot = rows % PAGE_ROWS
        self._k[page, :, slot] = k_new.permute(0, 2, 1, 3).to(self._k.dtype)
        self._v[page, :, slot] = v_new.permute(0, 2, 1, 3).to(self._v.dtype)

    def update(self, k_new: torch.Tensor, v_new: torch.Tensor, pos,
               chunk_lens=None):
        """k_new, v_new (B, Hkv, S, D).  An int ``pos`` of 0 is the prefill:
        rows [0, S) go to their pages and (k_new, v_new) come back for the
        flash kernel.  A (B,) tensor is the decode write of the active
        sequences at ``pos[b] + s`` (one element counts for every sequence);
        it returns :meth:`gather`.  An int ``pos`` > 0 has no paged form.

        ``chunk_lens`` (B,), with a tensor ``pos`` only: the chunked-prefill
        write of the first ``chunk_lens[b]`` rows of each sequence that is
        active by :meth:`active` with the same argument; the other rows are
        padding and nothing is stored for them."""
        B, _, S, D = k_new.shape
        dev = k_new.device
        if isinstance(pos, torch.Tensor):
            pos = pos.reshape(-1).expand(B)
            steps = torch.arange(S, device=dev)
            rows = pos.view(B, 1) + steps
            ok = self.active(pos, S, chunk_lens).view(B, 1).expand(B, S)
            if chunk_lens is not None:
                ok = ok & (steps < chunk_lens.reshape(B, 1))
            self._scatter(k_new, v_new, rows, ok)
            return self.gather()
        if chunk_lens is not None:
            raise ValueError("chunk_lens needs a device-tensor position")
        if pos != 0:
            raise NotImplementedError(
                "PagedKVCache takes a one-shot prefill from pos 0, then "
                "device-tensor positions")
        if k_new.is_cuda and D == 128 and k_new.dtype == torch.bfloat16 \
                and self._k.dtype == torch.bfloat16:
            from .. import ops

            ops.paged_kv_store(k_new, v_new, self.k_pages, self.v_pages,
                               self.pool.block_table, 0)
        else:
            rows = torch.arange(S, device=dev).expand(B, S)
            self._scatter(k_new, v_new, rows, rows >= 0)
        return k_new, v_new

    def gather(self):
        """Dense (B, Hkv, 16 * pages_per_seq, D) copies of K and V built
        from the table; pages without a valid entry read as zeros."""
        t = self.pool.block_table
        B, pps = t.shape
        valid = self._valid().view(B, 1, pps, 1, 1)
        idx = t.clamp(0, self.pool.num_pages - 1).long()
        out = []
        for pages in (self.k_pages, self.v_pages):
            x = pages[idx].transpose(1, 2)   # (B, Hkv, pps, 16, D)
            x = torch.where(valid, x, 0)
            out.append(x.reshape(B, x.shape[1], self.max_seq, x.shape[4]))
        return tuple(out)


class PagedMXKVCache(PagedKVCache):
    """One layer's K/V in MXFP8 inside the pages of a :class:`PagePool`:
    ``k_pages``, ``v_pages`` uint8 (num_pages, Hkv, PAGE_ROWS, D), the e4m3
    payload, and ``k_scale_pages``, ``v_scale_pages`` uint8 (num_pages, Hkv,
    PAGE_ROWS, D/32), biased e8m0.  A row's bytes are exactly
    ``pack_mx(*quantize_mx(row, "fp8_e4m3"), "fp8_e4m3")``, the layout of
    :class:`MXKVCache` row for row: 0.516 of the bf16 pools' bytes at
    D = 128, on top of what paging saves.

    Interface, activity rule and spare page are :class:`PagedKVCache`'s.  As
    with :class:`MXKVCache` the cache is the single source of truth:
    :meth:`gather`, and so what :meth:`update` returns for a tensor
    position, are DEQUANTIZED copies in the compute ``dtype``, the rows just
    written included.  Only the fused kernel (ops.paged_attn_mx_step) streams
    the quantized bytes.

    bf16 GPU tensors with D = 128 are stored by the native prefill kernel
    (ops.paged_mx_kv_store); CPU tensors and other dtypes quantize through
    quantization.microscaling and scatter, the reference."""

    def __init__(self, pool: PagePool, n_kv_heads: int, head_dim: int,
                 dtype=torch.bfloat16, device=None):
        if head_dim < 32 or head_dim % 32 != 0:
            raise ValueError(f"PagedMXKVCache: head_dim {head_dim} must be a "
                             f"multiple of the MX block (32)")
        self.pool = pool
        device = device or pool.block_table.device
        n = pool.num_pages
        # the spare page of PagedKVCache, in all four pools
        self._k = torch.zeros(n + 1, n_kv_heads, PAGE_ROWS, head_dim,
                              dtype=torch.uint8, device=device)
        self._v = torch.zeros_like(self._k)
        self._ks = torch.zeros(n + 1, n_kv_heads, PAGE_ROWS, head_dim // 32,
                               dtype=torch.uint8, device=device)
        self._vs = torch.zeros_like(self._ks)
        self.k_pages, self.v_pages = self._k[:n], self._v[:n]
        self.k_scale_pages, self.v_scale_pages = self._ks[:n], self._vs[:n]
        self.max_seq = PAGE_ROWS * pool.pages_per_seq
        self.dtype = dtype

    def _scatter(self, k_new, v_new, rows, ok) -> None:
        """:meth:`PagedKVCache._scatter` of the quantized rows: payload and
        scales go to the same (page, slot), skipped ones to the spare page."""
        pps, n = self.pool.pages_per_seq, self.pool.num_pages
        j = torch.div(rows, PAGE_ROWS, rounding_mode="floor")
        ok = ok & (j >= 0) & (j < pps)
        j = j.clamp(0, pps - 1)
        ok = ok & self._valid().gather(1, j)
        page = torch.where(ok, self.pool.block_table.gather(1, j).long(), n)
        slot = rows % PAGE_ROWS
        for new, pay, scl in ((k_new, self._k, self._ks),
                              (v_new, self._v, self._vs)):
            q, s = MXKVCache._quantize(new.permute(0, 2, 1, 3))
            pay[page, :, slot] = q
            scl[page, :, slot] = s

    def update(self, k_new: torch.Tensor, v_new: torch.Tensor, pos,
               chunk_lens=None):
        """Signature and modes of :meth:`PagedKVCache.update`.  The int
        ``pos`` = 0 prefill stores the quantized rows and returns
        (k_new, v_new); a tensor ``pos`` returns :meth:`gather`, dequantized
        copies of what the pages hold."""
        if isinstance(pos, torch.Tensor) or chunk_lens is not None \
                or pos != 0:
            return super().update(k_new, v_new, pos, chunk_lens)
        B, _, S, D = k_new.shape
        if k_new.is_cuda and D == 128 and k_new.dtype == torch.bfloat16 \
                and v_new.dtype == torch.bfloat16:
            from .. import ops

            ops.paged_mx_kv_store(k_new, v_new, self.k_pages,
                                  self.k_scale_pages, self.v_pages,
                                  self.v_scale_pages, self.pool.block_table,
                                  0)
        else:
            rows = torch.arange(S, device=k_new.device).expand(B, S)
            self._scatter(k_new, v_new, rows, rows >= 0)
        return k_new, v_new

    def gather(self):
        """Dense (B, Hkv, 16 * pages_per_seq, D) DEQUANTIZED copies of K and
        V in ``dtype`` built from the table; pages without a valid entry
        read as zeros."""
        from ..quantization.microscaling import dequantize_mx, unpack_mx

        t = self.pool.block_table
        B, pps = t.shape
        valid = self._valid().view(B, 1, pps, 1, 1)
        idx = t.clamp(0, self.pool.num_pages - 1).long()
        out = []
        for pay, scl in ((self.k_pages, self.k_scale_pages),
                         (self.v_pages, self.v_scale_pages)):
            # zero bytes dequantize to zero: 0 * 2^-127
            p = torch.where(valid, pay[idx].transpose(1, 2), 0)
            s = torch.where(valid, scl[idx].transpose(1, 2), 0)
            x = dequantize_mx(*unpack_mx(p, s, "fp8_e4m3"), dtype=self.dtype)
            out.append(x.reshape(B, x.shape[1], self.max_seq, x.shape[4]))
        return tuple(out)
