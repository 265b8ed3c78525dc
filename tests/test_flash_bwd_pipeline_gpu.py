"""GPU checks for the flash-attention backward pipeline: single dual-use
LDS image + hardware transposed reads, double-buffered staging, the
interior-tile fast path and dK/dV returned in the consumer's layout.

Shapes are the smallest that reach every path of the two backward kernels
(single tile, buffer swap, ragged S, GQA, all-interior, window edges)."""

import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops
from neuronx_distributed_amd.kernels.flash_attn import _torch_reference

D = 128


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    ops.build = __import__("neuronx_distributed_amd.ops.build",
                           fromlist=["build"])
    ops.build.build()
    assert ops.is_available(), ops._LIB_ERR


def _cmp(a, b, atol, rtol=2e-2, name=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{name}: max err {err} (ref max {ref})"


def _inputs(B, Hq, Hkv, S, seed, boost_k_rows=None):
    """bf16 BSHD storage (the model's activation layout), values * 0.5."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def mk(h):
        return torch.randn(B, S, h, D, dtype=torch.bfloat16, device="cuda",
                           generator=g) * 0.5

    q, k, v = mk(Hq), mk(Hkv), mk(Hkv)
    if boost_k_rows is not None:
        lo, hi = boost_k_rows
        k[:, lo:hi] *= 8
    dy = torch.randn(B, S, Hq, D, dtype=torch.bfloat16, device="cuda",
                     generator=g)
    return q, k, v, dy


def _run(q, k, v, dy, causal, window, bshd):
    """fwd + bwd through ops.flash_attn.  bshd=True feeds transpose VIEWS of
    the BSHD storage; otherwise contiguous BHSD copies.  Returns grads as
    (B,H,S,D)-indexed tensors plus the raw leaf grads."""
    if bshd:
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
        args = [t.transpose(1, 2) for t in leaves]
        dyv = dy.transpose(1, 2)
    else:
        leaves = [t.transpose(1, 2).contiguous().requires_grad_(True)
                  for t in (q, k, v)]
        args = leaves
        dyv = dy.transpose(1, 2).contiguous()
    out = ops.flash_attn(*args, causal=causal, window=window)
    out.backward(dyv)
    torch.cuda.synchronize()
    raw = [t.grad for t in leaves]
    grads = [g.transpose(1, 2) if bshd else g for g in raw]
    return grads, raw


def _reference(q, k, v, dy, causal, window):
    ref_in = [t.transpose(1, 2).float().requires_grad_(True)
              for t in (q, k, v)]
    kw = {"window": window} if window else {}
    ref = _torch_reference(*ref_in, causal=causal, **kw)
    ref.backward(dy.transpose(1, 2).float())
    return [t.grad for t in ref_in]


def _check(grads, ref, tag):
    for g, r, name in zip(grads, ref, ("dq", "dk", "dv")):
        assert torch.isfinite(g.float()).all(), f"{tag} {name}: non-finite"
        _cmp(g, r, atol=5e-2, rtol=5e-2, name=f"{tag} {name}")


# case: (B, Hq, Hkv, S, causal, window, both_layouts, boost_k_rows)
_CASES = {
    # single tile, diagonal only, one buffer
    "a": (1, 2, 2, 64, True, 0, False, None),
    # one kv block, two q tiles, buffer swap once
    "b": (1, 2, 2, 128, True, 0, False, None),
    # ragged S; >= 3 iterations so both buffers are reused; interior +
    # diagonal + ragged tiles in one kv block.  k rows [256, 300) are
    # multiplied by 8: a mask wrongly skipped on a diagonal or ragged tile
    # then shows as inf/NaN or a gross error, not a small one
    "c": (2, 2, 2, 300, True, 0, True, (256, 300)),
    # GQA path keeps contiguous per-Q-head dk/dv
    "d": (1, 4, 1, 300, True, 0, False, None),
    # non-causal: all-interior tiles
    "e": (1, 2, 2, 384, False, 0, False, None),
    # window < block; band edge crosses tile interiors
    "f": (1, 2, 2, 300, True, 96, True, None),
    # windowed, tile-aligned S
    "g": (1, 2, 2, 512, True, 200, False, None),
}


@pytest.mark.parametrize("case", sorted(_CASES))
def test_flash_bwd_pipeline(case):
    B, Hq, Hkv, S, causal, window, both, boost = _CASES[case]
    q, k, v, dy = _inputs(B, Hq, Hkv, S, seed=100 + ord(case),
                          boost_k_rows=boost)
    ref = _reference(q, k, v, dy, causal, window)

    grads_c, _ = _run(q, k, v, dy, causal, window, bshd=False)
    _check(grads_c, ref, f"case {case} BHSD")
    if not both:
        return

    grads_s, raw_s = _run(q, k, v, dy, causal, window, bshd=True)
    _check(grads_s, ref, f"case {case} BSHD")
    # Hq == Hkv: dk/dv arrive in k's/v's BSHD layout (the leaf grads are the
    # BSHD storage itself, so the (B,H,S,D) view's transpose is contiguous)
    assert Hq == Hkv
    for g, name in zip(grads_s, ("dq", "dk", "dv")):
        assert g.transpose(1, 2).is_contiguous(), f"{name} not BSHD"
    for gs, gc, name in zip(grads_s, grads_c, ("dq", "dk", "dv")):
        assert torch.equal(gs, gc), f"case {case} {name}: strided != contig"


def test_flash_bwd_bshd_grads_layout():
    """With Hq == Hkv and BSHD-view inputs the autograd Function itself
    returns dk/dv whose transpose(1, 2) is contiguous (no copy downstream)."""
    q, k, v, dy = _inputs(1, 2, 2, 128, seed=7)
    args = [t.transpose(1, 2).detach().requires_grad_(True)
            for t in (q, k, v)]
    out = ops.flash_attn(*args, causal=True)
    gq, gk, gv = torch.autograd.grad(out, args, dy.transpose(1, 2))
    for g, name in ((gq, "dq"), (gk, "dk"), (gv, "dv")):
        assert g.transpose(1, 2).is_contiguous(), f"{name} not BSHD"


def test_lds_image_fragment_maps():
    """One 32x128 tile of distinct 16-bit patterns staged in the dual-use
    LDS image: the row reads and the transposed reads must return, in every
    lane and element, exactly what the 32x32x16 operand maps prescribe
    (A: X[l&31][16c + 8(l>>5) + j]; B: X[16ck + 8(l>>5) + j][32nb + (l&31)])."""
    lib = ops._require_lib()
    tile = torch.arange(32 * D, dtype=torch.int16, device="cuda").view(32, D)
    row_out = torch.full((8, 64, 8), -1, dtype=torch.int16, device="cuda")
    tr_out = torch.full((2, 4, 64, 8), -1, dtype=torch.int16, device="cuda")
    lib.run_probe_lds_image(ctypes.c_void_p(tile.data_ptr()),
                            ctypes.c_void_p(row_out.data_ptr()),
                            ctypes.c_void_p(tr_out.data_ptr()),
                            ops._stream())
    torch.cuda.synchronize()
    t = tile.cpu()
    lane = torch.arange(64)
    col, hi = lane & 31, lane >> 5
    j = torch.arange(8)
    exp_row = torch.empty(8, 64, 8, dtype=torch.int16)
    for c in range(8):
        exp_row[c] = t[col[:, None], 16 * c + 8 * hi[:, None] + j[None, :]]
    exp_tr = torch.empty(2, 4, 64, 8, dtype=torch.int16)
    for ck in range(2):
        for nb in range(4):
            exp_tr[ck, nb] = t[16 * ck + 8 * hi[:, None] + j[None, :],
                               32 * nb + col[:, None]]
    assert torch.equal(row_out.cpu(), exp_row), "row-read fragment map"
    assert torch.equal(tr_out.cpu(), exp_tr), "transposed-read fragment map"
