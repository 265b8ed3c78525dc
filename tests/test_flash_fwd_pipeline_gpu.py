"""GPU checks for the flash-attention forward pipeline: K and V staged once
in the dual-use LDS image (row reads for QK^T, hardware transposed reads
for PV), two staging buffers, the online-softmax rescale and the
LDS-staged whole-row epilogue.

`out` and `lse` are compared with an fp32 composed reference under the
forward tolerances of tests/test_ops_gpu.py (out: 3e-2 + 3e-2 * max|ref|,
lse: 2e-3 + 2e-2 * max|ref|).  Shapes are the smallest that reach each
path: ragged last tile and idle waves, clamped staging rows, one and two
tiles (ring start-up), non-causal, GQA, window edges with t_begin > 0 and
lanes that are fully masked at first, BSHD transpose views, and a
constructed input whose row maxima move late, and only for some rows of
a wave (what a wave-uniform rescale skip would have to get right; the
kernel rescales unconditionally today)."""

import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from neuronx_distributed_amd import ops

D = 128
SCALE = 1.0 / math.sqrt(D)


@pytest.fixture(scope="module", autouse=True)
def _require_lib():
    assert torch.cuda.is_available()
    ops.build = __import__("neuronx_distributed_amd.ops.build",
                           fromlist=["build"])
    ops.build.build()
    assert ops.is_available(), ops._LIB_ERR


def _cmp(a, b, atol, rtol, name):
    a = a.float().cpu()
    b = b.float().cpu()
    assert torch.isfinite(a).all(), f"{name}: non-finite"
    err = (a - b).abs().max().item()
    ref = b.abs().max().item()
    assert err <= atol + rtol * ref, f"{name}: max err {err} (ref max {ref})"


def _inputs(B, Hq, Hkv, S, seed):
    """bf16 BSHD storage (the model's activation layout), values * 0.5."""
    g = torch.Generator(device="cuda").manual_seed(seed)

    def mk(h):
        return torch.randn(B, S, h, D, dtype=torch.bfloat16, device="cuda",
                           generator=g) * 0.5

    return mk(Hq), mk(Hkv), mk(Hkv)


def _reference(q, k, v, causal, window):
    """fp32 composed attention on (B,H,S,D) tensors -> (out, lse)."""
    q, k, v = q.float(), k.float(), v.float()
    rep = q.shape[1] // k.shape[1]
    if rep > 1:
        k = k.repeat_interleave(rep, dim=1)
        v = v.repeat_interleave(rep, dim=1)
    S = q.shape[2]
    scores = torch.matmul(q, k.transpose(-1, -2)) * SCALE
    if causal or window:
        i = torch.arange(S, device=q.device)[:, None]
        j = torch.arange(S, device=q.device)[None, :]
        mask = j <= i
        if window:
            mask &= j > i - window
        scores = scores.masked_fill(~mask, float("-inf"))
    lse = torch.logsumexp(scores, dim=-1)
    out = torch.matmul(torch.softmax(scores, dim=-1), v)
    return out, lse


def _fwd(q, k, v, causal, window):
    """Raw strided forward launch on (B,H,S,D)-indexed tensors of any
    (batch, head, seq) strides; out takes q's layout.  Returns out, lse."""
    lib = ops._require_lib()
    B, Hq, S, _ = q.shape
    out = ops._fa_alloc_like(q)
    lse = torch.empty(B, Hq, S, dtype=torch.float32, device=q.device)
    lib.flash_attn_fwd_strided(
        ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(out), ops._ptr(lse),
        ctypes.c_int(B), ctypes.c_int(Hq), ctypes.c_int(k.shape[1]),
        ctypes.c_int(S), ctypes.c_float(SCALE),
        ctypes.c_int(1 if causal else 0), ctypes.c_int(window),
        ops._fa_strides(q, k, v, out), ops._stream())
    torch.cuda.synchronize()
    return out, lse


def _check(q, k, v, causal, window, tag):
    ref_out, ref_lse = _reference(q, k, v, causal, window)
    out, lse = _fwd(q, k, v, causal, window)
    _cmp(out, ref_out, atol=3e-2, rtol=3e-2, name=f"{tag} out")
    _cmp(lse, ref_lse, atol=2e-3, rtol=2e-2, name=f"{tag} lse")
    return out, lse


# case: (B, Hq, Hkv, S, causal, window, bshd_views)
_CASES = {
    # ragged last tile; second q block has idle waves
    "ragged300": (2, 2, 2, 300, True, 0, False),
    # one row in the second 256-row block: clamped staging rows
    "s257": (1, 2, 2, 257, True, 0, False),
    # a single tile / two tiles: ring start-up
    "s64": (1, 2, 2, 64, True, 0, False),
    "s128": (1, 2, 2, 128, True, 0, False),
    "noncausal384": (1, 2, 2, 384, False, 0, False),
    "gqa1000": (1, 4, 1, 1000, True, 0, False),
    # band edge crosses tile interiors
    "win96_s300": (1, 2, 2, 300, True, 96, False),
    # t_begin > 0, lanes whose every score is masked in their first tiles
    "win200_s1024": (1, 2, 2, 1024, True, 200, False),
    # q/k/v/out as transpose views of BSHD storage
    "bshd300": (2, 2, 2, 300, True, 0, True),
}


@pytest.mark.parametrize("case", sorted(_CASES))
def test_flash_fwd_pipeline(case):
    B, Hq, Hkv, S, causal, window, bshd = _CASES[case]
    q, k, v = _inputs(B, Hq, Hkv, S, seed=200 + len(case) + S)
    args = [t.transpose(1, 2) for t in (q, k, v)]
    if not bshd:
        args = [t.contiguous() for t in args]
    out, _ = _check(*args, causal, window, f"case {case}")
    if bshd:
        assert out.transpose(1, 2).is_contiguous(), "out not BSHD"


def test_flash_fwd_entry_points_agree():
    """The contiguous and the window launchers run the same kernel as the
    strided one: bit-identical out and lse."""
    lib = ops._require_lib()
    B, H, S = 1, 2, 300
    q, k, v = [t.transpose(1, 2).contiguous() for t in _inputs(B, H, H, S, 5)]
    for window in (0, 96):
        out_s, lse_s = _fwd(q, k, v, True, window)
        out = torch.empty_like(q)
        lse = torch.empty(B, H, S, dtype=torch.float32, device="cuda")
        head = (ops._ptr(q), ops._ptr(k), ops._ptr(v), ops._ptr(out),
                ops._ptr(lse), ctypes.c_int(B), ctypes.c_int(H),
                ctypes.c_int(H), ctypes.c_int(S), ctypes.c_float(SCALE))
        if window:
            lib.flash_attn_fwd_window(*head, ctypes.c_int(window),
                                      ops._stream())
        else:
            lib.flash_attn_fwd(*head, ctypes.c_int(1), ops._stream())
        torch.cuda.synchronize()
        assert torch.equal(out, out_s), f"window {window}: out differs"
        assert torch.equal(lse, lse_s), f"window {window}: lse differs"


def test_flash_fwd_rescale_skip():
    """On bounded random data a wrong online-softmax rescale (or a wrongly
    skipped one) hardly shows, so the row maxima are placed by hand (S=512,
    causal, 64-row kv tiles, 32 q rows per wave):
      * kv row 3 (first tile) is boosted along u1 and EVERY q row leans
        towards u1, so each row's maximum is set in tile 0 and no later
        tile raises it (alpha is exactly 1 from then on);
      * kv row 330 (tile 5) is boosted along u2 and only q rows 448..463
        (half of one wave) lean towards u2: that wave's maxima jump at
        tile 5 while its neighbour's (rows 480..511) stay put;
      * kv row 401 (tile 6) likewise for q rows 480..495 along u3.
    A rescale missed at the jump leaves the old, e^5-times-too-heavy
    contributions in O and l for exactly those rows.  The kernel rescales
    unconditionally; a wave-uniform skip was measured slower and is not
    in it, and this case is what such a skip has to pass."""
    B, H, S = 1, 2, 512
    q, k, v = _inputs(B, H, H, S, seed=31)
    g = torch.Generator(device="cuda").manual_seed(32)
    u = torch.randn(3, D, device="cuda", generator=g)
    u = (u / u.norm(dim=-1, keepdim=True)).to(torch.bfloat16)
    q += 4 * u[0]
    k[:, 3] = 16 * u[0]
    q[:, 448:464] += 8 * u[1]
    k[:, 330] = 16 * u[1]
    q[:, 480:496] += 8 * u[2]
    k[:, 401] = 16 * u[2]
    args = [t.transpose(1, 2) for t in (q, k, v)]
    _, ref_lse = _reference(*args, True, 0)
    # the construction did what it says: the boosted rows dominate the
    # logsumexp of the rows that lean towards them (score ~ 11 vs ~ 5.6)
    assert (ref_lse[0, :, 448:464] > 9).all()
    assert (ref_lse[0, :, 464:480] < 8).all()
    _check(*args, True, 0, "rescale skip")
