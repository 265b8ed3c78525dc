"""CPU checks of the skinny MX linear's host logic (ops/csrc/mx_skinny.hip):
the split heuristic, the NXDA_MX_SKINNY switch and the dispatch gate."""

import itertools

import pytest
import torch

from neuronx_distributed_amd import ops

FMTS = ("fp8_e4m3", "fp4_e2m1")
CUS = 256


def _tile_n(M):
    return 16 if M <= 16 else 32     # mx_skinny.hip: NB = 16 * NF


@pytest.mark.parametrize("fmt", FMTS)
def test_splits_properties(fmt):
    Ms = (1, 8, 16, 17, 32)
    Ns = (16, 48, 272, 4096, 8192, 11008)
    Ks = (128, 384, 640, 4096, 11008 // 128 * 128)
    for M, N, K in itertools.product(Ms, Ns, Ks):
        ks = ops.mx_skinny_splits(M, N, K, fmt)
        assert isinstance(ks, int)
        assert 1 <= ks <= K // 128, (M, N, K, ks)
        groups = -(-N // _tile_n(M))
        if groups >= CUS:
            # the in-workgroup split alone gives a workgroup per CU
            assert ks == 1, (M, N, K, ks)
        else:
            # never more slices than fill the machine once
            assert groups * (ks - 1) < CUS, (M, N, K, ks)
    assert ops.mx_skinny_splits(1, 16, 128, fmt) == 1
    assert ops.mx_skinny_splits(32, 16, 128, fmt) == 1
    # a short-N, long-K projection does get split
    assert ops.mx_skinny_splits(32, 4096, 11008 // 128 * 128, fmt) > 1
    assert ops.mx_skinny_splits(1, 4096, 4096, fmt) == 1
    assert ops.mx_skinny_splits(32, 8192, 4096, fmt) == 1


def test_splits_rejects_out_of_contract():
    for bad in ((0, 16, 128), (33, 16, 128), (1, 8, 128), (1, 24, 128),
                (1, 16, 96), (1, 16, 0)):
        with pytest.raises(ValueError):
            ops.mx_skinny_splits(*bad, "fp8_e4m3")
    with pytest.raises(ValueError):
        ops.mx_skinny_splits(1, 16, 128, "fp8_e5m2")


def test_env_switch(monkeypatch):
    monkeypatch.delenv("NXDA_MX_SKINNY", raising=False)
    assert ops._mx_skinny_enabled()
    monkeypatch.setenv("NXDA_MX_SKINNY", "0")
    assert not ops._mx_skinny_enabled()
    monkeypatch.setenv("NXDA_MX_SKINNY", " 0 ")
    assert not ops._mx_skinny_enabled()
    monkeypatch.setenv("NXDA_MX_SKINNY", "1")
    assert ops._mx_skinny_enabled()
    # read per call, not cached at import
    monkeypatch.setenv("NXDA_MX_SKINNY", "0")
    assert not ops._mx_skinny_enabled()


def test_gate_cpu_and_m(monkeypatch):
    monkeypatch.delenv("NXDA_MX_SKINNY", raising=False)
    # even with the kernel present, CPU tensors and M = 33 never dispatch
    monkeypatch.setattr(ops, "mx_skinny_available", lambda: True)
    x = torch.zeros(4, 128, dtype=torch.bfloat16)
    assert ops._mx_skinny_gate(x, 4, 16, 128, "fp8_e4m3") is False
    x33 = torch.zeros(33, 128, dtype=torch.bfloat16)
    assert ops._mx_skinny_gate(x33, 33, 16, 128, "fp8_e4m3") is False

    class _OnGpu:                      # stands in for a GPU tensor
        is_cuda = True

    assert ops._mx_skinny_gate(_OnGpu(), 32, 16, 128, "fp4_e2m1") is True
    assert ops._mx_skinny_gate(_OnGpu(), 33, 16, 128, "fp4_e2m1") is False
    assert ops._mx_skinny_gate(_OnGpu(), 0, 16, 128, "fp4_e2m1") is False
    monkeypatch.setenv("NXDA_MX_SKINNY", "0")
    assert ops._mx_skinny_gate(_OnGpu(), 4, 16, 128, "fp4_e2m1") is False
    monkeypatch.delenv("NXDA_MX_SKINNY")
    monkeypatch.setattr(ops, "mx_skinny_available", lambda: False)
    assert ops._mx_skinny_gate(_OnGpu(), 4, 16, 128, "fp4_e2m1") is False
