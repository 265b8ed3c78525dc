"""MX (microscaling) tensor-parallel linears — inference only.

``MXColumnParallel`` / ``MXRowParallel`` keep the local weight shard in the
stored MX format of ``microscaling.pack_mx`` (uint8 payload + uint8 e8m0
scales, blocks of 32 along K) and run ``microscaling.mx_linear``: on the GPU
the native block-scaled MFMA GEMM with the activation quantized to MXFP8 on
the fly -- up to 32 rows (decode) in the fused split-K skinny kernel
(``ops/csrc/mx_skinny.hip``), more rows through ``mx_quantize_rows`` and the
128x128 tile (``ops/csrc/mx_gemm.hip``); ``ops.mx_linear`` picks, the layers
do not change -- elsewhere (CPU, or a local K that is not a multiple of 128)
the emulation.  The communication pattern is the
one of ``QuantizedColumnParallel`` / ``QuantizedRowParallel``.

Sharding along K (row parallel) cuts between 32-blocks, so a rank's payload
and scales are plain slices of the full layer's.
"""

import enum
from dataclasses import dataclass

import torch.nn as nn

from ..parallel.layers import (BaseParallelLinear, ColumnParallelLinear,
                               RowParallelLinear)
from ..parallel.mappings import (
    gather_from_sequence_parallel_region,
    gather_from_tensor_model_parallel_region,
    reduce_from_tensor_model_parallel_region,
    reduce_scatter_to_sequence_parallel_region,
    scatter_to_tensor_model_parallel_region,
)
from .microscaling import (MX_BLOCK, MX_NATIVE_FORMATS, mx_linear, pack_mx,
                           quantize_mx)


class MXDtype(enum.Enum):
    FP8_E4M3 = "fp8_e4m3"
    FP4_E2M1 = "fp4_e2m1"


@dataclass
class MXConfig:
    """Weight element format of the MX layers (activations are always
    fp8_e4m3)."""
    weight_fmt: str = "fp4_e2m1"

    def __post_init__(self):
        if self.weight_fmt not in MX_NATIVE_FORMATS:
            raise ValueError(f"MXConfig.weight_fmt {self.weight_fmt!r} not "
                             f"supported (one of {MX_NATIVE_FORMATS})")

    @property
    def quantized_dtype(self) -> MXDtype:  # what quantize.convert logs
        return MXDtype(self.weight_fmt)


class _MXParallelLinearBase(BaseParallelLinear):
    @classmethod
    def from_float(cls, float_layer, cfg=None):
        """Quantize a Column/RowParallel layer's local shard along K."""
        cfg = cfg or MXConfig()
        if not isinstance(cfg, MXConfig):
            raise TypeError(f"{cls.__name__}.from_float needs an MXConfig, "
                            f"got {type(cfg).__name__}")
        w = float_layer.weight.detach()
        if w.shape[-1] % MX_BLOCK:
            raise ValueError(
                f"{cls.__name__}: local K={w.shape[-1]} of weight "
                f"{tuple(w.shape)} is not a multiple of {MX_BLOCK}")
        layer = cls.__new__(cls)
        BaseParallelLinear.__init__(layer)
        layer.mx_config = cfg
        payload, scales = pack_mx(*quantize_mx(w, cfg.weight_fmt),
                                  cfg.weight_fmt)
        layer.weight = nn.Parameter(payload, requires_grad=False)
        layer.scale = nn.Parameter(scales, requires_grad=False)
        for attr in ("tensor_model_parallel", "partition_dim",
                     "partition_stride", "num_partitions"):
            if hasattr(float_layer.weight, attr):
                setattr(layer.weight, attr, getattr(float_layer.weight, attr))
                setattr(layer.scale, attr, getattr(float_layer.weight, attr))
        layer.bias = float_layer.bias
        layer._copy_cfg(float_layer)
        return layer

    def _mx_linear(self, x, bias):
        return mx_linear(x, self.weight, self.scale,
                         self.mx_config.weight_fmt, bias=bias)


class MXColumnParallel(_MXParallelLinearBase):
    def _copy_cfg(self, fl):
        self.gather_output = fl.gather_output
        self.sequence_parallel_enabled = fl.sequence_parallel_enabled
        self.skip_bias_add = getattr(fl, "skip_bias_add", False)

    def forward(self, input_):
        if self.sequence_parallel_enabled:
            input_ = gather_from_sequence_parallel_region(input_, seq_dim=0)
        bias = self.bias if not self.skip_bias_add else None
        out = self._mx_linear(input_, bias)
        if self.gather_output:
            out = gather_from_tensor_model_parallel_region(out)
        if self.skip_bias_add:
            return out, self.bias
        return out


class MXRowParallel(_MXParallelLinearBase):
    def _copy_cfg(self, fl):
        self.input_is_parallel = fl.input_is_parallel
        self.sequence_parallel_enabled = fl.sequence_parallel_enabled
        self.skip_bias_add = getattr(fl, "skip_bias_add", False)
        self.reduce_output = getattr(fl, "reduce_output", True)

    def forward(self, input_):
        if not self.input_is_parallel:
            input_ = scatter_to_tensor_model_parallel_region(input_)
        out = self._mx_linear(input_, None)
        if not self.reduce_output:
            pass
        elif self.sequence_parallel_enabled:
            out = reduce_scatter_to_sequence_parallel_region(out, seq_dim=0)
        else:
            out = reduce_from_tensor_model_parallel_region(out)
        if self.skip_bias_add:
            return out, self.bias
        if self.bias is not None:
            out = out + self.bias
        return out


MX_MAPPING = {
    ColumnParallelLinear: MXColumnParallel,
    RowParallelLinear: MXRowParallel,
}
