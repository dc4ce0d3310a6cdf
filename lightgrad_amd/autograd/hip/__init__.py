"""MI355X (gfx950) backend: HipTensor + its ops over the liblghip.so C ABI.
The package name `hip` is what makes `AbstractTensor.hip()` appear (tensor.py metaclass)."""
from .tensor import HipTensor, HipDevice, HipBuffer
from .tensor import HipTensor as Tensor
from . import ops_bf16  # noqa: F401  (registers dot_bf16 / linear_bf16 / bf16_round on HipTensor)
from . import ops_attention  # noqa: F401  (registers attention / masked_attention / long_attention / self_attention)
from .lib import HipError
from .graph import HipGraph, GraphedStep
from .profiler import HipProfiler
