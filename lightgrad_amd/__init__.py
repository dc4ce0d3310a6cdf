"""lightgrad_amd - an MI355X-native (gfx950) tensor backend behind lightgrad's
autograd surface.  Top-level names follow the reference's `lightgrad/__init__.py:1-6`."""
from . import autograd, data, guide, loss, metrics, nn, optim, random
from .autograd import Tensor, CpuTensor, HipTensor, Gradients, no_grad

empty, zeros, ones = Tensor.empty, Tensor.zeros, Tensor.ones
uniform, xavier = Tensor.uniform, Tensor.xavier
from_numpy = Tensor.from_numpy
manual_seed = random.manual_seed


def bf16_round(t):
    """every value of `t` rounded to bfloat16 (nearest, ties to even) and kept as float32: the rounding `dot_bf16` /
    `linear_bf16` apply to their operands (autograd/cpu/ops.py: bf16_round_array).  A tensor of t's backend, no gradient."""
    return t.bf16_round()


# the storage form of a bfloat16 key / value cache (nn.PagedKVCache(kv_dtype="bf16")): array functions, THE definition for both
# backends - bf16_bits(x) the int16 words of r(x), bf16_widen(w) the float32 values they stand for
from .autograd.cpu.ops import bf16_bits, bf16_widen  # noqa: E402
