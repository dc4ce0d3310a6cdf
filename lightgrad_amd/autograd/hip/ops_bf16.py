"""Products on the bf16 matrix cores: `dot_bf16`, `linear_bf16` and `bf16_round` of the HipTensor backend.

Tensors stay float32 in memory; `lg_gemm_bf16_f32` (csrc/gemm_bf16.hip) rounds both operands of a product to bfloat16 while it
stages them and sums in fp32 - the arithmetic autograd/cpu/ops.py defines (`bf16_round_array`, `dot_bf16`, `linear_bf16`).

These nodes are EAGER: one launch per product, no part in the lazy or bracketed forms of ops.py (head, lazy linear, pair,
group, held pair); a lazy operand (a relu nobody has looked at) is computed first.  Every gradient is returned as a fresh tensor
and reaches its parameter through `add_grad`, like the gradient of any op that is not an fp32 GEMM.
"""
import numpy as np
from ..func import Function
from .tensor import HipTensor
from . import lib as _l
from .ops import _as_mat, _collapse_batch, _swap_last, _rows, _reduce

_F32 = np.dtype(np.float32)


def _require_operands(name, a, b, bias=None):
    for t in (a, b, bias):
        if t is not None and t._dtype != _F32:
            raise TypeError("%s is float32-only (got %s)" % (name, t._dtype))
    if len(a._shape) < 2 or len(b._shape) != 2:
        raise ValueError("%s: (M, K) @ (K, N) or (..., M, K) @ (K, N) only (got %s and %s)" % (name, a._shape, b._shape))
    if a._shape[-1] != b._shape[-2]:
        raise ValueError("matmul: shapes %s and %s do not align" % (a._shape, b._shape))


def _gemm_bf16(a, b, bias=None):
    """r(a) (..., M, K) @ r(b) (K, N) [+ bias (N,)] -> dense (..., M, N); operands with a unit stride among their last two dims
    are consumed in place, leading dims that walk as one run make ONE tall product"""
    lead_shape, rows_per_matrix = a._shape[:-2], a._shape[-2]
    K, N = b._shape
    if len(a._shape) > 2:
        lead = _collapse_batch(a._shape[:-1], a._strides[:-1])
        if lead is None or not (a._strides[-1] == 1 or K == 1):
            a = a.contiguous()
            lead = _collapse_batch(a._shape[:-1], a._strides[:-1])
        rows, rstride = lead
        a = HipTensor(a.data, (rows, K), (rstride if rows > 1 else K, a._strides[-1]), a._offset, a._dtype)
    M = a._shape[0]
    ma, mb = _as_mat(a), _as_mat(b)
    out = HipTensor.empty((M, N))
    if bias is not None:
        if bias._shape != (N,):
            raise ValueError("linear_bf16: bias of shape %s for %d output features" % (bias._shape, N))
        bias = bias.contiguous()
    _l.check(_l.lib().lg_gemm_bf16_f32(1 if ma.colmajor else 0, 1 if mb.colmajor else 0, M, N, K, ma.t.ptr, ma.ld, mb.t.ptr, mb.ld,
                                       out.ptr, N, bias.ptr if bias is not None else None, 0))
    return out.reshape(*lead_shape, rows_per_matrix, N) if lead_shape else out


@HipTensor.register_op()
class dot_bf16(Function):
    """ a.dot_bf16(b) = r(a) @ r(b): (M, K) @ (K, N), or (..., M, K) @ (K, N) as one tall product, on v_mfma_f32_32x32x16_bf16.
    backward: dA = r(g) @ r(b)^T, dB = r(a)^T @ r(g) - the same kernel, every operand rounded again. """
    def forward(ctx, a, b):
        _require_operands("dot_bf16", a, b)
        ctx.save_for_backward(a, b)
        return _gemm_bf16(a, b)

    def backward(ctx, out_grad):
        a, b = ctx.get_saved_tensors()
        K, N = b._shape
        g2 = _rows(out_grad, N)
        ga = _gemm_bf16(g2, _swap_last(b)).reshape(*a._shape) if a.requires_grad else None
        gb = _gemm_bf16(_swap_last(_rows(a, K)), g2) if b.requires_grad else None
        return ga, gb


@HipTensor.register_op()
class linear_bf16(Function):
    """ x.linear_bf16(weight, bias=None) = r(x) @ r(weight)^T + bias with the bias added to the fp32 sum in the product's
    epilogue; weight as nn.Linear holds it ((out, in)).  backward: dx = r(g) @ r(W), dW = r(g)^T @ r(x), db = column sums
    of the fp32 g. """
    def forward(ctx, x, weight, bias=None):
        _require_operands("linear_bf16", x, _swap_last(weight) if len(weight._shape) == 2 else weight, bias)
        ctx.save_for_backward(x, weight, bias)
        return _gemm_bf16(x, _swap_last(weight), bias=bias)

    def backward(ctx, out_grad):
        x, weight, bias = ctx.get_saved_tensors()
        out_f, in_f = weight._shape
        g2 = _rows(out_grad, out_f)
        dx = _gemm_bf16(g2, weight).reshape(*x._shape) if x.requires_grad else None
        dw = _gemm_bf16(_swap_last(g2), _rows(x, in_f)) if weight.requires_grad else None
        if bias is None:
            return dx, dw
        return dx, dw, (_reduce(_l.RED_SUM, g2, (0,), False) if bias.requires_grad else None)


def _bf16_round(t):
    """ t.bf16_round() (also `lightgrad_amd.bf16_round(t)`): every value rounded to bfloat16 as the products above round their
    operands, kept as float32; a new dense tensor, a constant of the tape """
    if t._dtype != _F32:
        raise TypeError("bf16_round is float32-only (got %s)" % t._dtype)
    src = t.contiguous()
    out = HipTensor.empty(t._shape, requires_grad=False)
    _l.check(_l.lib().lg_bf16_round_f32(src.ptr, out.ptr, out.numel()))
    return out


HipTensor.bf16_round = _bf16_round
