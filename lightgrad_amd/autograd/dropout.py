"""Call protocol of `Tensor.dropout(p, residual=None)`, shared by the backends' dropout nodes.

`x.dropout(p)` zeroes each element with probability p and scales the others by 1 / (1 - p); with `residual=r` (same shape) the
result is `dropout(x) + r` from one kernel.  The mask comes from the counter-based stream of `lightgrad_amd.random` and is never
stored: the node keeps the call's number and the backward makes the mask again.

What is settled here, before a tape node exists:
  * 0 <= p < 1, otherwise ValueError; tensors of the backend's working float type only (float32), otherwise TypeError;
  * p == 0 is not a node at all: `x` itself, or `x + r` - nothing is drawn and `draws` stays where it is;
  * the residual is a PARENT of the node (it receives the gradient as it is, without a copy), so the keyword is moved to a
    positional argument: tensors passed by keyword cannot be parents (func.py).
"""
from .func import Function, _FunctionType
from ..random import check_probability


class _DropoutType(_FunctionType):

    def __call__(cls, x, p, residual=None):
        p = check_probability(p)
        cls.check_operands(x, residual)
        if p == 0.0:
            return x if residual is None else x + residual
        return _FunctionType.__call__(cls, x, residual, p)


class DropoutFunction(Function, metaclass=_DropoutType):
    """base of a backend's dropout node: forward(ctx, x, residual, p), backward -> (dx, out_grad)"""

    @staticmethod
    def check_operands(x, residual):
        raise NotImplementedError()

    @staticmethod
    def check_residual(x, residual):
        if residual is not None:
            if not isinstance(residual, x.__class__):
                raise TypeError("dropout: the residual must be a %s (got %s)" % (x.__class__.__name__, type(residual).__name__))
            if tuple(residual.shape) != tuple(x.shape):
                raise ValueError("dropout: the residual's shape %s differs from the input's %s" % (tuple(residual.shape), tuple(x.shape)))
