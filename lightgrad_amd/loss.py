"""Losses.  `mse` restates the reference's `lightgrad/loss.py:4-12`: value is
`mean((y - y_hat)^2) / 2`, gradient is `(y - y_hat) * out_grad` - WITHOUT the 1/N
of the mean (reference quirk kept for parity; it makes the data-parallel
gradient of a concatenated batch the SUM of per-rank gradients).
`cross_entropy` restates loss.py:14-24 (softmax, pick the label's probability with an index pair, -log, mean; backward
`(softmax - onehot) / N * out_grad`); the generic form needs fancy indexing (CpuTensor has it), HipTensor provides it
as one fused kernel through the optional `_fused_cross_entropy` hook.  `cross_entropy(..., ignore_index=k)` is the masked-LM
form: only the rows whose label differs from k count, and the mean is over their number."""
import numpy as np
from .autograd import Function


class mse(Function):
    """ Mean Squared Error """

    def forward(ctx, y, y_hat):
        fused = getattr(y, "_fused_mse", None)
        if fused is not None and y.shape == getattr(y_hat, "shape", None):
            # optional backend hook: the expression below in one kernel (same roundings at the scaling steps)
            loss, err = fused(y_hat)
            ctx.save_for_backward(err)
            return loss
        err = y - y_hat
        ctx.save_for_backward(err)
        return (err ** 2).mean() / 2

    def backward(ctx, out_grad):
        err, = ctx.get_saved_tensors()
        if getattr(out_grad, "_is_unit_constant", False):
            return err          # the loss is the root of backward(): its seed is the backend's constant 1.0, and x * 1.0 is x
        return err * out_grad


class cross_entropy(Function):
    """ Cross Entropy Loss of softmax(y) against integer class labels y_hat of shape (N,).

    `ignore_index=k` (an int, compared with the label as stored, before any negative-index wrap) is the masked-LM form: the rows
    whose label is k do not count.  With n the number of the other rows, the loss is the sum of their -log softmax(y)[r, label]
    times float32(1 / n), its gradient (softmax - onehot) * float32(1 / n) on those rows and exactly +0.0 on the ignored ones,
    whose logits influence nothing (they may hold NaN).  n == 0 gives a NaN loss and a zero gradient. """

    def forward(ctx, y, y_hat, axis: int = -1, ignore_index: int = None):
        fused = getattr(y, "_fused_cross_entropy", None)
        if ignore_index is not None:
            return ctx._forward_ignoring(y, y_hat, axis, int(ignore_index), fused)
        if fused is not None and len(y.shape) == 2 and axis in (-1, 1):
            loss, dlogits = fused(y_hat)                   # dlogits = (softmax - onehot) / N
            ctx.save_for_backward(dlogits, None, axis)
            return loss
        p = y.softmax(axis=axis)
        ctx.save_for_backward(p, y_hat, axis)
        n = y_hat.shape[0]
        return -p[range(n), y_hat].log().mean()

    def _forward_ignoring(ctx, y, y_hat, axis, ignore_index, fused):
        if fused is not None and len(y.shape) == 2 and axis in (-1, 1):
            loss, dlogits = fused(y_hat, ignore_index=ignore_index)        # the valid rows are counted on the device
            ctx.save_for_backward(dlogits, None, axis)
            return loss
        if not isinstance(y.data, np.ndarray):
            # the expression below picks the valid rows on the host: it is for tensors that live there.  A device backend takes
            # its fused hook or nothing - no copy of the labels to the host behind the caller's back
            raise NotImplementedError("cross_entropy(ignore_index=) on %s needs the backend's fused hook: 2-D logits with the "
                                      "classes on the last axis (got shape %s, axis %d%s)"
                                      % (type(y).__name__, tuple(y.shape), axis, "" if fused is not None else ", hook switched off"))
        labels = np.asarray(y_hat.numpy() if hasattr(y_hat, "numpy") else y_hat)
        ignored = labels == ignore_index
        rows = np.flatnonzero(~ignored)
        inv = float(np.float32(1.0 / rows.size)) if rows.size else float("inf")
        p = y.softmax(axis=axis)
        ctx.save_for_backward(p, (rows, labels[rows], np.flatnonzero(ignored), inv), axis)
        with np.errstate(invalid="ignore"):                 # no valid row: 0 * inf, the mean of nothing
            return -(p[rows, labels[rows]].log().sum() * inv)

    def backward(ctx, out_grad):
        p, y_hat, axis = ctx.get_saved_tensors()
        if y_hat is None:
            return p if getattr(out_grad, "_is_unit_constant", False) else p * out_grad
        if isinstance(y_hat, tuple):
            rows, picked, ignored, inv = y_hat
            if rows.size:
                p[rows, picked] -= 1
                p *= inv
            p[ignored] = 0                                  # +0.0 whatever the row's softmax holds
            return p * out_grad
        n = y_hat.shape[0]
        p[range(n), y_hat] -= 1
        p /= n
        return p * out_grad
