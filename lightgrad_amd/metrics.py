"""Evaluation metrics.  `accuracy` is top-1 counting: how many rows of a batch of logits put their maximum on the row's label.

    counts = accuracy(logits, labels)                      # int64 tensor of shape (2,): {correct, counted}
    total = accuracy(logits, labels, into=total)           # a running total over an evaluation set

The result stays on the logits' backend, so an evaluation loop over HipTensors reads the host once, at its end; the HipTensor
form is one launch (csrc/argreduce.hip) and may be captured in a graph.  The definition, in numpy, is `top1_counts` below:

  * a row is counted unless its label, as stored, equals `ignore_index` - the rule of `loss.cross_entropy(ignore_index=)`;
    ignored rows are not looked at and may hold NaN;
  * a negative label that is not ignored wraps by the number of classes; one out of range is an IndexError (on the device: at
    the next synchronising call, and that row is not counted);
  * a counted row is correct iff its label equals `argmax` of the row with numpy's rules: among equal maxima the lowest index
    (a label on the second of two tied maxima is wrong), and the first NaN of a row that holds one.
"""
import numpy as np


def top1_counts(logits: np.ndarray, labels: np.ndarray, ignore_index: int = None) -> np.ndarray:
    """{correct, counted} as an int64 array of shape (2,): the definition of `accuracy`"""
    rows, cols = logits.shape
    labels = np.asarray(labels)
    counted = np.ones(rows, dtype=bool) if ignore_index is None else labels != ignore_index
    wanted = labels[counted].astype(np.int64)
    wanted = np.where(wanted < 0, wanted + cols, wanted)
    if ((wanted < 0) | (wanted >= cols)).any():
        raise IndexError("accuracy: a label is out of range for %d classes" % cols)
    predicted = np.argmax(logits[counted], axis=1) if wanted.size else wanted
    return np.array([np.count_nonzero(predicted == wanted), wanted.size], dtype=np.int64)


def accuracy(logits, labels, ignore_index: int = None, into=None):
    """{correct, counted} of 2-D float32 `logits` (classes on the last axis) against int16 / int32 / int64 `labels` of shape
    (rows,), as an int64 tensor of shape (2,) on the logits' backend.  With `into` - an earlier result - the new counts are added
    to it and it is returned."""
    if len(logits.shape) != 2 or tuple(labels.shape) != (logits.shape[0],):
        raise ValueError("accuracy: logits %s and labels %s do not match ((rows, classes) and (rows,))"
                         % (tuple(logits.shape), tuple(labels.shape)))
    if np.dtype(labels.dtype) not in (np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError("accuracy: labels must be int16 / int32 / int64 (got %s)" % labels.dtype)
    if into is not None and (type(into) is not type(logits) or tuple(into.shape) != (2,) or np.dtype(into.dtype) != np.dtype(np.int64)):
        raise ValueError("accuracy: `into` must be an earlier result: an int64 tensor of shape (2,) on the logits' backend")
    if ignore_index is not None:
        ignore_index = int(ignore_index)
    if isinstance(logits.data, np.ndarray):
        counts = top1_counts(logits.data, labels.numpy() if hasattr(labels, "numpy") else labels, ignore_index)
        if into is None:
            return type(logits).from_numpy(counts, requires_grad=False)
        into.data[...] += counts
        return into
    from .autograd.hip.ops import top1_count
    return top1_count(logits, labels, ignore_index, into)
