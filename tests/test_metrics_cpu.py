"""metrics.accuracy on the numpy backend against a plain restatement, and the cases the GPU test (tests/test_hip_metrics.py) shares."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor

SHAPES = [(r, c) for r in (1, 4, 5, 257) for c in (2, 10, 64, 65)] + [(8, 30522)]
DTYPES = [np.int16, np.int32, np.int64]


def restated(logits, labels, ignore_index=None):
    """{correct, counted}, row by row"""
    correct = counted = 0
    for row, label in zip(logits, labels):
        if ignore_index is not None and label == ignore_index:
            continue
        label = int(label) + (logits.shape[1] if label < 0 else 0)
        assert 0 <= label < logits.shape[1]
        nans = np.flatnonzero(np.isnan(row))               # the first NaN, else the first of the largest
        best = nans[0] if nans.size else np.flatnonzero(row == row.max())[0]
        counted += 1
        correct += int(best == label)
    return np.array([correct, counted], np.int64)


def batch(rows, cols, dtype, ignore_index=None, seed=0):
    """logits of few distinct values (ties in most rows), labels on the first or on the second of the tied maxima or anywhere,
    negative (wrapping) labels, and - with ignore_index - about a third of the rows ignored and filled with NaN / infinities"""
    rng = np.random.RandomState(1000 * rows + cols + seed)
    logits = rng.randint(0, 6, (rows, cols)).astype(np.float32)
    labels = np.empty(rows, np.int64)
    for r in range(rows):
        top = np.flatnonzero(logits[r] == logits[r].max())
        kind = rng.randint(0, 4)
        if kind == 0:
            labels[r] = top[0]
        elif kind == 1:
            labels[r] = top[1] if len(top) > 1 else top[0]      # the second of two tied maxima: wrong
        elif kind == 2:
            labels[r] = top[0] - cols                           # wraps to the first maximum
        else:
            labels[r] = rng.randint(-cols, cols)
    if ignore_index is not None:
        labels[labels == ignore_index] = 1                      # a class that happens to equal ignore_index would be ignored too
        ignored = rng.rand(rows) < 0.35
        labels[ignored] = ignore_index
        logits[ignored] = np.where(rng.rand(int(ignored.sum()), cols) < 0.5, np.nan, np.inf)
    fits = np.iinfo(dtype).min <= -cols and cols - 1 <= np.iinfo(dtype).max
    return logits, (labels.astype(dtype) if fits else None)


def run(T, logits, labels, **kw):
    return light.metrics.accuracy(T.from_numpy(logits, requires_grad=False), T.from_numpy(labels, requires_grad=False), **kw)


@pytest.mark.parametrize("shape", SHAPES)
def test_accuracy_equals_the_restatement(shape):
    for dtype in DTYPES:
        for ignore_index in (None, -100, 0):
            logits, labels = batch(*shape, dtype, ignore_index)
            if labels is None:
                assert dtype == np.int16 and shape[1] > 2 ** 15
                continue
            got = run(CpuTensor, logits, labels, ignore_index=ignore_index)
            assert isinstance(got, CpuTensor) and got.dtype == np.int64 and got.shape == (2,) and not got.requires_grad
            np.testing.assert_array_equal(got.numpy(), restated(logits, labels, ignore_index))


def test_tied_maxima_and_nan_rows():
    logits = np.array([[1, 5, 5, 0], [1, 5, 5, 0], [3, np.nan, 9, np.nan], [3, np.nan, 9, np.nan], [3, np.nan, 9, np.nan],
                       [-np.inf] * 4, [-np.inf] * 4, [0.0, -0.0, 0.0, -0.0]], np.float32)
    labels = np.array([1, 2, 1, 3, 2, 0, 1, 0], np.int64)
    want = np.array([1, 0, 1, 0, 0, 1, 0, 1])
    for r in range(len(labels)):
        np.testing.assert_array_equal(run(CpuTensor, logits[r:r + 1], labels[r:r + 1]).numpy(), [want[r], 1])
    np.testing.assert_array_equal(run(CpuTensor, logits, labels).numpy(), [want.sum(), len(labels)])


def test_all_rows_ignored_and_no_rows():
    logits = np.full((5, 7), np.nan, np.float32)
    np.testing.assert_array_equal(run(CpuTensor, logits, np.full(5, -100, np.int32), ignore_index=-100).numpy(), [0, 0])
    np.testing.assert_array_equal(run(CpuTensor, np.zeros((0, 7), np.float32), np.zeros(0, np.int64)).numpy(), [0, 0])


def test_into_accumulates_over_batches():
    total, want = None, np.zeros(2, np.int64)
    for seed in range(3):
        logits, labels = batch(33, 10, np.int32, -100, seed=seed)
        total = run(CpuTensor, logits, labels, ignore_index=-100, into=total)
        want += restated(logits, labels, -100)
    np.testing.assert_array_equal(total.numpy(), want)
    again = run(CpuTensor, logits, labels, ignore_index=-100, into=total)
    assert again is total


def test_bad_arguments():
    logits, labels = batch(5, 10, np.int64)
    for bad in (10, -11):
        wrong = labels.copy()
        wrong[3] = bad
        with pytest.raises(IndexError):
            run(CpuTensor, logits, wrong)
        wrong[3] = 1
        run(CpuTensor, logits, wrong)
    with pytest.raises(ValueError):
        run(CpuTensor, logits, labels[:4])
    with pytest.raises(ValueError):
        run(CpuTensor, logits.reshape(5, 2, 5), labels)
    with pytest.raises(TypeError):
        run(CpuTensor, logits, labels.astype(np.float32))
    with pytest.raises(ValueError):
        run(CpuTensor, logits, labels, into=CpuTensor.from_numpy(np.zeros(3, np.int64), requires_grad=False))
