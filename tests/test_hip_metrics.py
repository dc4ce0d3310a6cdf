"""metrics.accuracy on the GPU (lg_top1_count_f32: the rows kernel of csrc/argreduce.hip with its counting flag) against the
restatement of tests/test_metrics_cpu.py and the numpy backend, bit for bit."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from test_metrics_cpu import SHAPES, DTYPES, restated, batch, run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", SHAPES)
def test_accuracy_equals_the_restatement_and_the_numpy_backend(hip, shape):
    for dtype in DTYPES:
        for ignore_index in (None, -100, 0):
            logits, labels = batch(*shape, dtype, ignore_index)
            if labels is None:
                continue                                                     # int16 labels do not reach a vocabulary
            got = run(hip, logits, labels, ignore_index=ignore_index)
            assert isinstance(got, hip) and got.dtype == np.int64 and tuple(got.shape) == (2,) and not got.requires_grad
            np.testing.assert_array_equal(got.numpy(), restated(logits, labels, ignore_index), err_msg="%s %s" % (dtype, ignore_index))
            np.testing.assert_array_equal(got.numpy(), run(CpuTensor, logits, labels, ignore_index=ignore_index).numpy())


def test_tied_maxima_and_nan_rows(hip):
    logits = np.array([[1, 5, 5, 0], [1, 5, 5, 0], [3, np.nan, 9, np.nan], [3, np.nan, 9, np.nan], [3, np.nan, 9, np.nan],
                       [-np.inf] * 4, [-np.inf] * 4, [0.0, -0.0, 0.0, -0.0]], np.float32)
    labels = np.array([1, 2, 1, 3, 2, 0, 1, 0], np.int64)
    want = np.array([1, 0, 1, 0, 0, 1, 0, 1])
    for r in range(len(labels)):
        np.testing.assert_array_equal(run(hip, logits[r:r + 1], labels[r:r + 1]).numpy(), [want[r], 1], err_msg="row %d" % r)
    np.testing.assert_array_equal(run(hip, logits, labels).numpy(), [want.sum(), len(labels)])
    wide = np.zeros((6, 300), np.float32)                                    # ties that straddle lanes and the lane + 64 k wrap
    wide[np.arange(6), [5, 64, 70, 128, 255, 299]] = 1
    wide[np.arange(6), [69, 65, 299, 129, 256, 0]] = 1
    first = np.argmax(wide, axis=1)
    np.testing.assert_array_equal(first, [5, 64, 70, 128, 255, 0])
    np.testing.assert_array_equal(run(hip, wide, first).numpy(), [6, 6])
    np.testing.assert_array_equal(run(hip, wide, np.array([69, 65, 299, 129, 256, 299])).numpy(), [0, 6])


def test_ignored_rows_are_not_read_and_all_ignored_counts_nothing(hip):
    logits, labels = batch(257, 65, np.int32, -100)
    clean = logits.copy()
    clean[labels == -100] = 0
    assert np.isnan(logits[labels == -100]).any() and (labels == -100).sum() > 10
    np.testing.assert_array_equal(run(hip, logits, labels, ignore_index=-100).numpy(), run(hip, clean, labels, ignore_index=-100).numpy())
    np.testing.assert_array_equal(run(hip, logits, np.full(257, -100, np.int32), ignore_index=-100).numpy(), [0, 0])
    np.testing.assert_array_equal(run(hip, np.zeros((0, 7), np.float32), np.zeros(0, np.int64)).numpy(), [0, 0])
    from lightgrad_amd.autograd.hip import HipDevice
    HipDevice.synchronize()                                                  # raises if a kernel has set the status flag


def test_into_accumulates_over_batches(hip):
    total, want = None, np.zeros(2, np.int64)
    for seed in range(3):
        logits, labels = batch(257, 10, np.int32, -100, seed=seed)
        total = run(hip, logits, labels, ignore_index=-100, into=total)
        want += restated(logits, labels, -100)
    np.testing.assert_array_equal(total.numpy(), want)
    assert run(hip, logits, labels, ignore_index=-100, into=total) is total


def test_label_out_of_range_is_an_index_error_at_the_next_synchronisation(hip):
    logits, labels = batch(9, 10, np.int64)
    good = restated(logits, labels)
    for bad in (10, -11):
        wrong = labels.copy()
        wrong[3] = bad
        counts = run(hip, logits, wrong)                                     # the launch itself cannot raise
        with pytest.raises(IndexError):
            counts.numpy()
        np.testing.assert_array_equal(run(hip, logits, labels).numpy(), good)   # the flag is cleared, a later call counts right
    with pytest.raises(TypeError):
        run(hip, logits.astype(np.float64), labels)
    with pytest.raises(TypeError):
        light.metrics.accuracy(hip.from_numpy(logits), CpuTensor.from_numpy(labels))


def test_captured_accuracy_counts_the_batch_of_every_replay(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    batches = [batch(257, 65, np.int32, -100, seed=s) for s in range(4)]
    logits = hip.from_numpy(batches[0][0], requires_grad=False)
    labels = hip.from_numpy(batches[0][1], requires_grad=False)
    total = hip.from_numpy(np.zeros(2, np.int64), requires_grad=False)
    light.metrics.accuracy(logits, labels, ignore_index=-100, into=total)    # eager once: pool, kernels
    want = restated(*batches[0], -100)
    graph = HipGraph()
    with graph.capture():
        light.metrics.accuracy(logits, labels, ignore_index=-100, into=total)
    assert graph.kernel_count() == 1                                         # ONE launch
    for lo, la in batches[1:]:
        logits.upload_(lo)
        labels.upload_(la)
        graph.replay()
        want += restated(lo, la, -100)
    np.testing.assert_array_equal(total.numpy(), want)
    graph.destroy()
