"""The case table of the argmax / argmin sweep on the host: numpy has the rules the kernels restate, the constructions force
the answers they claim, and CpuTensor.argmax / argmin are numpy's on every case."""
import numpy as np
import pytest
import argreduce_cases as A
from lightgrad_amd import CpuTensor

OPS = ("argmax", "argmin")


def test_numpy_has_the_rules_the_kernels_restate():
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    f = lambda *v: np.array(v, np.float32)      # noqa: E731
    assert np.argmax(f(1, 3, 3, 2)) == 1 and np.argmin(f(2, 1, 1, 3)) == 1                   # the lowest index among equal extrema
    assert np.argmax(f(-0.0, 0.0)) == 0 and np.argmax(f(0.0, -0.0)) == 0                     # -0.0 and +0.0 are equal
    assert np.argmin(f(-0.0, 0.0)) == 0 and np.argmin(f(0.0, -0.0)) == 0
    assert np.argmax(f(-inf, -inf, -inf)) == 0 and np.argmin(f(inf, inf, inf)) == 0          # nothing but the identity
    assert np.argmax(f(inf, inf)) == 0 and np.argmin(f(-inf, -inf)) == 0
    assert np.argmax(f(1e30, nan, inf, nan)) == 1 and np.argmin(f(-1e30, nan, -inf, nan)) == 1   # the first NaN, for both
    assert np.argmax(f(nan, nan)) == 0 and np.argmin(f(nan, nan)) == 0
    scalar = np.full((), 7, np.float32)                                                      # 0-d: its flattening has the one axis 0 / -1
    assert np.argmax(scalar) == 0 and np.argmax(scalar, axis=0) == 0 and np.argmin(scalar, axis=-1) == 0
    with pytest.raises(np.exceptions.AxisError):
        np.argmax(scalar, axis=1)
    t = np.arange(6, dtype=np.float32).reshape(2, 3).T                                       # axis=None: the flattening of the VIEW
    assert np.argmax(t) == 5 and t.reshape(-1)[5] == 5 and np.argmax(t[:, ::-1]) == 4
    assert np.argmax(t, axis=-1).tolist() == [1, 1, 1] and np.argmax(t, axis=0, keepdims=True).shape == (1, 2)
    assert np.argmax(t).dtype == np.int64
    for op in OPS:
        for shape, axis in A.EMPTY_REDUCTION:
            with pytest.raises(ValueError, match="attempt to get %s of an empty sequence" % op):
                getattr(np, op)(np.zeros(shape, np.float32), axis=axis)
        for shape, axis in A.EMPTY_OUTPUT:
            got = getattr(np, op)(np.zeros(shape, np.float32), axis=axis)
            assert got.size == 0 and got.dtype == np.int64


def test_table_is_well_formed():
    assert {c.kernel for c in A.CASES} == {A.ROWS_WAVE, A.ROWS_SPLIT, A.COLS}
    for c in A.CASES:
        for tag, view in c.make().items():
            assert view.dtype == np.float32 and view.size <= A.MAX_ELEMENTS, (c.name, tag)
            base, shape, strides, offset = A.layout(view)
            again = np.lib.stride_tricks.as_strided(base[offset:], shape, tuple(4 * s for s in strides)) if view.ndim else base[offset].reshape(())
            assert again.tobytes() == view.tobytes(), (c.name, tag)                            # the GPU test's view is this view
    from lightgrad_amd.autograd.hip.ops import _one_stride
    for view, axis in A.uncollapsible():                     # the dimensions in front of, or behind, the axis keep two strides
        _, shape, strides, _ = A.layout(view)
        parts = [(shape, strides)] if axis is None else [(shape[:axis], strides[:axis]), (shape[axis + 1:], strides[axis + 1:])]
        assert not all(_one_stride(*p) for p in parts), (shape, strides, axis)


@pytest.mark.parametrize("op", OPS)
def test_constructions_force_their_answers(op):
    checked = 0
    for c in A.CASES:
        if c.expect is None:
            continue
        for tag, view in c.make().items():
            np.testing.assert_array_equal(A.reference(op, view, c.axis, c.keepdims), c.expect, err_msg="%s/%s" % (c.name, tag))
            checked += 1
    assert checked >= 15


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensor_equals_numpy_on_every_case(op):
    for c in A.CASES:
        for tag, view in c.make().items():
            t = CpuTensor.from_numpy(view if op == "argmax" else -view)
            got = getattr(t, op)(axis=c.axis, keepdims=c.keepdims)
            want = A.reference(op, view, c.axis, c.keepdims)
            assert isinstance(got, CpuTensor) and got.dtype == np.int64 and not got.requires_grad and got._ctx is None, (c.name, tag)
            assert got.shape == want.shape, (c.name, tag)
            np.testing.assert_array_equal(got.numpy(), want, err_msg="%s/%s" % (c.name, tag))
    for view, axis in A.uncollapsible():
        np.testing.assert_array_equal(getattr(CpuTensor.from_numpy(view), op)(axis=axis).numpy(), getattr(np, op)(view, axis=axis))


@pytest.mark.parametrize("op", OPS)
def test_cpu_tensor_empties(op):
    for shape, axis in A.EMPTY_REDUCTION:
        with pytest.raises(ValueError, match="attempt to get %s of an empty sequence" % op):
            getattr(CpuTensor.from_numpy(np.zeros(shape, np.float32)), op)(axis=axis)
    for shape, axis in A.EMPTY_OUTPUT:
        got = getattr(CpuTensor.from_numpy(np.zeros(shape, np.float32)), op)(axis=axis)
        assert got.dtype == np.int64 and got.numpy().size == 0 and got.shape == np.zeros(shape).argmax(axis=axis).shape
