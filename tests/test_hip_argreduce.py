"""argmax / argmin on the GPU (csrc/argreduce.hip) against numpy and the numpy backend, bit for bit: the results are integers, so
every comparison is assert_array_equal.

The cases and their references are tests/argreduce_cases.py (checked on the host by tests/test_argreduce_cases_cpu.py).  After
every call the plan `lg_argreduce_last_plan` reports is compared with the kernel the case is meant for: when a retuned threshold
moves a case to another kernel the assertion fails and the SHAPE is to be adjusted."""
import ctypes
import numpy as np
import pytest
import argreduce_cases as A
from lightgrad_amd import CpuTensor

pytestmark = pytest.mark.gpu

OPS = ("argmax", "argmin")


@pytest.fixture(scope="module")
def L(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    hiplib.lib()
    return hiplib


def last_plan(L):
    p = (ctypes.c_int32 * 4)()
    L.check(L.lib().lg_argreduce_last_plan(p))
    return tuple(p)


def device_view(hip, view, negate=False):
    """the numpy view `view` (or of its negated base array) as the same strided view of device memory"""
    base, shape, strides, offset = A.layout(view)
    flat = hip.from_numpy(-base if negate else base, requires_grad=False)
    return hip(flat.data, shape, strides, flat._offset + offset, np.float32, requires_grad=False)


def assert_plan(case, plan):
    kernel, splits, merged, vec = plan
    assert kernel == case.kernel, "%s is meant for kernel %d, the library ran kernel %d (plan %s): adjust the shape" % (
        case.name, case.kernel, kernel, plan)
    got = {"splits": splits, "merged": merged, "vec": vec}
    for key, value in case.want.items():
        if key == "splits_gt":
            assert splits > value, (case.name, plan)
        else:
            assert got[key] == value, (case.name, key, value, plan)
    assert splits >= 1


@pytest.mark.parametrize("name", [c.name for c in A.CASES])
def test_case_equals_numpy_and_reaches_its_kernel(hip, L, name):
    c = A.BY_NAME[name]
    for tag, view in c.make().items():
        for op in OPS:
            t = device_view(hip, view, negate=(op == "argmin"))
            got = getattr(t, op)(axis=c.axis, keepdims=c.keepdims)
            plan = last_plan(L)
            want = A.reference(op, view, c.axis, c.keepdims)
            assert isinstance(got, hip) and got.dtype == np.int64 and not got.requires_grad and got._ctx is None
            assert tuple(got.shape) == want.shape, (name, tag, op)
            np.testing.assert_array_equal(got.numpy(), want, err_msg="%s/%s %s plan %s" % (name, tag, op, plan))
            assert_plan(c, plan)
            cpu = getattr(CpuTensor.from_numpy(view if op == "argmax" else -view), op)(axis=c.axis, keepdims=c.keepdims)
            np.testing.assert_array_equal(got.numpy(), cpu.numpy())
            if c.expect is not None:
                np.testing.assert_array_equal(got.numpy(), c.expect, err_msg="%s/%s %s" % (name, tag, op))


def test_table_reaches_every_kernel_with_and_without_a_fold(hip, L):
    seen = set()
    for c in A.CASES:
        view = next(iter(c.make().values()))
        device_view(hip, view).argmax(axis=c.axis)
        kernel, splits, merged, vec = last_plan(L)
        seen.add((kernel, splits > 1))
        if kernel == A.COLS:
            seen.add(("merged", merged))
        else:
            seen.add(("vec", kernel, vec))
    for want in ((A.ROWS_WAVE, False), (A.ROWS_SPLIT, True), (A.COLS, False), (A.COLS, True), ("merged", 0), ("merged", 1),
                 ("vec", A.ROWS_WAVE, 0), ("vec", A.ROWS_WAVE, 1), ("vec", A.ROWS_SPLIT, 1)):
        assert want in seen, (want, sorted(map(str, seen)))


def _poke(L, t, element, value):
    v = ctypes.c_float(value)
    L.check(L.lib().lg_memcpy_h2d(t.ptr + 4 * element, ctypes.addressof(v), 4))


def test_split_rows_extremum_at_every_segment_edge_and_ties_across_segments(hip, L):
    """axis=None on a dense tensor of a million elements: the extremum planted at the first and the last element of the first, a
    middle and the ragged last segment; then equal extrema in different segments - the lower index wins whichever workgroup
    arrives last"""
    base = A.BY_NAME["all_split"].make()["dense"]
    n = base.size
    t = hip.from_numpy(base, requires_grad=False)
    assert int(t.argmax().numpy()) == int(np.argmax(base))
    kernel, splits, _, _ = last_plan(L)
    assert kernel == A.ROWS_SPLIT and splits > 32, last_plan(L)              # more than one first-level fold group
    seg = ((n + splits - 1) // splits + 3) & ~3
    assert (n + seg - 1) // seg == splits and n % seg != 0, (n, seg, splits)  # the last segment is ragged
    flat = base.reshape(-1)
    values = {"argmax": 2.0, "argmin": -1.0}                                 # beyond [0, 1)

    def with_planted(positions, op):
        for p in positions:
            _poke(L, t, p, values[op])
        try:
            return int(getattr(t, op)().numpy())
        finally:
            for p in positions:
                _poke(L, t, p, float(flat[p]))

    edges = []
    for s in (0, splits // 2, splits - 1):
        edges += [s * seg, min(n, (s + 1) * seg) - 1]
    assert edges[-1] == n - 1
    for op in OPS:
        for p in edges:
            assert with_planted([p], op) == p, (op, p, seg)
        for group in ([edges[5], edges[2]], [edges[3], edges[0], edges[4]], [seg - 1, seg], [33 * seg + 7, 32 * seg - 1, 200 * seg]):
            assert with_planted(group, op) == min(group), (op, group, seg)
    assert int(t.argmax().numpy()) == int(np.argmax(base))                   # everything was put back


def test_views_the_abi_cannot_collapse(hip, L):
    lib = L.lib()
    for view, axis in A.uncollapsible():
        t = device_view(hip, view)
        for op in OPS:
            np.testing.assert_array_equal(getattr(t, op)(axis=axis).numpy(), getattr(np, op)(view, axis=axis))      # copied dense first
        out = hip.empty((view.size,), dtype=np.int64, requires_grad=False)
        rc = lib.lg_argreduce_f32(L.RED_MAX, view.ndim, L.i64(t.shape), t.ptr, L.i64(t.strides), -1 if axis is None else axis, out.ptr)
        assert rc == -1 and b"collapse" in lib.lg_last_error(), (rc, lib.lg_last_error())                           # LG_EINVAL, never an answer
        assert last_plan(L)[0] == A.NONE


def test_refusals_and_empties(hip, L):
    lib = L.lib()
    dummy = hip.from_numpy(np.arange(8, dtype=np.float32), requires_grad=False)
    out = hip.from_numpy(np.full(8, 7, np.int64), requires_grad=False)
    for op in OPS:
        for shape, axis in A.EMPTY_REDUCTION:
            with pytest.raises(ValueError, match="attempt to get %s of an empty sequence" % op):
                getattr(hip.from_numpy(np.zeros(shape, np.float32)), op)(axis=axis)
        for shape, axis in A.EMPTY_OUTPUT:
            got = getattr(hip.from_numpy(np.zeros(shape, np.float32)), op)(axis=axis)
            assert got.dtype == np.int64 and got.numpy().shape == np.zeros(shape).argmax(axis=axis).shape
        for dtype in (np.float64, np.int32):
            with pytest.raises(TypeError):
                getattr(hip.from_numpy(np.zeros((3, 4), dtype), requires_grad=False), op)(axis=1)
        with pytest.raises(np.exceptions.AxisError):
            getattr(dummy, op)(axis=1)
        scalar = hip.from_numpy(np.full((), 7, np.float32), requires_grad=False)             # 0-d: numpy takes axis 0 / -1 and no other
        assert int(getattr(scalar, op)(axis=0).numpy()) == 0 and int(getattr(scalar, op)(axis=-1, keepdims=True).numpy()) == 0
        with pytest.raises(np.exceptions.AxisError):
            getattr(scalar, op)(axis=1)
    raw = lambda shape, axis: lib.lg_argreduce_f32(L.RED_MAX, len(shape), L.i64(shape), dummy.ptr, L.i64(A.layout(np.zeros(shape, np.float32))[2]),   # noqa: E731
                                                   axis, out.ptr)
    dummy.argmax()
    assert last_plan(L)[0] == A.ROWS_WAVE
    assert raw((0, 3), 1) == 0 and last_plan(L)[0] == A.NONE                 # no output elements: nothing is launched
    assert raw((3, 0), 1) == -1 and b"empty sequence" in lib.lg_last_error() and last_plan(L)[0] == A.NONE
    assert raw((0, 0), 1) == -1 and raw((0,), -1) == -1
    assert raw((2, 4), 2) == -1 and raw((2, 4), -2) == -1                    # the ABI's axis is 0 .. ndim - 1, or -1 for all
    assert lib.lg_argreduce_f32(0, 1, L.i64((8,)), dummy.ptr, L.i64((1,)), 0, out.ptr) == -1      # LG_RED_SUM has no index
    assert lib.lg_argreduce_last_plan(None) == -1
    np.testing.assert_array_equal(out.numpy(), 7)                             # none of these wrote anything
    assert raw((2, 4), 1) == 0 and last_plan(L)[0] == A.ROWS_WAVE
    np.testing.assert_array_equal(out.numpy()[:2], [3, 3])


def test_captured_argmax_follows_the_data(hip, L):
    """a captured launch reads the tensor at every replay; the split kernels take their scratch from the pool inside the capture"""
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(5)
    data = [rng.standard_normal((3, 20001)).astype(np.float32) for _ in range(3)]
    x = hip.from_numpy(data[0], requires_grad=False)
    x.argmax(axis=1), x.argmin(axis=0), x.argmax()                            # eager once: pool, kernels
    graph = HipGraph()
    with graph.capture():
        rows, cols, whole = x.argmax(axis=1), x.argmin(axis=0), x.argmax()
    assert graph.kernel_count() == 3
    for a in data[1:]:
        x.upload_(a)
        graph.replay()
        np.testing.assert_array_equal(rows.numpy(), np.argmax(a, axis=1))
        np.testing.assert_array_equal(cols.numpy(), np.argmin(a, axis=0))
        np.testing.assert_array_equal(whole.numpy(), np.argmax(a))
    graph.destroy()
