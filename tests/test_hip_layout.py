"""Strided copy and strided fill on the GPU (csrc/layout.hip) against numpy, byte for byte, for every item size.

The cases are tests/layout_cases.py (checked on the host by tests/test_layout_index_typed_cases_cpu.py): programs that run here
on HipTensor views of device memory and there on numpy.  After every call a case names, `lg_layout_last_plan` is compared with the
path the case is meant for - and, for flat fills, with the head and the body its view's geometry gives - so a changed dispatch
fails the case instead of emptying it.  Besides the values a case returns, EVERY base array is read back and compared whole: an
item written outside a view shows as a changed sentinel.

`HipBackend` is also what the sweeps of tests/test_hip_index.py and tests/test_hip_typed.py run their tables on."""
import ctypes
import numpy as np
import pytest
import layout_cases as LC

pytestmark = pytest.mark.gpu


class HipBackend(LC.NumpyBackend):
    """the cases' tensors as HipTensor views of device copies of the bases"""
    name = "hip"

    def __init__(self, hip):
        LC.NumpyBackend.__init__(self)
        from lightgrad_amd.autograd.hip import lib as hiplib
        self.hip, self.L = hip, hiplib
        self.seen = []               # (path, item size, head, body) as the library reported them

    def _flat_copy(self, base):
        flat = self.hip.from_numpy(base, requires_grad=False)
        self._bases.append(flat)
        return flat

    def wrap(self, flat, shape, strides, offset):
        return self.hip(flat.data, shape, strides, flat._offset + offset, flat._dtype, requires_grad=False)

    def _unregistered(self, array):
        """a tensor the case does not write: dense arrays uploaded as they are, strided views as views of their uploaded base"""
        if array.flags["C_CONTIGUOUS"]:
            return self.hip.from_numpy(array, requires_grad=False)
        base, shape, strides, offset = LC.layout(array)
        return self.wrap(self.hip.from_numpy(base, requires_grad=False), shape, strides, offset)

    def idx(self, array, how):
        raw = LC.NumpyBackend.idx(self, array, how)
        return raw if how in ("host", "list") else self._unregistered(raw)

    def mask(self, array):
        return self._unregistered(LC.NumpyBackend.mask(self, array))

    def rng(self, n):
        return range(n)

    def take_grad(self, a, index, w):
        t = self.hip.from_numpy(a.copy())
        (t[index] * self.hip.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
        return t.grad

    def np(self, x):
        return x.numpy() if isinstance(x, self.hip) else np.array(x, copy=True)

    def base_arrays(self):
        return [b.numpy() for b in self._bases]

    def last_plan(self):
        p = (ctypes.c_int32 * 4)()
        self.L.check(self.L.lib().lg_layout_last_plan(p))
        return tuple(p)

    def plan(self, path, itemsize, head=0, body=0):
        got = self.last_plan()
        n = len(self.seen)
        assert got[0] == path, "call %d (%d-byte items) is meant for path %d, the library took path %d (plan %s)" % (n, itemsize, path, got[0], got)
        assert got[1] == (32 if path in (LC.COPY_GATHER, LC.FILL_GATHER) else 0), (n, got)
        assert got[2:] == (head, body), "call %d (%d-byte items): head and body %s, the view's geometry gives %s" % (n, itemsize, got[2:], (head, body))
        self.seen.append((path, itemsize, head, body))


_numpy = {}
_seen = {}


def numpy_result(table, name):
    if (table.__name__, name) not in _numpy:
        B = LC.NumpyBackend()
        _numpy[(table.__name__, name)] = LC.run_case(table.BY_NAME[name], B) + (B,)
    return _numpy[(table.__name__, name)]


def run_on_device(hip, table, name):
    """the case on HipTensor, compared with numpy by the rule it names; returns the backend"""
    case = table.BY_NAME[name]
    want = numpy_result(table, name)
    B = HipBackend(hip)
    got = LC.run_case(case, B)
    LC.compare(case, got, want[:2])
    assert B.seen == want[2].plans
    return B


@pytest.mark.parametrize("name", [c.name for c in LC.CASES])
def test_case_equals_numpy_and_takes_its_path(hip, name):
    _seen[name] = set(run_on_device(hip, LC, name).seen)


def test_table_reaches_every_path_for_every_item_size(hip):
    """the plans the library REPORTED over the whole table: every path for every item size it applies to; flat fills with a head
    of every size there is, with no body and with one"""
    seen = set()
    for c in LC.CASES:
        seen |= _seen[c.name] if c.name in _seen else set(run_on_device(hip, LC, c.name).seen)
    for path, sizes in LC.PATH_ITEM_SIZES.items():
        for size in sizes:
            assert any(p == path and s == size for p, s, _, _ in seen), (path, size)
    for size in (1, 2, 4, 8):
        flat = [(h, b) for p, s, h, b in seen if p == LC.FILL_FLAT and s == size]
        assert {h for h, _ in flat} == set(range(16 // size)), (size, sorted(flat))
        assert any(b == 0 for _, b in flat) and any(b > 0 for _, b in flat)
    named = set()
    for c in LC.CASES:
        named |= set(numpy_result(LC, c.name)[2].plans)
    assert seen == named
    print("layout (path, item size) reached: %s" % sorted({(p, s) for p, s, _, _ in seen}))
    for size in (1, 2, 4, 8):
        flat = [(h, b) for p, s, h, b in seen if p == LC.FILL_FLAT and s == size]
        print("flat fills of %d-byte items: heads %s, bodies %s" % (size, sorted({h for h, _ in flat}), sorted({b for _, b in flat})))


def test_plan_of_refused_and_empty_calls(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    B = HipBackend(hip)
    assert lib.lg_layout_last_plan(None) == -1
    t = hip.from_numpy(np.arange(12, dtype=np.int16).reshape(3, 4), requires_grad=False)
    t.transpose(1, 0).fill(5)
    assert B.last_plan() == (LC.FILL_GATHER, 32, 0, 0)
    assert lib.lg_fill_strided(3, 1, L.i64((4,)), t.ptr, L.i64((1,)), 0) == -1 and B.last_plan()[0] == LC.NONE      # refused: item size 3
    t.fill(7)
    assert B.last_plan() == (LC.FILL_FLAT, 0, 0, 1)
    assert lib.lg_copy_strided(2, 2, L.i64((3, 4)), t.ptr, L.i64((0, 1)), t.ptr, L.i64((4, 1))) == -1              # a destination of stride 0
    assert B.last_plan() == (LC.NONE, 0, 0, 0)
    np.testing.assert_array_equal(t.numpy(), np.full((3, 4), 7, np.int16))
    assert lib.lg_copy_strided(2, 2, L.i64((0, 4)), t.ptr, L.i64((4, 1)), t.ptr, L.i64((4, 1))) == 0 and B.last_plan()[0] == LC.NONE
