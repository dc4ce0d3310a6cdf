"""The case table of the layout sweep (tests/test_hip_layout.py): strided copy and strided fill for every item size, with numpy as
the reference.  No GPU code here: tests/test_layout_index_typed_cases_cpu.py checks on the host what the GPU test relies on.

A case is a small program written against the tensor interface that numpy arrays, CpuTensor and HipTensor share (views by
transposing and slicing, `fill`, `t[...] = value`, `t[...]`).  It runs on a BACKEND, which turns the numpy views the case builds
into tensors over a private copy of each view's base array:

    B.t(view)          the view as a tensor (same shape, strides and offset over a copy of the base)
    B.views(v, w, ..)  several views of ONE base as tensors over one shared copy (operands that overlap)
    B.plan(path, ..)   what `lg_layout_last_plan` is meant to report for the call just made (a no-op off the device)
    B.np(x)            a tensor's values as a numpy array

`run_case` returns the values a case hands back and EVERY base array as it stands afterwards; the tests compare both with
numpy's byte for byte, so an element written outside a view (a head or a tail one item too long) shows as a changed sentinel.

`lg_copy_strided` / `lg_fill_strided` (csrc/layout.hip) choose among a device memcpy, the elementwise engine (4-byte items), the
copy gather kernel, the flat fill and the fill gather kernel; every case names the path it is meant to reach and, for flat fills,
the head and body the geometry of its view gives.  The GPU test asserts that, so a changed dispatch fails the case instead of
silently emptying it.  The dispatch conditions are not restated here.
"""
from collections import namedtuple
import zlib
import numpy as np

MEMCPY, EW, COPY_GATHER, FILL_FLAT, FILL_GATHER, NONE = 0, 1, 2, 3, 4, -1
MAX_ELEMENTS = 4 << 20           # no case holds more

ITEM_DTYPES = {1: (np.uint8, np.bool_), 2: (np.int16,), 4: (np.float32, np.int32), 8: (np.int64, np.float64)}
ALL_DTYPES = tuple(np.dtype(d) for size in (1, 2, 4, 8) for d in ITEM_DTYPES[size])
# which item sizes each path applies to
PATH_ITEM_SIZES = {MEMCPY: (1, 2, 4, 8), EW: (4,), COPY_GATHER: (1, 2, 8), FILL_FLAT: (1, 2, 4, 8), FILL_GATHER: (1, 2, 4, 8)}


def rng_of(name):
    return np.random.RandomState(zlib.crc32(name.encode()))


def layout(view):
    """(flat base array, shape, strides in elements, offset in elements) of a numpy view of any item size"""
    base = view
    while base.base is not None:
        base = base.base
    assert isinstance(base, np.ndarray) and base.flags["C_CONTIGUOUS"] and base.dtype == view.dtype, "a view of one dense array"
    base = base.reshape(-1)
    size = view.dtype.itemsize
    offset = view.__array_interface__["data"][0] - base.__array_interface__["data"][0]
    assert offset % size == 0 and all(s % size == 0 for s in view.strides)
    if view.size == 0:
        return base, tuple(view.shape), tuple(s // size for s in view.strides), 0
    return base, tuple(view.shape), tuple(s // size for s in view.strides), offset // size


def view_of(flat, shape, strides, offset):
    """the view `layout` described, rebuilt over `flat` (a flat array of the base's length)"""
    size = flat.dtype.itemsize
    if len(shape) == 0:
        return flat[offset:offset + 1].reshape(())
    if 0 in shape:
        return np.empty(shape, flat.dtype)
    return np.lib.stride_tricks.as_strided(flat[offset:], shape, tuple(s * size for s in strides))


class NumpyBackend(object):
    """the reference: numpy arrays, on private copies of the bases; records what a case asks of the device"""
    name = "numpy"

    def __init__(self):
        self._bases = []
        self.plans = []              # (path, item size, head, body) named by the case
        self.puts = []               # flat positions every assignment through index arrays names (tests/index_cases.py)

    def _flat_copy(self, base):
        flat = base.copy()
        self._bases.append(flat)
        return flat

    def wrap(self, flat, shape, strides, offset):
        return view_of(flat, shape, strides, offset)

    def t(self, view, **kw):
        base, shape, strides, offset = layout(np.asarray(view))
        return self.wrap(self._flat_copy(base), shape, strides, offset, **kw)

    def views(self, *views):
        flat, first, out = None, None, []
        for v in views:
            base, shape, strides, offset = layout(v)
            if flat is None:
                flat, first = self._flat_copy(base), base
            assert base.__array_interface__["data"][0] == first.__array_interface__["data"][0], "views of one base"
            out.append(self.wrap(flat, shape, strides, offset))
        return out

    def plan(self, path, itemsize, head=0, body=0):
        self.plans.append((path, itemsize, head, body))

    def note_put(self, flat_positions):
        self.puts.append(np.asarray(flat_positions).reshape(-1))

    # what tests/index_cases.py asks besides
    def idx(self, array, how):
        if how == "list":
            assert isinstance(array, list)
            return array
        array = np.asarray(array)
        if how == "host":
            return array.astype(np.int64)
        assert np.array_equal(array.astype(how), array), "an index the dtype cannot hold"
        return array.astype(how) if array.dtype != np.dtype(how) else array

    def mask(self, array):
        assert array.dtype == np.bool_
        return array

    def rng(self, n):
        return np.arange(n)

    # and tests/typed_cases.py
    def force(self, x, value):
        """x, after checking that it holds `value` everywhere (NaN equals NaN): an answer the construction forces"""
        got = self.np(x)
        np.testing.assert_array_equal(got, np.broadcast_to(np.asarray(value, got.dtype), got.shape))
        self.forced = getattr(self, "forced", 0) + 1
        return x

    def take_grad(self, a, index, w):
        grad = np.zeros(a.shape, np.float32)
        np.add.at(grad, index, w)
        return grad

    def np(self, x):
        return np.array(x, copy=True)

    def base_arrays(self):
        return [np.array(b, copy=True) for b in self._bases]


def run_case(case, backend):
    """(values the case returns, every base array afterwards), all numpy arrays"""
    with np.errstate(all="ignore"):          # the operands hold every bit pattern: signalling NaNs, integers that wrap
        out = case.run(backend)
    out = [] if out is None else (list(out) if isinstance(out, (list, tuple)) else [out])
    return [backend.np(x) for x in out], backend.base_arrays()


def compare(case, got, want):
    """got, want: what `run_case` returned on a backend and on numpy.  Byte for byte, unless the case names another rule"""
    rule = getattr(case, "compare", None)
    if rule is not None:
        return rule(got, want)
    same_bytes(got[0], want[0], case.name + ": values")
    same_bytes(got[1], want[1], case.name + ": base arrays")


def same_bytes(got, want, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, "%s #%d: %s %s, numpy gives %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            gb, wb = g.reshape(-1).view(np.uint8), w.reshape(-1).view(np.uint8)
            bad = np.flatnonzero(gb != wb) // g.dtype.itemsize
            raise AssertionError("%s #%d: %d elements differ from numpy, the first at flat position %d (got %r, want %r)" % (
                what, k, len(np.unique(bad)), bad[0], g.reshape(-1)[bad[0]], w.reshape(-1)[bad[0]]))


Case = namedtuple("Case", "name run")
CASES = []


def case(name, run):
    CASES.append(Case(name, run))


def sentinel(name, n, dtype):
    """n items whose every byte lies in [0x10, 0x50): no item equals a fill value below, and every item is a finite number"""
    dtype = np.dtype(dtype)
    raw = rng_of(name).randint(0x10, 0x50, n * dtype.itemsize).astype(np.uint8)
    if dtype == np.bool_:
        return (raw & 1).astype(np.bool_)
    return raw.view(dtype).copy()


def values(name, shape, dtype):
    """random bytes as items: every bit pattern the item size holds, NaN payloads and -0.0 among them (booleans: 0 / 1)"""
    dtype = np.dtype(dtype)
    n = int(np.prod(shape, dtype=np.int64))
    raw = rng_of(name).randint(0, 256, n * dtype.itemsize).astype(np.uint8)
    if dtype == np.bool_:
        return (raw & 1).astype(np.bool_).reshape(shape)
    return raw.view(dtype).copy().reshape(shape)


def _bits(dtype, pattern):
    dtype = np.dtype(dtype)
    return np.array([pattern], {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dtype.itemsize]).view(dtype)[0]


# fill values with distinct bytes: a truncated or byte-swapped value shows
FILL_VALUES = {
    np.dtype(np.uint8): [_bits(np.uint8, 0x5A)],
    np.dtype(np.bool_): [np.bool_(True)],
    np.dtype(np.int16): [_bits(np.int16, 0xA55A)],
    np.dtype(np.float32): [_bits(np.float32, 0x80000000), _bits(np.float32, 0x7FC12345)],      # -0.0f, a NaN with a payload
    np.dtype(np.int32): [_bits(np.int32, 0x80000000), _bits(np.int32, 0x7FC12345)],
    np.dtype(np.int64): [_bits(np.int64, 0x0123456789ABCDEF)],
    np.dtype(np.float64): [_bits(np.float64, 0x0123456789ABCDEF)],
}


# ---- fill, the flat path: base[k : k + n] for every misalignment k and the lengths around every edge of head, body and tail --------
def flat_fill_lengths(per, head):
    """1; around the head; one body vector short of one item, exactly one; where the grid stops being the floor; ragged thousands"""
    want = [1, head - 1, head, head + 1, head + per - 1, head + per, head + 2 * per * per + 1, head + (2 * per + 1) * per, 3001 + head]
    return sorted({n for n in want if n >= 1})


def flat_fill_geometry(dtype):
    """(k, n, head, body) of every flat fill of the sweep: the base is 16-byte aligned, the view starts k items into it"""
    per = 16 // np.dtype(dtype).itemsize
    out = []
    for k in range(per):
        head = (per - k) % per
        for n in flat_fill_lengths(per, head):
            h = min(head, n)
            out.append((k, n, h, (n - h) // per))
    return out


def flat_plan(dtype, offset, n):
    """(path, item size, head, body) of a flat fill of n items that starts `offset` items into a 16-byte aligned base"""
    size = np.dtype(dtype).itemsize
    per = 16 // size
    head = min((-offset) % per, n)
    return FILL_FLAT, size, head, (n - head) // per


def _fill_flat(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        per = 16 // dtype.itemsize
        for value in FILL_VALUES[dtype]:
            for k, n, head, body in flat_fill_geometry(dtype):
                base = sentinel("fill_flat_%s_%d_%d" % (dtype, k, n), k + n + 2 * per + 3, dtype)
                t = B.t(base[k:k + n])
                t.fill(value)
                assert (FILL_FLAT, dtype.itemsize, head, body) == flat_plan(dtype, k, n)
                B.plan(FILL_FLAT, dtype.itemsize, head, body)
    return run


def _five_dims(flat):
    """five dimensions, none of which merges with a neighbour: (3, 2, 3, 2, 3) out of a dense (3, 3, 5, 2, 3)"""
    return flat[:270].reshape(3, 3, 5, 2, 3)[:, ::2, ::2, :, ::-1]


def _fill_strided(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        size = dtype.itemsize
        for value in FILL_VALUES[dtype]:
            s = lambda tag, n: sentinel("fill_strided_%s_%s" % (dtype, tag), n, dtype)      # noqa: E731
            for tag, view in (("step2", s("step2", 41)[1::2]), ("negative", s("negative", 37)[30:3:-1]),
                              ("negative_step3", s("negative3", 50)[::-3]), ("transposed", s("transposed", 7 * 9 + 2)[1:64].reshape(7, 9).T),
                              ("inner_step", s("inner", 6 * 10)[:60].reshape(6, 10)[1:5, ::3]), ("five", _five_dims(s("five", 275)))):
                t = B.t(view)
                t.fill(value)
                B.plan(FILL_GATHER, size)
            t = B.t(s("dense_nd", 40)[3:27].reshape(2, 3, 4))          # a dense N-d view is one run
            t.fill(value)
            B.plan(*flat_plan(dtype, 3, 24))
            t = B.t(s("scalar", 9)[6:7].reshape(()))                   # 0-d
            t.fill(value)
            B.plan(*flat_plan(dtype, 6, 1))
            t = B.t(s("one_strided", 30).reshape(5, 6)[2:3, ::-1][:, 1:2])      # a single element with strides of its own
            t.fill(value)
            B.plan(*flat_plan(dtype, 16, 1))
            for tag, view in (("empty", s("empty", 12)[5:5]), ("empty_2d", s("empty2", 12).reshape(3, 4)[:, 2:2])):
                t = B.t(view)
                t.fill(value)
                B.plan(NONE, size)
            # through __setitem__ with a scalar: the indexed view is filled
            t = B.t(s("setitem", 48).reshape(6, 8))
            t[1:5, ::2] = value
            B.plan(FILL_GATHER, size)
            t[2] = value
            B.plan(*flat_plan(dtype, 16, 8))
    return run


for _d in ALL_DTYPES:
    case("fill_flat_%s" % _d, _fill_flat(_d))
    case("fill_strided_%s" % _d, _fill_strided(_d))


# ---- copy ----------------------------------------------------------------------------------------------------------------------------
def gather_path(dtype):
    return EW if np.dtype(dtype).itemsize == 4 else COPY_GATHER


def _copy_sources(dtype):
    """`t[...]`: a dense copy of the view"""
    dtype = np.dtype(dtype)

    def run(B):
        size, out = dtype.itemsize, []
        v = lambda tag, *shape: values("copy_src_%s_%s" % (dtype, tag), shape, dtype)      # noqa: E731
        out.append(B.t(v("dense", 6, 11))[...])
        B.plan(MEMCPY, size)
        out.append(B.t(v("dense_1d", 4099))[...])
        B.plan(MEMCPY, size)
        out.append(B.t(v("offset", 100)[7:71].reshape(4, 16))[...])              # a dense view off the start of its base
        B.plan(MEMCPY, size)
        for tag, view in (("steps", v("steps", 9, 14)[::2, ::-1]), ("outer_negative", v("outer_negative", 9, 14)[::-1, 1::3]),
                          ("inner_step", v("inner_step", 70, 67)[:, ::2]), ("outer_step", v("outer_step", 70, 67)[1::3]),
                          ("reversed_1d", v("reversed", 300)[::-1]), ("five", _five_dims(v("five", 275))),
                          ("transposed_slice", v("tslice", 130, 66)[:, :65].T)):
            out.append(B.t(view)[...])
            B.plan(gather_path(dtype), size)
        out.append(B.t(v("scalar", 9)[4:5].reshape(()))[...])                    # 0-d
        B.plan(MEMCPY, size)
        out.append(B.t(v("one", 5, 6)[2:3, ::-1][:, 1:2].T)[...])                # a single element with strides of its own
        B.plan(MEMCPY, size)
        for view in (v("empty", 12)[5:5], v("empty2", 12).reshape(3, 4)[:, 2:2], v("empty3", 24).reshape(2, 3, 4)[::-1, 3:, ::2]):
            out.append(B.t(view)[...])
            B.plan(NONE, size)
        # dense in another dimension order: copied as one run in the view's own order, no strided call (the plan is not asked)
        out.append(B.t(v("permuted", 5, 6, 7).transpose(2, 0, 1))[...])
        out.append(B.t(v("permuted_2d", 130, 65).T)[...])
        return out
    return run


def _copy_into_views(dtype):
    """`d[...] = s`: destinations that are views of a sentinel base"""
    dtype = np.dtype(dtype)

    def run(B):
        size = dtype.itemsize
        v = lambda tag, *shape: values("copy_into_%s_%s" % (dtype, tag), shape, dtype)      # noqa: E731
        s = lambda tag, n: sentinel("copy_into_%s_%s" % (dtype, tag), n, dtype)             # noqa: E731
        gather = gather_path(dtype)

        def put(dst, src, path):
            d = B.t(dst)
            d[...] = B.t(src)
            B.plan(path, size)

        put(s("dense", 90)[5:71].reshape(6, 11), v("dense", 6, 11), MEMCPY)
        # transposed 2-D, both extents across 64: the source strided, then the destination
        put(s("t_src", 65 * 130 + 3)[3:].reshape(65, 130), v("t_src", 130, 65).T, gather)
        put(s("t_dst", 65 * 130 + 3)[3:].reshape(130, 65).T, v("t_dst", 65, 130), gather)
        put(s("t_both", 66 * 131).reshape(131, 66)[:130, :65].T, v("t_both", 65, 140)[:, 5:135], gather)
        # steps and negative steps, inner and outer, on either side
        put(s("steps_dst", 9 * 14).reshape(9, 14)[::-1, ::2], v("steps_dst", 9, 7), gather)
        put(s("steps_both", 9 * 14).reshape(9, 14)[1::2, ::-3], v("steps_both", 12, 5)[::3, ::-1], gather)
        put(s("rev", 300)[280:10:-1], v("rev", 270), gather)
        put(s("five_dst", 275), v("five_dst", 275), MEMCPY)
        put(_five_dims(s("five", 275)), np.ascontiguousarray(_five_dims(v("five", 275))), gather)
        put(_five_dims(s("five_both", 275)), _five_dims(v("five_both", 275)), gather)
        # a broadcast source: a stride of 0 over an extent > 1
        put(s("row", 70).reshape(7, 10)[1:6, 1:9], v("row", 8), gather)
        put(s("col", 70).reshape(7, 10)[1:6, 1:9], v("col", 5, 1), gather)
        put(s("row_dense", 5 * 130 + 2)[2:].reshape(5, 130), v("row_dense", 130), gather)
        put(s("col_dense", 70 * 9).reshape(70, 9), v("col_dense", 70, 1), gather)
        put(s("one_to_all", 35).reshape(5, 7)[:, 1:6], v("one_to_all", 1), gather)
        put(s("scalar", 9)[3:4].reshape(()), v("scalar", 9)[5:6].reshape(()), MEMCPY)
        put(s("one", 30).reshape(5, 6)[2:3, ::-1][:, 1:2], v("one", 4, 4)[::-1, ::2][1:2, 1:2], MEMCPY)
        put(s("empty", 12).reshape(3, 4)[:, 2:2], v("empty", 3, 4)[:, 1:1], NONE)
        # through __setitem__ with a basic index
        d = B.t(s("setitem", 6 * 8).reshape(6, 8))
        d[1:5, ::2] = B.t(v("setitem", 4, 4))
        B.plan(gather, size)
        d[5] = B.t(v("setitem_row", 8))
        B.plan(MEMCPY, size)
    return run


def _copy_overlapping(dtype):
    """source and destination are views of ONE tensor: numpy evaluates the right-hand side first"""
    dtype = np.dtype(dtype)

    def run(B):
        a = values("overlap_shift_%s" % dtype, (301,), dtype)
        d, s = B.views(a[1:], a[:-1])
        d[...] = s
        a = values("overlap_shift2d_%s" % dtype, (40, 9), dtype)
        d, s = B.views(a[:, 1:], a[:, :-1])
        d[...] = s
        a = values("overlap_reverse_%s" % dtype, (33, 70), dtype)
        d, s = B.views(a[:, ::-1], a)
        d[...] = s
        a = values("overlap_transpose_%s" % dtype, (65, 65), dtype)
        d, s = B.views(a, a.T)
        d[...] = s
        a = values("overlap_same_%s" % dtype, (6, 7), dtype)              # the identical view: nothing moves
        d, s = B.views(a[1:, ::2], a[1:, ::2])
        d[...] = s
    return run


for _d in ALL_DTYPES:
    case("copy_sources_%s" % _d, _copy_sources(_d))
    case("copy_into_views_%s" % _d, _copy_into_views(_d))
    case("copy_overlapping_%s" % _d, _copy_overlapping(_d))

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
