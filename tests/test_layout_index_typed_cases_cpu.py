"""The case tables of the layout, index and typed sweeps on the host (tests/layout_cases.py, tests/index_cases.py,
tests/typed_cases.py): the tables are well-formed - the view a device test rebuilds from `layout()` is the numpy view, byte for
byte -, the constructions force the answers they claim, numpy's own float32 np.add.at and float64 sum lie inside the derived
bounds, every path and edge the GPU tests assert is named somewhere in the tables, and CpuTensor agrees with numpy on every case."""
import numpy as np
import pytest
import layout_cases as LC
import index_cases as IC
import typed_cases as TC
from lightgrad_amd import CpuTensor

TABLES = {"layout": LC, "index": IC, "typed": TC}
ALL = [(table, c.name) for table, mod in TABLES.items() for c in mod.CASES]
_numpy_results = {}


class Checked(LC.NumpyBackend):
    """numpy, checking every view on its way in: what `layout` describes IS the view, and no base holds too many elements"""
    def _check(self, view):
        view = np.asarray(view)
        base, shape, strides, offset = LC.layout(view)
        assert base.size <= LC.MAX_ELEMENTS and view.size <= LC.MAX_ELEMENTS
        assert shape == view.shape
        assert LC.view_of(base, shape, strides, offset).tobytes() == view.tobytes()
        if view.size:
            reach = [offset + sum((n - 1) * s for n, s in zip(shape, strides) if s * sign > 0) for sign in (-1, 1)]
            assert 0 <= reach[0] and reach[1] < base.size, "the view leaves its base"

    def t(self, view, **kw):
        self._check(view)
        return LC.NumpyBackend.t(self, view, **kw)

    def views(self, *views):
        for v in views:
            self._check(v)
        return LC.NumpyBackend.views(self, *views)

    def idx(self, array, how):
        if how not in ("host", "list"):
            self._check(np.asarray(array).astype(how) if np.asarray(array).flags["C_CONTIGUOUS"] else array)
        return LC.NumpyBackend.idx(self, array, how)

    def mask(self, array):
        self._check(array)
        return LC.NumpyBackend.mask(self, array)


def numpy_result(table, name):
    """(values, base arrays, the backend) of a case on numpy: computed once"""
    key = (table, name)
    if key not in _numpy_results:
        B = Checked()
        out, bases = LC.run_case(TABLES[table].BY_NAME[name], B)
        _numpy_results[key] = (out, bases, B)
    return _numpy_results[key]


class CpuBackend(LC.NumpyBackend):
    name = "cpu"

    def wrap(self, flat, shape, strides, offset):
        return CpuTensor.from_numpy(LC.view_of(flat, shape, strides, offset), requires_grad=False)

    def np(self, x):
        return np.array(x.numpy() if isinstance(x, CpuTensor) else x, copy=True)

    def idx(self, array, how):
        raw = LC.NumpyBackend.idx(self, array, how)
        return raw if how in ("host", "list") else CpuTensor.from_numpy(raw, requires_grad=False)

    def mask(self, array):
        return CpuTensor.from_numpy(array, requires_grad=False)

    def rng(self, n):
        return range(n)

    def take_grad(self, a, index, w):
        t = CpuTensor.from_numpy(a.copy())
        (t[index] * CpuTensor.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
        return t.grad


@pytest.mark.parametrize("table,name", ALL)
def test_table_is_well_formed_and_cpu_tensor_equals_numpy(table, name):
    """every view of the case passes `Checked`; CpuTensor gives what numpy gives, by the rule the case names.  No case is
    unsupported on the numpy backend: none is left out here."""
    case = TABLES[table].BY_NAME[name]
    want = numpy_result(table, name)
    B = CpuBackend()
    got = LC.run_case(case, B)
    LC.compare(case, got, want[:2])
    assert len(want[0]) + len(want[1]) > 0
    assert B.plans == want[2].plans


def merged_ndim(shape, strides):
    """dimensions left after dropping extents of 1 and merging neighbours that one stride walks"""
    dims = [(n, s) for n, s in zip(shape, strides) if n != 1]
    out = []
    for n, s in dims:
        if out and out[-1][1] == s * n:
            out[-1] = (out[-1][0] * n, s)
        else:
            out.append((n, s))
    return len(out)


def test_five_dimensions_do_not_collapse():
    _, shape, strides, _ = LC.layout(LC._five_dims(np.arange(275, dtype=np.int16)))
    assert shape == (3, 2, 3, 2, 3) and merged_ndim(shape, strides) == 5
    assert merged_ndim((2, 3, 4), (12, 4, 1)) == 1 and merged_ndim((3, 2, 3, 2, 3), (60, 30, 12, 3, -1)) == 4


def test_layout_table_names_every_path_for_every_item_size():
    named = set()
    for c in LC.CASES:
        named |= set(numpy_result("layout", c.name)[2].plans)
    for path, sizes in LC.PATH_ITEM_SIZES.items():
        for size in sizes:
            assert any(p == path and s == size for p, s, _, _ in named), (path, size)
        assert not any(p == path and s not in sizes for p, s, _, _ in named), path
    assert any(p == LC.NONE for p, _, _, _ in named)
    for size in (1, 2, 4, 8):                               # flat fills: a head of every size there is, bodies of 0 and of more
        flat = [(h, b) for p, s, h, b in named if p == LC.FILL_FLAT and s == size]
        assert {h for h, _ in flat} == set(range(16 // size)), size
        assert any(b == 0 for _, b in flat) and any(b > 2 * (16 // size) for _, b in flat)
        assert any(h > 0 and b == 0 for h, b in flat) and any(h == 0 and b > 0 for h, b in flat)


def test_flat_fills_write_their_range_and_nothing_else():
    """numpy's side of the sentinel rule, spelled out: the filled range holds the value's bytes, every other item its sentinel"""
    for dtype in LC.ALL_DTYPES:
        per = 16 // dtype.itemsize
        bases = iter(numpy_result("layout", "fill_flat_%s" % dtype)[1])
        for value in LC.FILL_VALUES[dtype]:
            for k, n, head, body in LC.flat_fill_geometry(dtype):
                got = next(bases)
                before = LC.sentinel("fill_flat_%s_%d_%d" % (dtype, k, n), k + n + 2 * per + 3, dtype)
                assert got[:k].tobytes() == before[:k].tobytes() and got[k + n:].tobytes() == before[k + n:].tobytes()
                assert got[k:k + n].tobytes() == np.asarray(value).tobytes() * n
                assert not (before == value).any() or dtype == np.bool_
                assert 0 <= head <= min(n, per - 1) and head + body * per <= n < head + (body + 1) * per
    assert np.float32(LC.FILL_VALUES[np.dtype(np.float32)][1]).tobytes() == bytes([0x45, 0x23, 0xC1, 0x7F])


def test_overlapping_copies_are_numpy_right_hand_side_first():
    a = LC.values("overlap_shift_%s" % np.dtype(np.int16), (301,), np.int16)
    got = numpy_result("layout", "copy_overlapping_int16")[1][0]
    assert np.array_equal(got[1:], a[:-1]) and got[0] == a[0]


# ---- index ---------------------------------------------------------------------------------------------------------------------------
def test_no_assignment_but_one_names_a_position_twice():
    seen = 0
    for c in IC.CASES:
        puts = numpy_result("index", c.name)[2].puts
        seen += len(puts)
        for p in puts:
            if c.name == "put_repeats":
                a, i, _ = IC.put_repeats_data()
                repeated = IC.put_repeats_positions()
                assert len(repeated) == 2 and len(np.unique(p)) < len(p)
                assert len(repeated) * (a.size // 50) < 0.1 * a.size
            else:
                assert len(np.unique(p)) == len(p), c.name
    assert seen > 100
    IC.check_put_repeats(*[(r[0], r[1]) for r in [numpy_result("index", "put_repeats")] * 2])      # numpy's "last write" is one of them


def test_masks_cover_every_block_count_and_give_flatnonzero():
    assert {IC.mask_blocks(n) for n in IC.MASK_LENGTHS} == IC.MASK_BLOCK_COUNTS
    assert IC.mask_blocks(256 * 4096) == 256 and IC.mask_blocks(256 * 4096 + 1) == 257      # on either side of the scan's chunk
    for n in IC.MASK_LENGTHS:
        out, k, tags = numpy_result("index", "mask_length_%d" % n)[0], 0, []
        for tag, m in IC.mask_patterns(n):
            assert m.shape == (n,) and m.dtype == np.bool_
            np.testing.assert_array_equal(out[k], np.flatnonzero(m))
            assert out[k].dtype == np.int64
            k += 2 if (n <= 4097 or tag == "half") else 1
            tags.append(tag)
        assert k == len(out)
        assert "none" in tags and "only_0" in tags and "only_%d" % (n - 1) in tags and "half" in tags
        if n > 256 * 4096:
            assert "only_%d" % (256 * 4096) in tags and "block_255" in tags          # the first element of block 256; block 255 full
        if IC.mask_blocks(n) > 257:
            assert "block_256" in tags                                                # the first block of the scan's second chunk full
        if n > 2 * 4096:
            assert "block_1" in tags and "only_4095" in tags and "only_4096" in tags


def test_numpy_scatter_add_lies_inside_the_bound():
    for tier in ("exact", "general"):
        out = numpy_result("index", "scatter_" + tier)[0]
        assert IC.scatter_bound(tier, out) == 3 * len(IC.INDEX_KINDS)
    exact, k = numpy_result("index", "scatter_exact")[0], 0
    for shape, idx, w in IC.scatter_data("exact"):         # the exact tier: float32 np.add.at IS the float64 one
        ref = np.zeros(shape)
        np.add.at(ref, (slice(None), idx), w.astype(np.float64))
        assert np.abs(ref).max() < 2 ** 24 and np.abs(w).max() * IC.SCATTER_N < 2 ** 24
        for _ in IC.INDEX_KINDS:
            np.testing.assert_array_equal(exact[k].astype(np.float64), ref)
            k += 1


def test_long_axis_needs_more_than_int16():
    n = 40000
    assert n - 1 > np.iinfo(np.int16).max >= n - 32768 - 1 and -32768 + n == 7232


# ---- typed ---------------------------------------------------------------------------------------------------------------------------
def test_planted_casts_tell_a_direct_conversion_from_one_through_double():
    for v in (2 ** 53 + 2 ** 29 + 1, -(2 ** 53 + 2 ** 29 + 1), 2 ** 62 + 2 ** 38 + 1):
        direct = np.array([v], np.int64).astype(np.float32)[0]
        twice = np.array([v], np.int64).astype(np.float64).astype(np.float32)[0]
        assert direct != twice, v
        assert v in TC.cast_values(np.int64, np.float32)
    for v in (2 ** 24 + 1, 2 ** 24 + 3, 2 ** 53 + 1):
        assert v in TC.cast_values(np.int64, np.float32) and v in TC.cast_values(np.int64, np.float64)
    assert np.float32(2 ** 24 + 1) == 2 ** 24 and np.float32(2 ** 24 + 3) == 2 ** 24 + 4 and float(2 ** 53 + 1) == 2 ** 53      # ties to even
    x = TC.cast_values(np.float64, np.float32)
    with np.errstate(all="ignore"):
        y = x.astype(np.float32)
    assert np.isinf(y).sum() >= 6 and ((y != 0) & (np.abs(y) < 2.0 ** -126)).sum() >= 6 and np.signbit(y[y == 0]).any()
    assert y.reshape(-1)[0] == 1 and y.reshape(-1)[1] == np.float32(1 + 2.0 ** -22)                                    # the two ties
    for src in (np.float32, np.float64):
        for dst in (np.int16, np.int32, np.int64):
            x = TC.cast_values(src, dst).astype(np.float64)
            assert np.isfinite(x).all() and np.abs(x).max() < 2.0 ** (np.iinfo(dst).bits - 1)


def test_reduction_constructions_force_their_answers():
    assert TC.plant_positions(257) == [0, 1, 255, 256] and TC.plant_positions(3) == [0, 1, 2] and TC.plant_positions(1) == [0]
    assert TC.plant_positions(4097) == [0, 1, 255, 256, 4096] and TC.plant_positions(255) == [0, 1, 254]
    assert all(r1 * r2 == n for n in TC.RED_LENGTHS for r1, r2 in [TC.factors(n)])
    for dtype in TC.TYPED:
        assert numpy_result("typed", "extrema_%s" % dtype)[2].forced >= 2 * len(TC.RED_LENGTHS) * 9
        assert np.abs(TC.background("x", 3, 4097, dtype)).max() <= 2049
    # integer sums: rows that overflow their own type do not overflow int64; the int64 rows wrap
    for dtype, wraps in ((np.int16, False), (np.int32, False), (np.int64, True)):
        info = np.iinfo(dtype)
        assert (abs(info.min) * 4097 >= 2 ** 63) == wraps and info.max * 513 > info.max


def test_numpy_float64_sum_lies_inside_the_bound():
    out = numpy_result("typed", "sums_general_float64")
    TC.check_sums_general(out[:2], out[:2])
    for x in TC.general_sum_data():
        for row in x:
            ref, bound = TC.sum_bound(row)
            assert abs(float(np.sum(row)) - ref) <= bound and abs(float(np.sum(row[::-1])) - ref) <= bound
            assert bound <= len(row) * 2.0 ** -52 * np.abs(row).sum()
