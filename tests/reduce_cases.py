"""The case table of the float32 reduction sweep (tests/test_hip_reduce.py) and its references.  No GPU code here:
tests/test_reduce_cases_cpu.py checks on the host what the GPU test relies on.

`lg_reduce` / `lg_reduce_acc` (csrc/reduce.hip) pick one of four kernels after collapsing strides: red_rows_wave, red_rows_split
(two-level ticket fold over groups of 32 segments), red_cols_tile (up to 16 row chunks) and red_cols (odometer, up to 64
splits folded eight at a time).  Every case names the kernel - and where it matters the split and group count - it is MEANT
to reach; the GPU test asserts that against `lg_reduce_last_plan`, so a retuned threshold that moves a case to another
kernel fails the test instead of silently emptying it.  The thresholds themselves are not restated here.

A case is a strided view: `shape` and `strides` (elements) at element `offset` of a flat float32 array of `backing`
elements, reduced over `axes`.  Views the tensor API cannot make (a base one element off alignment, zero strides on a
reduced axis) are made from the pointer and the offset.

Inputs:
  exact  nonzero integers |v| <= vmax = min(8, 2**24 // rlen) stored as float32: every partial sum in every order is an integer
         of magnitude <= 2**24, exact in float32, so the kernel must return numpy's int64 sum bit for bit and ONE dropped,
         doubled or misplaced element shows at any size (the array outside the view is filled too)
  real   uniform(0.25, 1): judged against the float64 sum by the rule of tests/common.py (relative Frobenius distance at most
         max(1e-5, twice numpy's own float32 distance)), and max / min by exact equality with numpy

Two branches of the dispatch are not reached by any case, and no case is contorted to reach them: `n_out > 65535` inside the
split-rows path (that path is only entered with fewer than 256 rows) and a ticket count above the pool of 65536 (fewer than
256 rows times a few dozen groups).

`ndim == 0` is listed under rows_wave: a 0-d tensor collapses to one kept and one reduced dimension of extent 1, which is the
wave-per-row kernel's condition (`rlen == 1`), not the general kernel's.
"""
import zlib
from collections import namedtuple
from functools import lru_cache
import numpy as np

ROWS_WAVE, ROWS_SPLIT, COLS_TILE, COLS, NONE = 0, 1, 2, 3, -1
FAMILIES = {"rows_wave": ROWS_WAVE, "rows_split": ROWS_SPLIT, "cols_tile": COLS_TILE, "cols": COLS}
MAX_ELEMENTS = 4 << 20           # no case holds more
EXACT_LIMIT = 1 << 24            # integers of magnitude up to here are exact in float32
NUMPY32_CAP = 2.5e-6             # numpy's float32 sum of a real-valued case stays this close to float64 (CPU test)
FLOOR = 1e-5                     # the project's north-star distance


def contiguous(shape):
    st, n = [], 1
    for s in reversed(shape):
        st.append(n)
        n *= s
    return tuple(reversed(st))


class Case(namedtuple("Case", "name family shape strides offset backing axes want feature")):
    """want: {"splits": n} / {"splits_gt": 1} / {"groups": g, "splits_mod_32": m} / {"nk": ., "nr": ., "vec": 0 | 1} - asserted
    against the plan report in addition to the kernel of `family`"""

    @property
    def mask(self):
        m = 0
        for a in self.axes:
            m |= 1 << a
        return m

    @property
    def kept_shape(self):
        return tuple(s for i, s in enumerate(self.shape) if i not in self.axes)

    @property
    def reduced_shape(self):
        return tuple(s for i, s in enumerate(self.shape) if i in self.axes)

    @property
    def n_out(self):
        return int(np.prod(self.kept_shape, dtype=np.int64))

    @property
    def rlen(self):
        return int(np.prod(self.reduced_shape, dtype=np.int64))

    @property
    def vmax(self):
        return min(8, EXACT_LIMIT // max(self.rlen, 1))

    def view(self, flat):
        """the case's strided view of a flat array of `backing` elements (writable: zero strides alias on purpose)"""
        assert flat.shape == (self.backing,)
        return np.lib.stride_tricks.as_strided(flat[self.offset:], self.shape, tuple(s * flat.itemsize for s in self.strides))

    def element(self, o, r):
        """index into the flat array of reduced position r (row-major over the reduced axes) of output o (row-major over the kept axes)"""
        kept = np.unravel_index(o, self.kept_shape) if self.kept_shape else ()
        red = np.unravel_index(r, self.reduced_shape) if self.reduced_shape else ()
        kept, red, e = iter(kept), iter(red), self.offset
        for i, st in enumerate(self.strides):
            e += int(next(red) if i in self.axes else next(kept)) * st
        return e

    def row(self, o):
        """numpy index of the view selecting everything output o reduces over"""
        kept = iter(np.unravel_index(o, self.kept_shape) if self.kept_shape else ())
        return tuple(slice(None) if i in self.axes else int(next(kept)) for i in range(len(self.shape)))

    def rng(self, salt):
        return np.random.RandomState(zlib.crc32(("%s/%s" % (self.name, salt)).encode()) & 0x7FFFFFFF)


def _case(name, family, shape, axes, want=None, feature="", strides=None, offset=0, backing=None):
    shape = tuple(shape)
    strides = contiguous(shape) if strides is None else tuple(strides)
    if backing is None:
        backing = offset + (int(np.prod(shape, dtype=np.int64)) if shape else 1)
    axes = tuple(a % len(shape) for a in ((axes,) if isinstance(axes, int) else axes))
    return Case(name, family, shape, strides, offset, backing, axes, dict(want or {}), feature)


def _table():
    W, S, T, C = "rows_wave", "rows_split", "cols_tile", "cols"
    many = {"splits_gt": 1}
    t = [
        # ---- one wave per row: reducing the last axis ------------------------------------------------------------------
        _case("wave_1x1", W, (1, 1), 1, feature="one element"),
        _case("wave_5x1", W, (5, 1), 1, feature="rows of one element"),
        _case("wave_7x10", W, (7, 10), 1, {"vec": 1}, "aligned and unaligned rows alternate, 2-element tail"),
        _case("wave_3x63", W, (3, 63), 1, feature="one element short of a full wave of floats"),
        _case("wave_6x65", W, (6, 65), 1, feature="one float4 past 64 lanes' worth of scalars, odd pitch"),
        _case("wave_9x257", W, (9, 257), 1, feature="second trip of the float4 loop, 1-element tail"),
        _case("wave_2x8192", W, (2, 8192), 1, feature="the longest row that is not split when rows are few"),
        _case("wave_257x8195", W, (257, 8195), 1, feature="long rows, but many of them"),
        _case("wave_full_33x65", W, (33, 65), (0, 1), {"nr": 1}, "a full reduction: both axes collapse into one run"),
        _case("wave_transposed_50x300", W, (50, 300), 0, feature="reduced stride 1, rows 50 elements apart", strides=(1, 50)),
        _case("wave_9x257_base_off_3", W, (9, 257), 1, {"vec": 0}, "base pointer 12 bytes off alignment", offset=3),
        _case("wave_ndim0", W, (), (), {"nk": 1, "nr": 1}, "a 0-d tensor"),
        # ---- few long rows, split over workgroups -------------------------------------------------------------------------
        _case("split_1x8193", S, (1, 8193), 1, {"splits": 3, "groups": 1, "vec": 1}, "3 splits in one group"),
        _case("split_3x20001", S, (3, 20001), 1, {"splits": 5}, "rows 1 and 2 unaligned"),
        _case("split_255x8193", S, (255, 8193), 1, many, "the most rows the path takes: per-row tickets and partials"),
        _case("split_5x700000", S, (5, 700000), 1, {"splits": 154, "groups": 5, "splits_mod_32": 26}, "short last fold group"),
        _case("split_1x3200000", S, (1, 3200000), 1, {"splits": 768, "groups": 24, "splits_mod_32": 0}, "24 full fold groups"),
        _case("split_2x140000_view", S, (2, 140000), 1, dict(many, vec=0), "x[:, 1:]: row 0 unaligned, pitch differs from the row length",
              strides=(140001, 1), offset=1, backing=2 * 140001),
        # ---- 64-column tiles: reducing the leading axis -------------------------------------------------------------------
        _case("tile_64x64", T, (64, 64), 0, {"splits": 1}, "one chunk, one tile"),
        _case("tile_100x68", T, (100, 68), 0, feature="second tile with 4 live columns, row tail not a multiple of 16"),
        _case("tile_1000x192", T, (1000, 192), 0, {"splits": 13}, "13 chunks"),
        _case("tile_4100x512", T, (4100, 512), 0, {"splits": 16}, "16 chunks"),
        _case("tile_300x128_view", T, (300, 128), 0, many, "x[:, 4:132] of (300, 200): row pitch differs from the output count",
              strides=(200, 1), offset=4, backing=300 * 200),
        _case("tile_8x40x96", T, (8, 40, 96), (0, 1), dict(many, nr=1), "two reduced axes that collapse into one"),
        # ---- general kernel ---------------------------------------------------------------------------------------------------
        _case("cols_63x5", C, (63, 5), 0, {"splits": 1}, "no split"),
        _case("cols_200x8", C, (200, 8), 0, many, "fewer outputs than a tile"),
        _case("cols_1000x67", C, (1000, 67), 0, {"splits": 32}, "32 splits: four full trips of the fold"),
        _case("cols_650x10", C, (650, 10), 0, {"splits": 31}, "31 splits: the fold's scalar tail"),
        _case("cols_9000x10", C, (9000, 10), 0, {"splits": 64}, "64 splits"),
        _case("cols_40x33x50", C, (40, 33, 50), (0, 2), {"splits": 32, "nr": 2}, "odometer, 63-element chunks start and end mid-row"),
        _case("cols_6x5x7x4x9", C, (6, 5, 7, 4, 9), (0, 2, 4), dict(many, nk=2, nr=3), "three reduced dimensions"),
        _case("cols_7x100x9", C, (7, 100, 9), 1, dict(many, nk=2), "two kept dimensions"),
        _case("cols_300x64_base_off_1", C, (300, 64), 0, dict(many, vec=0), "a tile shape whose base is one element off alignment", offset=1),
        _case("cols_broadcast_rows", C, (300, 50), 0, many, "reducing a broadcast axis", strides=(0, 1), backing=50),
        _case("cols_broadcast_cols", C, (50, 300), 1, many, "reducing a broadcast trailing axis", strides=(1, 0), backing=50),
        _case("cols_8d", C, (2, 3) * 4, (1, 3, 5, 7), dict(many, nk=4, nr=4), "LG_MAX_DIMS dimensions, kept and reduced alternate"),
    ]
    return tuple(t)


CASES = _table()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# calls that launch nothing: (shape, axis) - n_out == 0, and a reduction over nothing
EMPTY_OUTPUT = ((0, 5), 1)
EMPTY_REDUCTION = ((4, 0), 1)


def family(name):
    return [c for c in CASES if c.family == name]


# ---- inputs (drawn once per case and kept: the tests share them and leave them unchanged) -------------------------------

@lru_cache(maxsize=None)
def exact_inputs(name):
    """(flat float32 array of nonzero integers, out0 of small integers, int64 sum over the view)"""
    c = BY_NAME[name]
    rng = c.rng("exact")
    v = rng.randint(1, c.vmax + 1, c.backing) * (2 * rng.randint(0, 2, c.backing) - 1)
    flat = v.astype(np.float32)
    out0 = rng.randint(-8, 9, c.kept_shape).astype(np.float32)
    ref = c.view(v.astype(np.int64)).sum(axis=c.axes, dtype=np.int64)
    for a in (flat, out0, ref):
        a.setflags(write=False)
    return flat, out0, ref


@lru_cache(maxsize=None)
def real_inputs(name):
    """(flat float32 array of uniform(0.25, 1), float64 sum, numpy's float32 sum, max, min over the view)"""
    c = BY_NAME[name]
    flat = c.rng("real").uniform(0.25, 1, c.backing).astype(np.float32)
    v = c.view(flat)
    out = (flat, v.sum(axis=c.axes, dtype=np.float64), v.sum(axis=c.axes, dtype=np.float32), v.max(axis=c.axes), v.min(axis=c.axes))
    for a in out:
        np.asarray(a).setflags(write=False)
    return out


def rel_frobenius(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300))


def sum_bound(name):
    """what a float32 sum of the case's real inputs may be away from float64: tests/common.py's rule"""
    _, ref64, np32, _, _ = real_inputs(name)
    return max(FLOOR, 2 * rel_frobenius(np32, ref64))


def boundary_positions(case, splits):
    """reduced positions at which one planted extremum tries every hand-over of a reduction cut into `splits` pieces: the
    ends of the run, both sides of the first and the last cut, and the last four elements (the scalar tail behind the
    float4 body).  The piece length follows from `splits` up to the kernels' rounding (to 4 rows_split, to 16 cols_tile,
    none red_cols): all three candidates are planted, which costs a few launches and needs no knowledge of who rounds how."""
    n = case.rlen
    pos = {0, n - 1, n - 2, n - 3, n - 4}
    if splits > 1:
        piece = -(-n // splits)
        for q in (1, 4, 16):
            seg = -(-piece // q) * q
            for cut in (seg, (splits - 1) * seg):
                pos.update((cut - 1, cut))
    return sorted(p for p in pos if 0 <= p < n)


def extremum_variants(name):
    """[(tag, flat array)] of the max / min edge inputs that need a whole array of their own: a row of ties, and one NaN in
    the tail of one row with +inf and -inf in another (apart when there is one row only)"""
    c = BY_NAME[name]
    base = real_inputs(name)[0]
    n_out, n = c.n_out, c.rlen
    out = []
    ties = base.copy()
    c.view(ties)[c.row(n_out // 2)] = 0.5
    out.append(("ties", ties))

    def poke(flat, o, what):
        if what == "nan":
            flat[c.element(o, n - 1)] = np.nan
        else:
            flat[c.element(o, n // 3)] = np.inf
            flat[c.element(o, (2 * n) // 3)] = -np.inf
    if n_out >= 2 and n >= 3:
        both = base.copy()
        poke(both, n_out - 1, "nan")
        poke(both, 0, "inf")
        out.append(("nan+inf", both))
    else:
        for what in ("nan", "inf"):
            if what == "inf" and n < 3:
                continue
            f = base.copy()
            poke(f, 0, what)
            out.append((what, f))
    return out
