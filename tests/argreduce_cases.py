"""The case table of the argmax / argmin sweep (tests/test_hip_argreduce.py) and its numpy references.  No GPU code here:
tests/test_argreduce_cases_cpu.py checks on the host what the GPU test relies on.

`lg_argreduce_f32` (csrc/argreduce.hip) picks one of three kernels after collapsing the view to [outer][axis][inner]:
arg_rows_wave (a wave per row), arg_rows_split (a workgroup per row segment, two-level ticket fold) and arg_cols (a thread per
output, the axis strided, split over blockIdx.y with a ticket fold).  Every case names the kernel it is MEANT to reach, and
where it matters whether the axis is split; the GPU test asserts that against `lg_argreduce_last_plan`, so a retuned threshold
that moves a case fails the test instead of silently emptying it.  The thresholds are not restated here.

A case builds the float32 array for ARGMAX; argmin runs on its negation (the extrema, ties, infinities and NaNs keep their
places).  `make()` returns {variant name: array}; an array may be a strided numpy view, which the GPU test turns into the same
view of device memory (`layout`).  `expect`, where given, is the answer the construction forces, for both ops.
"""
from collections import namedtuple
import numpy as np

ROWS_WAVE, ROWS_SPLIT, COLS, NONE = 0, 1, 2, -1
MAX_ELEMENTS = 4 << 20           # no case holds more

Case = namedtuple("Case", "name kernel axis make want expect keepdims")
CASES = []


def case(name, kernel, axis, make, want=None, expect=None, keepdims=False):
    CASES.append(Case(name, kernel, axis, make, want or {}, expect, keepdims))


def rng_of(name):
    import zlib
    return np.random.RandomState(zlib.crc32(name.encode()))


def distinct(rng, shape):
    """distinct values in [0, 1): a unique maximum and a unique minimum wherever they fall"""
    n = int(np.prod(shape))
    return (rng.permutation(n).astype(np.float32) / np.float32(n)).reshape(shape)


def layout(view):
    """(flat base array, shape, strides in elements, offset in elements) of a float32 numpy view"""
    base = view
    while base.base is not None:
        base = base.base
    base = base.reshape(-1) if base.flags["C_CONTIGUOUS"] else None
    assert base is not None and view.dtype == np.float32
    offset = (view.__array_interface__["data"][0] - base.__array_interface__["data"][0]) // 4
    return base, tuple(view.shape), tuple(s // 4 for s in view.strides), offset


def reference(op, view, axis, keepdims=False):
    """numpy's answer for the case's array (`op` "argmax") or its negation ("argmin"), as int64"""
    a = view if op == "argmax" else -view
    return np.asarray(getattr(np, op)(a, axis=axis, keepdims=keepdims), dtype=np.int64)


# ---- every position: a unique extremum on the diagonal of distinct background values ----------------------------------------------
def _diagonal():
    a = distinct(rng_of("diagonal"), (200, 200))
    a[np.arange(200), np.arange(200)] = 2.0
    return a


case("diag_axis1", ROWS_WAVE, 1, lambda: {"dense": _diagonal()}, expect=np.arange(200))
case("diag_axis0", COLS, 0, lambda: {"dense": _diagonal()}, expect=np.arange(200), want={"splits_gt": 1})
case("diag_T_axis1", COLS, 1, lambda: {"view": _diagonal().T}, expect=np.arange(200))          # the axis strided, the outputs contiguous
case("diag_T_axis0", ROWS_WAVE, 0, lambda: {"view": _diagonal().T}, expect=np.arange(200))      # rows numbered by the trailing dimension


# ---- the lowest index among ties ---------------------------------------------------------------------------------------------------
def _staircase():
    """row r holds the extremum at every position >= r: the ties straddle lanes and the lane + 64 k wrap"""
    a = distinct(rng_of("staircase"), (300, 300))
    a[np.arange(300)[None, :] >= np.arange(300)[:, None]] = 2.0
    return a


def _zeros_mix(shape):
    a = np.zeros(shape, np.float32)
    a[rng_of("zeros").randint(0, 2, shape) == 1] = -0.0
    return a


case("ties_rows", ROWS_WAVE, 1, lambda: {"staircase": _staircase()}, expect=np.arange(300))
case("ties_cols", COLS, 0, lambda: {"staircase": np.ascontiguousarray(_staircase().T)}, expect=np.arange(300), want={"splits_gt": 1})
case("equal_rows", ROWS_WAVE, 1, lambda: {"ones": np.ones((7, 300), np.float32), "zeros": _zeros_mix((7, 300))}, expect=np.zeros(7))
case("equal_cols", COLS, 0, lambda: {"ones": np.ones((300, 7), np.float32), "zeros": _zeros_mix((300, 7))}, expect=np.zeros(7),
     want={"splits_gt": 1})


# ---- infinities and NaN ----------------------------------------------------------------------------------------------------------------
NAN_WIDTH = 130
NAN_AT = [(0,), (63,), (64,), (NAN_WIDTH - 1,), (10, 70), (64, 65), (3, NAN_WIDTH - 1)]      # one NaN, then two: the first wins


def _constant_rows():
    a = np.empty((3, NAN_WIDTH), np.float32)
    a[0], a[1], a[2] = -np.inf, np.inf, np.nan
    return a


def _nan_rows():
    """row k: NaN at NAN_AT[k], a larger finite value in front of the first and +inf behind it"""
    a = distinct(rng_of("nan"), (len(NAN_AT), NAN_WIDTH))
    for k, at in enumerate(NAN_AT):
        first = at[0]
        if first > 0:
            a[k, first - 1] = 1e30
        if first + 1 < NAN_WIDTH:
            a[k, first + 1] = np.inf
        a[k, list(at)] = np.nan
    return a


NAN_EXPECT = np.array([at[0] for at in NAN_AT])
case("constant_rows", ROWS_WAVE, 1, lambda: {"inf_nan": _constant_rows()}, expect=np.zeros(3))
case("constant_cols", COLS, 0, lambda: {"inf_nan": np.ascontiguousarray(_constant_rows().T)}, expect=np.zeros(3), want={"splits_gt": 1})
case("nan_rows", ROWS_WAVE, 1, lambda: {"nan": _nan_rows()}, expect=NAN_EXPECT)
case("nan_cols", COLS, 0, lambda: {"nan": np.ascontiguousarray(_nan_rows().T)}, expect=NAN_EXPECT, want={"splits_gt": 1})


# ---- the rows kernels at their edges ---------------------------------------------------------------------------------------------
def _row_variants(name, rows, width, offset=0):
    """distinct values; the extremum where it falls, in the last element of every row, in the first"""
    def make():
        rng = rng_of(name)
        flat = np.empty(rows * width + offset, np.float32)
        flat[:] = distinct(rng, flat.shape)
        out = {}
        for tag, at in (("random", None), ("last", width - 1), ("first", 0)):
            f = flat.copy()
            v = f[offset:].reshape(rows, width)
            if at is not None:
                v[:, at] = 2.0
            out[tag] = v
        return out
    return make


for _w in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023):
    for _r in (1, 4, 5, 257):
        _n = "rows_%dx%d" % (_r, _w)
        # a single element per row is no walk along a row: the thread-per-output kernel answers 0
        case(_n, COLS if _w == 1 else ROWS_WAVE, 1, _row_variants(_n, _r, _w), want={"vec": 1} if _w >= 7 else {})
for _w in (4097, 8191, 8192):                            # eight loads in flight, the next eight issued ahead: several rounds per lane
    _n = "rows_5x%d" % _w
    case(_n, ROWS_WAVE, 1, _row_variants(_n, 5, _w), want={"vec": 1})
case("rows_5x30522", ROWS_SPLIT, 1, _row_variants("rows_5x30522", 5, 30522), want={"splits_gt": 1, "vec": 1})   # vocabulary rows, few of them
case("rows_3x20001", ROWS_SPLIT, 1, _row_variants("rows_3x20001", 3, 20001), want={"splits_gt": 1})
case("rows_2x8193", ROWS_SPLIT, 1, _row_variants("rows_2x8193", 2, 8193), want={"splits_gt": 1})
for _r, _w in ((5, 257), (5, 4097), (3, 20001)):         # the base one element off 16-byte alignment: flat[1:] reshaped
    _n = "offset_%dx%d" % (_r, _w)
    case(_n, ROWS_SPLIT if _w > 8192 else ROWS_WAVE, 1, _row_variants(_n, _r, _w, offset=1), want={"vec": 1})
case("rows_last_axis_of_3d", ROWS_WAVE, -1, lambda: {"dense": distinct(rng_of("3d"), (6, 7, 70))}, want={"merged": 1})
case("rows_keepdims", ROWS_WAVE, 1, lambda: {"dense": distinct(rng_of("keep"), (9, 33))}, keepdims=True)

# ---- the whole tensor: one long row, split over workgroups -----------------------------------------------------------------------
SPLIT_ALL = (1000, 1003)                                 # dense, axis=None: 1 003 000 elements in a few hundred segments, the last ragged
case("all_split", ROWS_SPLIT, None, lambda: {"dense": distinct(rng_of("all"), SPLIT_ALL)}, want={"splits_gt": 32})
case("all_small", ROWS_WAVE, None, lambda: {"dense": distinct(rng_of("small"), (37, 41))})
case("all_keepdims", ROWS_WAVE, None, lambda: {"dense": distinct(rng_of("allkeep"), (5, 6, 7))}, keepdims=True)
case("all_0d", COLS, None, lambda: {"scalar": np.full((), 3.5, np.float32)}, expect=np.zeros(()))


# ---- the columns kernel ------------------------------------------------------------------------------------------------------------
def _col_variants(name, shape, axis):
    def make():
        a = distinct(rng_of(name), shape)
        first, last = a.copy(), a.copy()
        idx = [slice(None)] * len(shape)
        idx[axis] = 0
        first[tuple(idx)] = 2.0
        idx[axis] = shape[axis] - 1
        last[tuple(idx)] = 2.0
        return {"random": a, "first": first, "last": last}
    return make


for _rlen in (1, 2, 63, 64, 65):
    for _n_out in (1, 255, 256, 257):
        _n = "cols_%dx%d" % (_rlen, _n_out)
        _k = ROWS_WAVE if (_n_out == 1 and _rlen > 1) else COLS          # one column of a dense matrix is a contiguous run
        case(_n, _k, 0, _col_variants(_n, (_rlen, _n_out), 0), want={"splits_gt": 1} if (_k == COLS and _rlen >= 64) else ({"splits": 1}))


def _split_ties():
    """every column holds its extremum twice, in two different chunks of a split axis: the lower row wins, whichever
    workgroup arrives last"""
    a = distinct(rng_of("split_ties"), (4096, 70))
    lo = np.arange(70) * 7 + 5
    a[lo, np.arange(70)] = 2.0
    a[lo + 2000, np.arange(70)] = 2.0
    return a


case("cols_split_ties", COLS, 0, lambda: {"two": _split_ties()}, want={"splits_gt": 1, "merged": 1}, expect=np.arange(70) * 7 + 5)
case("cols_split_equal", COLS, 0, lambda: {"equal": np.full((4096, 70), 0.5, np.float32)}, want={"splits_gt": 1}, expect=np.zeros(70))
case("cols_middle_3x5x7", COLS, 1, _col_variants("m357", (3, 5, 7), 1), want={"merged": 0, "splits": 1})
case("cols_middle_2x130x33", COLS, 1, _col_variants("m213033", (2, 130, 33), 1), want={"merged": 0, "splits_gt": 1})
case("cols_negative_axis", COLS, -2, _col_variants("neg", (4, 9, 35), 1), want={"merged": 0})
case("cols_keepdims", COLS, 0, _col_variants("ckeep", (20, 50), 0), keepdims=True)
case("cols_reversed_axis", COLS, 1, lambda: {"view": distinct(rng_of("rev"), (6, 90))[:, ::-1]})      # a negative stride along the axis

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)

# views whose leading / trailing dimensions do not merge into one stride: the C ABI refuses them, the tensor layer copies them first
def uncollapsible():
    a = distinct(rng_of("uncollapsible"), (6, 10, 12))
    return [(a[:, ::3, :], 2), (a[:, :, ::5], 0), (a[:, ::3, ::2], None), (a.transpose(2, 0, 1)[:, ::2], None)]


EMPTY_REDUCTION = [((0,), None), ((0,), 0), ((3, 0), 1), ((0, 3), 0), ((0, 0), 1), ((2, 0, 4), None)]      # ValueError
EMPTY_OUTPUT = [((0, 3), 1), ((3, 0, 4), 2), ((2, 0), 0)]                                                   # an empty int64 result
