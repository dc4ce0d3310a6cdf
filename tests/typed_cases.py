"""The case table of the typed sweep (the sweep tests at the end of tests/test_hip_typed.py): elementwise arithmetic, casts and
reductions of int16 / int32 / int64 / float64 tensors - csrc/typed.hip - with numpy on the same arrays as the reference.  No GPU
code here: tests/test_layout_index_typed_cases_cpu.py checks on the host what the GPU test relies on.

The cases are programs for a backend, as in tests/layout_cases.py; `B.force(x, value)` besides states an answer the construction
of the input forces (a planted extremum, a planted NaN), which every backend - numpy first - must give.

Comparison is bit for bit (the sign of a zero counts) with one canonicalisation: any NaN equals any NaN.  IEEE 754 leaves the
sign and the payload of a NaN result open, and processors differ (inf - inf); which NaN goes IN is data and is covered by the
layout sweep.  Two groups of float64 results are sums in an order the kernel chooses and are held to a derived bound instead
(`Case.compare`); max / min results are compared as values, so that the sign of a zero extremum - which depends on the order of
combination in numpy as well - does not count.

`A - B` and `A / B` as python operators are the composites `A + (-B)` and `A * B ** -1` on every backend (autograd/ops.py); the
first-class kernels are reached through `.sub()` / `.div()`, the reflected `5 - A` and the in-place forms, which the table uses.
"""
from collections import namedtuple
import math
import numpy as np
from layout_cases import rng_of, same_bytes, sentinel, NumpyBackend, _five_dims      # noqa: F401

MAX_ELEMENTS = 4 << 20
TYPED = tuple(np.dtype(d) for d in (np.int16, np.int32, np.int64, np.float64))
CASTABLE = TYPED + (np.dtype(np.float32),)

Case = namedtuple("Case", "name run compare")
CASES = []


def case(name, run, compare=None):
    CASES.append(Case(name, run, compare))


def canonical(x):
    """x with every NaN replaced by the one default NaN"""
    x = np.array(x, copy=True)
    if x.dtype.kind == "f":
        x[np.isnan(x)] = np.nan
    return x


def same_bits(got, want, what):
    same_bytes([canonical(g) for g in got], [canonical(w) for w in want], what)


def compare_bits(got, want):
    same_bits(got[0], want[0], "values")
    same_bits(got[1], want[1], "base arrays")


def compare_values(got, want):
    """max / min: equal as values (NaN where numpy has NaN); the base arrays untouched"""
    assert len(got[0]) == len(want[0])
    for g, w in zip(got[0], want[0]):
        assert g.dtype == w.dtype and g.shape == w.shape, (g.dtype, g.shape, w.dtype, w.shape)
        np.testing.assert_array_equal(g, w)
    same_bits(got[1], want[1], "base arrays")


def sub(x, y):
    return x.sub(y) if hasattr(x, "sub") else x - y


def div(x, y):
    return x.div(y) if hasattr(x, "div") else x / y


# ---- elementwise ---------------------------------------------------------------------------------------------------------------------
def edge_pool(dtype):
    dtype = np.dtype(dtype)
    if dtype.kind == "i":
        lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
        return np.array([lo, lo + 1, lo + 2, hi, hi - 1, hi - 2, -1, 0, 1, 2, -2, 3, lo // 2, hi // 2 + 1, lo // 2 - 1, hi // 2], dtype)
    eps = 2.0 ** -52
    return np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308,
                     1e-310, 2.225073858507201e-308, 1.0, -1.0, 1 + eps, 1 - eps, 1 - eps / 2, 1 + 2 * eps, 1 + 3 * eps, 1.5, 3.0,
                     1.0 / 3, 1.7976931348623157e308, -1.7976931348623157e308, 1e200, 1e-200, 0.1, 7.0], dtype)


def operands(name, shape, dtype):
    """half of the entries from the pool of edge values - so that pairs of them meet -, half anywhere in the type's range"""
    dtype = np.dtype(dtype)
    rng = rng_of(name)
    n = int(np.prod(shape, dtype=np.int64))
    if dtype.kind == "i":
        anywhere = rng.randint(0, 256, n * dtype.itemsize).astype(np.uint8).view(dtype).copy()
    else:
        anywhere = rng.standard_normal(n) * 10.0 ** rng.randint(-5, 6, n)
    pool = edge_pool(dtype)
    out = np.where(rng.randint(0, 2, n) == 1, pool[rng.randint(0, len(pool), n)], anywhere).astype(dtype)
    return out.reshape(shape)


def near_ties():
    """(1 + j 2^-52) and (1 + k 2^-52) for small j, k, in the binades below and above one: quotients and products whose exact
    value lies next to a rounding tie"""
    eps = 2.0 ** -52
    j = np.arange(-6, 7, dtype=np.float64)
    x = np.where(j < 0, 1 + j * eps / 2, 1 + j * eps)
    return np.ascontiguousarray(np.broadcast_to(x[:, None], (13, 13))), np.ascontiguousarray(np.broadcast_to(x[None, :], (13, 13)))


def _binary_forms(dtype):
    f64 = np.dtype(dtype) == np.float64
    forms = [lambda x, y: x + y, lambda x, y: x - y, sub, lambda x, y: x * y]
    return forms + [div] if f64 else forms


def _scalars(dtype):
    """python scalar operands, in the type's range"""
    if np.dtype(dtype) == np.float64:
        return [lambda x: x + 0.5, lambda x: 5 - x, lambda x: x * -1.0, lambda x: sub(x, 7.0), lambda x: div(x, 3.0), lambda x: 2.5 * x,
                lambda x: x + 3]
    hi = int(np.iinfo(dtype).max)
    return [lambda x: x + 3, lambda x: 5 - x, lambda x: x * -1, lambda x: sub(x, 7), lambda x: 5 * x, lambda x: x + hi, lambda x: x * hi,
            lambda x: sub(x, hi), lambda x: x * 2]


def _elementwise(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        with np.errstate(all="ignore"):
            out = []
            a, b = operands("ew_a_%s" % dtype, (7, 9), dtype), operands("ew_b_%s" % dtype, (7, 9), dtype)
            row, col = operands("ew_row_%s" % dtype, (9,), dtype), operands("ew_col_%s" % dtype, (7, 1), dtype)
            pairs = [(a, b)]
            if dtype.kind == "f":
                pairs.append(near_ties())
                pool = edge_pool(dtype)                                     # every edge value against every other
                pairs.append((np.ascontiguousarray(np.broadcast_to(pool[:, None], (len(pool),) * 2)),
                              np.ascontiguousarray(np.broadcast_to(pool[None, :], (len(pool),) * 2))))
            else:
                pool = edge_pool(dtype)
                pairs.append((np.ascontiguousarray(np.broadcast_to(pool[:, None], (len(pool),) * 2)),
                              np.ascontiguousarray(np.broadcast_to(pool[None, :], (len(pool),) * 2))))
            for x, y in pairs:
                X, Y = B.t(x), B.t(y)
                out.append(-X)
                for f in _binary_forms(dtype):
                    out.append(f(X, Y))
                for f in _scalars(dtype):
                    out.append(f(X))
            A, Bt = B.t(a), B.t(b)
            for f in _binary_forms(dtype):
                out.append(f(A, B.t(row)))                                  # a row and a column broadcast
                out.append(f(A, B.t(col)))
                out.append(f(B.t(col), B.t(row)))
                out.append(f(A.transpose(1, 0), Bt.transpose(1, 0)))        # both operands transposed
                out.append(f(B.t(a.T), B.t(np.ascontiguousarray(b.T))))
                out.append(f(B.t(a[::-1, ::-2]), B.t(b[:, ::2][:, ::-1])))     # negative steps
                out.append(f(B.t(a[::-1, ::-2]), B.t(row[::2])))
            big, other = operands("ew_five_a_%s" % dtype, (275,), dtype), operands("ew_five_b_%s" % dtype, (275,), dtype)
            for f in _binary_forms(dtype):
                out.append(f(B.t(_five_dims(big)), B.t(_five_dims(other))))      # five dimensions, none merges with a neighbour
                out.append(f(B.t(_five_dims(big)), B.t(np.ascontiguousarray(_five_dims(other)))))
            out.append(-B.t(_five_dims(big)))
            out.append(-B.t(a[::-1, ::-2]))
            out.append(-B.t(a.T))
            s0, s1 = B.t(a[3:4, 2:3].reshape(())), B.t(b[1:2, 4:5].reshape(()))      # 0-d
            out += [-s0, s0 + s1, sub(s0, s1), s0 * s1, 5 - s0, s0 + A]
            e = B.t(np.zeros((0, 4), dtype))                                          # no elements
            out += [-e, e + e, sub(e, e), e * 3, e + B.t(np.zeros((1, 4), dtype)), B.t(np.zeros((3, 0, 2), dtype)) * B.t(np.zeros((2,), dtype))]
            return out
    return run


def _inplace(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        with np.errstate(all="ignore"):
            big = operands("inplace_big_%s" % dtype, (9, 14), dtype)
            upd, row, col = (operands("inplace_%s_%s" % (tag, dtype), shape, dtype) for tag, shape in (("b", (7, 7)), ("row", (7,)), ("col", (7, 1))))
            for other in (upd, row, col, upd.T, upd[::-1, ::-1], None):
                v = B.t(big[1:-1, ::2])                                     # a view that is not dense: the whole base is compared
                v += B.t(other) if other is not None else 3
                v = B.t(big[1:-1, ::2])
                v -= B.t(other) if other is not None else 7
                v = B.t(big[1:-1, ::2])
                v *= B.t(other) if other is not None else (2.5 if dtype.kind == "f" else -1)
            v = B.t(big.T[::-2, 1:8])                                       # transposed, a negative step
            v += B.t(upd)
            v *= v
            v -= v
            v = B.t(_five_dims(sentinel("inplace_five_%s" % dtype, 275, dtype)))
            v += B.t(np.ascontiguousarray(_five_dims(operands("inplace_five_b_%s" % dtype, (275,), dtype))))
            v *= 3
            # through __setitem__ as python spells it: take, operate, put back
            t = B.t(big)
            t[1:-1, ::2] += B.t(upd)
            t[::3, 1] -= 7
            # operands that overlap the output
            t = B.t(operands("inplace_square_%s" % dtype, (65, 65), dtype))
            t += t.transpose(1, 0)
            t *= t
            d, s = B.views(big[:, 1:], big[:, :-1])
            d += s
            d, s = B.views(big[::-1], big)
            d -= s
            if dtype.kind == "f":
                v = B.t(big[1:-1, ::2])
                v /= B.t(upd)
    return run


for _d in TYPED:
    case("elementwise_%s" % _d, _elementwise(_d), compare_bits)
    case("inplace_%s" % _d, _inplace(_d), compare_bits)


# ---- casts: all 25 pairs ----------------------------------------------------------------------------------------------------------------
def cast_values(src, dst):
    """48 values of `src`: the ones planted for this pair, the rest anywhere `dst` defines a result for"""
    src, dst = np.dtype(src), np.dtype(dst)
    rng = rng_of("cast_%s_%s" % (src, dst))
    planted = []
    if src.kind == "i":
        info = np.iinfo(src)
        planted = [2 ** 24 - 1, 2 ** 24 + 1, 2 ** 24 + 3, -(2 ** 24 + 1), 2 ** 53 + 2 ** 29 + 1, -(2 ** 53 + 2 ** 29 + 1), 2 ** 62 + 2 ** 38 + 1,
                   2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 31 - 1, 2 ** 31 - 65, 2 ** 63 - 1, 2 ** 63 - 513, -2 ** 63, info.min, info.max,
                   32767, -32768, 32768, 65535, 65536, 2 ** 31, 2 ** 32 - 1, 2 ** 32, -1, 0, 1]
        planted = [v for v in planted if info.min <= v <= info.max]
        anywhere = rng.randint(0, 256, 48 * src.itemsize).astype(np.uint8).view(src).copy()
    elif dst.kind == "i":
        # float -> integer: in range only (numpy truncates toward zero; NaN and out-of-range values are undefined there too)
        digits = 24 if src == np.float32 else 53
        top = min(np.iinfo(dst).bits - 2, digits - 1)
        planted = [0.5, -0.5, 1.0 - 2.0 ** -digits, -(1.0 - 2.0 ** -digits), 1.5, -1.5, 2.5, -2.5, 0.0, -0.0, 1.0, -1.0]
        for k in sorted({1, 2, 7, 14, min(23, top), min(30, top), top}):
            planted += [2.0 ** k - 0.5, -(2.0 ** k - 0.5), 2.0 ** k]
        anywhere = rng.uniform(-2.0 ** top, 2.0 ** top, 48)
    elif src == np.float64 and dst == np.float32:
        big = float(np.finfo(np.float32).max)
        planted = [1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 - 2.0 ** -25, 1 - 3 * 2.0 ** -25, 1 + 2.0 ** -24 + 2.0 ** -50, 1 + 2.0 ** -24 - 2.0 ** -50,
                   big, big + 2.0 ** 102, big + 2.0 ** 103, big + 2.0 ** 103 - 2.0 ** 60, -(big + 2.0 ** 103), 1e39, -1e39, np.inf, -np.inf,   # to inf
                   1e-40, -1e-40, 2.0 ** -149, 2.0 ** -150, 2.0 ** -150 * 1.5, 2.0 ** -149 * 1.5, 2.0 ** -149 * 2.5, 2.0 ** -151,        # subnormal
                   2.0 ** -126, 2.0 ** -126 - 2.0 ** -150, 2.0 ** -126 - 2.0 ** -151, 0.0, -0.0, 5e-324, -5e-324]
        anywhere = rng.standard_normal(48) * 10.0 ** rng.randint(-30, 30, 48)
    else:                                                     # float32 -> float64 is exact; a dtype to itself is a copy
        planted = [0.0, -0.0, np.inf, -np.inf, 1e-40, -1e-45, 3.4028235e38, 1 + 2.0 ** -23, 2.0 ** -126, 1.0 / 3]
        anywhere = rng.standard_normal(48) * 10.0 ** rng.randint(-30, 30, 48)
    with np.errstate(all="ignore"):
        out = np.array(anywhere, dtype=src)
        assert len(planted) <= 48
        out[:len(planted)] = np.array(planted, dtype=np.float64 if src.kind == "f" else src).astype(src)
    return out.reshape(6, 8)


def _casts(src):
    src = np.dtype(src)

    def run(B):
        out = []
        with np.errstate(all="ignore"):
            for dst in CASTABLE:
                x = cast_values(src, dst)
                out.append(B.t(x).astype(dst))
                out.append(B.t(x.T).astype(dst))                             # transposed
                out.append(B.t(x[::-1, ::-2]).astype(dst))                   # negative steps
                out.append(B.t(x[2:3, 5:6].reshape(())).astype(dst))
                out.append(B.t(np.zeros((0, 3), src)).astype(dst))
        return out
    return run


for _d in CASTABLE:
    case("cast_from_%s" % _d, _casts(_d), compare_bits)


# ---- reductions --------------------------------------------------------------------------------------------------------------------------
RED_LENGTHS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 4097)
RED_TREE = 256                                       # threads of the workgroup that reduces one output


def plant_positions(rlen):
    """reduction positions the workgroup treats differently: the first two, the last live slot of its tree, the last of the first
    trip, the first of the second trip (thread 0 again), the last element"""
    live = min(rlen, RED_TREE)
    return sorted(p for p in {0, 1, live - 1, RED_TREE - 1, RED_TREE, rlen - 1} if 0 <= p < rlen)


def factors(rlen):
    """rlen = r1 * r2 with the smallest r1 >= 2 there is (a prime: r2 = 1)"""
    for r1 in range(2, int(math.isqrt(rlen)) + 1):
        if rlen % r1 == 0:
            return r1, rlen // r1
    return rlen, 1


def background(name, rows, rlen, dtype):
    """distinct values in every row, centred on zero (they fit int16 for every length of the sweep)"""
    rng = rng_of(name)
    x = np.stack([rng.permutation(rlen) for _ in range(rows)]) - rlen // 2
    return (x + 0.25).astype(dtype) if np.dtype(dtype).kind == "f" else x.astype(dtype)


def extreme(dtype, op):
    dtype = np.dtype(dtype)
    if dtype.kind == "f":
        return dtype.type(1e300 if op == "max" else -1e300)
    return dtype.type(np.iinfo(dtype).max if op == "max" else np.iinfo(dtype).min)


def reduce_forms(B, x, op, force=None):
    """x [rows][rlen], each row reduced: along the last axis, along the first axis (strided) of a dense and of a transposed tensor,
    over two non-adjacent axes of a 4-D tensor, with keepdims, and over all axes of the row as 1-D and 2-D tensors"""
    rows, rlen = x.shape
    r1, r2 = factors(rlen)
    out = []
    f = lambda y: (B.force(y, force) if force is not None else y)      # noqa: E731
    out.append(f(getattr(B.t(x), op)(axis=1)))
    out.append(f(getattr(B.t(x), op)(axis=-1, keepdims=True)))
    out.append(f(getattr(B.t(np.ascontiguousarray(x.T)), op)(axis=0)))
    out.append(f(getattr(B.t(x.T), op)(axis=0, keepdims=True)))
    four = np.empty((r1, rows, r2, 2), x.dtype)
    four[..., 0] = x.reshape(rows, r1, r2).transpose(1, 0, 2)
    four[..., 1] = x[::-1].reshape(rows, r1, r2).transpose(1, 0, 2)
    out.append(f(getattr(B.t(four), op)(axis=(0, 2))))
    out.append(f(getattr(B.t(four), op)(axis=(0, 2), keepdims=True)))
    for r in range(rows):
        out.append(f(getattr(B.t(x[r]), op)()))
        out.append(f(getattr(B.t(x[r].reshape(r1, r2)), op)(axis=None, keepdims=True)))
        out.append(f(getattr(B.t(x[r].reshape(r1, r2).T), op)()))
    return out


def _extrema(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        out = []
        for rlen in RED_LENGTHS:
            at = plant_positions(rlen)
            for op in ("max", "min"):
                x = background("extrema_%s_%d" % (dtype, rlen), len(at), rlen, dtype)
                out += reduce_forms(B, x, op)                                # the extremum where it falls
                x[np.arange(len(at)), at] = extreme(dtype, op)               # row r: the unique extremum at position at[r]
                out += reduce_forms(B, x, op, force=extreme(dtype, op))
                if dtype.kind == "f":
                    x[np.arange(len(at)), at] = np.nan                       # row r: one NaN at position at[r]
                    out += reduce_forms(B, x, op, force=np.nan)
        # step-sliced and transposed inputs, kept and reduced axes mixed
        a = background("extrema_views_%s" % dtype, 12, 70, dtype).reshape(4, 3, 70)
        for op in ("max", "min"):
            for view in (a[:, :, ::3], a[::-1, :, 5:60:2], a.transpose(2, 0, 1), a.transpose(1, 2, 0)[:, ::-7]):
                for axis in (0, 1, 2, (0, 1), (0, 2), (1, 2), None):
                    out.append(getattr(B.t(view), op)(axis=axis))
            out.append(getattr(B.t(np.zeros((0, 4), dtype)), op)(axis=1))    # no outputs
            out.append(getattr(B.t(np.zeros((3, 0, 4), dtype)), op)(axis=2, keepdims=True))
        return out
    return run


def _sums(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        out = []
        with np.errstate(all="ignore"):
            for rlen in RED_LENGTHS:
                x = background("sums_%s_%d" % (dtype, rlen), 3, rlen, dtype)         # integers (float64: n + 0.25), exact in any order
                out += reduce_forms(B, x, "sum")
                if dtype.kind == "i":
                    info = np.iinfo(dtype)
                    x[0], x[1] = info.max, info.min                                    # rows that overflow their own type ...
                    x[2] = np.where(np.arange(rlen) % 3 == 0, info.min, info.max)     # ... int64 rows wrap, as numpy's do
                    out += reduce_forms(B, x, "sum")
                else:
                    x = rng_of("sums_big_%d" % rlen).randint(-2 ** 40, 2 ** 40, (3, rlen)).astype(dtype)      # sums below 2^53
                    out += reduce_forms(B, x, "sum")
            a = background("sums_views_%s" % dtype, 12, 70, dtype).reshape(4, 3, 70)
            for view in (a[:, :, ::3], a[::-1, :, 5:60:2], a.transpose(2, 0, 1), a.transpose(1, 2, 0)[:, ::-7]):
                for axis in (0, 1, 2, (0, 1), (0, 2), (1, 2), None):
                    out.append(B.t(view).sum(axis=axis))
                    out.append(B.t(view).sum(axis=axis, keepdims=True))
            # sums of nothing, and no outputs
            for shape, axis in (((3, 0), 1), ((3, 0), None), ((0,), 0), ((0,), None), ((2, 0, 4), (1,)), ((2, 0, 4), (0, 1)), ((0, 4), 1),
                                ((3, 0, 4), 2), ((0, 0), 0)):
                out.append(B.t(np.zeros(shape, dtype)).sum(axis=axis))
                out.append(B.t(np.zeros(shape, dtype)).sum(axis=axis, keepdims=True))
        return out
    return run


for _d in TYPED:
    case("extrema_%s" % _d, _extrema(_d), compare_values)
    case("sums_%s" % _d, _sums(_d), compare_bits)


# ---- float64 sums of general values: an order the kernel chooses ------------------------------------------------------------------------
def general_sum_data():
    out = []
    for rlen in RED_LENGTHS:
        rng = rng_of("sums_general_%d" % rlen)
        out.append(rng.standard_normal((3, rlen)) * 10.0 ** rng.randint(-3, 4, (3, rlen)))
    return out


def _sums_general(B):
    out = []
    for x in general_sum_data():
        out += reduce_forms(B, x, "sum")
    return out


def sum_bound(row):
    """(math.fsum of the row, gamma(n - 1) * sum |x|), gamma(k) = k u / (1 - k u), u = 2^-53: valid for any order of summation"""
    n, u = len(row), 2.0 ** -53
    return math.fsum(row), (n - 1) * u / (1 - (n - 1) * u) * math.fsum(abs(v) for v in row)


def check_sums_general(got, want):
    got, k = got[0], 0
    for x in general_sum_data():
        rows = x.shape[0]
        ref = np.array([sum_bound(r)[0] for r in x])
        bound = np.array([sum_bound(r)[1] for r in x])
        forms = [(ref, bound)] * 4 + [(np.stack([ref, ref[::-1]], axis=1), np.stack([bound, bound[::-1]], axis=1))] * 2
        for r in range(rows):
            forms += [(ref[r], bound[r])] * 3
        for ref_k, bound_k in forms:
            g = got[k]
            assert g.dtype == np.float64 and g.size == np.size(ref_k), (k, g.shape)
            err = np.abs(g.reshape(np.shape(ref_k)) - ref_k)
            assert (err <= bound_k).all(), (k, x.shape, float(np.max(err)), float(np.max(bound_k)))
            k += 1
    assert k == len(got)
    assert [g.shape for g in got] == [w.shape for w in want[0]]


case("sums_general_float64", _sums_general, check_sums_general)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
