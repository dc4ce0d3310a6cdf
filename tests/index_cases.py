"""The case table of the index sweep (the sweep tests at the end of tests/test_hip_index.py): integer-array indexing along one
axis, the paired form `t[range(n), labels]`, assignment, the scatter-add of the backward pass, several index arrays folded into
one, and boolean masks - csrc/index.hip - with numpy on the same arrays as the reference.  No GPU code here:
tests/test_layout_index_typed_cases_cpu.py checks on the host what the GPU test relies on.

The cases are programs for a backend, as in tests/layout_cases.py.  The index sweep asks three more things of it:

    B.idx(array, how)           an index array as the backend takes it: how = "host" (an int64 ndarray), "list", or np.int16 /
                                np.int32 / np.int64 for a tensor of that dtype (a device tensor on HipTensor); a strided numpy
                                view of the right dtype becomes the same strided view of device memory
    B.mask(array)               a boolean mask as a tensor (a device tensor on HipTensor)
    B.take_grad(a, index, w)    the gradient of sum(t[index] * w) with respect to t = a: w scattered into zeros, repeated
                                positions ADD (np.add.at)
    B.note_put(positions)       the flat positions an assignment names (host bookkeeping: the CPU test proves that no assignment
                                but `put_repeats` names a position twice)

Everything is compared with numpy bit for bit, with two exceptions that the cases name themselves (`Case.compare`): the one
assignment with repeated indices, where any of the values written to a position may stay, and scatter-adds of general float32
values, which are sums in an unspecified order and are held to the recursive-summation bound against a float64 np.add.at.
"""
from collections import namedtuple
import numpy as np
from layout_cases import rng_of, values, sentinel, same_bytes, NumpyBackend      # noqa: F401

MAX_ELEMENTS = 4 << 20
SOURCE_DTYPES = tuple(np.dtype(d) for d in (np.uint8, np.int16, np.float32, np.float64))      # one per item size
DEVICE_INDEX = (np.int16, np.int32, np.int64)
INDEX_KINDS = ("host",) + DEVICE_INDEX

Case = namedtuple("Case", "name run compare")
CASES = []


def case(name, run, compare=None):
    CASES.append(Case(name, run, compare))


def _scalar(dtype, k=0):
    dtype = np.dtype(dtype)
    return dtype.type([0x5A, -0.0, 3.25, 0xA5][k]) if dtype.kind == "f" else dtype.type([0x5A, 0x33, 7, 0][k])


# ---- one index array along an axis: [outer][axis][inner] ----------------------------------------------------------------------------
OUTERS, INNERS, AXIS_LEN = (1, 3), (1, 7, 64, 65), 11


def index_patterns(name, axis_len):
    rng = rng_of("patterns_" + name)
    yield "repeats", rng.randint(-axis_len, axis_len, 9)
    yield "all_negative", rng.randint(-axis_len, 0, 6)
    yield "all_lowest", np.full(5, -axis_len)
    yield "all_highest", np.full(5, axis_len - 1)
    yield "shape_2x3x2", rng.randint(-axis_len, axis_len, (2, 3, 2))
    yield "0d", np.array(axis_len - 1)
    yield "0d_negative", np.array(-axis_len)
    yield "empty", np.zeros(0, np.int64)


def _take_plain(dtype):
    def run(B):
        out = []
        for outer in OUTERS:
            for inner in INNERS:
                name = "take_%s_%d_%d" % (dtype, outer, inner)
                t = B.t(values(name, (outer, AXIS_LEN, inner), dtype))
                for how in INDEX_KINDS:
                    for tag, i in index_patterns(name, AXIS_LEN):
                        out.append(t[:, B.idx(i, how)])
                out.append(t[:, B.idx(list(range(AXIS_LEN - 1, -1, -2)), "list")])
        # the axis first (inner > 1, outer == 1) and last (inner == 1), and a source that is a strided view
        a = values("take_ends_%s" % dtype, (AXIS_LEN, 5, 13), dtype)
        i = rng_of("take_ends").randint(-13, 13, 20)
        for how in INDEX_KINDS:
            out.append(B.t(a)[..., B.idx(i, how)])
            out.append(B.t(a.transpose(2, 0, 1))[B.idx(i, how), :])
            out.append(B.t(a[::2, :, ::-1])[:, B.idx(i % 5, how)])
        return out
    return run


def _take_axis_edges(B):
    out = []
    one = B.t(values("axis_of_one", (3, 1, 7), np.int16))
    for how in INDEX_KINDS:
        out.append(one[:, B.idx(np.array([0, -1, 0, 0, -1]), how)])
    # an axis of 40000: int16 cannot name its upper part from the front, but reaches it from the back (-32768 -> 7232)
    n = 40000
    for dtype in (np.int16, np.float32):
        long = B.t(values("axis_of_40000_%s" % np.dtype(dtype), (2, n, 3), dtype))
        rng = rng_of("axis_of_40000")
        for how in (np.int32, np.int64, "host"):
            i = np.concatenate([rng.randint(-n, n, 200), [n - 1, -n, 32767, 32768, -32768, -32769, 0, -1]])
            out.append(long[:, B.idx(i, how)])
        i = np.concatenate([rng.randint(-32768, 0, 200), rng.randint(0, 32768, 50), [-32768, -32767, 32767, -1, 0]])
        out.append(long[:, B.idx(i, np.int16)])
        out.append(long[:, B.idx(np.full(7, -32768), np.int16)])
    return out


for _d in SOURCE_DTYPES:
    case("take_plain_%s" % _d, _take_plain(_d))
case("take_axis_edges", _take_axis_edges)


# ---- assignment with distinct indices -----------------------------------------------------------------------------------------------
def _distinct(name, axis_len, n):
    """n distinct positions of an axis, about half of them written from the back"""
    rng = rng_of("distinct_" + name)
    pos = rng.permutation(axis_len)[:n]
    return np.where(rng.randint(0, 2, n) == 1, pos - axis_len, pos)


def _put_plain(dtype):
    def run(B):
        for outer in OUTERS:
            for inner in INNERS:
                name = "put_%s_%d_%d" % (dtype, outer, inner)
                shape, n = (outer, AXIS_LEN, inner), 6
                a = values(name, shape, dtype)
                for how in INDEX_KINDS + ("list",):
                    i = _distinct("%s_%s" % (name, how), AXIS_LEN, n)
                    forms = [("scalar", lambda: _scalar(dtype)), ("scalar2", lambda: _scalar(dtype, 1)),
                             ("tensor", lambda: B.t(values(name + "v", (outer, n, inner), dtype))),
                             ("row", lambda: B.t(values(name + "r", (inner,), dtype))),
                             ("column", lambda: B.t(values(name + "c", (n, 1), dtype))),
                             ("strided", lambda: B.t(values(name + "s", (inner, n, outer), dtype).transpose(2, 1, 0)))]
                    for tag, value in forms:
                        t = B.t(a)
                        B.note_put(i % AXIS_LEN)
                        t[:, B.idx(list(i) if how == "list" else i, how)] = value()
                if dtype != np.uint8:
                    for how in INDEX_KINDS:                     # `+=` through an index is take, add, put (numpy's too: no accumulation)
                        i = _distinct("%s_%s_iadd" % (name, how), AXIS_LEN, n)
                        t = B.t(a)
                        B.note_put(i % AXIS_LEN)
                        t[:, B.idx(i, how)] += 3
        # a destination that is a strided view of a sentinel base: the whole base is compared
        base = sentinel("put_view_%s" % dtype, 8 * 12 * 10, dtype).reshape(8, 12, 10)
        for how in INDEX_KINDS:
            i = _distinct("put_view_%s" % (how,), 6, 4)
            t = B.t(base[1:7, ::2, 9:2:-1].transpose(2, 1, 0))             # (7, 6, 6)
            B.note_put(i % 6)
            t[:, B.idx(i, how)] = B.t(values("put_view_v_%s" % dtype, (7, 4, 6), dtype))
            t = B.t(base[::3, 1:, 2:8])                                    # (3, 11, 6)
            B.note_put(i % 6)
            t[..., B.idx(i, how)] = _scalar(dtype)
        # the first axis, an index of shape (2, 2) and of no dimensions
        t = B.t(values("put_first_%s" % dtype, (9, 4), dtype))
        B.note_put(np.array([8, 0, 3, 5]))
        t[B.idx(np.array([[8, 0], [-6, 5]]), np.int32)] = B.t(values("put_first_v_%s" % dtype, (2, 2, 4), dtype))
        B.note_put(np.array([1]))
        t[B.idx(np.array(-8), np.int64)] = _scalar(dtype)
        t[B.idx(np.zeros(0, np.int64), np.int16)] = _scalar(dtype, 1)      # names nothing
    return run


for _d in SOURCE_DTYPES:
    case("put_plain_%s" % _d, _put_plain(_d))


# ---- the one assignment with repeated indices ---------------------------------------------------------------------------------------
def put_repeats_data():
    """rows 7 and 31 of 50 are each named three times, with different values: numpy keeps the last, the kernel keeps one of them"""
    a = values("put_repeats", (3, 50, 7), np.float32)
    i = np.array([4, 7, -43, 20, 31, 7, 49, -19, 0, 31, -50 + 12, 33])
    v = values("put_repeats_v", (3, len(i), 7), np.float32)
    return a, i, v


def put_repeats_positions():
    _, i, _ = put_repeats_data()
    named, counts = np.unique(i % 50, return_counts=True)
    return named[counts > 1]


def _put_repeats(B):
    a, i, v = put_repeats_data()
    t = B.t(a)
    B.note_put(i % 50)
    t[:, B.idx(i, np.int32)] = B.t(v)


def check_put_repeats(got, want):
    """every position the index names once is numpy's; a position named several times holds, element by element, one of the
    values written to it"""
    got, want = got[1][0], want[1][0]                  # the base of t: the first array the case wrapped
    a, i, v = put_repeats_data()
    got, want = got.reshape(a.shape), want.reshape(a.shape)
    repeated = put_repeats_positions()
    once = np.ones(50, bool)
    once[repeated] = False
    assert got[:, once].tobytes() == want[:, once].tobytes()
    for p in repeated:
        written = v[:, (i % 50) == p].view(np.uint32)                          # [outer][writes][inner]
        assert (written == got[:, p].view(np.uint32)[:, None, :]).any(axis=1).all(), "position %d holds a value nobody wrote" % p


case("put_repeats", _put_repeats, check_put_repeats)


# ---- the paired form: entry (o mod n) of the labels belongs to outer position o -----------------------------------------------------
PAIR_N, PAIR_K, PAIR_C = (1, 5, 257), (1, 3, 6), 9


def _labels(name, n, classes=PAIR_C):
    return rng_of("labels_" + name).randint(-classes, classes, n)


def _paired(dtype):
    dtype = np.dtype(dtype)

    def run(B):
        out = []
        for n in PAIR_N:
            for k in PAIR_K:
                for how in DEVICE_INDEX + ("list",):
                    name = "pair_%s_%d_%d_%s" % (dtype, n, k, how)
                    lab = _labels(name, n)
                    pick = lambda: B.idx(list(lab) if how == "list" else lab, how)      # noqa: E731
                    # outer = k n
                    a = values(name, (k, n, PAIR_C), dtype)
                    t = B.t(a)
                    out.append(t[:, B.rng(n), pick()])
                    t[:, B.rng(n), pick()] = _scalar(dtype)
                    t = B.t(a)
                    t[:, B.rng(n), pick()] = B.t(values(name + "v", (k, n), dtype))
                    k0 = {1: 1, 3: 3, 6: 2}[k]
                    t = B.t(a.reshape(k0, k // k0, n, PAIR_C))
                    out.append(t[:, :, B.rng(n), pick()])
                    t[:, :, B.rng(n), pick()] = B.t(values(name + "w", (k // k0, n), dtype))       # a value that is broadcast
                    if dtype != np.uint8:
                        t = B.t(a)
                        t[:, B.rng(n), pick()] -= 1                            # loss.cross_entropy's backward: take, subtract, put
                for inner in (2, 65):
                    for how in DEVICE_INDEX + ("list",):
                        name = "pair_inner_%s_%d_%d_%s" % (dtype, n, inner, how)
                        lab = _labels(name, n)
                        pick = lambda: B.idx(list(lab) if how == "list" else lab, how)      # noqa: E731
                        a = values(name, (n, PAIR_C, inner), dtype)
                        t = B.t(a)
                        out.append(t[B.rng(n), pick(), :])
                        out.append(t[B.rng(n), pick()])
                        t[B.rng(n), pick(), :] = B.t(values(name + "v", (n, inner), dtype))
                        t = B.t(a)
                        t[B.rng(n), pick()] = _scalar(dtype, 1)
        return out
    return run


for _d in SOURCE_DTYPES:
    case("paired_%s" % _d, _paired(_d))


# ---- scatter-add: the backward of t[index] -------------------------------------------------------------------------------------------
SCATTER_N = 4096


def scatter_data(tier):
    """[(shape of t, index along axis 1, contributions)]: 4096 contributions into 3 rows, and all of them into one.  Exact tier:
    integers of magnitude <= 8, so every partial sum is an integer below 2^24 and any order of adding gives the same float32"""
    out = []
    for tag, low, high in (("three_rows", 0, 3), ("one_row", 1, 2), ("from_the_back", -3, 0)):
        rng = rng_of("scatter_%s_%s" % (tier, tag))
        idx = rng.randint(low, high, SCATTER_N)
        shape = (2, SCATTER_N, 5)
        w = rng.randint(-8, 9, shape).astype(np.float32) if tier == "exact" else rng.uniform(-1, 1, shape).astype(np.float32)
        out.append(((2, 3, 5), idx, w))
    return out


def _scatter(tier):
    def run(B):
        out = []
        for k, (shape, idx, w) in enumerate(scatter_data(tier)):
            a = np.zeros(shape, np.float32)
            for how in INDEX_KINDS:
                out.append(B.take_grad(a, (slice(None), B.idx(idx, how)), w))
        # the paired form and a folded pair of index arrays, inner > 1 and the labels wrapping (outer = 3 n)
        rng = rng_of("scatter_pair_" + tier)
        n = 257
        lab = rng.randint(-PAIR_C, PAIR_C, n)
        w = rng.randint(-8, 9, (3, n)).astype(np.float32)
        for how in DEVICE_INDEX:
            out.append(B.take_grad(np.zeros((3, n, PAIR_C), np.float32), (slice(None), B.rng(n), B.idx(lab, how)), w))
            out.append(B.take_grad(np.zeros((n, PAIR_C, 2), np.float32), (B.rng(n), B.idx(lab, how)), w.T[:, :2].copy()))
        return out
    return run


def scatter_bound(tier, got):
    """|got - float64 np.add.at| <= gamma(m - 1) * sum |contribution| per destination, gamma(k) = k u / (1 - k u), u = 2^-24, m the
    addends of the destination with its initial value: the bound of recursive summation, whatever the order"""
    u, k = 2.0 ** -24, 0
    for shape, idx, w in scatter_data(tier):
        ref, mag, count = np.zeros(shape), np.zeros(shape), np.zeros(shape)
        np.add.at(ref, (slice(None), idx), w.astype(np.float64))
        np.add.at(mag, (slice(None), idx), np.abs(w.astype(np.float64)))
        np.add.at(count, (slice(None), idx), 1.0)
        gamma = count * u / (1 - count * u)                  # m - 1 = the number of contributions: the initial value is the m-th
        for _ in INDEX_KINDS:
            assert got[k].dtype == np.float32 and got[k].shape == shape
            err = np.abs(got[k].astype(np.float64) - ref)
            assert (err <= gamma * mag).all(), (tier, k, float(err.max()), float((gamma * mag).max()))
            k += 1
    return k


def check_scatter_general(got, want):
    k = scatter_bound("general", got[0])
    same_bytes(got[0][k:], want[0][k:], "scatter_general (the paired forms hold integers)")


case("scatter_exact", _scatter("exact"))
case("scatter_general", _scatter("general"), check_scatter_general)


# ---- several index arrays folded into one --------------------------------------------------------------------------------------------
def _fold(B):
    out = []
    rng = rng_of("fold")
    a = values("fold", (6, 5, 7), np.float32)
    i16, i32, i64 = np.int16, np.int32, np.int64
    r = lambda n, shape: rng.randint(-n, n, shape)      # noqa: E731
    t = B.t(a)
    # two and three arrays, each broadcast along a different dimension
    out.append(t[B.idx(r(6, (4, 1)), i16), B.idx(r(5, (1, 3)), i64)])
    out.append(t[B.idx(r(6, (4, 1, 1)), i16), B.idx(r(5, (1, 3, 1)), i32), B.idx(r(7, (1, 1, 2)), i64)])
    out.append(t[:, B.idx(r(5, (3, 1)), i32), B.idx(r(7, (4,)), i16)])
    # a transposed device index array
    out.append(t[B.idx(r(6, (3, 4)).astype(i32).T, i32), B.idx(r(5, (4, 3)), i64)])
    out.append(t[B.idx(r(6, (3, 4)).astype(i16).T, i16), :, B.idx(r(7, (3, 4)).astype(i64).T, i64)])
    # plain integers among the arrays, arrays apart (the index dimensions go first)
    out.append(t[B.idx(r(6, (4,)), i64), 2, B.idx(r(7, (4,)), i16)])
    out.append(t[-6, B.idx(r(5, (2, 3)), i32), B.idx(r(7, (3,)), i32)])
    out.append(t[B.idx(r(6, (2, 1)), i32), :, B.idx(r(7, (3,)), i64)])
    # index tensors of no dimensions
    out.append(t[B.idx(np.array(-6), i32), B.idx(r(5, (4,)), i16)])
    out.append(t[B.idx(np.array(5), i64), :, B.idx(np.array(-1), i16)])
    # every index at -len and at len - 1
    for how in DEVICE_INDEX:
        out.append(t[B.idx(np.full(3, -6), how), B.idx(np.full(3, -5), how), B.idx(np.full(3, -7), how)])
        out.append(t[B.idx(np.full(3, 5), how), B.idx(np.full(3, 4), how), B.idx(np.full(3, 6), how)])
    # eight arrays of mixed dtypes on eight axes, two of them broadcast
    shape8 = (2, 3, 2, 3, 2, 3, 2, 3)
    for dtype in SOURCE_DTYPES:
        t8 = B.t(values("fold8_%s" % dtype, shape8, dtype))
        index = [B.idx(r(n, (1,) if d in (2, 5) else (10,)), DEVICE_INDEX[d % 3]) for d, n in enumerate(shape8)]
        out.append(t8[tuple(index)])
        out.append(t8[tuple(index[:3])])
    # assignment through folded indices: distinct positions
    flat = rng.permutation(30)[:8]
    i0, i1 = flat // 5, flat % 5
    t = B.t(a)
    B.note_put(flat)
    t[B.idx(i0 - 6, i16), B.idx(i1, i64)] = B.t(values("fold_put", (8, 7), np.float32))
    B.note_put(flat)
    t[B.idx(i0, i32), B.idx(i1 - 5, i32), B.idx(np.full(8, 3), i16)] = np.float32(-0.0)
    # its backward: contributions that are integers (any order of adding)
    j0, j1 = r(6, (300,)), r(5, (300,))
    out.append(B.take_grad(np.zeros((6, 5, 7), np.float32), (B.idx(j0, i16), B.idx(j1, i64)), rng.randint(-8, 9, (300, 7)).astype(np.float32)))
    return out


case("fold", _fold)


# ---- boolean masks ---------------------------------------------------------------------------------------------------------------------
MASK_BLOCK, MASK_RUN = 4096, 16                      # one workgroup's and one thread's share of a mask
MASK_LENGTHS = (1, 15, 16, 17, 4095, 4096, 4097, 256 * 4096 - 1, 256 * 4096, 256 * 4096 + 1, 258 * 4096 + 17)
MASK_BLOCK_COUNTS = {1, 2, 256, 257, 259}


def mask_blocks(n):
    return (n + MASK_BLOCK - 1) // MASK_BLOCK


def mask_patterns(n):
    rng = rng_of("mask_%d" % n)
    empty = np.zeros(n, bool)
    yield "none", empty
    if n <= 4097 or n == 256 * 4096 + 1:
        yield "all", np.ones(n, bool)
    for at in sorted({0, n - 1, 4095, 4096, 256 * 4096}):
        if at < n:
            m = empty.copy()
            m[at] = True
            yield "only_%d" % at, m
    yield "half", rng.uniform(0, 1, n) < 0.5
    yield "hundredth", rng.uniform(0, 1, n) < 0.01
    blocks = mask_blocks(n)
    for b in sorted({1, 255, 256, blocks - 2}):
        if 0 < b < blocks - 1:                          # one block entirely True between empty blocks
            m = empty.copy()
            m[b * MASK_BLOCK:(b + 1) * MASK_BLOCK] = True
            yield "block_%d" % b, m
    if n >= 3 * MASK_RUN:                               # one thread's run entirely True
        m = empty.copy()
        m[MASK_RUN:2 * MASK_RUN] = True
        yield "run_1", m


def _mask_length(n):
    def run(B):
        out = []
        where = B.t(np.arange(n, dtype=np.int64))      # t[mask] of the positions themselves IS flatnonzero(mask)
        data = B.t(values("mask_values_%d" % n, (n,), np.uint8))
        for tag, m in mask_patterns(n):
            out.append(where[B.mask(m)])
            if n <= 4097 or tag == "half":
                out.append(data[B.mask(m)])
        return out
    return run


for _n in MASK_LENGTHS:
    case("mask_length_%d" % _n, _mask_length(_n))


def _mask_forms(B):
    out = []
    rng = rng_of("mask_forms")
    a = values("mask_forms", (5, 6, 7, 3), np.float32)
    t = B.t(a)
    m3 = rng.uniform(0, 1, (5, 6, 7)) < 0.4
    out.append(t[B.mask(m3)])                                                   # three leading axes of four
    out.append(t[B.mask(m3[:, :, 0])])
    out.append(t[B.mask(np.ascontiguousarray(m3.transpose(1, 0, 2)).transpose(1, 0, 2))])      # a mask that is not dense
    wide = rng.uniform(0, 1, (130, 70)) < 0.3
    out.append(B.t(values("mask_wide", (70, 130), np.int16))[B.mask(wide.T)])
    out.append(t[:, B.mask(m3[0, :, :])])
    out.append(t[B.idx(rng.randint(0, 5, 42), np.int32), B.mask(np.ones((6, 7), bool))])       # a mask next to an index array
    for dtype in SOURCE_DTYPES:
        d = B.t(values("mask_put_%s" % dtype, (5, 6, 7), dtype))
        B.note_put(np.flatnonzero(m3))
        d[B.mask(m3)] = _scalar(dtype)
        B.note_put(np.flatnonzero(~m3))
        d[B.mask(~m3)] = B.t(values("mask_put_v_%s" % dtype, (int((~m3).sum()),), dtype))
        d = B.t(sentinel("mask_put_view_%s" % dtype, 6 * 8 * 4, dtype).reshape(6, 8, 4)[:5, 1:7].transpose(1, 0, 2))
        B.note_put(np.flatnonzero(m3[:, :, 0].T))
        d[B.mask(m3[:, :, 0].T)] = B.t(values("mask_put_w_%s" % dtype, (4,), dtype))          # a row broadcast over the selection
    return out


case("mask_forms", _mask_forms)

BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)
