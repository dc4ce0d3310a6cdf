"""The case table of the row-wise kernel sweep (tests/test_hip_rowwise.py) and its references.  No GPU code here:
tests/test_rowwise_cases_cpu.py checks on the host what the GPU test relies on.

csrc/rowwise.hip and csrc/tail_jobs.h hold softmax (forward: 2 / 8 / 32 floats per lane in registers, or a loop that re-reads
the row; backward with a double shift), LayerNorm forward / backward, the LayerNorm parameter gradients (rows split over
workgroups, ticket-elected fold), the embedding gather and its scatter-add (chunked and ordered, or plain atomics), and the
three launch forms of the jobs queued inside a `lg_gemm_group_*` bracket.  Every case names the path it is MEANT to reach
(`regs`, `splits` and `chunk`, `path`); the GPU test asserts that against `lg_rowwise_last_plan`, so a retuned threshold that
moves a case to another path fails the test instead of silently emptying it.  The thresholds themselves are not restated.

All device work goes through the C ABI on flat buffers made by `padded`: GUARD elements in front of and behind the payload -
NaN around every float input (a kernel that reads outside spoils its result), an id no table holds around every id array (read,
it raises the index error at the next synchronisation), SENTINEL around every output (a kernel that writes outside changes it).

Inputs:
  exact  the parameter gradients and the scatter-add: small integers stored as float32, so every partial sum in every order is
         an exactly representable integer and the kernel must return numpy's int64 result bit for bit - ONE dropped, doubled or
         misplaced row shows at any size.
  real   softmax, LayerNorm, the real-valued scatter-adds: judged PER ROW against float64 by the rule of tests/common.py -
         relative Frobenius distance at most max(FLOOR, twice the float32 numpy composite's distance on that row); the CPU
         test keeps every composite within FLOOR / 2, so the floor is the bound in force everywhere.
"""
import zlib
from collections import namedtuple
from functools import lru_cache
import numpy as np

# lg_rowwise_last_plan: {kernel, a, b, queued}
SOFTMAX_FWD, SOFTMAX_BWD, LAYERNORM_FWD, LAYERNORM_BWD, PARAM_GRADS, SCATTER_ADD, GATHER, NONE = 0, 1, 2, 3, 4, 5, 6, -1
SCATTER_QUEUED, SCATTER_CHUNKED, SCATTER_ATOMIC = 0, 1, 2

GUARD = 2112                     # elements on either side of a payload: more than the widest register tile (64 lanes x 32) reaches
SENTINEL = -777.25
BAD_ID = 1 << 30                 # in no table: the guard of id arrays
MAX_ELEMENTS = 4 << 20           # no buffer holds more
MAX_TABLE_ELEMENTS = 16 << 20    # all cases together
EXACT_LIMIT = 1 << 24            # integers of magnitude up to here are exact in float32
FLOOR = 1e-5                     # the project's north-star distance
COMPOSITE_CAP = FLOOR / 2        # every float32 numpy composite stays this close to float64, per row (CPU test)
ROW_SUM_BOUND = 2.0 ** -22       # softmax backward: |sum(dx)| <= this * sum(|dx|) per row (two fp32 roundings per element, twice over)
LN_EPS = 1e-5


def rng_for(name, salt=""):
    return np.random.RandomState(zlib.crc32(("%s/%s" % (name, salt)).encode()) & 0x7FFFFFFF)


def padded(payload, fill):
    """flat array: GUARD x fill, the payload, GUARD x fill"""
    payload = np.ascontiguousarray(payload)
    flat = np.full(payload.size + 2 * GUARD, fill, payload.dtype)
    flat[GUARD:GUARD + payload.size] = payload.reshape(-1)
    return flat


def payload_of(flat, shape):
    n = int(np.prod(shape, dtype=np.int64))
    assert flat.shape == (n + 2 * GUARD,)
    return flat[GUARD:GUARD + n].reshape(shape)


def guards_of(flat):
    return np.concatenate([flat[:GUARD], flat[-GUARD:]])


def rel_frobenius(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-300))


def row_distances(got, ref):
    """relative Frobenius distance of every row (the last axis) of `got` to `ref`; a row whose reference is all zero: 0 when `got`
    is all zero there too, else inf"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    got, ref = got.reshape(-1, got.shape[-1] if got.ndim else 1), ref.reshape(-1, ref.shape[-1] if ref.ndim else 1)
    num, den = np.linalg.norm(got - ref, axis=1), np.linalg.norm(ref, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0, num / np.where(den > 0, den, 1), np.where(num > 0, np.inf, 0.0))


def row_bounds(composite32, ref):
    """the distance each row of a float32 kernel result may have: tests/common.py's rule, per row"""
    return np.maximum(FLOOR, 2 * row_distances(composite32, ref))


def _frozen(*arrays):
    for a in arrays:
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return arrays


# ---- softmax --------------------------------------------------------------------------------------------------------------

SOFTMAX_REGS = {1: 2, 2: 2, 63: 2, 64: 2, 65: 2, 127: 2, 128: 2, 129: 8, 511: 8, 512: 8, 513: 32, 2047: 32, 2048: 32, 2049: 0, 4100: 0}
SOFTMAX_COLS = tuple(SOFTMAX_REGS)
ROWS = (1, 3, 4, 5, 9)                       # every residue of the four rows a block holds, and more than one block
SCALES = (1.0, 0.125)
TILE_WIDTHS = (128, 512, 2048)               # 64 lanes x the register counts

SoftmaxCase = namedtuple("SoftmaxCase", "name rows cols scale kind regs")


def _softmax_table():
    t = []
    for ci, cols in enumerate(SOFTMAX_COLS):
        regs = SOFTMAX_REGS[cols]
        for ri, rows in enumerate(ROWS):                               # (a): the whole product, the scales alternating
            scale = SCALES[(ci + ri) % 2]
            t.append(SoftmaxCase("softmax_uniform_%dx%d_s%g" % (rows, cols, scale), rows, cols, scale, "uniform", regs))
        rows = 9 if cols > 512 else ROWS[ci % 5]                       # (b): wide rows have more boundaries than few rows can visit
        t.append(SoftmaxCase("softmax_spike_%dx%d" % (rows, cols), rows, cols, SCALES[ci % 2], "spike", regs))
        if cols > 1:                                                   # (c): a row of one column cannot lose it
            rows = ROWS[(ci + 1) % 5]
            t.append(SoftmaxCase("softmax_neginf_%dx%d" % (rows, cols), rows, cols, SCALES[(ci + 1) % 2], "neginf", regs))
        rows = (3, 4, 5, 9)[ci % 4]                                    # (d): needs a good row next to the two bad ones
        t.append(SoftmaxCase("softmax_badrows_%dx%d" % (rows, cols), rows, cols, SCALES[ci % 2], "badrows", regs))
    return tuple(t)


def spike_columns(cols):
    """where a skipped element hurts most: the ends of the row, and the columns at and just before every boundary between
    lanes' register slots (multiples of 64) - first those that are also the edge of a register tile"""
    first = [cols - 1, 0]
    for w in reversed(TILE_WIDTHS):
        first += [w - 1, w]
    first += [63, 64]
    rest = []
    for b in range(128, cols + 64, 64):
        rest += [b - 1, b]
    seen, out = set(), []
    for c in first + rest:
        if 0 <= c < cols and c not in seen:
            seen.add(c)
            out.append(c)
    return out


def softmax_rows_bad(case):
    """(the row that is -inf throughout, the row that holds one NaN) of a `badrows` case"""
    return case.rows // 2, case.rows - 1


def softmax_reference(x, scale):
    """float64 softmax of the float32 product x * scale; a row whose maximum is -inf or NaN is NaN throughout, like the composite"""
    t = (np.asarray(x, np.float32) * np.float32(scale)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        e = np.exp(t - t.max(axis=-1, keepdims=True))
        return e / e.sum(axis=-1, keepdims=True)


def softmax_composite32(x, scale):
    """autograd/ops.py:62-66 in float32 numpy"""
    t = np.asarray(x, np.float32) * np.float32(scale)
    with np.errstate(invalid="ignore"):
        e = np.exp(t - t.max(axis=-1, keepdims=True))
        return (e / e.sum(axis=-1, keepdims=True)).astype(np.float32)


@lru_cache(maxsize=None)
def softmax_inputs(name):
    """(x, float64 reference, float32 composite, x without the bad rows' damage or None)"""
    c = SOFTMAX_BY_NAME[name]
    rng = rng_for("softmax_%dx%d" % (c.rows, c.cols))                  # the kinds of one shape share their base
    x = rng.uniform(-3, 3, (c.rows, c.cols)).astype(np.float32)
    clean = None
    if c.kind == "spike":
        cand = spike_columns(c.cols)
        for r in range(c.rows):
            x[r, cand[r % len(cand)]] += np.float32(25)
    elif c.kind == "neginf":
        mask = rng_for(name, "mask").uniform(0, 1, x.shape) < 0.3
        mask[:, -1] = True                                             # the last column always: the ragged end of the register tile
        keep = rng_for(name, "keep").randint(0, c.cols - 1, c.rows)    # one finite column per row at least
        mask[np.arange(c.rows), keep] = False
        x[mask] = -np.inf
    elif c.kind == "badrows":
        clean = x.copy()
        inf_row, nan_row = softmax_rows_bad(c)
        x[inf_row] = -np.inf
        x[nan_row, spike_columns(c.cols)[0]] = np.nan                  # the last column
    return _frozen(x, softmax_reference(x, c.scale), softmax_composite32(x, c.scale), clean)


SoftmaxBwdCase = namedtuple("SoftmaxBwdCase", "name rows cols scale")


def softmax_bwd_reference(y, g, scale):
    """y * (g - sum(g * y) / sum(y)) * scale in float64 on the float32 arrays"""
    y, g = np.asarray(y, np.float64), np.asarray(g, np.float64)
    return y * (g - (g * y).sum(-1, keepdims=True) / y.sum(-1, keepdims=True)) * float(scale)


def softmax_bwd_float_shift(y, g, scale):
    """the same formula with the shift formed, divided and subtracted in float32: what the kernel must NOT do"""
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    shift = (g * y).sum(-1, keepdims=True, dtype=np.float32) / y.sum(-1, keepdims=True, dtype=np.float32)
    return ((y * (g - shift)) * np.float32(scale)).astype(np.float32)


def softmax_bwd_composite32(y, g, scale):
    """the float32 numpy composite of the distance rule: float32 throughout, but the common offset of g is taken off first
    (g - g[:, :1] is exact in float32 for g within a factor of two of each other) - the formula is invariant under it, and
    the shift that is left is of the size of dx, which is how float32 reaches what the kernel's double shift reaches"""
    y, g = np.asarray(y, np.float32), np.asarray(g, np.float32)
    return softmax_bwd_float_shift(y, g - g[:, :1], scale)


def row_sum_excess(dx):
    """|sum(dx)| / sum(|dx|) per row in float64 (0 for a row of zeros): at most ROW_SUM_BOUND for a double shift"""
    dx = np.asarray(dx, np.float64)
    s, a = np.abs(dx.sum(-1)), np.abs(dx).sum(-1)
    return np.where(a > 0, s / np.where(a > 0, a, 1), 0.0)


@lru_cache(maxsize=None)
def softmax_bwd_inputs(name):
    """(y, g, float64 reference, the float32-shift counter-example, float32 composite)"""
    c = SOFTMAX_BWD_BY_NAME[name]
    rng = rng_for(name)
    y = softmax_composite32(rng.uniform(-3, 3, (c.rows, c.cols)).astype(np.float32), 1.0)
    g = (30 + rng.uniform(-1, 1, (c.rows, c.cols))).astype(np.float32)   # the common offset: |shift| ~ 30 |dx|
    return _frozen(y, g, softmax_bwd_reference(y, g, c.scale), softmax_bwd_float_shift(y, g, c.scale), softmax_bwd_composite32(y, g, c.scale))


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------

LAYERNORM_COLS = (1, 2, 63, 64, 65, 128, 130, 1000, 4100)
LayerNormCase = namedtuple("LayerNormCase", "name rows cols kind")


def layernorm_reference(x, w, b, dtype):
    """nn.py:109-124 in `dtype`: (y, xhat, rstd)"""
    x, w, b = (np.asarray(a, dtype) for a in (x, w, b))
    d = x - x.mean(-1, keepdims=True, dtype=dtype)
    v = (d * d).mean(-1, keepdims=True, dtype=dtype)
    rstd = dtype(1) / np.sqrt(v + dtype(LN_EPS))
    xhat = d * rstd
    return xhat * w + b, xhat, rstd[..., 0]


def layernorm_bwd_reference(g, w, xhat, rstd, dtype):
    """dx = rstd * (gh - mean(gh) - xhat * mean(gh * xhat)), gh = g * w (the kernel's comment) in `dtype`"""
    g, w, xhat, rstd = (np.asarray(a, dtype) for a in (g, w, xhat, rstd))
    gh = g * w
    return rstd[:, None] * (gh - gh.mean(-1, keepdims=True, dtype=dtype) - xhat * (gh * xhat).mean(-1, keepdims=True, dtype=dtype))


@lru_cache(maxsize=None)
def layernorm_inputs(name):
    """x, w, b, g; the backward's inputs xhat32 and rstd32 are the float64 forward rounded to float32"""
    c = LAYERNORM_BY_NAME[name]
    rng = rng_for(name)
    if c.kind == "const":
        x = np.full((c.rows, c.cols), 0.5, np.float32)
    else:
        x = (rng.uniform(-3, 3, (c.rows, 1)) + rng.uniform(-2, 2, (c.rows, c.cols))).astype(np.float32)
        if c.cols == 2:
            # two columns normalise to +1 and -1 whatever they hold, and dx is then what cancellation leaves of it (no float32
            # composite gets within the floor of that): scaled by 2**-9 the variance is of the size of eps and dx is well conditioned
            x *= np.float32(2.0 ** -9)
    w = rng.uniform(0.5, 1.5, c.cols).astype(np.float32)
    b = rng.uniform(-1, 1, c.cols).astype(np.float32)
    g = rng.uniform(-1, 1, (c.rows, c.cols)).astype(np.float32)
    _, xhat, rstd = layernorm_reference(x, w, b, np.float64)
    return _frozen(x, w, b, g, xhat.astype(np.float32), rstd.astype(np.float32))


# ---- LayerNorm parameter gradients (exact) ----------------------------------------------------------------------------------

# rows -> (splits, chunk) the host is expected to settle on while the columns fill at most 16 blocks of 256
PARAM_GRAD_PLAN = {1: (1, 1), 3: (1, 3), 4: (1, 4), 5: (1, 5), 63: (1, 63), 64: (4, 16), 65: (4, 17), 100: (6, 17), 511: (31, 17),
                   512: (32, 16), 513: (31, 17), 1000: (32, 32), 1025: (32, 33)}
PARAM_GRAD_COLS = (1, 96, 255, 256, 257, 1000)
FLAG_COMBINATIONS = ((0, 0), (0, 1), (1, 0), (1, 1))      # (dw accumulates, db accumulates)
ParamGradCase = namedtuple("ParamGradCase", "name rows cols splits chunk feature")


def _param_grad_table():
    t = []

    def add(rows, cols, plan=None, feature=""):
        splits, chunk = plan or PARAM_GRAD_PLAN[rows]
        t.append(ParamGradCase("param_grads_%dx%d" % (rows, cols), rows, cols, splits, chunk, feature))
    for rows in (1, 3, 4, 5, 63, 64, 65, 100):                           # few rows: the whole product
        for cols in PARAM_GRAD_COLS:
            add(rows, cols)
    for rows in (511, 512, 513, 1000, 1025):                            # many rows: two widths each, and every width once more
        add(rows, 96)
        add(rows, 257)
    add(511, 255)
    add(512, 256)
    add(513, 1)
    add(1000, 1)
    add(1025, 1)
    add(70, 16640, (4, 18), "65 column blocks: never queued")
    return tuple(t)


@lru_cache(maxsize=None)
def param_grad_inputs(name):
    """(g, xhat, dw0, db0, int64 dw, int64 db): integers, g in [-4, 4], xhat in [-3, 3], the accumulate prefill in [-8, 8]"""
    c = PARAM_GRAD_BY_NAME[name]
    rng = rng_for(name)
    g = rng.randint(-4, 5, (c.rows, c.cols))
    xhat = rng.randint(-3, 4, (c.rows, c.cols))
    dw0, db0 = rng.randint(-8, 9, c.cols), rng.randint(-8, 9, c.cols)
    return _frozen(g.astype(np.float32), xhat.astype(np.float32), dw0.astype(np.float32), db0.astype(np.float32),
                   (g.astype(np.int64) * xhat).sum(0), g.astype(np.int64).sum(0))


def param_grad_expected(name, acc_w, acc_b):
    _, _, dw0, db0, dw, db = param_grad_inputs(name)
    return (dw + dw0.astype(np.int64) if acc_w else dw).astype(np.float64), (db + db0.astype(np.int64) if acc_b else db).astype(np.float64)


# ---- embedding scatter-add and gather ------------------------------------------------------------------------------------

ScatterCase = namedtuple("ScatterCase", "name pattern n_ids row_len table_rows path real exact_bits bad feature")
ROW_LENS = (1, 12, 255, 256, 257, 700)
HOT = 7                                                                # the repeated id of the patterns below


def _others(n_ids, table_rows, rng):
    """distinct ids none of which is HOT, the last row or its alias"""
    pool = np.array([r for r in range(table_rows - 1) if r != HOT])
    assert len(pool) >= n_ids
    return rng.permutation(pool)[:n_ids]


def make_ids(case):
    """the id pattern of a case, built by hand around ids that occur once each"""
    rng = rng_for(case.name, "ids")
    n, rows = case.n_ids, case.table_rows
    kind, _, arg = case.pattern.partition(":")
    if kind == "equal":
        return np.full(n, HOT, np.int64)
    ids = _others(n, rows, rng)
    if kind == "distinct":
        pass
    elif kind == "adjacent":                 # HOT at `arg` consecutive positions
        k = int(arg)
        start = 0 if k == n else min(3, n - k)
        ids[start:start + k] = HOT
    elif kind == "spread":                   # HOT every `arg` positions: consecutive occurrences more than a ballot window (or two) apart
        ids[5::int(arg)] = HOT
    elif kind == "cluster":                  # HOT alone, once more two windows on, then 40 times in a row: 42 occurrences
        ids[5] = ids[300] = HOT
        ids[600:640] = HOT
    elif kind == "alias":                    # -1 and table_rows - 1 alternate at `arg` positions three apart: one row, two spellings
        where = 2 + 3 * np.arange(int(arg))
        ids[where[0::2]] = -1
        ids[where[1::2]] = rows - 1
    elif kind == "negative":                 # every second id spelled from the end
        ids[1::2] -= rows
    else:
        raise ValueError(case.pattern)
    if case.bad:
        ids[n // 2] = rows                   # one id out of range
    return ids


def occurrences(ids, table_rows):
    return np.bincount(np.where(ids < 0, ids + table_rows, ids)[(ids >= -table_rows) & (ids < table_rows)], minlength=table_rows)


def _scatter_table():
    t = []

    def add(name, pattern, n_ids, row_len, table_rows=None, real=False, exact_bits=True, bad=False, feature=""):
        if table_rows is None:
            table_rows = n_ids + 40
        path = SCATTER_CHUNKED if n_ids <= 4096 else SCATTER_ATOMIC
        t.append(ScatterCase("scatter_" + name, pattern, n_ids, row_len, table_rows, path, real, exact_bits, bad, feature))
    C = 4096                                                                   # the most ids the chunked kernel takes
    for k in (1, 2, 31, 32, 33, 64, 65, 700):
        add("occ%d_adjacent_n%d" % (k, C), "adjacent:%d" % k, C, 12, feature="one id %d times in a row" % k)
    for k in (2, 31, 32, 33):
        add("occ%d_adjacent_n33" % k, "adjacent:%d" % k, 33, 257, feature="row_len past one trip of the column loop")
    add("occ65_adjacent_n4097", "adjacent:65", 4097, 12, feature="the atomic kernel")
    add("occ700_adjacent_n4097", "adjacent:700", 4097, 1)
    add("spread257_n4096", "spread:257", C, 12, feature="16 occurrences, each in a ballot window of its own")
    add("spread513_n4096", "spread:513", C, 1, feature="8 occurrences, an empty window between any two")
    add("spread257_n4097", "spread:257", 4097, 12)
    add("window_overfull_n4096", "adjacent:50", C, 1, feature="the first window holds 49 matches, the first chunk wants 31, the second 17")
    add("late_cluster_n4096", "cluster", C, 12, feature="an empty window, one match, then a window with 40 matches for the 30 still wanted")
    add("alias32_n4096", "alias:32", C, 12, feature="-1 and table_rows - 1: 32 positions of one row, ordered adds")
    add("alias40_n4096", "alias:40", C, 12, feature="-1 and table_rows - 1: 40 positions of one row, atomics")
    add("alias10_n33", "alias:10", 33, 700)
    add("alias40_n4097", "alias:40", 4097, 1)
    for n in (1, 33, C, 4097):
        add("distinct_n%d" % n, "distinct", n, 12)
        add("equal_n%d" % n, "equal", n, 12 if n < C else 1, feature="every position the same row")
    for row_len in ROW_LENS:
        add("negative_n33_len%d" % row_len, "negative", 33, row_len, feature="row_len %d" % row_len)
        add("equal_n33_len%d" % row_len, "equal", 33, row_len, table_rows=9)
    add("single_len700", "distinct", 1, 700, table_rows=9)
    # real-valued: at most 32 occurrences give np.add.at's float32 bits (the documented order), more are judged by distance
    add("real_occ32_n4096", "adjacent:32", C, 12, real=True)
    add("real_spread257_n4096", "spread:257", C, 12, real=True)
    add("real_occ33_n4096", "adjacent:33", C, 12, real=True, exact_bits=False)
    add("real_occ700_n4096", "adjacent:700", C, 12, real=True, exact_bits=False)
    add("real_occ700_n4097", "adjacent:700", 4097, 12, real=True, exact_bits=False)
    # one id out of range: reported at the next synchronisation, that position adds nothing, every other one is added
    add("bad_id_n33", "adjacent:5", 33, 12, bad=True)
    add("bad_id_n4097", "adjacent:5", 4097, 1, bad=True)
    return tuple(t)


@lru_cache(maxsize=None)
def scatter_inputs(name):
    """(ids int64, grad_out, table0, reference table float64, float32 np.add.at result)"""
    c = SCATTER_BY_NAME[name]
    rng = rng_for(name)
    ids = make_ids(c)
    if c.real:
        grad = rng.uniform(-1, 1, (c.n_ids, c.row_len)).astype(np.float32)
        table0 = rng.uniform(-1, 1, (c.table_rows, c.row_len)).astype(np.float32)
    else:
        grad = rng.randint(-8, 9, (c.n_ids, c.row_len)).astype(np.float32)
        table0 = rng.randint(-8, 9, (c.table_rows, c.row_len)).astype(np.float32)
    ok = (ids >= -c.table_rows) & (ids < c.table_rows)
    ref = table0.astype(np.float64)
    np.add.at(ref, ids[ok], grad[ok].astype(np.float64))
    np32 = table0.copy()
    np.add.at(np32, ids[ok], grad[ok])
    return _frozen(ids, grad, table0, ref, np32)


GatherCase = namedtuple("GatherCase", "name n_ids row_len table_rows")


@lru_cache(maxsize=None)
def gather_inputs(name):
    """(ids int64 with negative spellings and repeats, table)"""
    c = GATHER_BY_NAME[name]
    rng = rng_for(name)
    ids = rng.randint(-c.table_rows, c.table_rows, c.n_ids).astype(np.int64)
    edge = (-1, c.table_rows - 1, 0, -c.table_rows)
    ids[:4] = edge[:c.n_ids]
    table = rng.uniform(-1, 1, (c.table_rows, c.row_len)).astype(np.float32)
    return _frozen(ids, table)


# ---- the queued forms ----------------------------------------------------------------------------------------------------------
# the same jobs immediately, alone inside a lg_gemm_group_* bracket, and beside weight-gradient products: bit-equal throughout
QUEUED_PARAM_GRADS = ("param_grads_65x96", "param_grads_100x257", "param_grads_513x96")
QUEUED_SCATTERS = ("scatter_equal_n33", "scatter_spread257_n4096", "scatter_alias40_n4096")
LN_GROUP_MAX, SCATTER_GROUP_MAX = 8, 4               # what one bracket queues before it flushes (csrc/tail_jobs.h)
WGRAD_SHAPES = ((256, 96, 80), (512, 128, 128))      # (k, m, n) of dW[m, n] = g[k, m]^T @ x[k, n]: products a bracket queues


@lru_cache(maxsize=None)
def wgrad_inputs(index):
    """(g, x, int64 g^T @ x): integers in [-2, 2], every partial sum exact"""
    k, m, n = WGRAD_SHAPES[index]
    rng = rng_for("wgrad%d" % index)
    g, x = rng.randint(-2, 3, (k, m)), rng.randint(-2, 3, (k, n))
    return _frozen(g.astype(np.float32), x.astype(np.float32), (g.T.astype(np.int64) @ x).astype(np.float64))


# ---- the tables ----------------------------------------------------------------------------------------------------------------

SOFTMAX_CASES = _softmax_table()
SOFTMAX_BWD_CASES = tuple(SoftmaxBwdCase("softmax_bwd_%dx%d_s%g" % (ROWS[i % 5], cols, SCALES[i % 2]), ROWS[i % 5], cols, SCALES[i % 2])
                          for i, cols in enumerate(SOFTMAX_COLS))
LAYERNORM_CASES = tuple(LayerNormCase("layernorm_%dx%d" % (rows, cols), rows, cols, "real") for cols in LAYERNORM_COLS for rows in ROWS) + (
    LayerNormCase("layernorm_const_5x64", 5, 64, "const"),)
PARAM_GRAD_CASES = _param_grad_table()
SCATTER_CASES = _scatter_table()
GATHER_CASES = tuple(GatherCase("gather_n%d_len%d" % (n, row_len), n, row_len, 40) for row_len in ROW_LENS for n in ((1, 50) if row_len == 12 else (50,)))

SOFTMAX_BY_NAME = {c.name: c for c in SOFTMAX_CASES}
SOFTMAX_BWD_BY_NAME = {c.name: c for c in SOFTMAX_BWD_CASES}
LAYERNORM_BY_NAME = {c.name: c for c in LAYERNORM_CASES}
PARAM_GRAD_BY_NAME = {c.name: c for c in PARAM_GRAD_CASES}
SCATTER_BY_NAME = {c.name: c for c in SCATTER_CASES}
GATHER_BY_NAME = {c.name: c for c in GATHER_CASES}
ALL_CASES = SOFTMAX_CASES + SOFTMAX_BWD_CASES + LAYERNORM_CASES + PARAM_GRAD_CASES + SCATTER_CASES + GATHER_CASES


def buffers(case):
    """payload element counts of every buffer a case puts on the device"""
    if isinstance(case, SoftmaxCase):
        return [case.rows * case.cols] * 2
    if isinstance(case, SoftmaxBwdCase):
        return [case.rows * case.cols] * 3
    if isinstance(case, LayerNormCase):
        return [case.rows * case.cols] * 5 + [case.cols] * 2 + [case.rows]
    if isinstance(case, ParamGradCase):
        return [case.rows * case.cols] * 2 + [case.cols] * 2
    if isinstance(case, ScatterCase):
        return [case.n_ids, case.n_ids * case.row_len, case.table_rows * case.row_len]
    return [case.n_ids, case.n_ids * case.row_len, case.table_rows * case.row_len]
