"""Every dispatch edge of the row-wise kernels (csrc/rowwise.hip, csrc/tail_jobs.h) against exact references, through the raw
C ABI on flat buffers.

The cases, their inputs and references are tests/rowwise_cases.py (checked on the host by tests/test_rowwise_cases_cpu.py).
After every call the plan `lg_rowwise_last_plan` reports is compared with the path the case is meant for: when a retuned
threshold moves a case to another path the assertion fails and the SHAPE is to be adjusted.  Every float input lies between
NaN guards, every id array between ids no table holds, every output between sentinels that must come back untouched.  The
integer families (LayerNorm parameter gradients, scatter-add, gather, the queued forms) must equal numpy's int64 result bit
for bit; real-valued outputs are judged PER ROW against float64 by the rule of tests/common.py - relative Frobenius distance at
most max(1e-5, twice the float32 numpy composite's distance on that row) - so that one bad row cannot hide in the array.

Two branches of the dispatch are not reached by any case, and no case is contorted to reach them: `blocks_x >
tickets_tail_count()` in the parameter gradients (more than 8 million columns) and row counts at or above 2**31.

The queued forms: a bracket that holds ONE weight-gradient product launches it alone and the jobs behind it; with two products
the jobs ride as extra workgroups of the products' launch.  Both are run."""
import ctypes
import numpy as np
import pytest
import rowwise_cases as R

pytestmark = pytest.mark.gpu

_device = {}          # key -> device buffer of a shared input: uploaded once, left unchanged


@pytest.fixture(scope="module")
def L(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    hiplib.lib()
    return hiplib


class Buf(object):
    """a payload between guards on the device; `ptr` is the payload's address"""

    def __init__(self, hip, payload, fill):
        payload = np.asarray(payload)
        self.shape, self.fill, self.dtype = payload.shape, fill, payload.dtype
        self.t = hip.from_numpy(R.padded(payload, fill), requires_grad=False)
        self.ptr = self.t.ptr + R.GUARD * payload.dtype.itemsize

    def read(self, what=""):
        """the payload, after checking that the guards are what they were"""
        flat = self.t.numpy()
        np.testing.assert_array_equal(R.guards_of(flat), np.full(2 * R.GUARD, self.fill, self.dtype), err_msg="written outside the payload: " + what)
        return R.payload_of(flat, self.shape).copy()


def fin(hip, payload):
    """a float input: NaN all around"""
    return Buf(hip, np.asarray(payload, np.float32), np.nan)


def fout(hip, shape_or_prefill):
    """an output: sentinels all around; the payload NaN (anything that reads it before writing shows) unless a prefill is given"""
    pre = np.full(shape_or_prefill, np.nan, np.float32) if isinstance(shape_or_prefill, (tuple, int)) else np.asarray(shape_or_prefill, np.float32)
    return Buf(hip, pre, R.SENTINEL)


def idbuf(hip, ids, dtype):
    return Buf(hip, np.asarray(ids).astype(dtype), R.BAD_ID)


def shared(hip, key, make):
    if key not in _device:
        _device[key] = make()
    return _device[key]


def last_plan(L):
    p = (ctypes.c_int32 * 4)()
    L.check(L.lib().lg_rowwise_last_plan(p))
    return tuple(p)


def assert_plan(L, name, *want):
    got = last_plan(L)
    assert got == tuple(want), "%s is meant for plan %s, the library chose %s: adjust the shape" % (name, want, got)


def assert_rows_close(got, ref, composite32, what):
    d, bound = R.row_distances(got, ref), R.row_bounds(composite32, ref)
    worst = int(np.argmax(d - bound))
    print("rowwise-distance %-34s worst row %d: %.3g from float64 (bound %.3g)" % (what, worst, d[worst], bound[worst]))
    assert np.all(d <= bound), "%s: row %d is %.3g from float64, bound %.3g" % (what, worst, d[worst], bound[worst])


# ---- softmax --------------------------------------------------------------------------------------------------------------

def run_softmax(hip, L, c, x):
    xb, yb = fin(hip, x), fout(hip, (c.rows, c.cols))
    L.check(L.lib().lg_softmax_scaled_f32(xb.ptr, yb.ptr, c.rows, c.cols, c.scale))
    assert_plan(L, c.name, R.SOFTMAX_FWD, c.regs, 0, 0)
    return yb.read(c.name)


@pytest.mark.parametrize("name", [c.name for c in R.SOFTMAX_CASES])
def test_softmax_forward(hip, L, name):
    c = R.SOFTMAX_BY_NAME[name]
    x, ref, np32, clean = R.softmax_inputs(name)
    got = run_softmax(hip, L, c, x)
    good = np.ones(c.rows, bool)
    if c.kind == "badrows":
        good[list(R.softmax_rows_bad(c))] = False
        assert np.isnan(got[~good]).all(), "a row that is -inf throughout and a row with a NaN are NaN throughout"
        # the rows beside them are what they are without them, bit for bit
        np.testing.assert_array_equal(got[good], run_softmax(hip, L, c, clean)[good])
    assert np.isfinite(got[good]).all()
    assert_rows_close(got[good], ref[good], np32[good], name)
    if c.kind == "neginf":
        gone = np.isneginf(x)
        np.testing.assert_array_equal(got[gone], 0.0)
    if c.scale == 1.0 and c.kind == "uniform":                        # lg_softmax_f32 is the scaled form at scale 1
        xb, yb = fin(hip, x), fout(hip, (c.rows, c.cols))
        L.check(L.lib().lg_softmax_f32(xb.ptr, yb.ptr, c.rows, c.cols))
        assert_plan(L, name, R.SOFTMAX_FWD, c.regs, 0, 0)
        np.testing.assert_array_equal(yb.read(name), got)


@pytest.mark.parametrize("name", [c.name for c in R.SOFTMAX_BWD_CASES])
def test_softmax_backward_rows_sum_to_zero(hip, L, name):
    """the distance rule, and per row |sum(dx)| <= 2**-22 * sum(|dx|): two float32 roundings per element (the product and the scale)
    give at most 2 * 2**-24 per element, the bound is twice that.  A float32 shift misses it by an order of magnitude on these
    inputs (tests/test_rowwise_cases_cpu.py)."""
    c = R.SOFTMAX_BWD_BY_NAME[name]
    y, g, ref, _, np32 = R.softmax_bwd_inputs(name)
    yb, gb, db = fin(hip, y), fin(hip, g), fout(hip, (c.rows, c.cols))
    L.check(L.lib().lg_softmax_scaled_bwd_f32(yb.ptr, gb.ptr, db.ptr, c.rows, c.cols, c.scale))
    assert_plan(L, name, R.SOFTMAX_BWD, 0, 0, 0)
    got = db.read(name)
    assert np.isfinite(got).all()
    assert_rows_close(got, ref, np32, name)
    excess = R.row_sum_excess(got)
    print("rowwise-rowsum %-30s max |sum dx| / sum |dx| = %.3g (bound %.3g)" % (name, excess.max(), R.ROW_SUM_BOUND))
    assert np.all(excess <= R.ROW_SUM_BOUND), (name, excess)


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in R.LAYERNORM_CASES])
def test_layernorm_forward_and_backward(hip, L, name):
    c = R.LAYERNORM_BY_NAME[name]
    x, w, b, g, xhat32, rstd32 = R.layernorm_inputs(name)
    xb, wb, bb = fin(hip, x), fin(hip, w), fin(hip, b)
    yb, hb, rb = fout(hip, (c.rows, c.cols)), fout(hip, (c.rows, c.cols)), fout(hip, (c.rows,))
    L.check(L.lib().lg_layernorm_f32(xb.ptr, wb.ptr, bb.ptr, yb.ptr, hb.ptr, rb.ptr, c.rows, c.cols, R.LN_EPS))
    assert_plan(L, name, R.LAYERNORM_FWD, 0, 0, 0)
    y, xhat, rstd = yb.read(name + " y"), hb.read(name + " xhat"), rb.read(name + " rstd")
    gb, h32, r32, dxb = fin(hip, g), fin(hip, xhat32), fin(hip, rstd32), fout(hip, (c.rows, c.cols))
    L.check(L.lib().lg_layernorm_bwd_f32(gb.ptr, wb.ptr, h32.ptr, r32.ptr, dxb.ptr, c.rows, c.cols))
    assert_plan(L, name, R.LAYERNORM_BWD, 0, 0, 0)
    dx = dxb.read(name + " dx")
    ref = R.layernorm_reference(x, w, b, np.float64)
    np32 = R.layernorm_reference(x, w, b, np.float32)
    dx_ref = R.layernorm_bwd_reference(g, w, xhat32, rstd32, np.float64)
    dx32 = R.layernorm_bwd_reference(g, w, xhat32, rstd32, np.float32)
    if c.kind == "const" or c.cols == 1:
        # mean and deviations are exact: xhat == 0 and y == beta bit for bit, rstd == 1 / sqrt(eps) to float32 rounding
        np.testing.assert_array_equal(xhat, 0.0)
        np.testing.assert_array_equal(y, np.broadcast_to(b, y.shape))
        assert np.all(np.abs(rstd.astype(np.float64) * np.sqrt(float(np.float32(R.LN_EPS))) - 1) <= 2.0 ** -23), rstd
        if c.cols == 1:
            np.testing.assert_array_equal(dx, 0.0)
        else:
            assert_rows_close(dx, dx_ref, dx32, name + " dx")
        return
    for what, got, a64, a32 in (("y", y, ref[0], np32[0]), ("xhat", xhat, ref[1], np32[1]),
                                ("rstd", rstd[:, None], ref[2][:, None], np32[2][:, None]), ("dx", dx, dx_ref, dx32)):
        assert np.isfinite(got).all()
        assert_rows_close(got, a64, a32, name + " " + what)


# ---- LayerNorm parameter gradients ------------------------------------------------------------------------------------------

def param_grad_call(L, c, gb, hb, dwb, dbb, acc_w, acc_b, queued=0):
    L.check(L.lib().lg_layernorm_param_grads_f32(gb.ptr, hb.ptr, dwb.ptr, dbb.ptr, c.rows, c.cols, acc_w, acc_b))
    assert_plan(L, c.name, R.PARAM_GRADS, c.splits, c.chunk, queued)


def param_grad_outputs(hip, name, acc_w, acc_b):
    """accumulated outputs start from integers, overwritten ones from NaN: an overwrite that reads its destination shows"""
    c = R.PARAM_GRAD_BY_NAME[name]
    _, _, dw0, db0, _, _ = R.param_grad_inputs(name)
    return fout(hip, dw0 if acc_w else (c.cols,)), fout(hip, db0 if acc_b else (c.cols,))


def param_grad_device_inputs(hip, name):
    g, xhat = R.param_grad_inputs(name)[:2]
    return shared(hip, ("pg", name), lambda: (fin(hip, g), fin(hip, xhat)))


@pytest.mark.parametrize("name", [c.name for c in R.PARAM_GRAD_CASES])
def test_layernorm_param_grads_are_exact(hip, L, name):
    """all four accumulate / overwrite combinations, each twice back to back into fresh outputs: a ticket that was not reset makes
    the second run's last workgroup miss its turn"""
    c = R.PARAM_GRAD_BY_NAME[name]
    gb, hb = param_grad_device_inputs(hip, name)
    for acc_w, acc_b in R.FLAG_COMBINATIONS:
        outs = [param_grad_outputs(hip, name, acc_w, acc_b) for _ in range(2)]
        for dwb, dbb in outs:
            param_grad_call(L, c, gb, hb, dwb, dbb, acc_w, acc_b)
        want_w, want_b = R.param_grad_expected(name, acc_w, acc_b)
        for run, (dwb, dbb) in enumerate(outs):
            what = "%s acc=(%d, %d) run %d" % (name, acc_w, acc_b, run)
            np.testing.assert_array_equal(dwb.read(what).astype(np.float64), want_w, err_msg=what + " dw")
            np.testing.assert_array_equal(dbb.read(what).astype(np.float64), want_b, err_msg=what + " db")


# ---- scatter-add and gather ---------------------------------------------------------------------------------------------------

def scatter_call(L, c, gb, ib, tb, queued=0):
    L.check(L.lib().lg_scatter_add_rows_f32(gb.ptr, ib.ptr, ib.dtype.itemsize, tb.ptr, c.n_ids, c.row_len, c.table_rows))
    assert_plan(L, c.name, R.SCATTER_ADD, R.SCATTER_QUEUED if queued else c.path, 0, queued)


def scatter_device_inputs(hip, name, dtype):
    ids, grad = R.scatter_inputs(name)[:2]
    return shared(hip, ("sc", name, dtype), lambda: (fin(hip, grad), idbuf(hip, ids, dtype)))


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("name", [c.name for c in R.SCATTER_CASES])
def test_scatter_add(hip, L, name, dtype):
    c = R.SCATTER_BY_NAME[name]
    ids, grad, table0, ref, np32 = R.scatter_inputs(name)
    gb, ib = scatter_device_inputs(hip, name, dtype)
    tb = fout(hip, table0)
    scatter_call(L, c, gb, ib, tb)
    if c.bad:
        # documented behaviour: the next synchronisation reports the index error, once; that position adds nothing
        with pytest.raises(IndexError):
            L.check(L.lib().lg_sync())
    L.check(L.lib().lg_sync())
    got = tb.read(name)
    if not c.real:
        np.testing.assert_array_equal(got.astype(np.float64), ref, err_msg=name)
    elif c.exact_bits:
        assert got.tobytes() == np32.tobytes(), "%s: at most 32 positions per row are added in np.add.at's order" % name
    else:
        assert_rows_close(got, ref, np32, name)
        untouched = R.occurrences(ids, c.table_rows) == 0
        np.testing.assert_array_equal(got[untouched], table0[untouched])


@pytest.mark.parametrize("dtype", ["int32", "int64"])
@pytest.mark.parametrize("name", [c.name for c in R.GATHER_CASES])
def test_gather(hip, L, name, dtype):
    c = R.GATHER_BY_NAME[name]
    ids, table = R.gather_inputs(name)
    tb, ib, ob = fin(hip, table), idbuf(hip, ids, dtype), fout(hip, (c.n_ids, c.row_len))
    L.check(L.lib().lg_gather_rows_f32(tb.ptr, ib.ptr, ib.dtype.itemsize, ob.ptr, c.n_ids, c.row_len, c.table_rows))
    assert_plan(L, name, R.GATHER, 0, 0, 0)
    L.check(L.lib().lg_sync())
    assert ob.read(name).tobytes() == table[ids].tobytes()


def test_calls_that_launch_nothing(hip, L):
    lib = L.lib()
    keep = fout(hip, np.full(8, 7, np.float32))
    src = fin(hip, np.ones(8))
    L.check(lib.lg_softmax_scaled_f32(src.ptr, keep.ptr, 4, 2, 1.0))
    assert last_plan(L)[0] == R.SOFTMAX_FWD
    for call in (lambda: lib.lg_softmax_scaled_f32(src.ptr, keep.ptr, 0, 8, 1.0),
                 lambda: lib.lg_softmax_scaled_bwd_f32(src.ptr, src.ptr, keep.ptr, 0, 8, 1.0),
                 lambda: lib.lg_layernorm_bwd_f32(src.ptr, src.ptr, src.ptr, src.ptr, keep.ptr, 0, 8),
                 lambda: lib.lg_gather_rows_f32(src.ptr, src.ptr, 4, keep.ptr, 0, 8, 1),
                 lambda: lib.lg_scatter_add_rows_f32(src.ptr, src.ptr, 4, keep.ptr, 0, 8, 1)):
        L.check(lib.lg_softmax_scaled_bwd_f32(src.ptr, src.ptr, keep.ptr, 1, 8, 1.0))
        assert last_plan(L) == (R.SOFTMAX_BWD, 0, 0, 0)                      # the report follows the most recent call
        L.check(call())
        assert last_plan(L) == (R.NONE, 0, 0, 0)
    assert lib.lg_softmax_scaled_f32(src.ptr, keep.ptr, 1, 0, 1.0) == -1 and last_plan(L)[0] == R.NONE      # refused
    assert lib.lg_rowwise_last_plan(None) == -1
    L.check(lib.lg_sync())


# ---- the queued forms ----------------------------------------------------------------------------------------------------------

def wgrad_call(L, gb, xb, ob, k, m, n, accumulate=0):
    L.check(L.lib().lg_gemm_f32(1, 0, m, n, k, gb.ptr, m, 0, xb.ptr, n, 0, ob.ptr, n, 0, 1, accumulate))


class Jobs(object):
    """LayerNorm parameter-gradient jobs [(case name, acc_w, acc_b)] and scatter jobs [case name] with fresh outputs each"""

    def __init__(self, hip, L, ln, sc, products=0):
        self.hip, self.L, self.ln, self.sc, self.products = hip, L, list(ln), list(sc), products
        self.ln_out = [param_grad_outputs(hip, n, aw, ab) for n, aw, ab in self.ln]
        self.sc_out = [fout(hip, R.scatter_inputs(n)[2]) for n in self.sc]
        self.wg = []
        for i in range(products):
            g, x, _ = R.wgrad_inputs(i)
            gb, xb = shared(hip, ("wg", i), lambda: (fin(hip, g), fin(hip, x)))
            self.wg.append((gb, xb, fout(hip, (g.shape[1], x.shape[1]))))

    def run(self, queued):
        L, lib = self.L, self.L.lib()
        if queued:
            L.check(lib.lg_gemm_group_begin())
        for i, (gb, xb, ob) in enumerate(self.wg):
            k, m, n = R.WGRAD_SHAPES[i]
            wgrad_call(L, gb, xb, ob, k, m, n)
        for (name, aw, ab), (dwb, dbb) in zip(self.ln, self.ln_out):
            gb, hb = param_grad_device_inputs(self.hip, name)
            param_grad_call(L, R.PARAM_GRAD_BY_NAME[name], gb, hb, dwb, dbb, aw, ab, queued)
        for k, (name, tb) in enumerate(zip(self.sc, self.sc_out)):
            gb, ib = scatter_device_inputs(self.hip, name, ("int32", "int64")[k % 2])
            scatter_call(L, R.SCATTER_BY_NAME[name], gb, ib, tb, queued)
        if queued:
            L.check(lib.lg_gemm_group_end())
        L.check(lib.lg_sync())                                   # launches what is still queued
        return self

    def results(self, what):
        out = []
        for (dwb, dbb) in self.ln_out:
            out += [dwb.read(what), dbb.read(what)]
        out += [tb.read(what) for tb in self.sc_out]
        out += [ob.read(what) for _, _, ob in self.wg]
        return out

    def check(self, what):
        """against numpy's int64 results; returns the raw arrays"""
        got = self.results(what)
        want = []
        for name, aw, ab in self.ln:
            want += list(R.param_grad_expected(name, aw, ab))
        want += [R.scatter_inputs(n)[3] for n in self.sc]
        want += [R.wgrad_inputs(i)[2] for i in range(self.products)]
        for k, (a, b) in enumerate(zip(got, want)):
            np.testing.assert_array_equal(a.astype(np.float64), b, err_msg="%s: output %d" % (what, k))
        return got


LN3 = [(n, k % 2, (k // 2) % 2) for k, n in enumerate(R.QUEUED_PARAM_GRADS, 1)]
QUEUED_FORMS = {
    "one_entry_0": (LN3[:1], [], 0), "one_entry_1": (LN3[1:2], [], 0), "one_entry_2": (LN3[2:], [], 0),       # flushed as layernorm_param_grads
    "several_entries": (LN3, [], 0),                                                                         # param_grads_tail_group
    "one_scatter": ([], list(R.QUEUED_SCATTERS[:1]), 0),
    "entries_and_scatters": (LN3, list(R.QUEUED_SCATTERS), 0),
    "beside_one_product": (LN3, list(R.QUEUED_SCATTERS), 1),       # the product leaves alone, the jobs in a launch behind it
    "beside_two_products": (LN3, list(R.QUEUED_SCATTERS), 2),      # the jobs ride as extra workgroups of the products' launch
    "one_entry_beside_two_products": (LN3[2:], [], 2),
}


@pytest.mark.parametrize("form", list(QUEUED_FORMS))
def test_queued_forms_equal_immediate_calls(hip, L, form):
    ln, sc, products = QUEUED_FORMS[form]
    now = Jobs(hip, L, ln, sc, products).run(queued=0).check(form + " immediately")
    for attempt in range(2):                                      # twice: the tickets of the queued launch are reset too
        later = Jobs(hip, L, ln, sc, products).run(queued=1).check("%s queued, run %d" % (form, attempt))
        for a, b in zip(now, later):
            assert a.tobytes() == b.tobytes(), form


def test_a_ninth_layernorm_entry_and_a_fifth_scatter_job_force_a_flush(hip, L):
    names = [R.QUEUED_PARAM_GRADS[k % 3] for k in range(R.LN_GROUP_MAX + 1)]
    Jobs(hip, L, [(n, k % 2, (k // 2) % 2) for k, n in enumerate(names)], []).run(queued=1).check("nine LayerNorm entries")
    sc = [R.QUEUED_SCATTERS[k % 3] for k in range(R.SCATTER_GROUP_MAX + 1)]
    Jobs(hip, L, [], sc).run(queued=1).check("five scatter jobs")
    Jobs(hip, L, [(n, 1, 0) for n in names], sc, 2).run(queued=1).check("nine entries, five scatter jobs, two products")


def test_the_same_destination_queued_twice_keeps_call_order(hip, L):
    lib = L.lib()
    a, b = R.PARAM_GRAD_BY_NAME["param_grads_65x96"], R.PARAM_GRAD_BY_NAME["param_grads_513x96"]
    (ga, ha), (gb_, hb_) = param_grad_device_inputs(hip, a.name), param_grad_device_inputs(hip, b.name)
    wa, ba = R.param_grad_expected(a.name, 0, 0)
    wb, bb = R.param_grad_expected(b.name, 0, 0)
    dwb, dbb = fout(hip, (96,)), fout(hip, (96,))                 # NaN: accumulating before the overwrite would show
    L.check(lib.lg_gemm_group_begin())
    param_grad_call(L, a, ga, ha, dwb, dbb, 0, 0, queued=1)
    param_grad_call(L, b, gb_, hb_, dwb, dbb, 1, 1, queued=1)    # the same dw and db: the first entry leaves first
    param_grad_call(L, a, ga, ha, dwb, dbb, 1, 1, queued=1)
    L.check(lib.lg_gemm_group_end())
    L.check(lib.lg_sync())
    np.testing.assert_array_equal(dwb.read("dw").astype(np.float64), 2 * wa + wb)
    np.testing.assert_array_equal(dbb.read("db").astype(np.float64), 2 * ba + bb)
    # one table, two scatter jobs
    s1, s2 = R.SCATTER_BY_NAME["scatter_alias40_n4096"], R.SCATTER_BY_NAME["scatter_spread257_n4096"]
    assert (s1.row_len, s1.table_rows) == (s2.row_len, s2.table_rows)
    i1, g1, table0, _, _ = R.scatter_inputs(s1.name)
    i2, g2 = R.scatter_inputs(s2.name)[:2]
    want = table0.astype(np.float64)
    np.add.at(want, i1, g1.astype(np.float64))
    np.add.at(want, i2, g2.astype(np.float64))
    tb = fout(hip, table0)
    L.check(lib.lg_gemm_group_begin())
    scatter_call(L, s1, *scatter_device_inputs(hip, s1.name, "int32"), tb, queued=1)
    scatter_call(L, s2, *scatter_device_inputs(hip, s2.name, "int64"), tb, queued=1)
    L.check(lib.lg_gemm_group_end())
    L.check(lib.lg_sync())
    np.testing.assert_array_equal(tb.read("table").astype(np.float64), want)
