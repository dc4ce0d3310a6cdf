"""What tests/test_hip_rowwise.py relies on, checked on the host: the case table of tests/rowwise_cases.py keeps its exact
families exact, its real-valued inputs harmless to numpy's own float32 composites (so the 1e-5 floor is the bound in force
everywhere), its buffers small, its id patterns what their names say, and the float32-shift counter-example of the softmax
backward outside the row-sum bound the kernel has to meet."""
import numpy as np
import pytest
import rowwise_cases as R


def ids_of(cases):
    return [c.name for c in cases]


def test_names_are_unique_and_the_table_is_small():
    names = ids_of(R.ALL_CASES)
    assert len(set(names)) == len(names)
    total = 0
    for c in R.ALL_CASES:
        for n in R.buffers(c):
            assert 0 < n + 2 * R.GUARD <= R.MAX_ELEMENTS, c.name
            total += n + 2 * R.GUARD
    assert total < R.MAX_TABLE_ELEMENTS, total
    print("rowwise-cases %d cases, %d elements" % (len(names), total))


def test_views_lie_inside_their_buffers():
    for shape, fill in (((3, 5), np.nan), ((1,), R.SENTINEL), ((7, 1, 2), 0.0)):
        pay = np.arange(int(np.prod(shape)), dtype=np.float32).reshape(shape) + 1
        flat = R.padded(pay, fill)
        assert flat.shape == (pay.size + 2 * R.GUARD,) and R.GUARD % 4 == 0 and R.GUARD > 64 * 32
        view = R.payload_of(flat, shape)
        assert np.shares_memory(view, flat) and np.array_equal(view, pay)
        np.testing.assert_array_equal(R.guards_of(flat), np.full(2 * R.GUARD, fill, np.float32))
    ids = R.padded(np.arange(5, dtype=np.int32), R.BAD_ID)
    assert ids.dtype == np.int32 and ids[0] == R.BAD_ID == ids[-1]
    for c in R.SCATTER_CASES + R.GATHER_CASES:
        assert R.BAD_ID >= c.table_rows and -R.BAD_ID < -c.table_rows


def test_every_path_and_every_split_count_occurs():
    assert {c.regs for c in R.SOFTMAX_CASES} == {2, 8, 32, 0}
    assert {c.cols for c in R.SOFTMAX_CASES} == set(R.SOFTMAX_COLS) == {c.cols for c in R.SOFTMAX_BWD_CASES}
    for kind in ("uniform", "spike", "neginf", "badrows"):
        cases = [c for c in R.SOFTMAX_CASES if c.kind == kind]
        assert {c.cols for c in cases} >= set(R.SOFTMAX_COLS) - ({1} if kind == "neginf" else set()), kind
        assert {c.rows % 4 for c in cases} == {0, 1, 3} or kind == "badrows", kind        # (1, 3, 4, 5, 9: no row count is 2 mod 4)
        assert {c.scale for c in cases} == set(R.SCALES), kind
    assert {(c.rows, c.cols) for c in R.SOFTMAX_CASES if c.kind == "uniform"} == {(r, c) for r in R.ROWS for c in R.SOFTMAX_COLS}
    assert {(c.rows, c.cols) for c in R.LAYERNORM_CASES if c.kind == "real"} == {(r, c) for r in R.ROWS for c in R.LAYERNORM_COLS}
    assert [c for c in R.LAYERNORM_CASES if c.kind == "const" and c.cols == 64]
    assert {c.rows for c in R.PARAM_GRAD_CASES} == set(R.PARAM_GRAD_PLAN) | {70}
    assert {c.cols for c in R.PARAM_GRAD_CASES} == set(R.PARAM_GRAD_COLS) | {16640}
    assert {c.splits for c in R.PARAM_GRAD_CASES} == {s for s, _ in R.PARAM_GRAD_PLAN.values()} == {1, 4, 6, 31, 32}
    assert {c.path for c in R.SCATTER_CASES} == {R.SCATTER_CHUNKED, R.SCATTER_ATOMIC}
    assert {c.row_len for c in R.SCATTER_CASES} == set(R.ROW_LENS) == {c.row_len for c in R.GATHER_CASES}
    assert {c.n_ids for c in R.SCATTER_CASES} == {1, 33, 4096, 4097}
    for name in R.QUEUED_PARAM_GRADS:
        assert (R.PARAM_GRAD_BY_NAME[name].cols + 255) // 256 <= 64
    assert len({R.PARAM_GRAD_BY_NAME[n].splits for n in R.QUEUED_PARAM_GRADS}) == 3
    for name in R.QUEUED_SCATTERS:
        c = R.SCATTER_BY_NAME[name]
        assert c.path == R.SCATTER_CHUNKED and not c.real and not c.bad


# ---- softmax ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ids_of(R.SOFTMAX_CASES))
def test_softmax_case(name):
    c = R.SOFTMAX_BY_NAME[name]
    x, ref, np32, clean = R.softmax_inputs(name)
    assert x.shape == ref.shape == np32.shape == (c.rows, c.cols) and x.dtype == np.float32
    bad = np.zeros(c.rows, bool)
    if c.kind == "badrows":
        inf_row, nan_row = R.softmax_rows_bad(c)
        assert inf_row != nan_row and c.rows >= 3
        bad[[inf_row, nan_row]] = True
        assert np.all(np.isneginf(x[inf_row])) and np.isnan(x[nan_row]).sum() == 1
        assert np.array_equal(x[~bad], clean[~bad]) and np.isfinite(clean).all()
    assert np.isnan(ref[bad]).all() and np.isnan(np32[bad]).all()          # like the composite: NaN throughout
    good_ref, good32 = ref[~bad], np32[~bad]
    assert np.isfinite(good_ref).all() and np.allclose(good_ref.sum(-1), 1, rtol=1e-12, atol=0)
    assert R.row_distances(good32, good_ref).max() <= R.COMPOSITE_CAP
    assert np.all(R.row_bounds(good32, good_ref) == R.FLOOR)
    if c.kind == "spike":
        cand = R.spike_columns(c.cols)
        assert cand[0] == c.cols - 1 and len(set(cand)) == len(cand) and all(0 <= k < c.cols for k in cand)
        peak = x.argmax(-1)
        assert [int(p) for p in peak] == [cand[r % len(cand)] for r in range(c.rows)]
        assert np.all(x[np.arange(c.rows), peak] >= 22)
        # a kernel that skips the spike is wrong in every other element of that row, hundreds of times the bound at the least
        for r in range(c.rows):
            if c.cols > 1:
                x_skipped = np.delete(x[r], peak[r])
                assert R.row_distances(R.softmax_reference(x_skipped, c.scale), np.delete(ref[r], peak[r]))[0] > 100 * R.FLOOR
    if c.kind == "neginf":
        gone = np.isneginf(x)
        assert gone.any(-1).all() and (~gone).any(-1).all() and gone[:, -1].all()
        assert np.all(ref[gone] == 0) and np.all(np32[gone] == 0)


def test_spike_columns_visit_every_tile_edge_that_exists():
    for cols in R.SOFTMAX_COLS:
        cand = set(R.spike_columns(cols))
        want = {0, cols - 1} | {k for w in R.TILE_WIDTHS + (64,) for k in (w - 1, w) if k < cols}
        assert want <= cand, (cols, want - cand)
        visited = {R.softmax_inputs(c.name)[0].argmax(-1)[r] for c in R.SOFTMAX_CASES if c.kind == "spike" and c.cols == cols for r in range(c.rows)}
        assert cols - 1 in visited


@pytest.mark.parametrize("name", ids_of(R.SOFTMAX_BWD_CASES))
def test_softmax_backward_case_and_the_float_shift_counter_example(name):
    c = R.SOFTMAX_BWD_BY_NAME[name]
    y, g, ref, float_shift, np32 = R.softmax_bwd_inputs(name)
    assert y.dtype == g.dtype == float_shift.dtype == np32.dtype == np.float32 and y.shape == g.shape == ref.shape == (c.rows, c.cols)
    assert np.all((g >= 29) & (g <= 31))
    # the reference itself sums to zero far below the bound, and rounding it to float32 stays inside it
    assert R.row_sum_excess(ref).max() <= 2.0 ** -40
    assert R.row_sum_excess(ref.astype(np.float32)).max() <= R.ROW_SUM_BOUND / 2
    assert R.row_distances(np32, ref).max() <= R.COMPOSITE_CAP
    assert np.all(R.row_bounds(np32, ref) == R.FLOOR)
    # the distance rule alone would not catch a float32 shift (which is why the row-sum condition exists)
    assert R.row_distances(float_shift, ref).max() <= 2 * R.FLOOR
    if c.cols == 1:
        assert np.all(ref == 0) and np.all(float_shift == 0)
        return
    shift = (g.astype(np.float64) * y).sum(-1) / y.astype(np.float64).sum(-1)
    assert np.all(np.abs(shift) >= 25 * np.abs(ref / c.scale).max(-1))      # the regime of csrc/rowwise.hip's comment on softmax_bwd


def test_a_float32_shift_violates_the_row_sum_bound():
    """y * (g - shift) with the shift rounded to float32: every element of a row carries the same error eps * |shift|, which the
    row sum collects.  Every case of more than one column has a row that violates the bound, nine rows in ten do, the median row by
    about an order of magnitude (measured: 9 times the bound, up to 67 times); a row passes only when its shift happens to round
    well."""
    excess = []
    for c in R.SOFTMAX_BWD_CASES:
        if c.cols > 1:
            excess += list(R.row_sum_excess(R.softmax_bwd_inputs(c.name)[3]))
    excess = np.asarray(excess)
    assert len(excess) >= 40
    print("float32-shift row-sum excess / bound: median %.3g, max %.3g, violating %d of %d" % (
        np.median(excess) / R.ROW_SUM_BOUND, excess.max() / R.ROW_SUM_BOUND, (excess > R.ROW_SUM_BOUND).sum(), len(excess)))
    assert np.median(excess) >= 5 * R.ROW_SUM_BOUND and excess.max() >= 30 * R.ROW_SUM_BOUND
    assert (excess > R.ROW_SUM_BOUND).mean() >= 0.9
    for c in R.SOFTMAX_BWD_CASES:                     # and every case of more than one column has a row that shows it
        if c.cols > 1:
            assert R.row_sum_excess(R.softmax_bwd_inputs(c.name)[3]).max() > R.ROW_SUM_BOUND, c.name


# ---- LayerNorm ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ids_of(R.LAYERNORM_CASES))
def test_layernorm_case(name):
    c = R.LAYERNORM_BY_NAME[name]
    x, w, b, g, xhat32, rstd32 = R.layernorm_inputs(name)
    assert x.shape == g.shape == xhat32.shape == (c.rows, c.cols) and w.shape == b.shape == (c.cols,) and rstd32.shape == (c.rows,)
    assert np.all((w >= 0.5) & (w <= 1.5)) and np.all(np.abs(b) <= 1) and np.all(np.abs(g) <= 1)
    ref = R.layernorm_reference(x, w, b, np.float64)
    np32 = R.layernorm_reference(x, w, b, np.float32)
    dx_ref = R.layernorm_bwd_reference(g, w, xhat32, rstd32, np.float64)
    dx32 = R.layernorm_bwd_reference(g, w, xhat32, rstd32, np.float32)
    assert all(a.dtype == np.float32 for a in np32) and dx32.dtype == np.float32
    if c.kind == "const" or c.cols == 1:
        # mean and deviations are exact: xhat is 0, y is beta, bit for bit, in float32 as in float64
        assert np.all(ref[1] == 0) and np.all(np32[1] == 0)
        np.testing.assert_array_equal(np32[0], np.broadcast_to(b, x.shape))
        np.testing.assert_array_equal(ref[2], 1 / np.sqrt(R.LN_EPS))
        assert np.all(dx_ref == 0) or c.kind == "const"
        return
    pairs = [(np32[0], ref[0]), (np32[1], ref[1]), (np32[2][:, None], ref[2][:, None]), (dx32, dx_ref)]
    for k, (a32, a64) in enumerate(pairs):
        assert R.row_distances(a32, a64).max() <= R.COMPOSITE_CAP, (name, k, R.row_distances(a32, a64).max())
        assert np.all(R.row_bounds(a32, a64) == R.FLOOR)


# ---- LayerNorm parameter gradients ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ids_of(R.PARAM_GRAD_CASES))
def test_param_grad_case_stays_exact(name):
    c = R.PARAM_GRAD_BY_NAME[name]
    g, xhat, dw0, db0, dw, db = R.param_grad_inputs(name)
    for a, lim in ((g, 4), (xhat, 3), (dw0, 8), (db0, 8)):
        assert a.dtype == np.float32 and np.all(a == np.rint(a)) and np.abs(a).max() <= lim
    assert g.shape == xhat.shape == (c.rows, c.cols) and dw.shape == db.shape == (c.cols,)
    assert c.rows * 12 + 8 <= R.EXACT_LIMIT                         # the worst case of any partial sum in any order, prefill on top
    assert np.abs(g * xhat).astype(np.int64).sum(0).max() + 8 <= R.EXACT_LIMIT
    for acc_w, acc_b in R.FLAG_COMBINATIONS:
        ew, eb = R.param_grad_expected(name, acc_w, acc_b)
        np.testing.assert_array_equal(ew - dw, dw0 if acc_w else 0)
        np.testing.assert_array_equal(eb - db, db0 if acc_b else 0)
    # the plan the case names covers the rows: `splits` chunks of `chunk` rows, the last one not empty
    assert c.splits >= 1 and (c.splits - 1) * c.chunk < c.rows <= c.splits * c.chunk


def test_param_grad_plans_have_ragged_last_chunks_and_every_fold_tail():
    ragged = [c.name for c in R.PARAM_GRAD_CASES if c.splits > 1 and c.rows % c.chunk]
    assert len({R.PARAM_GRAD_BY_NAME[n].rows for n in ragged}) >= 3, ragged
    assert {c.splits % 4 for c in R.PARAM_GRAD_CASES if c.splits > 1} >= {0, 2, 3}           # the fold takes four splits at a time
    assert {c.cols % 256 for c in R.PARAM_GRAD_CASES} >= {0, 1, 255}                          # full, nearly empty and nearly full last block
    assert {c.rows for c in R.PARAM_GRAD_CASES} >= {63, 64, 65}                                  # both sides of the first split


# ---- scatter-add and gather ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ids_of(R.SCATTER_CASES))
def test_scatter_case(name):
    c = R.SCATTER_BY_NAME[name]
    ids, grad, table0, ref, np32 = R.scatter_inputs(name)
    assert ids.shape == (c.n_ids,) and ids.dtype == np.int64 and grad.shape == (c.n_ids, c.row_len) and table0.shape == ref.shape == (c.table_rows, c.row_len)
    in_range = (ids >= -c.table_rows) & (ids < c.table_rows)
    assert (~in_range).sum() == (1 if c.bad else 0)
    assert np.array_equal(ids.astype(np.int32), ids)
    occ = R.occurrences(ids, c.table_rows)
    assert occ.sum() == c.n_ids - (1 if c.bad else 0)
    kind, _, arg = c.pattern.partition(":")
    where = np.flatnonzero(np.where(ids < 0, ids + c.table_rows, ids) == (c.table_rows - 1 if kind == "alias" else R.HOT))
    if kind == "adjacent":
        assert occ[R.HOT] == int(arg) == len(where) and where[-1] - where[0] == int(arg) - 1 and np.sort(occ)[-2] <= 1
    elif kind == "spread":
        assert np.all(np.diff(where) == int(arg)) and int(arg) > 256 and len(where) == occ[R.HOT] >= 8 and len(where) <= 32
    elif kind == "cluster":
        assert len(where) == 42 and where[1] - where[0] > 256 and where[2] - where[1] > 256 and where[-1] - where[2] == 39
    elif kind == "alias":
        assert len(where) == int(arg) and (ids[where] == -1).sum() == (ids[where] == c.table_rows - 1).sum() == int(arg) // 2
    elif kind == "distinct":
        assert occ.max() == 1
    elif kind == "equal":
        assert occ[R.HOT] == c.n_ids
    elif kind == "negative":
        assert (ids < 0).sum() == c.n_ids // 2 and occ.max() == 1
    if c.real:
        assert (occ.max() <= 32) == c.exact_bits
        assert R.row_distances(np32, ref).max() <= R.COMPOSITE_CAP
        assert np.all(R.row_bounds(np32, ref) == R.FLOOR)
        untouched = occ == 0
        np.testing.assert_array_equal(np32[untouched], table0[untouched])
    else:
        for a in (grad, table0):
            assert np.all(a == np.rint(a)) and np.abs(a).max() <= 8
        assert 8 * (c.n_ids + 1) <= R.EXACT_LIMIT
        np.testing.assert_array_equal(np32, ref)                    # float32 np.add.at is exact here too


def test_scatter_table_holds_every_occurrence_count_and_both_sides_of_the_chunk():
    hot = {}
    for c in R.SCATTER_CASES:
        if not c.real and not c.bad:
            hot.setdefault(c.path, set()).add(int(R.occurrences(R.scatter_inputs(c.name)[0], c.table_rows).max()))
    assert hot[R.SCATTER_CHUNKED] >= {1, 2, 31, 32, 33, 64, 65, 700, 4096}, hot
    assert hot[R.SCATTER_ATOMIC] >= {1, 65, 700, 4097}, hot
    assert {c.n_ids for c in R.SCATTER_CASES if c.bad} == {33, 4097}


@pytest.mark.parametrize("name", ids_of(R.GATHER_CASES))
def test_gather_case(name):
    c = R.GATHER_BY_NAME[name]
    ids, table = R.gather_inputs(name)
    assert np.all((ids >= -c.table_rows) & (ids < c.table_rows)) and (ids < 0).any() and table.shape == (c.table_rows, c.row_len)
    assert len(np.unique(table)) > table.size // 2                # rows tell each other apart


def test_weight_gradient_products_of_the_queued_forms_are_exact():
    for i, (k, m, n) in enumerate(R.WGRAD_SHAPES):
        g, x, ref = R.wgrad_inputs(i)
        assert g.shape == (k, m) and x.shape == (k, n) and ref.shape == (m, n) and 4 * k <= R.EXACT_LIMIT
        assert m % 4 == 0 and n % 4 == 0                             # vector loads: the form a bracket queues
