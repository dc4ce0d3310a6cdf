"""Every float32 reduction kernel path (csrc/reduce.hip) against exact references, through the raw C ABI and the tape.

The cases, their inputs and references are tests/reduce_cases.py (checked on the host by tests/test_reduce_cases_cpu.py).
After every call the plan `lg_reduce_last_plan` reports is compared with the kernel - and split / group counts - the case is
meant for: when a retuned threshold moves a case to another kernel the assertion fails and the SHAPE is to be adjusted.
Sums of the integer inputs must equal numpy's int64 sum bit for bit (no tolerance: one dropped, doubled or misplaced element
fails at any size), real-valued sums are judged against float64 by the rule of tests/common.py and must repeat bit for bit,
max / min must equal numpy exactly, NaN and infinities included."""
import ctypes
import numpy as np
import pytest
import reduce_cases as R

pytestmark = pytest.mark.gpu

FAMILY_IDS = list(R.FAMILIES)
_device = {}          # (kind, case name) -> flat device tensor: uploaded once, left unchanged


@pytest.fixture(scope="module")
def L(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    hiplib.lib()
    return hiplib


def on_device(hip, kind, name):
    key = (kind, name)
    if key not in _device:
        flat = (R.exact_inputs if kind == "exact" else R.real_inputs)(name)[0]
        _device[key] = hip.from_numpy(flat, requires_grad=False)
    return _device[key]


def last_plan(L):
    p = (ctypes.c_int32 * 6)()
    L.check(L.lib().lg_reduce_last_plan(p))
    return tuple(p)


def reduce_raw(L, op, case, src, out, accumulate=None):
    """lg_reduce (accumulate None) or lg_reduce_acc on the case's view of the flat device tensor `src`; returns the plan"""
    ptr = src.ptr + 4 * case.offset
    args = (op, len(case.shape), L.i64(case.shape), ptr, L.i64(case.strides), case.mask, out.ptr)
    if accumulate is None:
        L.check(L.lib().lg_reduce(*args))
    else:
        L.check(L.lib().lg_reduce_acc(*(args + (accumulate,))))
    return last_plan(L)


def assert_plan(case, plan):
    kernel, splits, groups, nk, nr, vec = plan
    assert kernel == R.FAMILIES[case.family], "%s is meant for %s, the library ran kernel %d (plan %s): adjust the shape" % (
        case.name, case.family, kernel, plan)
    got = {"splits": splits, "splits_gt": None, "groups": groups, "splits_mod_32": splits % 32, "nk": nk, "nr": nr, "vec": vec}
    for key, value in case.want.items():
        if key == "splits_gt":
            assert splits > value, (case.name, plan)
        else:
            assert got[key] == value, (case.name, key, value, plan)
    assert splits >= 1 and (groups >= 1) == (kernel == R.ROWS_SPLIT and splits > 1), (case.name, plan)


@pytest.mark.parametrize("family", FAMILY_IDS)
def test_integer_sums_are_exact_with_and_without_accumulate(hip, L, family):
    for c in R.family(family):
        _, out0, ref = R.exact_inputs(c.name)
        src = on_device(hip, "exact", c.name)
        for accumulate, want in ((None, ref), (0, ref), (1, ref + out0.astype(np.int64))):
            out = hip.from_numpy(out0, requires_grad=False)               # overwritten unless accumulate == 1
            assert_plan(c, reduce_raw(L, L.RED_SUM, c, src, out, accumulate))
            got = out.numpy()
            assert got.shape == c.kept_shape
            np.testing.assert_array_equal(got.astype(np.float64), want.astype(np.float64),
                                          err_msg="%s accumulate=%s (%s)" % (c.name, accumulate, c.feature))


@pytest.mark.parametrize("family", FAMILY_IDS)
def test_real_sums_against_float64_and_bit_reproducible(hip, L, family):
    for c in R.family(family):
        _, ref64, np32, _, _ = R.real_inputs(c.name)
        src = on_device(hip, "real", c.name)
        outs = []
        for _ in range(2):
            out = hip.empty(c.kept_shape, requires_grad=False)
            plan = reduce_raw(L, L.RED_SUM, c, src, out)
            assert_plan(c, plan)
            outs.append(out.numpy())
        e, e_np = R.rel_frobenius(outs[0], ref64), R.rel_frobenius(np32, ref64)
        print("reduce-distance %-26s kernel %d splits %3d: %.3g from float64 (numpy float32 %.3g)" % (c.name, plan[0], plan[1], e, e_np))
        assert e <= R.sum_bound(c.name), "%s: %.3g from the float64 sum, numpy's float32 sum %.3g" % (c.name, e, e_np)
        assert outs[0].tobytes() == outs[1].tobytes(), "%s: two runs of the same sum differ" % c.name


def _poke(L, src, element, value):
    v = ctypes.c_float(value)
    L.check(L.lib().lg_memcpy_h2d(src.ptr + 4 * element, ctypes.addressof(v), 4))


@pytest.mark.parametrize("family", FAMILY_IDS)
def test_max_min_equal_numpy(hip, L, family):
    """the real-valued inputs; on every path that hands partials between workgroups also the unique extremum planted at each
    boundary position in turn, a row of ties, and NaN / infinities (NaN reaches its own output only, as np.max has it)"""
    ops = ((L.RED_MAX, np.max, 2.0), (L.RED_MIN, np.min, 0.125))            # (op, numpy, a value beyond uniform(0.25, 1))
    for c in R.family(family):
        base, _, _, ref_max, ref_min = R.real_inputs(c.name)
        src = on_device(hip, "real", c.name)
        out = hip.empty(c.kept_shape, requires_grad=False)
        for (op, _, _), ref in zip(ops, (ref_max, ref_min)):
            plan = reduce_raw(L, op, c, src, out)
            assert_plan(c, plan)
            np.testing.assert_array_equal(out.numpy(), ref, err_msg=c.name)
        if plan[1] == 1:
            continue
        work = base.copy()
        for k, r in enumerate(R.boundary_positions(c, plan[1])):
            e = c.element(k % c.n_out, r)
            for op, np_fn, value in ops:
                work[e] = value
                _poke(L, src, e, value)
                try:
                    reduce_raw(L, op, c, src, out)
                    got = out.numpy()
                finally:
                    _poke(L, src, e, float(base[e]))
                np.testing.assert_array_equal(got, np_fn(c.view(work), axis=c.axes), err_msg="%s: extremum planted at %d of output %d" % (
                    c.name, r, k % c.n_out))
                work[e] = base[e]
        for tag, flat in R.extremum_variants(c.name):
            dev = hip.from_numpy(flat, requires_grad=False)
            for op, np_fn, _ in ops:
                assert_plan(c, reduce_raw(L, op, c, dev, out))
                np.testing.assert_array_equal(out.numpy(), np_fn(c.view(flat), axis=c.axes), err_msg="%s: %s" % (c.name, tag))


def test_calls_that_launch_nothing(hip, L):
    lib = L.lib()
    dummy = hip.from_numpy(np.full(4, 7, np.float32), requires_grad=False)
    shape, axis = R.EMPTY_OUTPUT                                             # no output elements
    args = lambda op, sh, ax: (op, len(sh), L.i64(sh), dummy.ptr, L.i64(R.contiguous(sh)), 1 << ax, dummy.ptr)   # noqa: E731
    L.check(lib.lg_reduce(*args(L.RED_SUM, shape, axis)))
    assert last_plan(L)[0] == R.NONE
    np.testing.assert_array_equal(dummy.numpy(), 7)
    shape, axis = R.EMPTY_REDUCTION                                          # a sum over nothing: zeros, or `out` left alone
    L.check(lib.lg_reduce_acc(*(args(L.RED_SUM, shape, axis) + (1,))))
    assert last_plan(L)[0] == R.NONE
    np.testing.assert_array_equal(dummy.numpy(), 7)
    reduce_raw(L, L.RED_SUM, R.BY_NAME["wave_7x10"], on_device(hip, "exact", "wave_7x10"), hip.empty((7,)))
    assert last_plan(L)[0] == R.ROWS_WAVE                                    # the report follows the most recent call
    L.check(lib.lg_reduce(*args(L.RED_SUM, shape, axis)))
    assert last_plan(L)[0] == R.NONE
    np.testing.assert_array_equal(dummy.numpy(), 0)
    for op in (L.RED_MAX, L.RED_MIN):                                        # no identity: refused
        assert lib.lg_reduce(*args(op, shape, axis)) == -1
        assert b"zero-size" in lib.lg_last_error() and last_plan(L)[0] == R.NONE
    assert lib.lg_reduce_last_plan(None) == -1


def _sweep(hip, L, cases):
    plans = {}
    for c in cases:
        _, out0, ref = R.exact_inputs(c.name)
        out = hip.from_numpy(out0, requires_grad=False)
        plans[c.name] = reduce_raw(L, L.RED_SUM, c, on_device(hip, "exact", c.name), out)
        assert_plan(c, plans[c.name])
        np.testing.assert_array_equal(out.numpy().astype(np.float64), ref.astype(np.float64), err_msg=c.name)
    return plans


def test_table_reaches_every_kernel_and_fold_variant(hip, L):
    plans = _sweep(hip, L, R.CASES)
    seen = {}
    for kernel, splits, groups, nk, nr, vec in plans.values():
        s = seen.setdefault(kernel, {"one": False, "many": False, "short_group": False, "full_groups": False, "vec": set()})
        s["one" if splits == 1 else "many"] = True
        s["vec"].add(vec)
        if kernel == R.ROWS_SPLIT and groups > 1:
            s["short_group" if splits % 32 else "full_groups"] = True
    assert sorted(seen) == [R.ROWS_WAVE, R.ROWS_SPLIT, R.COLS_TILE, R.COLS], seen
    for kernel in (R.COLS_TILE, R.COLS):
        assert seen[kernel]["one"] and seen[kernel]["many"], (kernel, seen[kernel])
    assert seen[R.ROWS_SPLIT]["many"] and seen[R.ROWS_SPLIT]["short_group"] and seen[R.ROWS_SPLIT]["full_groups"], seen[R.ROWS_SPLIT]
    for kernel in (R.ROWS_WAVE, R.ROWS_SPLIT):
        assert seen[kernel]["vec"] == {0, 1}, (kernel, seen[kernel])
    print("reduce-coverage", {k: {n: (sorted(v) if isinstance(v, set) else v) for n, v in s.items()} for k, s in sorted(seen.items())})


def test_tickets_are_left_at_zero_for_the_split_k_consumers(hip, L):
    """the whole table forward, then in reverse order, then two in-launch folds that count in the same ticket pool - a row-sum
    product with a split K and the mean of a cross-entropy over vocabulary-sized rows - against float64: a ticket a reduction
    left non-zero makes their last workgroup miss its turn"""
    from lightgrad_amd.autograd.hip import ops as H
    _sweep(hip, L, R.CASES)
    _sweep(hip, L, R.CASES[::-1])
    for M, K, N in [(10, 1024, 512), (128, 2048, 128)]:
        rng = np.random.RandomState(M + 13 * K + 101 * N)
        a, b = rng.uniform(-1, 1, (M, K)).astype(np.float32), rng.uniform(-1, 1, (K, N)).astype(np.float32)
        out, rs = H._gemm_fused(hip.from_numpy(a), hip.from_numpy(b), want_rowsum=True)
        ref = a.astype(np.float64) @ b.astype(np.float64)
        assert R.rel_frobenius(out.numpy(), ref) <= 1e-5, (M, K, N)
        np.testing.assert_allclose(rs.numpy(), a.astype(np.float64).sum(1), rtol=1e-5, atol=1e-6 * K ** 0.5 * 4)
    rng = np.random.RandomState(5)
    n, c = 5, 4096
    logits, labels = rng.uniform(-8, 8, (n, c)).astype(np.float32), rng.randint(0, c, n).astype(np.int64)
    loss, dlogits = H.cross_entropy_forward(hip.from_numpy(logits), hip.from_numpy(labels, requires_grad=False))
    x = logits.astype(np.float64)
    x = x - x.max(1, keepdims=True)
    logp = x - np.log(np.exp(x).sum(1, keepdims=True))
    want_grad = np.exp(logp)
    want_grad[np.arange(n), labels] -= 1
    np.testing.assert_allclose(loss.item(), -logp[np.arange(n), labels].mean(), rtol=1e-5)
    assert R.rel_frobenius(dlogits.numpy(), want_grad / n) <= 1e-5


# ---- through the tape ------------------------------------------------------------------------------------------------

TAPE = [("wave_9x257", 1), ("split_3x20001", 1), ("tile_1000x192", 0), ("cols_650x10", 0)]


@pytest.mark.parametrize("name,axis", TAPE)
def test_tape_sum_and_max_forward(hip, L, name, axis):
    c = R.BY_NAME[name]
    flat, _, ref = R.exact_inputs(name)
    got = hip.from_numpy(flat.reshape(c.shape)).sum(axis=axis)
    assert last_plan(L)[0] == R.FAMILIES[c.family]
    np.testing.assert_array_equal(got.numpy().astype(np.float64), ref.astype(np.float64))
    real, _, _, ref_max, ref_min = R.real_inputs(name)
    t = hip.from_numpy(real.reshape(c.shape))
    np.testing.assert_array_equal(t.max(axis=axis).numpy(), ref_max)
    assert last_plan(L)[0] == R.FAMILIES[c.family]
    np.testing.assert_array_equal(t.min(axis=axis).numpy(), ref_min)


@pytest.mark.parametrize("name,axis", [("split_3x20001", 1), ("cols_650x10", 0)])
def test_tape_max_min_gradient_with_ties(hip, L, name, axis):
    """g * (x == extremum): every tied element receives the gradient"""
    c = R.BY_NAME[name]
    rng = c.rng("ties")
    x = rng.randint(0, 40, c.shape).astype(np.float32)                      # few values: each extremum is tied many times
    w = rng.randint(-8, 9, c.kept_shape).astype(np.float32)
    for fn, np_fn in (("max", np.max), ("min", np.min)):
        t = hip.from_numpy(x)
        y = getattr(t, fn)(axis=axis)
        kernel, splits = last_plan(L)[:2]
        assert kernel == R.FAMILIES[c.family] and splits > 1, last_plan(L)
        (y * hip.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
        ext = np_fn(x, axis=axis, keepdims=True)
        assert ((x == ext).sum(axis=axis) > 1).all()
        np.testing.assert_array_equal(y.numpy(), ext.reshape(c.kept_shape))
        np.testing.assert_array_equal(t.grad.numpy(), np.expand_dims(w, axis) * (x == ext))


@pytest.mark.parametrize("name", ["tile_100x68", "tile_1000x192", "cols_650x10"])
@pytest.mark.parametrize("bias_ndim", [2, 1])
def test_tape_bias_gradient_unbroadcast_is_exact(hip, L, name, bias_ndim):
    """(x + b).backward with b of shape (1, C) and (C,): the gradient of b is the column sum of the upstream gradient"""
    c = R.BY_NAME[name]
    n, cols = c.shape
    rng = c.rng("bias%d" % bias_ndim)
    x = rng.randint(-8, 9, (n, cols)).astype(np.float32)
    b = rng.randint(-8, 9, (1, cols) if bias_ndim == 2 else (cols,)).astype(np.float32)
    w = rng.randint(-8, 9, (n, cols))
    tx, tb = hip.from_numpy(x), hip.from_numpy(b)
    ((tx + tb) * hip.from_numpy(w.astype(np.float32), requires_grad=False)).backward(allow_fill=True)
    assert last_plan(L)[0] == R.FAMILIES[c.family], last_plan(L)
    np.testing.assert_array_equal(tb.grad.numpy().astype(np.float64), w.sum(0, dtype=np.int64).reshape(b.shape).astype(np.float64))
    np.testing.assert_array_equal(tx.grad.numpy(), w.astype(np.float32))
