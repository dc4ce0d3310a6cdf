"""What tests/test_hip_reduce.py relies on, checked on the host: the case table of tests/reduce_cases.py keeps its exact
sums exact, its real-valued inputs harmless to numpy's own float32 sum, its views inside their arrays and its sizes small."""
import numpy as np
import pytest
import reduce_cases as R

IDS = [c.name for c in R.CASES]


@pytest.mark.parametrize("name", IDS)
def test_case_is_well_formed(name):
    c = R.BY_NAME[name]
    assert c.family in R.FAMILIES and len(c.shape) == len(c.strides) <= 8 and len(set(c.axes)) == len(c.axes)
    assert 0 < c.backing <= R.MAX_ELEMENTS
    assert all(s >= 1 for s in c.shape) and all(st >= 0 for st in c.strides)
    last = c.offset + sum((s - 1) * st for s, st in zip(c.shape, c.strides))
    assert 0 <= c.offset <= last < c.backing, "the view leaves its backing array"
    # element() and row() agree with the view
    flat = np.arange(c.backing, dtype=np.int64)
    v = c.view(flat)
    rng = c.rng("wellformed")
    for _ in range(4):
        o, r = int(rng.randint(c.n_out)), int(rng.randint(c.rlen))
        assert c.element(o, r) in v[c.row(o)].reshape(-1)
        assert v[c.row(o)].reshape(-1)[r] == c.element(o, r)


@pytest.mark.parametrize("name", IDS)
def test_exact_case_stays_exact_in_float32(name):
    c = R.BY_NAME[name]
    flat, out0, ref = R.exact_inputs(name)
    assert c.vmax >= 1 and c.vmax * c.rlen <= R.EXACT_LIMIT
    assert np.all(flat != 0) and np.all(flat == np.rint(flat)) and np.abs(flat).max() <= c.vmax
    assert ref.shape == c.kept_shape == out0.shape
    # with the accumulate pre-fill on top every value the kernel may form is still an exactly representable integer
    assert np.abs(c.view(flat).astype(np.int64)).sum(axis=c.axes).max() <= R.EXACT_LIMIT
    assert np.abs(ref).max() + np.abs(out0).max() <= R.EXACT_LIMIT


@pytest.mark.parametrize("name", IDS)
def test_numpy_float32_sum_of_the_real_case_is_close_to_float64(name):
    """so that the 1e-5 floor measures the kernel, not the inputs"""
    _, ref64, np32, _, _ = R.real_inputs(name)
    e = R.rel_frobenius(np32, ref64)
    assert e <= R.NUMPY32_CAP, e
    assert R.sum_bound(name) == R.FLOOR


def test_table_covers_every_family_and_names_are_unique():
    assert {c.family for c in R.CASES} == set(R.FAMILIES)
    assert len({c.name for c in R.CASES}) == len(R.CASES)
    assert sum(c.backing for c in R.CASES) <= 16 << 20


@pytest.mark.parametrize("name", ["split_5x700000", "tile_1000x192", "cols_650x10", "wave_7x10"])
def test_boundary_positions_and_variants(name):
    c = R.BY_NAME[name]
    splits = c.want.get("splits", 1)
    pos = R.boundary_positions(c, splits)
    assert pos[0] == 0 and pos[-1] == c.rlen - 1 and len(set(pos)) == len(pos)
    if splits > 1:
        piece = -(-c.rlen // splits)
        assert piece - 1 in pos and piece in pos
    base = R.real_inputs(name)[0]
    for tag, flat in R.extremum_variants(name):
        assert flat.shape == base.shape and not np.array_equal(flat, base, equal_nan=True), tag
