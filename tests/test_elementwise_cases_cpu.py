"""What tests/test_hip_elementwise.py relies on, checked on the host: the case table of tests/elementwise_cases.py is small, every
path family holds every arity class, the scalar operand in every slot and an in-place case, every view stays inside its payload, no
output view writes an element twice, the references have the views' shapes, the conditions of the `close` class hold for numpy's
own float32 results, and the overlap expressions mean on CpuTensor what they mean in numpy."""
import numpy as np
import pytest
import elementwise_cases as E


def test_names_are_unique_and_the_table_is_small():
    names = [c.name for c in E.SWEEP_CASES]
    assert len(set(names)) == len(names)
    assert len(names) + len(E.OPS) < E.MAX_CASES, len(names)
    total = 0
    for c in E.SWEEP_CASES:
        for v in [v for v in c.ins if v is not None] + [v for v in c.outs if not isinstance(v, int)]:
            assert 0 < v.size + 2 * E.GUARD <= E.MAX_ELEMENTS, c.name
            total += v.size + 2 * E.GUARD
    assert E.VALUE_N + 2 * E.GUARD <= E.MAX_ELEMENTS
    assert len(E.OPS) == 31 and len({v[0] for v in E.OPS.values()}) == 31
    assert {v[1:3] for v in E.OPS.values()} == E.ARITY_CLASSES == {E.OPS[op][1:3] for op in E.SWEEP_OPS}
    print("elementwise-cases %d cases, %d elements" % (len(names), total))


def test_every_family_has_its_arity_classes_scalar_slots_and_in_place_case():
    for family, label in E.FAMILIES.items():
        cases = [c for c in E.SWEEP_CASES if c.family == family]
        assert cases, label
        assert {E.OPS[c.op][1:3] for c in cases} == E.ARITY_CLASSES, label
        slots = {i for c in cases for i, v in enumerate(c.ins) if v is None}
        assert slots == {0, 1, 2, 3}, (label, slots)
        assert any(E.in_place_slots(c) for c in cases), label
        for c in cases:
            assert c.plan[0] == family and len(c.plan) == 4
            assert sum(v is None for v in c.ins) <= 1 and any(v is not None for v in c.ins), c.name
    tiles = {c.plan[1] for c in E.SWEEP_CASES if c.family == E.TILE}
    assert tiles == {E.TILE_SCALAR, E.TILE_V4_ONE, E.TILE_V4_TWO}                     # the 128 x 128 tile: see the module docstring
    assert {c.plan[1] for c in E.SWEEP_CASES if c.family == E.FLAT} == {E.VEC, E.TAIL, E.VEC | E.TAIL}
    assert {c.shape[0] for c in E.SWEEP_CASES if c.family == E.FLAT and len(c.shape) == 1} >= set(E.FLAT_FORM)
    assert max(c.plan[2] for c in E.SWEEP_CASES) == 8


@pytest.mark.parametrize("name", [c.name for c in E.SWEEP_CASES])
def test_sweep_case(name):
    c = E.SWEEP_BY_NAME[name]
    nin, nout = E.OPS[c.op][1:3]
    ins, ref32, ref64 = E.sweep_arrays(name)
    assert len(ins) == nin and len(ref32) == len(ref64) == nout
    for i, v in enumerate(c.ins):
        if v is None:
            assert ins[i] is None
            continue
        assert len(v.strides) == len(c.shape) and ins[i].shape == c.shape and ins[i].dtype == np.float32
        idx = E.element_index(v, c.shape)
        assert idx.shape == c.shape and idx.min() >= 0 and idx.max() < v.size, "input %d leaves its payload" % i
        flat = E.input_buffer(c, i)
        assert flat.shape == (v.size + 2 * E.GUARD,) and np.isnan(E.guards_of(flat)).all()
        np.testing.assert_array_equal(flat[E.GUARD + idx], ins[i])                    # the view reads back what was meant
        assert np.isnan(flat).sum() == flat.size - np.unique(idx).size                # NaN wherever the view does not reach
    for o in range(nout):
        v = E.out_view(c, o)
        idx = E.element_index(v, c.shape)
        assert idx.min() >= 0 and idx.max() < v.size, "output %d leaves its payload" % o
        assert np.unique(idx).size == idx.size, "output %d writes an element twice" % o
        assert ref32[o].shape == ref64[o].shape == c.shape and ref32[o].dtype == np.float32 and ref64[o].dtype == np.float64
        assert np.isfinite(ref32[o]).all() and np.isfinite(ref64[o]).all()
        pre, want = E.output_buffers(c, o)
        assert pre.shape == want.shape == (v.size + 2 * E.GUARD,)
        np.testing.assert_array_equal(E.guards_of(want), np.full(2 * E.GUARD, E.SENTINEL, np.float32))
        np.testing.assert_array_equal(want[E.GUARD + idx], ref32[o])
        outside = np.ones(pre.size, bool)
        outside[E.GUARD + idx] = False
        assert np.all(pre[outside] == E.SENTINEL) and np.all(want[outside] == E.SENTINEL)
        if isinstance(c.outs[o], int):
            np.testing.assert_array_equal(pre[E.GUARD + idx], ins[c.outs[o]])         # in place: the output starts as its input
        else:
            assert np.isnan(pre[E.GUARD + idx]).all()
    # float32 numpy is within the rule's floor of float64 here: the exact ops are one to three roundings from it
    bad, kept, dist, bound = E.close_violations(ref32[0], ref64[0], ref32[0])
    assert kept.all() and not bad.any()
    if c.op == "max_bwd":
        assert 0 < np.count_nonzero(ref32[0]) < ref32[0].size or ref32[0].size < 16    # ties and non-ties both occur


def test_sweep_inputs_tell_operands_apart():
    """swapped operands, a transposed index or a dropped broadcast change the result of every sweep op"""
    for op in E.SWEEP_OPS:
        if E.OPS[op][1] < 2:
            continue
        rng = E.rng_for("swap_" + op)
        ins = [(rng.randint(0, 3, 64) if op == "max_bwd" else rng.uniform(0.5, 2, 64)).astype(np.float32) for _ in range(E.OPS[op][1])]
        base = E.evaluate(op, ins, np.float32)
        for i in range(len(ins) - 1):
            swapped = list(ins)
            swapped[i], swapped[i + 1] = swapped[i + 1], swapped[i]
            other = E.evaluate(op, swapped, np.float32)
            if op in ("fma", "max_bwd") and i == 0:
                continue                                                             # a * b + c and g * (x == m) are symmetric in their first two
            assert any(not np.array_equal(x, y) for x, y in zip(base, other)), (op, i)


@pytest.mark.parametrize("op", list(E.OPS))
def test_value_case(op):
    nin, nout, klass = E.OPS[op][1:]
    ins = E.value_inputs(op)
    ref32, ref64 = E.value_references(op)
    assert len(ins) == nin and all(a.shape == (E.VALUE_N,) and a.dtype == np.float32 for a in ins)
    assert len(ref32) == len(ref64) == nout and all(a.shape == (E.VALUE_N,) for a in ref32 + ref64)
    a = ins[0]
    assert np.isnan(a).any() and np.isposinf(a).any() and (a == 0).any() and np.signbit(a[a == 0]).any()
    if op not in ("pow", "pow_bwd", "div_bwd"):
        for v in (E.DENORMAL, E.TINY, E.HUGE):
            assert (a == np.float32(v)).any() or v in E.NOT_PAIRED.get(op, ()), (op, v)
        assert np.isneginf(a).any() and (a == 1).any() and (a == -1).any()
    if op in ("exp", "sigmoid"):
        assert {88.7, -88.7, 87.3, -87.3, -104.0} <= {round(float(v), 1) for v in a[:len(E.COMMON)] if np.isfinite(v) and abs(v) < 200}
    if op in ("sin", "cos", "sin_bwd", "cos_bwd"):
        assert (a == 1e4).any() and (a == 1e6).any()
    if op in ("tanh", "sigmoid", "gelu", "gelu_bwd"):
        assert (a == 20).any() and (a == -20).any()
    if op == "gelu_bwd":
        random = a[(len(E.COMMON) - len(E.NOT_PAIRED[op])) * len(E.GRADS):]               # behind the special values
        assert random.size > E.VALUE_N // 2 and np.all(np.abs(random) <= 2.25) and E.gelu_slope(random).min() >= E.GELU_SLOPE_MIN
    if op == "log":
        assert (a == np.float32(1 - 2.0 ** -24)).any() and (a == np.float32(1 + 2.0 ** -23)).any() and (a < 0).any()
    if op == "pow":
        b = ins[1]
        assert ((a == 0) & (b == 0)).any() and (np.isinf(a) & (b == 0)).any()
        assert ((a < 0) & (b == np.rint(b)) & np.isfinite(b) & np.isfinite(a)).any() and ((a < 0) & (b != np.rint(b)) & np.isfinite(b)).any()
        assert np.isnan(ref64[0][(a == -2.5) & (b == 0.5)]).all() and np.all(ref64[0][(a == 0) & (b == 0)] == 1)
    if klass == "exact":
        for r32, r64 in zip(ref32, ref64):
            # every exact op is a composition of correctly rounded operations: float32 numpy IS the reference
            assert r32.dtype == np.float32 and r64.dtype == np.float64
        if nin == 1 or op in ("add", "sub", "mul", "div"):
            sub = np.abs(ref32[0][np.isfinite(ref32[0])])
            assert ((sub > 0) & (sub < np.float32(E.TINY))).any() or op in ("relu", "sqrt"), "no denormal result"
        return
    for o, (r32, r64) in enumerate(zip(ref32, ref64)):
        bad, kept, dist, bound = E.close_violations(r32, r64, r32)
        left = int((~kept).sum())
        print("elementwise-value %-12s output %d: %d of %d elements leave" % (op, o, left, kept.size))
        assert left <= E.LEAVE_CAP * kept.size, (op, o, left)
        assert not bad.any(), (op, o, np.flatnonzero(bad)[:8])                        # numpy float32 itself satisfies the rule
        assert (~np.isfinite(r64)).any() and np.isfinite(r64[kept]).sum() > 0.9 * kept.size


def test_the_rule_catches_what_it_should():
    ref = np.float64([1.0, 1.0, np.inf, np.nan, 0.0, 1e-40, 1e39, -np.inf])
    with np.errstate(over="ignore"):
        np32 = ref.astype(np.float32)
    for got, want_bad in (([1.0, 1.0, np.inf, np.nan, 0.0, 0.0, np.inf, -np.inf], []),
                          ([1.00002, 1.0, np.inf, np.nan, 0.0, 5.0, 7.0, -np.inf], [0]),
                          ([1.0, 1.0, -np.inf, 1.0, 1e-45, 0.0, 0.0, np.inf], [2, 3, 4, 7]),
                          ([np.nan, np.inf, np.nan, np.inf, np.nan, 0.0, 0.0, np.nan], [0, 1, 2, 3, 4, 7])):
        bad, kept, _, _ = E.close_violations(np.float64(got), ref, np32)
        assert list(np.flatnonzero(bad)) == want_bad and list(np.flatnonzero(~kept)) == [5, 6]


# ---- the overlap expressions on the CPU backend ------------------------------------------------------------------------------------

def test_overlap_expressions_on_the_cpu_backend_equal_numpy():
    """what tests/test_hip_elementwise.py expects of HipTensor is numpy's answer - the right-hand side first - and CpuTensor gives it"""
    import lightgrad_amd as light
    from lightgrad_amd import CpuTensor
    rng = E.rng_for("overlap_cpu")
    for n in (12, 128, 130):
        for op in ("__iadd__", "__isub__", "__imul__"):
            x = rng.uniform(-2, 2, (n, n)).astype(np.float32)
            t = CpuTensor.from_numpy(x.copy())
            with light.no_grad():
                getattr(t, op)(t.transpose(1, 0))
            getattr(x, op)(x.T)
            np.testing.assert_array_equal(t.numpy(), x)
    for dtype in (np.float32, np.int32, np.float64, np.uint8):
        x = rng.randint(0, 200, 5000).astype(dtype)
        t = CpuTensor.from_numpy(x.copy())
        with light.no_grad():
            t[1:] += t[:-1]
            t[:-1] += t[1:]
            t -= t[::-1]
            t[1:] = t[:-1]
        x[1:] += x[:-1]
        x[:-1] += x[1:]
        x -= x[::-1]
        x[1:] = x[:-1]
        np.testing.assert_array_equal(t.numpy(), x)
        y = rng.randint(0, 200, (33, 65)).astype(dtype)
        u = CpuTensor.from_numpy(y.copy())
        with light.no_grad():
            u[:, 1:] = u[:, :-1]
        y[:, 1:] = y[:, :-1]
        np.testing.assert_array_equal(u.numpy(), y)
        # the answer IS "the right-hand side first"
        z = rng.randint(0, 200, 64).astype(dtype)
        w = z.copy()
        w[1:] += z[:-1]
        v = z.copy()
        v[1:] += v[:-1]
        np.testing.assert_array_equal(v, w)
