"""Every path edge of the elementwise dispatch (csrc/elementwise.hip) against numpy, through the raw C ABI on flat guarded
buffers, and the operands that overlap their output, through HipTensor.

The cases, their views and references are tests/elementwise_cases.py (checked on the host by tests/test_elementwise_cases_cpu.py).
After every `lg_ew` call the plan `lg_ew_last_plan` reports is compared with the plan the case names: when a retuned condition
moves a case to another kernel the assertion fails and the SHAPE is to be adjusted.  The WHOLE output buffer is compared - guards,
the gaps of pitched views and the payload together - bit for bit for the sweep (pow_bwd: by the distance rule inside its view),
so a float4 that runs past a view's end or into the gap between two rows shows.

The overlap tests: an in-place operand, or the value of an assignment, that is ANOTHER view of the storage being written.  numpy
(and so the CPU backend) answers as if the right-hand side were copied first; autograd/hip/ops.py makes that copy (`_apart_from`),
the kernels stay as they are.  `t[...]` on this backend is a copy already, so each expression is run twice: as written, and with
the views the tape's internals use (`ops._idx_view`: same storage, no copy), which is where the hazard is."""
import ctypes
import numpy as np
import pytest
import elementwise_cases as E
import lightgrad_amd as light

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    hiplib.lib()
    return hiplib


def last_plan(L):
    p = (ctypes.c_int32 * 4)()
    L.check(L.lib().lg_ew_last_plan(p))
    return tuple(p)


def assert_plan(L, name, want):
    got = last_plan(L)
    assert got == tuple(want), "%s is meant for plan %s, the library chose %s: adjust the shape" % (name, tuple(want), got)


def address(t, view):
    return t.ptr + (E.GUARD + view.offset) * 4


def same_bits(got, want, what):
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%s: %d of %d buffer elements differ, first at %d (payload starts at %d): got %r, expected %r" % (
        what, bad.size, got.size, bad[0], E.GUARD, got[bad[0]], want[bad[0]])


def assert_close(got, ref, np32, what):
    """the rule of the `close` class, per element; prints the worst element like assert_rows_close"""
    bad, kept, dist, bound = E.close_violations(got, ref, np32)
    with np.errstate(all="ignore"):                                   # the worst element: the largest share of its bound used
        share = np.where(kept, np.where(bound > 0, dist / bound, np.where(dist > 0, np.inf, 0.0)), -1.0)
    w = int(np.argmax(share))
    print("elementwise-distance %-24s worst element %d: %.3g from float64 %.9g (bound %.3g); %d of %d left out" % (
        what, w, dist.flat[w], np.asarray(ref).flat[w], bound.flat[w], (~kept).sum(), kept.size))
    assert not bad.any(), "%s: %d elements break the rule, first at %d: got %r, float64 %r, numpy float32 %r" % (
        what, bad.sum(), np.flatnonzero(bad)[0], np.asarray(got).flat[np.flatnonzero(bad)[0]], np.asarray(ref).flat[np.flatnonzero(bad)[0]],
        np.asarray(np32).flat[np.flatnonzero(bad)[0]])


def call_ew(L, op, shape, outs, ins, scalar):
    """outs / ins: (address, strides) pairs; None for the second output or the scalar operand"""
    args = []
    for p in list(outs) + [None] * (2 - len(outs)) + list(ins) + [None] * (4 - len(ins)):
        args += [None, None] if p is None else [p[0], L.i64(p[1])]
    return L.lib().lg_ew(E.OPS[op][0], len(shape), L.i64(shape), *args, scalar)


# ---- (a) the path sweep -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [c.name for c in E.SWEEP_CASES])
def test_path_sweep(hip, L, name):
    c = E.SWEEP_BY_NAME[name]
    nout = E.OPS[c.op][2]
    in_place = E.in_place_slots(c)                                    # input slot -> the output it is
    prefill, want = zip(*[E.output_buffers(c, o) for o in range(nout)])
    out_t = [hip.from_numpy(p, requires_grad=False) for p in prefill]
    outs = [(address(out_t[o], E.out_view(c, o)), E.out_view(c, o).strides) for o in range(nout)]
    ins = []
    keep = []
    for i, v in enumerate(c.ins):
        if v is None:
            ins.append(None)
        elif i in in_place:
            ins.append(outs[in_place[i]])                             # the very same view
        else:
            keep.append(hip.from_numpy(E.input_buffer(c, i), requires_grad=False))
            ins.append((address(keep[-1], v), v.strides))
    L.check(call_ew(L, c.op, c.shape, outs, ins, E.SCALAR))
    assert_plan(L, name, c.plan)
    _, ref32, ref64 = E.sweep_arrays(name)
    for o in range(nout):
        got = out_t[o].numpy()
        what = "%s output %d" % (name, o)
        if c.op != "pow_bwd":
            same_bits(got, want[o], what)
            continue
        idx = E.GUARD + E.element_index(E.out_view(c, o), c.shape)
        inside = got[idx]
        outside_got, outside_want = got.copy(), want[o].copy()
        outside_got[idx] = 0
        outside_want[idx] = 0
        same_bits(outside_got, outside_want, what + " outside the view")
        bad, kept, dist, bound = E.close_violations(inside, ref64[o], ref32[o])
        assert kept.all() and not bad.any(), "%s: %d elements break the rule, worst %.3g (bound %.3g)" % (
            what, bad.sum(), (dist - bound).max(), bound.flat[int(np.argmax(dist - bound))])


def test_calls_that_launch_nothing(hip, L):
    lib = L.lib()
    keep = hip.from_numpy(np.full(8, 7, np.float32), requires_grad=False)
    src = hip.from_numpy(np.ones(8, np.float32), requires_grad=False)
    one = (src.ptr, (1,))
    L.check(call_ew(L, "neg", (8,), [(keep.ptr, (1,))], [one], 0.0))
    assert last_plan(L) == (E.FLAT, E.VEC, 1, 1)
    L.check(call_ew(L, "neg", (0,), [(keep.ptr, (1,))], [one], 0.0))        # no elements
    assert last_plan(L) == (E.NONE, 0, 0, 0)
    L.check(call_ew(L, "neg", (8,), [(keep.ptr, (1,))], [one], 0.0))        # the report follows the most recent call
    assert last_plan(L)[0] == E.FLAT
    assert call_ew(L, "sub", (8,), [(keep.ptr, (1,))], [None, None], 0.0) == -1 and last_plan(L) == (E.NONE, 0, 0, 0)     # refused
    assert call_ew(L, "neg", (8,), [(keep.ptr, (0,))], [one], 0.0) == -1 and last_plan(L)[0] == E.NONE                    # a broadcast output
    assert lib.lg_ew_last_plan(None) == -1
    # a 4-byte strided copy reports the lg_ew launch it is; other item sizes and one dense run launch no elementwise kernel
    L.check(lib.lg_copy_strided(4, 1, L.i64((4,)), keep.ptr, L.i64((2,)), src.ptr, L.i64((1,))))
    assert last_plan(L) == (E.GATHER, 0, 1, 0)
    np.testing.assert_array_equal(keep.numpy(), np.float32([1, -1, 1, -1, 1, -1, 1, -1]))


# ---- (b) the value sweep ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("op", list(E.OPS))
def test_value_sweep(hip, L, op):
    """special values and random ones through the flat path, one case per op id.
    exact: numpy float32's result, denormals included (a flushed denormal is a finding).  close: the distance rule against float64."""
    nin, nout, klass = E.OPS[op][1:]
    ins = E.value_inputs(op)
    ref32, ref64 = E.value_references(op)
    in_t = [hip.from_numpy(E.padded(a, np.nan), requires_grad=False) for a in ins]
    out_t = [hip.from_numpy(E.padded(np.full(E.VALUE_N, np.nan, np.float32), E.SENTINEL), requires_grad=False) for _ in range(nout)]
    at = lambda t: (t.ptr + E.GUARD * 4, (1,))                        # noqa: E731
    L.check(call_ew(L, op, (E.VALUE_N,), [at(t) for t in out_t], [at(t) for t in in_t], 0.0))
    assert_plan(L, "value sweep of " + op, (E.FLAT, E.VEC, 1, (1 << nin) - 1))
    for o in range(nout):
        flat = out_t[o].numpy()
        np.testing.assert_array_equal(E.guards_of(flat), np.full(2 * E.GUARD, E.SENTINEL, np.float32), err_msg=op + ": written outside the payload")
        got = flat[E.GUARD:E.GUARD + E.VALUE_N]
        what = "%s output %d" % (op, o)
        if klass == "exact":
            np.testing.assert_array_equal(got, ref32[o], err_msg=what)
        else:
            assert_close(got, ref64[o], ref32[o], what)


# ---- operands that overlap the output -----------------------------------------------------------------------------------------------

def tensor_and_array(hip, shape, dtype=np.float32, salt=""):
    rng = E.rng_for("overlap_%s_%s%s" % (shape, np.dtype(dtype).name, salt))
    x = rng.randint(0, 200, shape).astype(dtype) if np.dtype(dtype).kind in "iu" else rng.uniform(-2, 2, shape).astype(dtype)
    return hip.from_numpy(x.copy(), requires_grad=False), x


def part(t, idx, how):
    """`t[idx]` as written (a copy on this backend), or the view the tape's internals make of it (the same storage)"""
    if how == "index":
        return t[idx]
    from lightgrad_amd.autograd.hip import ops
    return ops._idx_view(t, idx)


INPLACE = {"iadd": lambda a, b: a.__iadd__(b), "isub": lambda a, b: a.__isub__(b), "imul": lambda a, b: a.__imul__(b)}
TRANSPOSED_PLAN = {12: (E.FLAT2D, 0, 2, 0b01), 13: (E.GATHER, 0, 2, 0), 128: (E.TILE, E.TILE_V4_ONE, 2, 0b10), 130: (E.TILE, E.TILE_SCALAR, 2, 0b10)}


@pytest.mark.parametrize("op", list(INPLACE))
@pytest.mark.parametrize("n", list(TRANSPOSED_PLAN))
def test_in_place_with_its_own_transpose(hip, L, n, op):
    """t += t.transpose(1, 0): the workgroup of tile (i, j) stages tile (j, i) while another one writes it"""
    t, x = tensor_and_array(hip, (n, n))
    with light.no_grad():
        INPLACE[op](t, t.transpose(1, 0))
    assert_plan(L, "t %s t.T at %d" % (op, n), TRANSPOSED_PLAN[n])     # the copy keeps the transposed layout: the same kernel as for a foreign operand
    INPLACE[op](x, x.T)
    np.testing.assert_array_equal(t.numpy(), x)


@pytest.mark.parametrize("how", ["index", "view"])
@pytest.mark.parametrize("expr", ["up", "down", "reversed"])
def test_in_place_with_a_shifted_or_reversed_part_of_itself(hip, L, expr, how):
    t, x = tensor_and_array(hip, (5000,), salt=expr)
    lo, hi, rev = slice(None, -1), slice(1, None), slice(None, None, -1)
    with light.no_grad():
        if expr == "up":                      # t[1:] += t[:-1]
            if how == "index":
                t[hi] += t[lo]
            else:
                v = part(t, hi, how)
                v += part(t, lo, how)
            x[hi] += x[lo]
        elif expr == "down":                  # t[:-1] += t[1:]
            if how == "index":
                t[lo] += t[hi]
            else:
                v = part(t, lo, how)
                v += part(t, hi, how)
            x[lo] += x[hi]
        else:                                 # t -= t[::-1]
            t -= part(t, rev, how)
            x -= x[rev]
    np.testing.assert_array_equal(t.numpy(), x)


@pytest.mark.parametrize("how", ["index", "view"])
@pytest.mark.parametrize("dtype", [np.float32, np.int32, np.float64, np.uint8])
def test_assignment_from_a_shifted_part_of_itself(hip, L, dtype, how):
    """t[:, 1:] = t[:, :-1] (the strided copy) and t[1:] = t[:-1] on one dense run (the device-to-device memcpy branch)"""
    t, x = tensor_and_array(hip, (33, 65), dtype)
    with light.no_grad():
        t[:, 1:] = part(t, (slice(None), slice(None, -1)), how)
    x[:, 1:] = x[:, :-1]
    np.testing.assert_array_equal(t.numpy(), x)
    t, x = tensor_and_array(hip, (5000,), dtype)
    with light.no_grad():
        t[1:] = part(t, slice(None, -1), how)
    x[1:] = x[:-1]
    np.testing.assert_array_equal(t.numpy(), x)
    t, x = tensor_and_array(hip, (5000,), dtype, "down")
    with light.no_grad():
        t[:-1] = part(t, slice(1, None), how)
    x[:-1] = x[1:]
    np.testing.assert_array_equal(t.numpy(), x)


@pytest.mark.parametrize("dtype", [np.int32, np.float64])
def test_typed_in_place_with_an_overlapping_view(hip, L, dtype):
    """the same hazard through lg_ew_typed"""
    t, x = tensor_and_array(hip, (48, 48), dtype)
    with light.no_grad():
        t += t.transpose(1, 0)
    x += x.T
    np.testing.assert_array_equal(t.numpy(), x)
    t, x = tensor_and_array(hip, (5000,), dtype)
    with light.no_grad():
        v = part(t, slice(1, None), "view")
        v += part(t, slice(None, -1), "view")
    x[1:] += x[:-1]
    np.testing.assert_array_equal(t.numpy(), x)


def test_the_identical_view_takes_no_copy(hip, L):
    """control: t += t and t *= t keep the plan they have always had - the fast case is not copied"""
    from lightgrad_amd.autograd.hip import ops
    t, x = tensor_and_array(hip, (1027,))
    stats = lambda: [ctypes.c_uint64() for _ in range(3)]             # noqa: E731
    with light.no_grad():
        before = stats()
        L.check(L.lib().lg_pool_stats(*[ctypes.byref(s) for s in before]))
        t += t
        assert_plan(L, "t += t", (E.FLAT, E.VEC | E.TAIL, 1, 0b11))
        t *= t
        assert_plan(L, "t *= t", (E.FLAT, E.VEC | E.TAIL, 1, 0b11))
        after = stats()
        L.check(L.lib().lg_pool_stats(*[ctypes.byref(s) for s in after]))
        assert after[1].value == before[1].value, "an in-place operation on the identical view allocated memory"
        assert ops._apart_from(t, t) is t
    x += x
    x *= x
    np.testing.assert_array_equal(t.numpy(), x)
    m, y = tensor_and_array(hip, (64, 64))
    with light.no_grad():
        v = m.transpose(1, 0)
        v *= m.transpose(1, 0)                                         # the identical VIEW, two tensor objects
        assert_plan(L, "m.T *= m.T", (E.GATHER, 0, 2, 0))
    np.testing.assert_array_equal(m.numpy(), y * y)
