"""HipTensor.conv2d / max_pool / min_pool on their own kernels (csrc/conv.hip): the sweep of tests/conv2d_cases.py against the same
tape in float64, both dW paths, run-to-run bits, launch counts, views, the lazy relu, the fallbacks, pooling against the CPU
backend bit for bit, a captured CNN step and the C ABI on guarded flat buffers.

The error rule is that of test_hip_cnn.py::test_cnn_training_matches_cpu_backend: a result is within 1e-5 (relative Frobenius) of
the float64 tape, or no further from it than twice the float32 CPU composite is."""
import ctypes
import importlib.util
import os
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from conftest import ROOT
from common import check_gradients, float64_tape, rel_frobenius
from conv2d_cases import CASES, IDS, draw, run_tape, out_shape, strides_of

pytestmark = pytest.mark.gpu

_reference = {}


def reference(i):
    """(float64 tape, float32 CPU tape) of sweep case i, computed once"""
    if i not in _reference:
        arrays = draw(CASES[i], 100 + i)
        with float64_tape():
            f64 = run_tape(CpuTensor, CASES[i], arrays, np.float64)
        _reference[i] = (arrays, f64, run_tape(CpuTensor, CASES[i], arrays))
    return _reference[i]


def assert_within_yardstick(got, cpu32, f64, what):
    for name in f64:
        e_hip, e_cpu = rel_frobenius(got[name], f64[name]), rel_frobenius(cpu32[name], f64[name])
        print("%s %s: hip %.3g cpu %.3g" % (what, name, e_hip, e_cpu))
        assert got[name].shape == f64[name].shape, (what, name)
        assert e_hip <= max(1e-5, 2 * e_cpu), (what, name, e_hip, e_cpu)


def plan():
    from lightgrad_amd.autograd.hip import ops
    return ops.conv2d_last_plan()


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_against_the_float64_tape(hip, i):
    arrays, f64, cpu32 = reference(i)
    got = run_tape(hip, CASES[i], arrays)
    assert plan()["kernel"] is not None and plan()["tile"][0] == 32          # the kernels ran, not the composite
    assert_within_yardstick(got, cpu32, f64, IDS[i])


def expected_dw_slices(case):
    """the rule of lg_conv2d_dw_f32, a function of the shape: chunks of 128 positions, at least two per slice, at most 256 slices"""
    n, _, oh, ow = out_shape(case)
    chunks = -(-(n * oh * ow) // 128)
    return -(-chunks // max(2, -(-chunks // 256)))


def test_both_dw_paths_are_taken(hip):
    """one workgroup per output tile when there are at most 256 positions, a split with the in-launch fold beyond: cases 0 and 4
    have 1 and 60 positions, cases 1, 2 and 8 have 1352, 363 and 3136"""
    slices = []
    for i in (0, 4, 1, 2, 8):
        run_tape(hip, CASES[i], reference(i)[0])
        p = plan()
        slices.append(p["dw_slices"])
        assert p["dw_slices"] == expected_dw_slices(CASES[i]) and p["kernel"] == "dx", (i, p)
    assert slices[:2] == [1, 1] and min(slices[2:]) > 1, slices


# no case of the sweep has more than 13 slices, so none lets one thread of the fold sum more than one batch of eight partials or
# reaches the cap: 8 * 1 * 258 * 258 -> 256 x 256 positions a sample = 524288 positions, 4096 chunks, 16 per slice, 256 slices
MANY_SLICES_CASE = (8, 1, 258, 258, 2, 3, 3, 1, 0, True)


def test_dw_fold_at_the_slice_cap(hip):
    assert expected_dw_slices(MANY_SLICES_CASE) == 256
    arrays = draw(MANY_SLICES_CASE, 21)
    with float64_tape():
        f64 = run_tape(CpuTensor, MANY_SLICES_CASE, arrays, np.float64)
    got = run_tape(hip, MANY_SLICES_CASE, arrays)
    assert plan()["dw_slices"] == 256, plan()
    assert_within_yardstick(got, run_tape(CpuTensor, MANY_SLICES_CASE, arrays), f64, "256 slices")
    again = run_tape(hip, MANY_SLICES_CASE, arrays)
    for name in got:
        np.testing.assert_array_equal(again[name], got[name], err_msg=name)


@pytest.mark.parametrize("i", [1, 8])
def test_same_bits_twice(hip, i):
    arrays = reference(i)[0]
    first, second = run_tape(hip, CASES[i], arrays), run_tape(hip, CASES[i], arrays)
    for name in first:
        np.testing.assert_array_equal(first[name], second[name], err_msg=name)


def test_launch_counts(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    case = CASES[2]
    xa, wa, ba, ga = draw(case, 3)

    def count(fn):
        graph = HipGraph()
        with graph.capture():
            keep = fn()
        n = graph.kernel_count()
        graph.destroy()
        del keep
        return n
    x, w, b, g = hip.from_numpy(xa), hip.from_numpy(wa), hip.from_numpy(ba), hip.from_numpy(ga, requires_grad=False)
    y = x.conv2d(w, b)                                                        # eager once: pool, kernels
    assert count(lambda: x.conv2d(w, b)) == 1
    assert count(lambda: y.ctx.backward(g)) == 2
    x_const = hip.from_numpy(xa, requires_grad=False)
    y_const = x_const.conv2d(w, b)
    assert count(lambda: y_const.ctx.backward(g)) == 1
    (y_const * g).sum().backward()
    assert x_const.grad is None and w.grad is not None and b.grad is not None
    p = x.max_pool()
    gp = hip.from_numpy(np.ones(p.shape, np.float32), requires_grad=False)
    assert count(lambda: x.max_pool()) == 1
    assert count(lambda: p.ctx.backward(gp)) == 1
    pre = hip.from_numpy(xa)
    assert count(lambda: pre.relu().conv2d(w)) == 1                           # the relu is applied while x is staged


def test_views_give_the_values_of_their_dense_copies(hip):
    case = CASES[3]
    xa, wa, ba, ga = draw(case, 5)
    dense = run_tape(hip, case, (xa, wa, ba, ga))
    x = hip.from_numpy(np.ascontiguousarray(xa.transpose(0, 1, 3, 2))).transpose(0, 1, 3, 2)      # x as a transposed view
    assert not x.is_contiguous()
    w, b = hip.from_numpy(wa), hip.from_numpy(ba)
    g_t = hip.from_numpy(np.ascontiguousarray(ga.transpose(0, 1, 3, 2)), requires_grad=False)
    y = x.conv2d(w, b, stride=case[7], pad=case[8])
    (y.transpose(0, 1, 3, 2) * g_t).sum().backward()                                             # out_grad arrives through a transpose
    np.testing.assert_array_equal(y.numpy(), dense["y"])
    for name, t in (("dx", x), ("dw", w), ("db", b)):
        np.testing.assert_array_equal(t.grad.numpy(), dense[name], err_msg=name)


def test_lazy_relu_input(hip):
    """pre.relu().conv2d(w): the relu never runs.  Against the CPU tape by the yardstick; pre.grad and everything else equal the bits
    of the same tape with the relu made real first (the same dx kernel, the same relu.backward)"""
    case = CASES[2]
    xa, wa, ba, ga = draw(case, 9)

    def tape(T, dtype=np.float32, real=False):
        pre, w, b = (T.from_numpy(a.astype(dtype)) for a in (xa, wa, ba))
        r = pre.relu()
        if real:
            r.numpy()
        y = r.conv2d(w, b)
        (y * T.from_numpy(ga.astype(dtype), requires_grad=False)).sum().backward()
        return {"y": y.numpy(), "dw": w.grad.numpy(), "db": b.grad.numpy(), "dpre": pre.grad.numpy(), "relu": r.numpy()}
    got = tape(hip)
    assert plan()["kernel"] == "dx"
    real = tape(hip, real=True)
    with float64_tape():
        f64 = tape(CpuTensor, np.float64)
    assert_within_yardstick(got, tape(CpuTensor), f64, "lazy relu")
    for name in got:
        np.testing.assert_array_equal(got[name], real[name], err_msg=name)
    np.testing.assert_array_equal(got["relu"], np.maximum(xa, 0))
    # and the kernels did apply it: the dW launch of the lazy tape reported relu_x
    pre, w = hip.from_numpy(xa), hip.from_numpy(wa)
    y = pre.relu().conv2d(w)
    assert plan()["relu_x"] and plan()["kernel"] == "fwd"
    y.ctx.backward(hip.from_numpy(ga, requires_grad=False))
    assert plan()["kernel"] == "dx"


def test_fallbacks_go_through_the_composite(hip):
    rng = np.random.RandomState(2)

    def both(xa, wa, ba=None, **kw):
        out = []
        for T in (CpuTensor, hip):
            x, w, b = T.from_numpy(xa), T.from_numpy(wa), (T.from_numpy(ba) if ba is not None else None)
            y = x.conv2d(w, b, **kw)
            (y * y).sum().backward()
            out.append([y.numpy(), x.grad.numpy(), w.grad.numpy()] + ([b.grad.numpy()] if b is not None else []))
        return out
    # float64 (the CPU side on a float64 tape: its gradient buffers follow the default dtype), a 3-D input (no batch axis), and a
    # shape the C ABI refuses (C*KH*KW = 2304 > 2048).  Tolerances: 1e-12 between two float64 sums of at most 18 terms in another
    # order; 1e-5, the sweep's floor, between two float32 composites
    with float64_tape():
        cpu, dev = both(rng.uniform(-1, 1, (2, 2, 7, 6)), rng.uniform(-1, 1, (3, 2, 3, 3)), rng.uniform(-1, 1, (3,)), pad=1, stride=(2, 1))
    runs = [(cpu, dev, 1e-12)]
    for xa, wa, kw in ((rng.uniform(-1, 1, (2, 6, 6)), rng.uniform(-1, 1, (3, 2, 3, 3)), {}),
                       (rng.uniform(-1, 1, (1, 256, 4, 4)), rng.uniform(-1, 1, (2, 256, 3, 3)), dict(pad=1))):
        plan_before = plan()
        runs.append(both(xa.astype(np.float32), wa.astype(np.float32), **kw) + [1e-5])
        assert plan() == plan_before                                               # no lg_conv2d_* launch
    for cpu, dev, tol in runs:
        for a, b in zip(cpu, dev):
            assert a.dtype == b.dtype and a.shape == b.shape
            assert rel_frobenius(b, a) <= tol, (rel_frobenius(b, a), tol)


POOL_KERNELS = [(2, 2), (3, 2), (2, 3), (1, 1)]
POOL_SHAPES = [(2, 3, 8, 8), (1, 1, 7, 9), (5, 6)]


def pool_both(hip, xa, name, kernel, seed=0):
    out = []
    for T in (CpuTensor, hip):
        x = T.from_numpy(xa)
        y = getattr(x, name)(kernel=kernel)
        g = np.random.RandomState(seed).uniform(-1, 1, y.shape).astype(np.float32)
        (y * T.from_numpy(g, requires_grad=False)).sum().backward()
        out.append((y.numpy(), x.grad.numpy()))
    return out


@pytest.mark.parametrize("name", ["max_pool", "min_pool"])
def test_pooling_equals_the_cpu_backend(hip, name):
    rng = np.random.RandomState(4)
    for shape in POOL_SHAPES:
        inputs = [rng.uniform(-1, 1, shape).astype(np.float32),
                  rng.randint(-2, 3, shape).astype(np.float32)]                       # small integers: ties in most windows
        with_nan = inputs[0].copy()
        with_nan.reshape(-1)[::5] = np.nan
        inputs.append(with_nan)
        for xa in inputs:
            for kernel in POOL_KERNELS:
                (y_cpu, dx_cpu), (y_hip, dx_hip) = pool_both(hip, xa, name, kernel)
                assert y_hip.shape == y_cpu.shape == shape[:-2] + (shape[-2] // kernel[0], shape[-1] // kernel[1])
                np.testing.assert_array_equal(y_hip, y_cpu, err_msg="%s %s %s" % (name, shape, kernel))
                np.testing.assert_array_equal(dx_hip, dx_cpu, err_msg="%s %s %s" % (name, shape, kernel))


def test_pooling_gradcheck_and_composite_kinds(hip):
    np.random.seed(12)
    check_gradients(hip, lambda x: x.max_pool(), shapes=[(2, 4, 6)])
    check_gradients(hip, lambda x: x.min_pool(kernel=(2, 3)), shapes=[(2, 4, 6)])
    xa = np.random.uniform(-1, 1, (2, 3, 4, 6)).astype(np.float32)
    for name, kernel in (("max_pool", (2, 2, 2)), ("mean_pool", (2, 2))):              # other kernel lengths and mean_pool: the composite
        (y_cpu, dx_cpu), (y_hip, dx_hip) = pool_both(hip, xa, name, kernel)
        np.testing.assert_allclose(y_hip, y_cpu, rtol=1e-6)
        np.testing.assert_allclose(dx_hip, dx_cpu, rtol=1e-6)


def test_captured_cnn_step_equals_eager_steps(hip):
    """the CNN of examples/mnist.py, batch 8, AdaBelief(fused, device_step): three eager steps, one captured, three replays - the
    parameters of six eager steps"""
    from lightgrad_amd.autograd.hip import HipGraph
    spec = importlib.util.spec_from_file_location("mnist_example", os.path.join(ROOT, "examples", "mnist.py"))
    mnist = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mnist)
    np.random.seed(0)
    start = [(n, p.numpy().copy()) for n, p in mnist.CNN().named_parameters()]
    x, t = mnist.synthetic_batch(np.random.RandomState(1), 8)

    def make():
        model = mnist.CNN()
        model.load_parameters(start)
        model.map_parameters(lambda p: p.hip())
        opt = light.optim.AdaBelief(model.parameters(), lr=0.001, fused=True, device_step=True)
        xs, ts = hip.from_numpy(x), hip.from_numpy(t)

        def step():
            l = light.loss.mse(model(xs), ts)
            opt.zero_grad()
            l.backward()
            opt.step()
            return l
        return model, opt, step
    eager_model, _, eager_step = make()
    for _ in range(6):
        eager_step()
    model, opt, step = make()
    for _ in range(3):
        step()
    graph = HipGraph()
    with graph.capture():
        loss = step()
    opt.t -= len(opt.parameters)
    for _ in range(3):
        graph.replay()
        opt.on_graph_replay()
    assert np.isfinite(loss.item())
    for (n, a), (_, b) in zip(eager_model.named_parameters(), model.named_parameters()):
        np.testing.assert_array_equal(b.numpy(), a.numpy(), err_msg=n)
    graph.destroy()


GUARD = 64


class Guarded(object):
    """n floats between two runs of GUARD NaNs in one device buffer"""
    def __init__(self, hip, n):
        self.n, self.t = n, hip.from_numpy(np.full(n + 2 * GUARD, np.nan, np.float32), requires_grad=False)
        self.ptr = self.t.ptr + 4 * GUARD

    def read(self):
        a = self.t.numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + self.n:]).all(), "a write outside the output"
        assert not np.isnan(a[GUARD:GUARD + self.n]).any(), "an output element was not written"
        return a[GUARD:GUARD + self.n]


@pytest.mark.parametrize("i", [0, 3, 4, 8])
def test_c_abi_writes_nothing_outside_its_outputs(hip, i):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    case = CASES[i]
    n, c, h, w, o, kh, kw, stride, p, has_bias = case
    sh, sw = strides_of(stride)
    xa, wa, ba, ga = draw(case, 100 + i)
    expect = run_tape(hip, case, (xa, wa, ba, ga))
    x, wt, g = (hip.from_numpy(a, requires_grad=False) for a in (xa, wa, ga))
    b = hip.from_numpy(ba, requires_grad=False) if has_bias else None
    geom = (n, c, h, w, o, kh, kw, sh, sw, p)
    y, dx, dw, db = Guarded(hip, ga.size), Guarded(hip, xa.size), Guarded(hip, wa.size), Guarded(hip, o)
    L.check(lib.lg_conv2d_fwd_f32(x.ptr, wt.ptr, b.ptr if b is not None else None, y.ptr, *geom, 0))
    L.check(lib.lg_conv2d_dx_f32(g.ptr, wt.ptr, dx.ptr, *geom))
    L.check(lib.lg_conv2d_dw_f32(g.ptr, x.ptr, dw.ptr, db.ptr if has_bias else None, *geom, 0))
    np.testing.assert_array_equal(y.read().reshape(ga.shape), expect["y"])
    np.testing.assert_array_equal(dx.read().reshape(xa.shape), expect["dx"])
    np.testing.assert_array_equal(dw.read().reshape(wa.shape), expect["dw"])
    if has_bias:
        np.testing.assert_array_equal(db.read().reshape(ba.shape), expect["db"])
    # pooling on the same input: a cropped plane
    oh, ow = h // 2, w // 3
    if oh and ow:
        py, pdx = Guarded(hip, n * c * oh * ow), Guarded(hip, xa.size)
        pg = hip.from_numpy(np.ones(n * c * oh * ow, np.float32), requires_grad=False)
        L.check(lib.lg_pool2d_fwd_f32(0, x.ptr, py.ptr, n * c, h, w, 2, 3))
        L.check(lib.lg_pool2d_bwd_f32(x.ptr, py.ptr, pg.ptr, pdx.ptr, n * c, h, w, 2, 3))
        crop = xa[:, :, :oh * 2, :ow * 3].reshape(n, c, oh, 2, ow, 3)
        np.testing.assert_array_equal(py.read().reshape(n, c, oh, ow), crop.max(axis=(3, 5)))
        assert pdx.read().sum() == n * c * oh * ow                                 # random floats: one maximum per window


def test_c_abi_refuses_what_the_header_says(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    t = hip.from_numpy(np.zeros(64, np.float32), requires_grad=False)
    ok = dict(N=1, C=1, H=4, W=4, O=1, KH=3, KW=3, sh=1, sw=1, pad=0)

    def calls(**change):
        a = dict(ok, **change)
        geom = tuple(a[k] for k in ("N", "C", "H", "W", "O", "KH", "KW", "sh", "sw", "pad"))
        return (lib.lg_conv2d_fwd_f32(t.ptr, t.ptr, None, t.ptr, *geom, 0), lib.lg_conv2d_dx_f32(t.ptr, t.ptr, t.ptr, *geom),
                lib.lg_conv2d_dw_f32(t.ptr, t.ptr, t.ptr, None, *geom, 0))
    for change, word in ((dict(N=0), b"at least 1"), (dict(sh=0), b"strides"), (dict(pad=-1), b"padding"), (dict(KH=5), b"does not fit"),
                         (dict(H=16385, KH=1, KW=1), b"limited to 16384"), (dict(C=256), b"limited to 2048"),
                         (dict(O=256), b"limited to 2048"), (dict(N=1 << 20, H=64, W=64, KH=1, KW=1), b"below 2^31")):
        assert calls(**change) == (-1, -1, -1), change                            # the three refuse the same shapes
        assert word in lib.lg_last_error(), (change, lib.lg_last_error())
    assert lib.lg_conv2d_fwd_f32(None, t.ptr, None, t.ptr, 1, 1, 4, 4, 1, 3, 3, 1, 1, 0, 0) == -1
    assert lib.lg_pool2d_fwd_f32(2, t.ptr, t.ptr, 1, 4, 4, 2, 2) == -1 and b"op must be" in lib.lg_last_error()
    assert lib.lg_pool2d_fwd_f32(0, t.ptr, t.ptr, 1, 4, 4, 5, 2) == -1 and b"larger than the input" in lib.lg_last_error()
    assert lib.lg_pool2d_bwd_f32(t.ptr, t.ptr, t.ptr, t.ptr, 1 << 20, 64, 64, 2, 2) == -1 and b"2^31" in lib.lg_last_error()
    assert lib.lg_pool2d_bwd_f32(t.ptr, t.ptr, t.ptr, t.ptr, 0, 4, 4, 2, 2) == -1
    out = (ctypes.c_int32 * 6)()
    assert lib.lg_conv2d_last_plan(out) == 0 and lib.lg_conv2d_last_plan(None) == -1
