"""HipTensor.batch_norm / batch_norm_infer on their own kernels (csrc/batchnorm.hip): the sweep of tests/batchnorm_cases.py against
the float64 definition, inputs far from zero, run-to-run bits of the multi-slice fold, launch counts, views, the lazy relu, a
captured training step with running statistics, evaluation mode, the fallbacks and the C ABI on guarded flat buffers.

The error rule is that of test_hip_conv2d.py: a result is within 1e-5 (relative Frobenius) of the float64 result, or no further from
it than twice the float32 CPU composite is."""
import ctypes
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from common import float64_tape, rel_frobenius, assert_as_close_to_float64_as_the_cpu_backend
from batchnorm_cases import CASES, IDS, MULTI_SLICE, draw, run_tape, direct, direct_infer, run_infer_tape, expected_slices

pytestmark = pytest.mark.gpu

_reference = {}


def reference(i, offset=0.0):
    """(arrays, float64 tape with the saved statistics of the definition, float32 CPU tape) of sweep case i, computed once"""
    if (i, offset) not in _reference:
        arrays = draw(CASES[i], 100 + i, offset)
        with float64_tape():
            f64 = run_tape(CpuTensor, arrays, np.float64)
        exact, base32 = direct(arrays, np.float64), direct(arrays, np.float32)
        cpu32 = run_tape(CpuTensor, arrays)
        for name in ("save_mean", "save_rstd"):                      # the composite keeps no such tensors: the definition's
            f64[name], cpu32[name] = exact[name], base32[name]
        _reference[i, offset] = (arrays, f64, cpu32)
    return _reference[i, offset]


def assert_within_yardstick(got, cpu32, f64, what):
    assert sorted(got) == sorted(f64), (what, sorted(got), sorted(f64))
    for name in f64:
        e_hip, e_cpu = rel_frobenius(got[name], f64[name]), rel_frobenius(cpu32[name], f64[name])
        print("%s %s: hip %.3g cpu %.3g" % (what, name, e_hip, e_cpu))
        assert got[name].shape == f64[name].shape and got[name].dtype == np.float32, (what, name)
        assert e_hip <= max(1e-5, 2 * e_cpu), (what, name, e_hip, e_cpu)


def plan():
    from lightgrad_amd.autograd.hip import ops
    return ops.batchnorm_last_plan()


def vec_of(shape):
    """16-byte units along L: what dense tensors fresh from the allocator get when L is a multiple of 4"""
    length = int(np.prod(shape[2:], dtype=np.int64))
    return 4 if length > 1 and length % 4 == 0 else 1


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_sweep_against_the_float64_tape(hip, i):
    arrays, f64, cpu32 = reference(i)
    got = run_tape(hip, arrays)
    p = plan()
    shape = CASES[i][0]
    assert p["kernel"] == "bwd" and not p["relu_x"]                               # the kernels ran, not the composite
    assert p["form"] == ("across_c" if int(np.prod(shape[2:], dtype=np.int64)) == 1 else "along_l")
    assert p["slices"] == expected_slices(shape, vec_of(shape)), p
    assert p["slices"] > 1 or i not in MULTI_SLICE, p
    assert_within_yardstick(got, cpu32, f64, IDS[i])


@pytest.mark.parametrize("i", [1, 7, 8], ids=[IDS[1], IDS[7], IDS[8]])
def test_inputs_far_from_zero(hip, i):
    """randn + 100: a float32 two-pass evaluation lands about 1e-5 from float64, E[x^2] - E[x]^2 about 1e-3 - the yardstick
    separates the two by a factor of 50"""
    arrays, f64, cpu32 = reference(i, 100.0)
    assert_within_yardstick(run_tape(hip, arrays), cpu32, f64, IDS[i] + " + 100")


@pytest.mark.parametrize("i", MULTI_SLICE, ids=[IDS[i] for i in MULTI_SLICE])
def test_same_bits_twice(hip, i):
    arrays = reference(i)[0]
    first = run_tape(hip, arrays)
    assert plan()["slices"] > 1, plan()
    second = run_tape(hip, arrays)
    for name in first:
        np.testing.assert_array_equal(first[name], second[name], err_msg=name)


def test_launch_counts(hip):
    from lightgrad_amd.autograd.hip import HipGraph

    def count(fn):
        graph = HipGraph()
        with graph.capture():
            keep = fn()
        n = graph.kernel_count()
        graph.destroy()
        del keep
        return n
    for i in (1, 5, 7):                                                            # one slice, and both forms with a fold
        xa, wa, ba, ga = reference(i)[0]
        c = xa.shape[1]
        x, w, b, g = hip.from_numpy(xa), hip.from_numpy(wa), hip.from_numpy(ba), hip.from_numpy(ga, requires_grad=False)
        rm, rv = hip.from_numpy(np.zeros(c, np.float32), requires_grad=False), hip.from_numpy(np.ones(c, np.float32), requires_grad=False)
        y = x.batch_norm(w, b, rm, rv)                                             # eager once: pool, kernels
        assert count(lambda: x.batch_norm(w, b, rm, rv)) <= 2
        assert count(lambda: y.ctx.backward(g)) <= 2
        x_const = hip.from_numpy(xa, requires_grad=False)
        y_const = x_const.batch_norm(w, b, rm, rv)
        assert count(lambda: y_const.ctx.backward(g)) == 1
        (y_const * g).sum().backward()
        assert x_const.grad is None and w.grad is not None and b.grad is not None
        assert count(lambda: x.batch_norm_infer(w, b, rm, rv)) == 1
        assert plan()["kernel"] == "infer"
    pre = hip.from_numpy(reference(1)[0][0])
    assert count(lambda: pre.relu().batch_norm(None, None)) <= 2                    # the relu is applied on load


def test_views_give_the_values_of_their_dense_copies(hip):
    xa, wa, ba, ga = reference(1)[0]
    dense = run_tape(hip, (xa, wa, ba, ga))
    stored = np.ascontiguousarray(xa.transpose(0, 1, 3, 2))                        # the op receives a transposed view of this
    seen = []

    def view(t):
        v = t.transpose(0, 1, 3, 2)
        seen.append(v.is_contiguous())
        return v
    got = run_tape(hip, (stored, wa, ba, ga), x_of=view)
    assert seen == [False, False]
    got["dx"] = got["dx"].transpose(0, 1, 3, 2)
    for name in dense:
        np.testing.assert_array_equal(got[name], dense[name], err_msg=name)


@pytest.mark.parametrize("i", [1, 6], ids=[IDS[1], IDS[6]])
def test_lazy_relu_input(hip, i):
    """pre.relu().batch_norm(...): the relu never runs.  Against the definition by the yardstick; every result equals the bits of the
    same tape with the relu made real first (the same kernels read the same values)"""
    arrays = reference(i)[0]
    lazy_seen = []

    def lazy(t):
        r = t.relu()
        lazy_seen.append(r.is_lazy())
        return r

    def real(t):
        r = t.relu()
        r.numpy()
        return r
    got = run_tape(hip, arrays, x_of=lazy)
    assert lazy_seen == [True, True] and plan()["relu_x"] and plan()["kernel"] == "bwd"
    made_real = run_tape(hip, arrays, x_of=real)
    assert not plan()["relu_x"]
    for name in got:
        np.testing.assert_array_equal(got[name], made_real[name], err_msg=name)
    cpu32 = run_tape(CpuTensor, arrays, x_of=lambda t: t.relu())
    exact, base32 = direct(arrays, np.float64, relu=True), direct(arrays, np.float32, relu=True)
    for name in ("save_mean", "save_rstd"):
        cpu32[name] = base32[name]
    assert_within_yardstick(got, cpu32, exact, IDS[i] + " lazy relu")


class Net(nn.Module):
    """conv -> BN -> relu -> Linear on (N, 1, 8, 8)"""
    def __init__(self):
        nn.Module.__init__(self)
        self.conv = nn.Conv2d(1, 4, kernelsize=3, pad=0)
        self.bn = nn.BatchNorm2d(4)
        self.out = nn.Linear(4 * 6 * 6, 3)

    def forward(self, x):
        return self.out(self.bn(self.conv(x)).relu().reshape(-1, 4 * 6 * 6))


def state_of(model):
    out = {n: p.numpy().copy() for n, p in model.named_parameters()}
    out.update({n: b.numpy().copy() for n, b in model.named_buffers()})
    return out


def test_captured_step_with_running_statistics(hip):
    """one eager step, one captured, three replays on fresh batches, flat-bucket AdaBelief: parameters and both buffers against the
    same four steps on CpuTensor, judged by their distance to the float64 trajectory; the buffers move at every replay"""
    from lightgrad_amd.autograd.hip import HipGraph
    from lightgrad_amd.dist import DataParallel, SingleProcess
    np.random.seed(3)
    start = state_of(Net())
    rng = np.random.RandomState(4)
    batches = [(rng.standard_normal((8, 1, 8, 8)).astype(np.float32), rng.uniform(0, 1, (8, 3)).astype(np.float32)) for _ in range(4)]

    def load(model, dtype):
        model.load_parameters({n: start[n].astype(dtype) for n, _ in model.named_parameters()})
        model.load_buffers({n: start[n].astype(dtype) for n, _ in model.named_buffers()})

    def on_cpu(dtype):
        model = Net()
        load(model, dtype)
        opt = light.optim.AdaBelief(model.parameters(), lr=1e-3)
        for x, t in batches:
            l = light.loss.mse(model(CpuTensor.from_numpy(x.astype(dtype), requires_grad=False)), CpuTensor.from_numpy(t.astype(dtype), requires_grad=False))
            opt.zero_grad()
            l.backward()
            opt.step()
        return state_of(model)
    with float64_tape():
        ref64 = on_cpu(np.float64)
    assert ref64["bn.running_var"].dtype == np.float64
    cpu32 = on_cpu(np.float32)

    model = Net()
    load(model, np.float32)
    model.map_parameters(lambda p: p.hip())
    dp = DataParallel(model.parameters(), SingleProcess(), flatten=True)
    opt = light.optim.AdaBelief(model.parameters(), lr=1e-3, fused=True, device_step=True)
    dp.attach(opt)
    xs, ts = hip.from_numpy(batches[0][0], requires_grad=False), hip.from_numpy(batches[0][1], requires_grad=False)

    def step():
        l = light.loss.mse(model(xs), ts)
        opt.zero_grad()
        l.backward()
        opt.step()
        return l
    step()
    graph = HipGraph()
    with graph.capture():
        loss = step()
    opt.t -= len(opt.parameters)
    seen = [state_of(model)]
    for x, t in batches[1:]:
        xs.upload_(x)
        ts.upload_(t)
        graph.replay()
        opt.on_graph_replay()
        seen.append(state_of(model))
        for name in ("bn.running_mean", "bn.running_var"):
            assert not np.array_equal(seen[-1][name], seen[-2][name]), name
    assert np.isfinite(loss.item())
    graph.destroy()
    assert sorted(seen[-1]) == sorted(ref64) and len(ref64) == 8
    assert_as_close_to_float64_as_the_cpu_backend(seen[-1], cpu32, ref64, what="captured conv-BN step")


def test_evaluation_mode(hip):
    from lightgrad_amd.autograd.hip.ops import _batch_norm_infer_composite
    arrays = xa, wa, ba, ga = reference(8)[0]
    layer = nn.BatchNorm2d(8)
    layer.load_parameters({"weight": wa, "bias": ba})
    layer.map_parameters(lambda p: p.hip())
    assert all(isinstance(b, hip) and not b.requires_grad for b in layer.buffers())
    x = hip.from_numpy(xa)
    layer(x)
    assert plan()["kernel"] == "fwd"
    rm, rv = layer.running_mean.numpy().copy(), layer.running_var.numpy().copy()
    assert rm.any() and not np.array_equal(rv, np.ones(8, np.float32))
    layer.eval()
    y = layer(x)
    assert plan() == {"kernel": "infer", "form": "along_l", "slices": 1, "relu_x": False}
    composite = _batch_norm_infer_composite(x, layer.weight, layer.bias, layer.running_mean, layer.running_var, eps=layer.eps)
    exact = direct_infer(arrays, rm, rv)
    e_kernel, e_composite = rel_frobenius(y.numpy(), exact["y"]), rel_frobenius(composite.numpy(), exact["y"])
    print("eval y: kernel %.3g composite %.3g" % (e_kernel, e_composite))
    assert e_kernel <= max(1e-5, 2 * e_composite)
    np.testing.assert_array_equal(layer.running_mean.numpy(), rm)                  # bit-unchanged by an evaluation pass
    np.testing.assert_array_equal(layer.running_var.numpy(), rv)
    # and the three gradients of the evaluation form, two layouts
    for i in (8, 3):
        arrays = reference(i)[0]
        c = CASES[i][0][1]
        rng = np.random.RandomState(i)
        rm, rv = rng.uniform(-1, 1, c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32)
        got = run_infer_tape(hip, arrays, rm, rv)
        assert plan()["kernel"] == "bwd"
        assert_within_yardstick(got, run_infer_tape(CpuTensor, arrays, rm, rv), direct_infer(arrays, rm, rv), IDS[i] + " infer")


def test_fallbacks_go_through_the_composite(hip):
    before = plan()
    # float64: HipTensor computes the composite in float64 (1e-12: two float64 evaluations, sums of 140 terms in another order)
    arrays = reference(1)[0]
    got = run_tape(hip, arrays, np.float64)
    exact = direct(arrays, np.float64)
    for name in got:
        assert got[name].dtype == np.float64
        assert rel_frobenius(got[name], exact[name]) <= 1e-12, (name, rel_frobenius(got[name], exact[name]))
    # more channels than the C ABI takes (L > 1: one ticket per channel, 65536 of them), and a 5-D input is an error on both backends
    wide = ((2, 65537, 2), True)
    arrays = draw(wide, 9)
    got = run_tape(hip, arrays)
    assert "save_mean" not in got
    assert_within_yardstick(got, run_tape(CpuTensor, arrays), {k: v for k, v in direct(arrays, np.float64).items() if k in got}, "65537 channels")
    assert plan() == before                                                        # no lg_batchnorm_* launch
    with pytest.raises(ValueError, match="more than one value"):
        hip.from_numpy(np.ones((1, 3), np.float32)).batch_norm(None, None)
    with pytest.raises(ValueError, match="momentum"):
        hip.from_numpy(np.ones((4, 3), np.float32)).batch_norm(None, None, momentum=0.0)
    with pytest.raises(ValueError):
        hip.from_numpy(np.ones((2, 2, 2, 2, 2), np.float32)).batch_norm(None, None)


GUARD = 64


class Guarded(object):
    """n floats between two runs of GUARD NaNs in one device buffer"""
    def __init__(self, hip, n, values=None):
        self.n = n
        a = np.full(n + 2 * GUARD, np.nan, np.float32)
        if values is not None:
            a[GUARD:GUARD + n] = values
        self.t = hip.from_numpy(a, requires_grad=False)
        self.ptr = self.t.ptr + 4 * GUARD

    def read(self):
        a = self.t.numpy()
        assert np.isnan(a[:GUARD]).all() and np.isnan(a[GUARD + self.n:]).all(), "a write outside the output"
        assert not np.isnan(a[GUARD:GUARD + self.n]).any(), "an output element was not written"
        return a[GUARD:GUARD + self.n]


@pytest.mark.parametrize("i", [1, 3, 6], ids=[IDS[1], IDS[3], IDS[6]])
def test_c_abi_writes_nothing_outside_its_outputs(hip, i):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    shape = CASES[i][0]
    n, c = shape[:2]
    length = int(np.prod(shape[2:], dtype=np.int64))
    xa, wa, ba, ga = arrays = reference(i)[0]
    expect = run_tape(hip, arrays, calls=1)
    x, w, b, g = (hip.from_numpy(a, requires_grad=False) for a in (xa, wa, ba, ga))
    y, dx = Guarded(hip, xa.size), Guarded(hip, xa.size)
    mean, rstd, dw, db = (Guarded(hip, c) for _ in range(4))
    rm, rv = Guarded(hip, c, np.zeros(c, np.float32)), Guarded(hip, c, np.ones(c, np.float32))
    L.check(lib.lg_batchnorm_fwd_f32(x.ptr, w.ptr, b.ptr, y.ptr, mean.ptr, rstd.ptr, rm.ptr, rv.ptr, n, c, length, 1e-5, 0.1, 0))
    L.check(lib.lg_batchnorm_bwd_f32(g.ptr, x.ptr, w.ptr, mean.ptr, rstd.ptr, dx.ptr, dw.ptr, db.ptr, n, c, length, 0))
    # (the guarded buffers start 256 bytes into an allocation: the same 16-byte alignment, so the same plan and the same bits)
    for name, buf in (("y", y), ("dx", dx), ("dw", dw), ("db", db), ("save_mean", mean), ("save_rstd", rstd), ("running_mean", rm),
                      ("running_var", rv)):
        np.testing.assert_array_equal(buf.read().reshape(expect[name].shape), expect[name], err_msg=name)
    out = Guarded(hip, xa.size)
    L.check(lib.lg_batchnorm_infer_f32(x.ptr, w.ptr, b.ptr, rm.ptr, rv.ptr, out.ptr, n, c, length, 1e-5, 0))
    exact = direct_infer(arrays, expect["running_mean"], expect["running_var"])
    assert rel_frobenius(out.read().reshape(shape), exact["y"]) <= 1e-5            # elementwise: a few roundings per element
    # every optional pointer NULL: statistics alone, and a backward that has nothing to do
    L.check(lib.lg_batchnorm_fwd_f32(x.ptr, None, None, y.ptr, mean.ptr, rstd.ptr, None, None, n, c, length, 1e-5, 0.1, 0))
    np.testing.assert_array_equal(mean.read(), expect["save_mean"])
    L.check(lib.lg_batchnorm_bwd_f32(g.ptr, x.ptr, None, mean.ptr, rstd.ptr, None, None, None, n, c, length, 0))


def test_c_abi_refuses_what_the_header_says(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    t = hip.from_numpy(np.zeros(64, np.float32), requires_grad=False)

    def calls(n, c, length):
        return (lib.lg_batchnorm_fwd_f32(t.ptr, None, None, t.ptr, t.ptr, t.ptr, None, None, n, c, length, 1e-5, 0.1, 0),
                lib.lg_batchnorm_bwd_f32(t.ptr, t.ptr, None, t.ptr, t.ptr, t.ptr, None, None, n, c, length, 0),
                lib.lg_batchnorm_infer_f32(t.ptr, None, None, t.ptr, t.ptr, t.ptr, n, c, length, 1e-5, 0))
    for geometry, word in (((0, 4, 4), b"at least 1"), ((4, 4, 0), b"at least 1"), ((1 << 20, 1 << 6, 1 << 6), b"2^31"),
                           ((2, 65537, 2), b"ticket pool")):
        assert calls(*geometry) == (-1, -1, -1), geometry
        assert word in lib.lg_last_error(), (geometry, lib.lg_last_error())
    # one value per channel: no batch statistics
    assert lib.lg_batchnorm_fwd_f32(t.ptr, None, None, t.ptr, t.ptr, t.ptr, None, None, 1, 8, 1, 1e-5, 0.1, 0) == -1
    assert b"at least 2 values" in lib.lg_last_error()
    for momentum in (0.0, 1.5):
        assert lib.lg_batchnorm_fwd_f32(t.ptr, None, None, t.ptr, t.ptr, t.ptr, None, None, 2, 4, 4, 1e-5, momentum, 0) == -1
        assert b"momentum" in lib.lg_last_error()
    assert lib.lg_batchnorm_fwd_f32(None, None, None, t.ptr, t.ptr, t.ptr, None, None, 2, 4, 4, 1e-5, 0.1, 0) == -1
    assert lib.lg_batchnorm_infer_f32(t.ptr, None, None, None, t.ptr, t.ptr, 2, 4, 4, 1e-5, 0) == -1
    out = (ctypes.c_int32 * 4)()
    assert lib.lg_batchnorm_last_plan(out) == 0 and lib.lg_batchnorm_last_plan(None) == -1
