"""Weight decay, clipping by the global gradient norm and the warmup / linear-decay schedule in the flat-bucket update
(include/lghip.h: lg_grad_norm_clip_f32, lg_adamw_multi_dev_f32; optim.Adam / AdaBelief).  The norm launch is compared with
float64 numpy, the neutral update bit for bit with lg_adam_multi_dev_f32, the whole recipe with the expression form run on
CpuTensor in float64, and a replayed hipGraph bit for bit with eager steps."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd import Gradients
from common import float64_tape, mlp_trajectory_on_cpu, assert_as_close_to_float64_as_the_cpu_backend
import np_oracle as O
from test_cpu_backend import MLP

pytestmark = pytest.mark.gpu

SEGMENTS = (1, 3, 4, 0, 1023, 1024, 1025, 4097)          # a zero-length segment, offsets that are no multiples of 4
SHAPES_A = ((1,), (3,), (2, 2), (0,), (1023,), (32, 32), (1025,), (17, 241))
SHAPES_B = tuple((5,) if i % 3 else (1, 5) for i in range(65))      # 65 segments: one past the 64-segment group edge
LR, WD = 1e-2, 0.1


def offsets_of(lengths):
    return tuple(int(o) for o in np.concatenate([[0], np.cumsum(lengths)]))


# ---- the norm launch alone ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gscale", [1.0, 0.25])
def test_norm_launch_against_float64(hip, gscale):
    from lightgrad_amd.autograd.hip import lib as hiplib
    L = hiplib.lib()
    rng = np.random.RandomState(7)
    partial, ticket, out = hip._new_grad_norm_scratch()
    for n in (1, 3, 4, 255, 256, 1023, 1024, 1025, 4097, 100003):
        host = rng.uniform(-1, 1, n + 1).astype(np.float32)
        buf = hip.from_numpy(host, requires_grad=False)
        for shift in (0, 1):                                  # shift 1: the base pointer is not 16-byte aligned
            g32 = host[shift:shift + n] * np.float32(gscale)
            exact = np.sqrt(np.sum(g32.astype(np.float64) ** 2))
            numpy32 = np.sqrt(np.sum(g32 * g32, dtype=np.float32))
            numpy_err = abs(float(numpy32) - exact) / exact
            tol = max(1e-6, 2 * numpy_err)
            seen = []
            for max_norm in (0.5 * exact, 0.5 * exact, 4.0 * exact):          # clipping, the same again, not clipping
                hiplib.check(L.lg_grad_norm_clip_f32(buf.ptr + 4 * shift, n, gscale, max_norm, partial.ptr, ticket.ptr, out.ptr))
                norm, coef = out.numpy()
                assert ticket.numpy()[0] == 0, (n, shift)                      # ready for the next call
                err = abs(float(norm) - exact) / exact
                print("norm n=%d shift=%d gscale=%g: rel err %.3g (float32 numpy %.3g)" % (n, shift, gscale, err, numpy_err))
                assert err <= tol, (n, shift, err, tol)
                assert coef == np.float32(min(1.0, max_norm / (float(norm) + 1e-6))), (n, shift, coef)
                seen.append((norm.tobytes(), coef.tobytes(), float(coef)))
            assert seen[0][:2] == seen[1][:2], (n, shift)                      # the same input: the same bits
            assert seen[0][0] == seen[2][0] and seen[0][2] < 1.0 and seen[2][2] == 1.0


# ---- the update launch through the tensor hooks ------------------------------------------------------------------------------
class Bucket(object):
    """p, g, m, v of one flat bucket on the device and a step counter, for direct calls of the two update entry points"""

    def __init__(self, hip, lengths, seed):
        rng = np.random.RandomState(seed)
        self.offsets = offsets_of(lengths)
        n = self.offsets[-1]
        self.p = hip.from_numpy(rng.uniform(-1, 1, n).astype(np.float32), requires_grad=False)
        self.g = hip.from_numpy(rng.uniform(-1, 1, n).astype(np.float32), requires_grad=False)
        self.m, self.v = hip.zeros((n,), requires_grad=False), hip.zeros((n,), requires_grad=False)
        self.counter = hip._new_step_counter(0, slots=max(1, len(lengths) * -(-max(lengths) // 1024)))
        self.nseg = len(lengths)

    def old(self, gscale, belief):
        self.p._fused_adam_multi_dev(self.g, self.m, self.v, self.offsets, LR, 0.9, 0.999, 1e-8, self.counter, gscale, belief)

    def new(self, gscale, belief, weight_decay=0.0, flags=None, clip=None, kind=0, warmup=0, total=0):
        self.p._fused_adamw_multi_dev(self.g, self.m, self.v, self.offsets, LR, 0.9, 0.999, 1e-8, self.counter, gscale, belief,
                                      weight_decay, flags if flags is not None else (False,) * self.nseg, clip, kind, warmup, total)

    def state(self):
        return self.p.numpy(), self.m.numpy(), self.v.numpy(), int(self.counter.numpy()[0])


@pytest.mark.parametrize("lengths", [SEGMENTS, (5,) * 65], ids=["ragged", "65_segments"])
@pytest.mark.parametrize("belief,gscale", [(False, 1.0), (True, 0.5)], ids=["adam", "adabelief_scaled"])
def test_neutral_update_is_the_old_launch_bit_for_bit(hip, lengths, belief, gscale):
    a, b = Bucket(hip, lengths, 3), Bucket(hip, lengths, 3)
    for _ in range(3):
        a.old(gscale, belief)
        b.new(gscale, belief)
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(x, y)
    assert a.state()[3] == 3
    assert not np.array_equal(a.state()[0], Bucket(hip, lengths, 3).state()[0])       # (and the launches did move the parameters)


@pytest.mark.parametrize("lengths", [SEGMENTS, (5,) * 65], ids=["ragged", "65_segments"])
def test_a_coefficient_of_one_changes_no_bit(hip, lengths):
    a, b = Bucket(hip, lengths, 5), Bucket(hip, lengths, 5)
    flags = tuple(i % 2 == 0 for i in range(len(lengths)))
    scratch = hip._new_grad_norm_scratch()
    for _ in range(3):
        a.new(1.0, True, WD, flags, None, 1, 2, 5)
        b.g._grad_norm_clip(1.0, 1e9, scratch)                                        # far above the norm: coef == 1
        b.new(1.0, True, WD, flags, scratch[2], 1, 2, 5)
    assert scratch[2].numpy()[1] == 1.0 and scratch[2].numpy()[0] > 1.0
    for x, y in zip(a.state(), b.state()):
        np.testing.assert_array_equal(x, y)


# ---- the whole recipe against the expression form ----------------------------------------------------------------------------
def fixed_problem(shapes, steps, sizes, seed):
    rng = np.random.RandomState(seed)
    p0 = [rng.uniform(-1, 1, s).astype(np.float32) for s in shapes]
    grads = [[(size * rng.uniform(-1, 1, s)).astype(np.float32) for s in shapes] for size in sizes[:steps]]
    return p0, grads


def set_gradients(cls, opt, params, step_grads, dtype):
    opt.zero_grad()
    with Gradients.no_grad():
        for p, g in zip(params, step_grads):
            if g.size > 0:
                p.grad[...] = cls.from_numpy(g.astype(dtype), requires_grad=False)


def run_on_cpu(opt_cls, p0, grads, dtype, **options):
    """the expression form on CpuTensor: ({name: array} of parameters, the norms of every step)"""
    def run():
        params = [CpuTensor.from_numpy(a.astype(dtype)) for a in p0]
        opt = opt_cls(params, lr=LR, **options)
        norms = []
        for step_grads in grads:
            set_gradients(CpuTensor, opt, params, step_grads, dtype)
            opt.step()
            if opt.max_grad_norm is not None:
                norms.append(float(opt.grad_norm().item()))
        out = {"p%d" % i: p.numpy().copy() for i, p in enumerate(params)}
        out.update({"m%d" % i: np.asarray(m.numpy() if hasattr(m, "numpy") else m).copy() for i, m in enumerate(opt.m)})
        out.update({"v%d" % i: np.asarray(v.numpy() if hasattr(v, "numpy") else v).copy() for i, v in enumerate(opt.v)})
        return out, norms
    if np.dtype(dtype) == np.float64:
        with float64_tape():
            return run()
    return run()


def run_on_hip_flat(hip, opt_cls, p0, grads, **options):
    from lightgrad_amd.dist import DataParallel, SingleProcess
    params = [hip.from_numpy(a) for a in p0]
    dp = DataParallel(params, SingleProcess(), flatten=True)
    opt = opt_cls(params, lr=LR, fused=True, device_step=True, **options)
    dp.attach(opt)
    norms = []
    for step_grads in grads:
        set_gradients(hip, opt, params, step_grads, np.float32)
        opt.step()
        if opt.max_grad_norm is not None:
            norm = opt.grad_norm()
            assert norm.shape == () and isinstance(norm, hip)
            norms.append(float(norm.item()))
    offsets = dp.offsets
    m, v = opt._flat[1].numpy(), opt._flat[2].numpy()
    out = {"p%d" % i: p.numpy().copy() for i, p in enumerate(params)}
    out.update({"m%d" % i: m[a:b].reshape(p0[i].shape) for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))})
    out.update({"v%d" % i: v[a:b].reshape(p0[i].shape) for i, (a, b) in enumerate(zip(offsets[:-1], offsets[1:]))})
    assert int(opt._step_counter.numpy()[0]) == len(grads) and opt.t == len(grads) * len(params)
    return out, norms


GRAD_SIZES = (0.001, 3.0, 0.002, 4.0, 0.001, 5.0)


@pytest.mark.parametrize("opt_cls", [light.optim.Adam, light.optim.AdaBelief], ids=["adam", "adabelief"])
def test_full_recipe_on_the_ragged_bucket(hip, opt_cls):
    p0, grads = fixed_problem(SHAPES_A, 6, GRAD_SIZES, 11)
    assert tuple(a.size for a in p0) == SEGMENTS
    recipe = dict(weight_decay=WD, max_grad_norm=1.0, schedule=light.optim.WarmupLinear(2, 5))      # default mask: the 2-D ones decay
    ref64, norms64 = run_on_cpu(opt_cls, p0, grads, np.float64, **recipe)
    cpu32, _ = run_on_cpu(opt_cls, p0, grads, np.float32, **recipe)
    got, norms = run_on_hip_flat(hip, opt_cls, p0, grads, **recipe)
    assert min(norms64) < 1.0 < max(norms64)                                           # clipped steps and unclipped ones
    np.testing.assert_allclose(norms, norms64, rtol=1e-6)
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, what="ragged bucket")


def test_full_recipe_across_the_group_edge(hip):
    sizes = (0.01, 3.0, 0.02, 4.0, 0.01, 5.0)
    p0, grads = fixed_problem(SHAPES_B, 6, sizes, 13)
    for g in grads[3][:64]:
        g[...] = 0                        # step 4: only parameter 65 - alone in the second launch - has a gradient, and it is clipped
    mask = tuple(i % 2 == 0 for i in range(65))                                        # alternating: 63 decays, 64 not, 65 decays
    recipe = dict(weight_decay=WD, decay_mask=mask, max_grad_norm=1.0, schedule=light.optim.WarmupLinear(2, 5))
    ref64, norms64 = run_on_cpu(light.optim.AdaBelief, p0, grads, np.float64, **recipe)
    cpu32, _ = run_on_cpu(light.optim.AdaBelief, p0, grads, np.float32, **recipe)
    got, norms = run_on_hip_flat(hip, light.optim.AdaBelief, p0, grads, **recipe)
    np.testing.assert_allclose(norms, norms64, rtol=1e-6)                              # the norm covers both launches' parameters
    assert norms64[3] > 1.0 and abs(norms64[3] - np.sqrt(np.sum(grads[3][64].astype(np.float64) ** 2))) < 1e-12
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, what="65 segments")
    # the flags land on the right parameters: without the decay exactly the masked-out ones end with the same bits
    undecayed, _ = run_on_hip_flat(hip, light.optim.AdaBelief, p0, grads, max_grad_norm=1.0, schedule=light.optim.WarmupLinear(2, 5))
    for i in range(65):
        same = np.array_equal(got["p%d" % i], undecayed["p%d" % i])
        assert same == (not mask[i]), "parameter %d of 65: decay flag %s, same bits as without decay: %s" % (i + 1, mask[i], same)


# ---- a model ---------------------------------------------------------------------------------------------------------------
DIMS, BATCH = (16, 8, 4), 8


def mlp_on_hip(hip, w0, x, onehot, opt_cls, **options):
    from lightgrad_amd.dist import DataParallel, SingleProcess
    model = MLP(*DIMS)
    model.load_parameters(w0)
    model.map_parameters(lambda p: p.hip())
    dp = DataParallel(model.parameters(), SingleProcess(), flatten=True)
    opt = opt_cls(model.parameters(), lr=1e-3, fused=True, device_step=True, **options)
    dp.attach(opt)
    tx, tt = hip.from_numpy(x), hip.from_numpy(onehot)

    def step():
        loss = light.loss.mse(model(tx), tt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    return model, opt, step


def mlp_recipe():
    return dict(weight_decay=WD, max_grad_norm=0.05, schedule=light.optim.WarmupLinear(3, 8))


@pytest.mark.parametrize("opt_cls", [light.optim.Adam, light.optim.AdaBelief], ids=["adam", "adabelief"])
def test_mlp_trajectory_with_the_whole_recipe(hip, opt_cls):
    w0, x, onehot, _ = O.synthetic_mlp_problem(4, DIMS[0], DIMS[1], DIMS[2], BATCH)
    make = lambda ps: opt_cls(ps, lr=1e-3, **mlp_recipe())      # noqa: E731
    _, ref64 = mlp_trajectory_on_cpu(w0, x, onehot, 6, make, np.float64)
    _, cpu32 = mlp_trajectory_on_cpu(w0, x, onehot, 6, make, np.float32)
    model, opt, step = mlp_on_hip(hip, w0, x, onehot, opt_cls, **mlp_recipe())
    for _ in range(6):
        step()
    got = {n: p.numpy() for n, p in model.named_parameters()}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, what="MLP")
    assert float(opt.grad_norm().item()) > 0


# ---- a captured step -----------------------------------------------------------------------------------------------------------
def test_replayed_graph_follows_the_schedule(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    w0, x, onehot, _ = O.synthetic_mlp_problem(6, DIMS[0], DIMS[1], DIMS[2], BATCH)

    def state(model, opt):
        return ([p.numpy().copy() for p in model.parameters()], opt._flat[1].numpy().copy(), opt._flat[2].numpy().copy(),
                opt.grad_norm().numpy().copy())

    model_e, opt_e, step_e = mlp_on_hip(hip, w0, x, onehot, light.optim.AdaBelief, **mlp_recipe())
    eager = []
    for _ in range(10):
        step_e()
        eager.append(state(model_e, opt_e))
    assert all(np.array_equal(a, b) for a, b in zip(eager[9][0], eager[7][0]))        # steps 9 and 10: factor 0, nothing moves
    assert not any(np.array_equal(a, b) for a, b in zip(eager[7][0], eager[6][0]))    # (step 8 still did)
    assert not np.array_equal(eager[9][1], eager[7][1])                               # ... while m keeps following the gradient

    model, opt, step = mlp_on_hip(hip, w0, x, onehot, light.optim.AdaBelief, **mlp_recipe())
    step()
    graph = HipGraph()
    with graph.capture():
        step()
    opt.t -= len(opt.parameters)                    # the capture pass ran the python bookkeeping, not the kernels
    for k in range(9):
        graph.replay()
        opt.on_graph_replay()
        got = state(model, opt)
        for a, b in zip(got[0], eager[k + 1][0]):
            np.testing.assert_array_equal(a, b, err_msg="parameters after step %d" % (k + 2))
        for a, b in zip(got[1:], eager[k + 1][1:]):
            np.testing.assert_array_equal(a, b, err_msg="m, v, norm after step %d" % (k + 2))
    assert opt.t == opt_e.t == 10 * len(opt.parameters)
    graph.destroy()


def test_launches_of_a_captured_step(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    w0, x, onehot, _ = O.synthetic_mlp_problem(6, DIMS[0], DIMS[1], DIMS[2], BATCH)
    counts = {}
    for name, options in (("neutral", {}), ("decay_schedule", dict(weight_decay=WD, schedule=light.optim.WarmupLinear(3, 8))),
                          ("clipping", mlp_recipe())):
        model, opt, step = mlp_on_hip(hip, w0, x, onehot, light.optim.AdaBelief, **options)
        step()
        graph = HipGraph()
        with graph.capture():
            step()
        counts[name] = graph.kernel_count()
        graph.destroy()
    assert counts["decay_schedule"] == counts["neutral"], counts                       # decay and schedule ride in the update launch
    assert counts["clipping"] == counts["neutral"] + 1, counts                         # the norm launch


# ---- guards ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("options", [dict(weight_decay=WD), dict(max_grad_norm=1.0), dict(schedule=light.optim.WarmupLinear(1, 2))],
                         ids=["decay", "clipping", "schedule"])
def test_forms_that_do_not_carry_the_recipe_refuse_it(hip, options):
    from lightgrad_amd.dist import DataParallel, SingleProcess
    params = [hip.from_numpy(np.ones((4, 3), np.float32)), hip.from_numpy(np.ones((3,), np.float32))]
    opt = light.optim.Adam(params, lr=LR, fused=True, device_step=True, **options)
    DataParallel(params, SingleProcess(), flatten=True).attach(opt)
    with pytest.raises(AssertionError, match="backward kernels"):
        opt.fuse_update_into_backward()
    with pytest.raises(AssertionError, match="exchange"):
        opt.use_peer_exchange(object())
    assert opt._backward_update is None and opt._peer_exchange is None


def test_fused_without_flat_buckets_takes_the_expression_form(hip):
    p0, grads = fixed_problem(((5, 3), (3,), (1025,)), 4, (0.01, 3.0, 0.02, 4.0), 17)
    recipe = dict(weight_decay=WD, max_grad_norm=1.0, schedule=light.optim.WarmupLinear(2, 5))
    results = []
    for fused in (False, True):
        params = [hip.from_numpy(a) for a in p0]
        opt = light.optim.AdaBelief(params, lr=LR, fused=fused, **recipe)
        for step_grads in grads:
            set_gradients(hip, opt, params, step_grads, np.float32)
            opt.step()
        results.append([p.numpy() for p in params] + [opt.grad_norm().numpy()])
    for a, b in zip(*results):
        np.testing.assert_array_equal(a, b)
    ref64, _ = run_on_cpu(light.optim.AdaBelief, p0, grads, np.float64, **recipe)
    cpu32, _ = run_on_cpu(light.optim.AdaBelief, p0, grads, np.float32, **recipe)
    got = {"p%d" % i: a for i, a in enumerate(results[1][:3])}
    assert_as_close_to_float64_as_the_cpu_backend(got, {k: cpu32[k] for k in got}, {k: ref64[k] for k in got}, what="expression form on HIP")
