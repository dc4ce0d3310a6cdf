"""Adam / AdaBelief with the rest of a training recipe - decoupled weight decay, clipping by the global gradient norm, a
warmup / linear-decay schedule (lightgrad_amd/optim.py) - in the expression form, which defines it on every backend.
The yardstick is a straight-line float64 numpy restatement written here, which never calls optim.py."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd import Gradients
from common import float64_tape, mlp_trajectory_on_cpu, assert_as_close_to_float64_as_the_cpu_backend
import np_oracle as O

SHAPES = ((3, 5), (5,), (7, 3))
STEPS, LR, WD, MAX_NORM = 6, 1e-2, 0.1, 1.0
GRAD_SIZES = (0.1, 3.0, 0.2, 4.0, 0.1, 5.0)      # gradient norms of about 0.37 and 11 to 18: below and above MAX_NORM in turn


def problem():
    rng = np.random.RandomState(20261018)
    p0 = [rng.uniform(-1, 1, s) for s in SHAPES]
    grads = [[size * rng.uniform(-1, 1, s) for s in SHAPES] for size in GRAD_SIZES]
    return p0, grads


def warmup_linear(s, warmup, total):
    if s < warmup:
        return (s + 1) / warmup
    return max(0.0, (total - s) / max(1, total - warmup))


def numpy_recipe(p0, grads, belief, decays, warmup=2, total=5, b1=0.9, b2=0.999, eps=1e-8, dtype=np.float64):
    """one statement per line of the recipe's definition, in float64 (the yardstick) or float32 (a companion for the float32 run);
    returns (parameters, m, v, norm, coef) after every step"""
    p = [a.astype(dtype).copy() for a in p0]
    m = [np.zeros_like(a) for a in p]
    v = [np.zeros_like(a) for a in p]
    t, history = 0, []
    for s, step_grads in enumerate(grads):
        g = [a.astype(dtype) for a in step_grads]
        norm = float(np.sqrt(sum(np.sum(a * a) for a in g)))
        coef = min(1.0, MAX_NORM / (norm + 1e-6))
        g = [a * coef for a in g]
        lr_s = LR * warmup_linear(s, warmup, total)
        for i in range(len(p)):
            t += 1                                                   # once per PARAMETER: the reference's quirk
            m[i] = b1 * m[i] + (1 - b1) * g[i]
            surprise = g[i] - m[i] if belief else g[i]
            v[i] = b2 * v[i] + (1 - b2) * surprise ** 2
            mh, vh = m[i] / (1 - b1 ** t), v[i] / (1 - b2 ** t)
            delta = -lr_s * mh / (np.sqrt(vh) + eps)
            if decays[i]:
                delta = delta - lr_s * WD * p[i]
            p[i] = p[i] + delta
        history.append(([a.copy() for a in p], [a.copy() for a in m], [a.copy() for a in v], norm, coef))
    return history


def run_expression_form(opt_cls, p0, grads, dtype, **options):
    """the same steps through optim.py on CpuTensor in `dtype`; (parameters, m, v, grad_norm) after every step"""
    def run():
        params = [CpuTensor.from_numpy(a.astype(dtype)) for a in p0]
        opt = opt_cls(params, lr=LR, **options)
        history = []
        for step_grads in grads:
            opt.zero_grad()
            with Gradients.no_grad():
                for p, g in zip(params, step_grads):
                    p.grad[...] = CpuTensor.from_numpy(g.astype(dtype), requires_grad=False)
            opt.step()
            norm = opt.grad_norm() if opt.max_grad_norm is not None else None
            if norm is not None:
                assert norm.shape == () and isinstance(norm, CpuTensor) and norm.dtype == dtype
            history.append(([p.numpy().copy() for p in params], [m.numpy().copy() for m in opt.m], [v.numpy().copy() for v in opt.v],
                            None if norm is None else float(norm.item())))
        assert opt.t == len(grads) * len(params)
        return history
    if np.dtype(dtype) == np.float64:
        with float64_tape():
            return run()
    return run()


RECIPE = dict(weight_decay=WD, max_grad_norm=MAX_NORM, schedule=light.optim.WarmupLinear(2, 5))


@pytest.mark.parametrize("warmup,total", [(3, 8), (0, 4), (4, 4)])
def test_warmup_linear_factor(warmup, total):
    sched = light.optim.WarmupLinear(warmup, total)
    for s in (0, warmup - 1, warmup, total - 1, total, total + 5):
        if s < 0:
            continue
        if s < warmup:
            expected = (s + 1) / warmup
        elif s >= total:
            expected = 0.0
        else:
            expected = (total - s) / max(1, total - warmup)
        got = sched.factor(s)
        assert isinstance(got, float) and got == expected, (warmup, total, s, got, expected)
        assert 0.0 <= got <= 1.0
    if warmup > 0:
        assert sched.factor(warmup - 1) == 1.0                  # the last warmup step reaches the full learning rate
    if warmup < total:
        assert sched.factor(warmup) == 1.0                      # ... and the decay starts from it
    for bad in ((-1, 4), (5, 4)):
        with pytest.raises(AssertionError):
            light.optim.WarmupLinear(*bad)


@pytest.mark.parametrize("opt_cls", [light.optim.Adam, light.optim.AdaBelief], ids=["adam", "adabelief"])
def test_expression_form_against_a_numpy_restatement(opt_cls):
    p0, grads = problem()
    ref = numpy_recipe(p0, grads, opt_cls.belief, decays=(True, False, True))
    coefs = [h[4] for h in ref]
    assert any(c < 1.0 for c in coefs) and any(c == 1.0 for c in coefs), coefs       # clipping active on some steps, not on others
    got64 = run_expression_form(opt_cls, p0, grads, np.float64, **RECIPE)
    for (p, m, v, norm), (rp, rm, rv, rnorm, _) in zip(got64, ref):
        for a, b in zip(p + m + v, rp + rm + rv):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
        np.testing.assert_allclose(norm, rnorm, rtol=1e-12)                          # the norm BEFORE clipping
    # float32: as close to the float64 result as float32 arithmetic gets - the companion is the restatement above in float32
    got32 = run_expression_form(opt_cls, p0, grads, np.float32, **RECIPE)
    ref32 = numpy_recipe(p0, grads, opt_cls.belief, decays=(True, False, True), dtype=np.float32)
    names = ["p%d" % i for i in range(len(p0))]
    for step in range(STEPS):
        for k, what in enumerate(("parameters", "m", "v")):
            assert all(a.dtype == np.float32 for a in got32[step][k])
            assert_as_close_to_float64_as_the_cpu_backend(dict(zip(names, got32[step][k])), dict(zip(names, ref32[step][k])),
                                                          dict(zip(names, ref[step][k])), what="float32 %s after step %d" % (what, step + 1))
    np.testing.assert_allclose([h[3] for h in got32], [h[3] for h in ref], rtol=1e-6)


@pytest.mark.parametrize("opt_cls", [light.optim.Adam, light.optim.AdaBelief], ids=["adam", "adabelief"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_a_step_with_factor_zero_moves_the_moments_only(opt_cls, dtype):
    p0, grads = problem()
    assert light.optim.WarmupLinear(2, 5).factor(5) == 0.0
    h = run_expression_form(opt_cls, p0, grads, dtype, **RECIPE)
    for a, b in zip(h[5][0], h[4][0]):
        np.testing.assert_array_equal(a, b)                                          # step 6: parameters bit-unchanged
    for k in (1, 2):
        for a, b in zip(h[5][k], h[4][k]):
            assert np.all(a != b)                                                    # m and v still follow the gradient
    for a, b in zip(h[4][0], h[3][0]):
        assert np.all(a != b)                                                        # (step 5 did move the parameters)


def test_decay_mask():
    p0, grads = problem()
    default = run_expression_form(light.optim.Adam, p0, grads[:2], np.float64, weight_decay=WD)
    explicit = run_expression_form(light.optim.Adam, p0, grads[:2], np.float64, weight_decay=WD, decay_mask=(True, False, True))
    flipped = run_expression_form(light.optim.Adam, p0, grads[:2], np.float64, weight_decay=WD, decay_mask=[False, True, False])
    plain = run_expression_form(light.optim.Adam, p0, grads[:2], np.float64)
    for i, decays_by_default in enumerate((True, False, True)):
        np.testing.assert_array_equal(default[-1][0][i], explicit[-1][0][i])         # None = "2 or more dimensions"
        same_as_plain = np.array_equal(flipped[-1][0][i], plain[-1][0][i])
        assert same_as_plain == decays_by_default                                    # the explicit mask overrides the default
        assert np.array_equal(default[-1][0][i], plain[-1][0][i]) == (not decays_by_default)
    params = [CpuTensor.from_numpy(a.astype(np.float32)) for a in p0]
    with pytest.raises(AssertionError, match="decay_mask"):
        light.optim.Adam(params, lr=LR, weight_decay=WD, decay_mask=(True, False))
    light.optim.Adam(params, lr=LR, weight_decay=0.0, decay_mask=(True, False))      # ignored without a decay


@pytest.mark.parametrize("opt_cls", [light.optim.Adam, light.optim.AdaBelief], ids=["adam", "adabelief"])
def test_neutral_options_change_no_bit(opt_cls):
    w0, x, onehot, _ = O.synthetic_mlp_problem(4, 16, 8, 4, 8)
    before = mlp_trajectory_on_cpu(w0, x, onehot, 5, lambda ps: opt_cls(ps, lr=1e-3), np.float32)
    after = mlp_trajectory_on_cpu(w0, x, onehot, 5, lambda ps: opt_cls(ps, lr=1e-3, weight_decay=0.0, decay_mask=None, max_grad_norm=None,
                                                                        schedule=None), np.float32)
    np.testing.assert_array_equal(before[0], after[0])
    for n in before[1]:
        np.testing.assert_array_equal(before[1][n], after[1][n], err_msg=n)


def test_grad_norm_is_the_norm_before_clipping():
    p0, grads = problem()
    for dtype, rtol in ((np.float64, 1e-14), (np.float32, 1e-6)):
        h = run_expression_form(light.optim.Adam, p0, grads, dtype, max_grad_norm=MAX_NORM)
        expected = [np.sqrt(sum(np.sum(g.astype(dtype).astype(np.float64) ** 2) for g in step_grads)) for step_grads in grads]
        assert max(expected) > 10 * MAX_NORM                                         # clipped steps report the unclipped norm
        np.testing.assert_allclose([s[3] for s in h], expected, rtol=rtol)
    opt = light.optim.Adam([CpuTensor.from_numpy(p0[0].astype(np.float32))], lr=LR)
    with pytest.raises(AssertionError, match="max_grad_norm"):
        opt.grad_norm()
