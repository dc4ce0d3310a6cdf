"""bf16 products on the CPU backend: the rounding itself (exact bit patterns, torch's bfloat16 round trip), `dot_bf16` and
`linear_bf16` forward and backward against the float64 product of the rounded operands, and nn.Linear's `precision` switch."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from common import float64_tape
from bf16_cases import round_np, product64, operands, rel, TOL


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


def test_rounding_table():
    x = np.array([1.00390625, 1.01171875, 3.3895314e38, 3.4e38, -3.4e38, 0.0, -0.0, np.inf, -np.inf, 1.0, -2.5], np.float32)
    want = np.array([1.0, 1.015625, 3.3895314e38, np.inf, -np.inf, 0.0, -0.0, np.inf, -np.inf, 1.0, -2.5], np.float32)
    # 1 + 2^-8 lies halfway between 1 and 1 + 2^-7 (even: 1); 1 + 3 * 2^-8 halfway between 1 + 2^-7 and 1 + 2^-6 (even: the latter)
    np.testing.assert_array_equal(bits(round_np(x)), bits(want))
    assert bits(np.float32(3.3895314e38)) == 0x7F7F0000                       # the largest bfloat16
    nan = round_np(np.array([np.nan, -np.nan, 1.0], np.float32))
    assert np.isnan(nan[0]) and np.isnan(nan[1]) and nan[2] == 1.0
    assert np.all(bits(round_np(np.random.RandomState(0).uniform(-4, 4, 1000))) & 0xFFFF == 0)


def test_rounding_is_idempotent_and_is_torchs():
    import torch
    u = np.random.RandomState(1).randint(0, 2 ** 32, 150000, dtype=np.uint64).astype(np.uint32)
    f = u.view(np.float32)
    f = f[np.isfinite(f) & (np.abs(f) >= np.float32(2.0 ** -126))]            # finite, normal
    assert f.size >= 100000
    r = round_np(f)
    np.testing.assert_array_equal(bits(round_np(r)), bits(r))
    via_torch = torch.from_numpy(f.copy()).to(torch.bfloat16).to(torch.float32).numpy()
    np.testing.assert_array_equal(bits(r), bits(via_torch))


def test_bf16_round_is_a_constant_of_the_tape():
    t = CpuTensor.from_numpy(np.array([[1.00390625, 3.0]], np.float32))
    r = light.bf16_round(t)
    assert isinstance(r, CpuTensor) and not r.requires_grad and r.ctx is None and r.shape == (1, 2)
    np.testing.assert_array_equal(r.numpy(), [[1.0, 3.0]])
    np.testing.assert_array_equal(t.numpy(), np.array([[1.00390625, 3.0]], np.float32))       # the input is untouched


@pytest.mark.parametrize("mnk", [(33, 31, 35), (65, 129, 67), (16, 24, 3000), (5, 7, 8)])
def test_dot_bf16_forward_and_gradients(mnk):
    M, N, K = mnk
    a, b, ref = operands(M, N, K)
    w = np.random.RandomState(9).uniform(-1, 1, (M, N)).astype(np.float32)
    ta, tb = CpuTensor.from_numpy(a.copy()), CpuTensor.from_numpy(b.copy())
    y = ta.dot_bf16(tb)
    assert y.dtype == np.float32 and rel(y.numpy(), ref) <= TOL
    (y * CpuTensor.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
    assert rel(ta.grad.numpy(), product64(w, b.T)) <= TOL                      # dA = r(g) @ r(b)^T
    assert rel(tb.grad.numpy(), product64(a.T, w)) <= TOL                      # dB = r(a)^T @ r(g)
    # ... and it is NOT the fp32 product: 8 significand bits per operand leave about 2e-3 on uniform(-1, 1) data
    far = rel(y.numpy(), (CpuTensor.from_numpy(a.copy()) @ CpuTensor.from_numpy(b.copy())).numpy())
    assert far > 1e-4, far


def test_dot_bf16_tall_product():
    rng = np.random.RandomState(2)
    a, b = rng.uniform(-1, 1, (2, 3, 5, 16)).astype(np.float32), rng.uniform(-1, 1, (16, 9)).astype(np.float32)
    w = rng.uniform(-1, 1, (2, 3, 5, 9)).astype(np.float32)
    ta, tb = CpuTensor.from_numpy(a), CpuTensor.from_numpy(b)
    y = ta.dot_bf16(tb)
    assert y.shape == (2, 3, 5, 9) and rel(y.numpy(), product64(a.reshape(30, 16), b).reshape(2, 3, 5, 9)) <= TOL
    (y * CpuTensor.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
    assert ta.grad.shape == a.shape and rel(ta.grad.numpy(), product64(w.reshape(30, 9), b.T).reshape(a.shape)) <= TOL
    assert tb.grad.shape == b.shape and rel(tb.grad.numpy(), product64(a.reshape(30, 16).T, w.reshape(30, 9))) <= TOL


@pytest.mark.parametrize("x_shape", [(33, 35), (2, 17, 35)], ids=["2d", "bsh"])
@pytest.mark.parametrize("with_bias", [True, False], ids=["bias", "no-bias"])
def test_linear_bf16_forward_and_gradients(x_shape, with_bias):
    rng = np.random.RandomState(3)
    x, wt = rng.uniform(-1, 1, x_shape).astype(np.float32), rng.uniform(-1, 1, (31, 35)).astype(np.float32)
    bias = rng.uniform(-1, 1, (31,)).astype(np.float32)
    g = rng.uniform(-1, 1, x_shape[:-1] + (31,)).astype(np.float32)
    tx, tw, tb = CpuTensor.from_numpy(x), CpuTensor.from_numpy(wt), CpuTensor.from_numpy(bias)
    y = tx.linear_bf16(tw, tb) if with_bias else tx.linear_bf16(tw)
    x2, g2 = x.reshape(-1, 35), g.reshape(-1, 31)
    ref = product64(x2, wt.T) + (bias.astype(np.float64) if with_bias else 0.0)
    assert y.shape == g.shape and rel(y.numpy().reshape(-1, 31), ref) <= TOL
    if with_bias:
        # the sum is rounded to fp32 BEFORE the bias is added: the two-op form, bit for bit
        two_ops = CpuTensor.from_numpy(x).linear_bf16(CpuTensor.from_numpy(wt)).numpy() + bias
        np.testing.assert_array_equal(y.numpy(), two_ops)
    (y * CpuTensor.from_numpy(g, requires_grad=False)).backward(allow_fill=True)
    assert rel(tx.grad.numpy().reshape(-1, 35), product64(g2, wt)) <= TOL       # dx = r(g) @ r(W)
    assert rel(tw.grad.numpy(), product64(g2.T, x2)) <= TOL                     # dW = r(g)^T @ r(x)
    if with_bias:
        assert rel(tb.grad.numpy(), g2.astype(np.float64).sum(axis=0)) <= TOL   # db: the fp32 g, not rounded
        assert rel(tb.grad.numpy(), round_np(g2).astype(np.float64).sum(axis=0)) > 1e-4
    else:
        assert tb.grad is None


def test_float64_tape_rounds_the_operands_and_multiplies_in_double():
    a, b, ref = operands(33, 31, 35)
    with float64_tape():
        y = CpuTensor.from_numpy(a.astype(np.float64)).dot_bf16(CpuTensor.from_numpy(b.astype(np.float64)))
        z = CpuTensor.from_numpy(a.astype(np.float64)).linear_bf16(CpuTensor.from_numpy(np.ascontiguousarray(b.T).astype(np.float64)))
    assert y.dtype == np.float64 and rel(y.numpy(), ref) <= 1e-15
    assert z.dtype == np.float64 and rel(z.numpy(), ref) <= 1e-15


def _node_names(t):
    seen, names, stack = set(), [], [t.ctx]
    while stack:
        c = stack.pop()
        if c is None or id(c) in seen:
            continue
        seen.add(id(c))
        names.append(type(c).__name__)
        stack.extend(p.ctx for p in c.parent_tensors)
    return sorted(names)


def test_linear_precision_switch():
    rng = np.random.RandomState(4)
    x = rng.uniform(-1, 1, (6, 24)).astype(np.float32)
    np.random.seed(8)
    plain = light.nn.Linear(24, 10)
    np.random.seed(8)
    same = light.nn.Linear(24, 10, precision=None)
    np.random.seed(8)
    low = light.nn.Linear(24, 10, precision="bf16")
    np.testing.assert_array_equal(plain.weight.numpy(), low.weight.numpy())
    y_plain, y_same, y_low = (m(CpuTensor.from_numpy(x)) for m in (plain, same, low))
    composite = CpuTensor.from_numpy(x) @ plain.weight.T(1, 0) + plain.bias
    np.testing.assert_array_equal(y_same.numpy(), composite.numpy())                     # None: today's ops, today's bits
    assert _node_names(y_same) == _node_names(y_plain) == _node_names(composite) and "linear_bf16" not in _node_names(y_same)
    assert _node_names(y_low) == ["linear_bf16"]
    assert rel(y_low.numpy(), product64(x, low.weight.numpy().T) + low.bias.numpy()) <= TOL
    assert rel(y_low.numpy(), y_plain.numpy()) > 1e-4
    res = rng.uniform(-1, 1, (6, 10)).astype(np.float32)
    with_res = low(CpuTensor.from_numpy(x), residual=CpuTensor.from_numpy(res))
    np.testing.assert_array_equal(with_res.numpy(), y_low.numpy() + res)                 # the ordinary `+`
    for bad in ("fp16", "bfloat16", 16, ""):
        with pytest.raises(ValueError):
            light.nn.Linear(24, 10, precision=bad)


def test_rank_and_dtype_errors():
    f = lambda *s: CpuTensor.from_numpy(np.ones(s, np.float32))      # noqa: E731
    for a, b in [(f(4), f(4, 3)), (f(2, 4), f(4)), (f(2, 4), f(2, 4, 3)), (f(2, 3, 4), f(2, 4, 5))]:
        with pytest.raises(ValueError):
            a.dot_bf16(b)
    with pytest.raises(ValueError):
        f(2, 5).dot_bf16(f(4, 3))                                    # K mismatch
    with pytest.raises(ValueError):
        f(4).linear_bf16(f(3, 4))
    i32 = CpuTensor.from_numpy(np.ones((4, 3), np.int32))
    f64 = CpuTensor.from_numpy(np.ones((4, 3), np.float64))
    for other in (i32, f64):
        with pytest.raises(TypeError):
            f(2, 4).dot_bf16(other)
        with pytest.raises(TypeError):
            f(2, 3).linear_bf16(other)
