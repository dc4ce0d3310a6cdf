"""batch_norm / batch_norm_infer on the CPU backend (no GPU), the module buffers and the BatchNorm layers.

Error rule: the float64 tape of the composite is the yardstick once it is shown to be the definition (a direct numpy float64
formula, 1e-12: two float64 evaluations whose sums of at most 43264 terms run in different orders).  A float32 result is then within
1e-5 (relative Frobenius) of it, or no further from it than twice what the same two-pass formula evaluated by numpy in float32 is
(`e_cpu32`): the error the number format itself leaves."""
import os
import re
import numpy as np
import pytest
from conftest import ROOT
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from common import check_gradients, float64_tape, rel_frobenius
from batchnorm_cases import CASES, IDS, draw, run_tape, direct, direct_infer, run_infer_tape

NEW_ENTRY_POINTS = {"lg_batchnorm_fwd_f32": 14, "lg_batchnorm_bwd_f32": 12, "lg_batchnorm_infer_f32": 11, "lg_batchnorm_last_plan": 1}


def assert_within_yardstick(got, base32, f64, what):
    for name in got:
        e_got, e_base = rel_frobenius(got[name], f64[name]), rel_frobenius(base32[name], f64[name])
        print("%s %s: composite %.3g numpy float32 %.3g" % (what, name, e_got, e_base))
        assert got[name].shape == f64[name].shape and got[name].dtype == np.float32, (what, name)
        assert e_got <= max(1e-5, 2 * e_base), (what, name, e_got, e_base)


@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_composite_against_numpy(i):
    arrays = draw(CASES[i], 40 + i)
    exact = direct(arrays, np.float64, calls=3)
    with float64_tape():
        tape64 = run_tape(CpuTensor, arrays, np.float64, calls=3)
    for name in tape64:
        assert tape64[name].dtype == np.float64
        assert rel_frobenius(tape64[name], exact[name]) <= 1e-12, (name, rel_frobenius(tape64[name], exact[name]))
    got = run_tape(CpuTensor, arrays, calls=3)
    assert sorted(got) == sorted(tape64) and "running_var" in got and ("dw" in got) == CASES[i][1]
    assert_within_yardstick(got, direct(arrays, np.float32, calls=3), exact, IDS[i])


def test_composite_on_inputs_far_from_zero():
    """randn + 100: the two-pass composite stays at the float32 two-pass error (about 1e-5 of the float64 result)"""
    arrays = draw(CASES[8], 3, offset=100.0)
    got = run_tape(CpuTensor, arrays, calls=3)
    assert_within_yardstick(got, direct(arrays, np.float32, calls=3), direct(arrays, np.float64, calls=3), "offset 100")


def test_infer_against_numpy():
    for i in (1, 3, 4, 9):
        arrays = draw(CASES[i], 60 + i)
        c = CASES[i][0][1]
        rng = np.random.RandomState(i)
        rm, rv = rng.uniform(-1, 1, c).astype(np.float32), rng.uniform(0.5, 2, c).astype(np.float32)
        exact = direct_infer(arrays, rm, rv)
        with float64_tape():
            tape64 = run_infer_tape(CpuTensor, arrays, rm, rv, np.float64)
        for name in tape64:
            assert rel_frobenius(tape64[name], exact[name]) <= 1e-12, name
        assert_within_yardstick(run_infer_tape(CpuTensor, arrays, rm, rv), direct_infer(arrays, rm, rv, np.float32), exact, IDS[i])


def test_gradient_check_of_both_ops():
    np.random.seed(5)
    # eps of the op at 1e-2 keeps the second derivative small enough for central differences with a step of 1e-3
    check_gradients(CpuTensor, lambda x, w, b: x.batch_norm(w, b, eps=1e-2), shapes=[(4, 3, 2, 3), (3,), (3,)])
    check_gradients(CpuTensor, lambda x, w, b: x.batch_norm(w, b, eps=1e-2), shapes=[(6, 3), (3,), (3,)])
    check_gradients(CpuTensor, lambda x: x.batch_norm(None, None, eps=1e-2), shapes=[(3, 2, 5)])
    rm = CpuTensor.from_numpy(np.array([0.3, -0.2, 0.1], np.float32), requires_grad=False)
    rv = CpuTensor.from_numpy(np.array([0.5, 1.5, 1.0], np.float32), requires_grad=False)
    check_gradients(CpuTensor, lambda x, w, b: x.batch_norm_infer(w, b, rm, rv), shapes=[(4, 3, 2, 3), (3,), (3,)])
    check_gradients(CpuTensor, lambda x: x.batch_norm_infer(None, None, rm, rv), shapes=[(5, 3)])


class Net(nn.Module):
    def __init__(self):
        nn.Module.__init__(self)
        self.conv = nn.Conv2d(1, 3, kernelsize=3, pad=0)
        self.bn = nn.BatchNorm2d(3)
        self.head = nn.ModuleList(nn.BatchNorm1d(4, affine=False), nn.Linear(4, 2))

    def forward(self, x):
        h = self.bn(self.conv(x)).relu()
        h = h.sum(axis=(2, 3)) @ CpuTensor.from_numpy(np.ones((3, 4), np.float32), requires_grad=False)
        return self.head[1](self.head[0](h))


def test_buffers_are_not_parameters():
    np.random.seed(0)
    net = Net()
    names = [n for n, _ in net.named_parameters()]
    assert names == ["conv.w", "conv.b", "bn.weight", "bn.bias", "head.1.weight", "head.1.bias"]
    assert [n for n, _ in net.named_buffers()] == ["bn.running_mean", "bn.running_var", "head.0.running_mean", "head.0.running_var"]
    assert [n for n, _ in net.named_buffers("m", "/")] == ["m/bn/running_mean", "m/bn/running_var", "m/head/0/running_mean",
                                                            "m/head/0/running_var"]
    params, buffers = list(net.parameters()), list(net.buffers())
    assert len(params) == 6 and len(buffers) == 4
    assert not any(b is p for b in buffers for p in params)
    assert all(not b.requires_grad for b in buffers) and all(p.requires_grad for p in params)
    assert net.bn.running_mean is buffers[0] and net.bn.weight.shape == (3,) and net.bn.running_var.shape == (3,)
    np.testing.assert_array_equal(net.bn.weight.numpy(), np.ones(3, np.float32))
    np.testing.assert_array_equal(net.bn.bias.numpy(), np.zeros(3, np.float32))
    np.testing.assert_array_equal(net.bn.running_mean.numpy(), np.zeros(3, np.float32))
    np.testing.assert_array_equal(net.bn.running_var.numpy(), np.ones(3, np.float32))
    assert net.head[0].weight is None and net.head[0].bias is None
    # load_parameters keeps its contract: it neither needs nor touches a buffer
    net.load_parameters([(n, p.numpy() * 2) for n, p in net.named_parameters()])
    assert [n for n, _ in net.named_parameters()] == names
    np.testing.assert_array_equal(net.bn.weight.numpy(), np.full(3, 2, np.float32))
    np.testing.assert_array_equal(net.bn.running_var.numpy(), np.ones(3, np.float32))


def test_map_parameters_moves_buffers_and_load_buffers_round_trips():
    np.random.seed(1)
    net = Net()
    seen = []

    def moved(t):
        seen.append(t)
        return CpuTensor.from_numpy(t.numpy() + 1)
    before = list(net.parameters()) + list(net.buffers())
    net.map_parameters(moved)
    assert len(seen) == 10 and all(any(s is b for s in seen) for b in before)
    assert [n for n, _ in net.named_buffers()] == ["bn.running_mean", "bn.running_var", "head.0.running_mean", "head.0.running_var"]
    assert len(list(net.parameters())) == 6
    np.testing.assert_array_equal(net.bn.running_mean.numpy(), np.ones(3, np.float32))
    np.testing.assert_array_equal(net.bn.running_var.numpy(), np.full(3, 2, np.float32))
    assert all(not b.requires_grad for b in net.buffers())                       # a mapped buffer is still one
    x = CpuTensor.from_numpy(np.random.uniform(-1, 1, (5, 1, 6, 6)).astype(np.float32), requires_grad=False)
    net(x).sum().backward()
    state = {n: b.numpy().copy() for n, b in net.named_buffers()}
    assert not np.array_equal(state["bn.running_mean"], np.ones(3, np.float32))
    other = Net()
    other.load_buffers(state)
    for (n, b), (_, a) in zip(other.named_buffers(), net.named_buffers()):
        np.testing.assert_array_equal(b.numpy(), a.numpy(), err_msg=n)
        assert not b.requires_grad
    other.load_buffers(dict(net.named_buffers("p")), prefix="p")                     # tensors, with a prefix
    with pytest.raises(AssertionError, match="running_var"):
        other.load_buffers({n: a for n, a in state.items() if n != "bn.running_var"})
    with pytest.raises(AssertionError, match="shape"):
        other.load_buffers(dict(state, **{"bn.running_mean": np.zeros(4, np.float32)}))
    # no optimizer ever sees a buffer, and the default decay mask leaves the (C,) parameters alone
    import lightgrad_amd as light
    opt = light.optim.AdaBelief(net.parameters(), lr=1e-3)
    assert len(opt.parameters) == 6 and not any(b is p for b in net.buffers() for p in opt.parameters)


def test_modes_and_errors():
    np.random.seed(2)
    xa = np.random.standard_normal((6, 3, 4, 5)).astype(np.float32)
    layer = nn.BatchNorm2d(3, eps=1e-3, momentum=0.25)
    x = CpuTensor.from_numpy(xa)
    y = layer(x)
    mean, var = xa.mean(axis=(0, 2, 3)), xa.var(axis=(0, 2, 3))
    np.testing.assert_allclose(layer.running_mean.numpy(), 0.25 * mean, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(layer.running_var.numpy(), 0.75 + 0.25 * var * 120 / 119, rtol=1e-5)
    np.testing.assert_allclose(y.numpy(), (xa - mean.reshape(1, 3, 1, 1)) / np.sqrt(var.reshape(1, 3, 1, 1) + 1e-3), rtol=1e-4, atol=1e-5)
    rm, rv = layer.running_mean.numpy().copy(), layer.running_var.numpy().copy()
    assert layer.eval() is layer and not layer.training
    y_eval = layer(x)
    np.testing.assert_array_equal(layer.running_mean.numpy(), rm)                # evaluation leaves the buffers alone
    np.testing.assert_array_equal(layer.running_var.numpy(), rv)
    np.testing.assert_array_equal(y_eval.numpy(), x.batch_norm_infer(layer.weight, layer.bias, layer.running_mean, layer.running_var,
                                                                     eps=1e-3).numpy())
    np.testing.assert_allclose(y_eval.numpy(), (xa - rm.reshape(1, 3, 1, 1)) / np.sqrt(rv.reshape(1, 3, 1, 1) + 1e-3), rtol=1e-4, atol=1e-5)
    y_eval.sum().backward()
    assert layer.running_mean.grad is None and layer.weight.grad is not None and x.grad is not None
    layer.train()
    layer(x)
    assert not np.array_equal(layer.running_mean.numpy(), rm)
    # momentum = 1: the running statistics ARE the batch's
    last = nn.BatchNorm1d(3, momentum=1.0)
    last(CpuTensor.from_numpy(xa.reshape(6, 3, 20)))
    np.testing.assert_allclose(last.running_mean.numpy(), mean, rtol=1e-5, atol=1e-7)
    # one value per channel, momenta outside (0, 1], ranks the layers do not take
    with pytest.raises(ValueError, match="more than one value"):
        CpuTensor.from_numpy(xa[:1, :, :1, :1]).batch_norm(None, None)
    with pytest.raises(ValueError, match="more than one value"):
        nn.BatchNorm1d(3)(CpuTensor.from_numpy(xa[:1, :, 0, 0]))
    nn.BatchNorm1d(3).eval()(CpuTensor.from_numpy(xa[:1, :, 0, 0]))              # evaluation of one sample is fine
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="momentum"):
            x.batch_norm(None, None, momentum=bad)
        with pytest.raises(ValueError, match="momentum"):
            nn.BatchNorm2d(3, momentum=bad)
    with pytest.raises(AssertionError):
        nn.BatchNorm2d(3)(CpuTensor.from_numpy(xa.reshape(6, 3, 20)))
    with pytest.raises(AssertionError):
        nn.BatchNorm1d(3)(x)
    with pytest.raises(AssertionError):
        nn.BatchNorm2d(4)(x)


def test_header_declares_and_binding_prototypes_the_new_entry_points():
    from lightgrad_amd.autograd.hip import lib as hiplib
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRY_POINTS.items():
        m = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        assert len(hiplib.PROTOTYPES[name][1]) == n_args, name
    assert "batchnorm.hip" in open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()
