"""conv2d on the CPU backend (no GPU): the op exists, equals the composite `pad -> conv -> + bias` bit for bit, sits within 1e-5
(relative Frobenius) of a direct float64 loop for the output and all three gradients, and the C ABI declares and binds the
kernels behind HipTensor.conv2d / max_pool / min_pool with matching argument counts."""
import os
import re
import numpy as np
import pytest
from conftest import ROOT
from lightgrad_amd import CpuTensor
import lightgrad_amd.nn as nn
from common import rel_frobenius
from conv2d_cases import CASES, IDS, draw, run_tape, direct_float64

NEW_ENTRY_POINTS = {"lg_conv2d_fwd_f32": 15, "lg_conv2d_dx_f32": 13, "lg_conv2d_dw_f32": 15, "lg_conv2d_last_plan": 1,
                    "lg_pool2d_fwd_f32": 8, "lg_pool2d_bwd_f32": 9}


def composite_tape(case, arrays):
    x, w, b, g = (None if a is None else CpuTensor.from_numpy(a) for a in arrays)
    g._requires_grad = False
    y = (x.pad(case[8]) if case[8] else x).conv(w, strides=case[7])
    if b is not None:
        y = y + b
    (y * g).sum().backward()
    out = {"y": y.numpy(), "dx": x.grad.numpy(), "dw": w.grad.numpy()}
    if b is not None:
        out["db"] = b.grad.numpy()
    return out


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_cpu_conv2d_is_the_composite_and_close_to_the_definition(case):
    arrays = draw(case, 7)
    got, composite, exact = run_tape(CpuTensor, case, arrays), composite_tape(case, arrays), direct_float64(case, arrays)
    assert sorted(got) == sorted(exact) == sorted(composite)
    for name in exact:
        assert got[name].dtype == np.float32 and got[name].shape == exact[name].shape, name
        np.testing.assert_array_equal(got[name], composite[name], err_msg=name)
        assert rel_frobenius(got[name], exact[name]) <= 1e-5, (name, rel_frobenius(got[name], exact[name]))


def test_bias_as_a_vector_and_the_module():
    case = CASES[3]
    x, w, b, g = draw(case, 11)
    ref = run_tape(CpuTensor, case, (x, w, b, g))
    got = run_tape(CpuTensor, case, (x, w, b.reshape(-1), g))
    assert got["db"].shape == (case[4],)
    for name in ref:
        np.testing.assert_array_equal(got[name].reshape(ref[name].shape), ref[name], err_msg=name)
    layer = nn.Conv2d(3, 5, kernelsize=3, stride=2, pad=1)
    xt = CpuTensor.from_numpy(x)
    y = layer(xt)
    expect = xt.pad(1).conv(layer.w, strides=2) + layer.b
    np.testing.assert_array_equal(y.numpy(), expect.numpy())


@pytest.mark.parametrize("i", [3, 5, 9])
def test_tap_by_tap_composite_of_the_hip_backend_is_the_definition(i):
    """what HipTensor.conv2d uses for float64 operands is backend-independent tape code: run here on CpuTensor in float64"""
    from lightgrad_amd.autograd.hip.ops import _conv2d_by_taps
    from common import float64_tape
    case, arrays = CASES[i], draw(CASES[i], 13)
    with float64_tape():
        x, w, b, g = (None if a is None else CpuTensor.from_numpy(a.astype(np.float64)) for a in arrays)
        y = _conv2d_by_taps(x, w, b, stride=case[7], pad=case[8])
        (y * g).sum().backward()
    exact = direct_float64(case, arrays)
    got = {"y": y.numpy(), "dx": x.grad.numpy(), "dw": w.grad.numpy()}
    if b is not None:
        got["db"] = b.grad.numpy()
    for name in exact:
        assert got[name].dtype == np.float64
        assert rel_frobenius(got[name], exact[name]) <= 1e-13, (name, rel_frobenius(got[name], exact[name]))


def test_header_declares_and_binding_prototypes_the_new_entry_points():
    from lightgrad_amd.autograd.hip import lib as hiplib
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRY_POINTS.items():
        m = re.search(r"^int %s\((.*?)\);" % name, text, re.M | re.S)
        assert m, name
        assert len(m.group(1).split(",")) == n_args, (name, m.group(1))
        restype, argtypes = hiplib.PROTOTYPES[name]
        assert len(argtypes) == n_args, name
    assert "conv.hip" in open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()
