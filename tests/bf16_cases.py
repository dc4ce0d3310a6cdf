"""Shapes, operands and references shared by tests/test_bf16_cpu.py and tests/test_hip_bf16.py.

The reference of a bf16 product is the float64 product of the operands after `lightgrad_amd.bf16_round`: products of two
bfloat16 values are exact in fp32 (and in float64), so only the order and the fp32 rounding of the SUM separate an
implementation from it.  References are computed once per shape and handed out read-only."""
import functools
import importlib.util
import os
import numpy as np
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, N, K): the smallest shapes at which a 128 x 128 tile walked in 32-deep steps can go wrong - one element, less than one
# MFMA tile, odd sizes around 32 / 64 / 128, exactly one tile, more than one workgroup in M and in N, a long K on one tile
# (the chunks along K and their fold), a short K under many rows
SHAPES = [(1, 1, 1), (3, 5, 2), (33, 31, 35), (65, 129, 67), (128, 128, 128), (129, 127, 33), (16, 24, 3000), (257, 130, 8)]
K_SWEEP = [1, 7, 8, 15, 16, 17, 31, 32, 33, 65]            # at (40, 72, K): around the float4, the MFMA step (16) and the tile step (32)
LAYOUTS = [(0, 0, "NN"), (0, 1, "NT"), (1, 0, "TN"), (1, 1, "TT")]
TOL = 1e-5                                                 # relative Frobenius; fp32 accumulation of exact products measures 9e-9 .. 2.2e-7


def round_np(x):
    """r(x) through the public entry point on the CPU backend"""
    return light.bf16_round(CpuTensor.from_numpy(np.ascontiguousarray(x, dtype=np.float32), requires_grad=False)).numpy()


def product64(a, b):
    return round_np(a).astype(np.float64) @ round_np(b).astype(np.float64)


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def operands(M, N, K):
    """(a (M, K), b (K, N), float64 reference) on uniform(-1, 1) data"""
    rng = np.random.RandomState(M * 7 + K * 3 + N)
    a, b = rng.uniform(-1, 1, (M, K)).astype(np.float32), rng.uniform(-1, 1, (K, N)).astype(np.float32)
    return _frozen(a, b, product64(a, b))


@functools.lru_cache(maxsize=None)
def integer_operands(M, N, K):
    """operands of integers in [-8, 8] with K <= 256: every partial sum stays below 2^24, so ANY summation order gives numpy's
    integer product bit for bit"""
    assert K <= 256
    rng = np.random.RandomState(M + 31 * N + 977 * K)
    a, b = rng.randint(-8, 9, (M, K)), rng.randint(-8, 9, (K, N))
    return _frozen(a.astype(np.float32), b.astype(np.float32), (a @ b).astype(np.float32))


def rel(got, ref):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


def assert_close_to_product(got, ref, K, what):
    err = rel(got, ref)
    print("%s: %.3g" % (what, err))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert err <= TOL, (what, err)
    np.testing.assert_allclose(got, ref, rtol=0, atol=1e-5 * K ** 0.5, err_msg=str(what))


class TwoLayer(nn.Module):
    """Linear(24, 40, precision) -> relu -> Linear(40, 10)"""

    def __init__(self, precision):
        nn.Module.__init__(self)
        self.l1 = nn.Linear(24, 40, precision=precision)
        self.l2 = nn.Linear(40, 10)

    def forward(self, x):
        return self.l2(self.l1(x).relu())


def two_layer_problem(seed=4, batch=16):
    rng = np.random.RandomState(seed)
    w0 = {"l1.weight": rng.uniform(-1, 1, (40, 24)) / 6, "l1.bias": rng.uniform(-1, 1, (40,)) / 6,
          "l2.weight": rng.uniform(-1, 1, (10, 40)) / 6, "l2.bias": rng.uniform(-1, 1, (10,)) / 6}
    w0 = {n: a.astype(np.float32) for n, a in w0.items()}
    return w0, rng.uniform(-1, 1, (batch, 24)).astype(np.float32), rng.uniform(-1, 1, (batch, 10)).astype(np.float32)


def load_bert_example():
    spec = importlib.util.spec_from_file_location("bert_example_bf16", os.path.join(ROOT, "examples", "bert.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


BERT_IDS = np.random.RandomState(77).randint(1000, 30522, (2, 128)).astype(np.int32)
BERT_SEED = 5


def tiny_bert(bert, decoder_precision, seed=42):
    np.random.seed(seed)
    return bert.BertForMaskedLM(**dict(bert.TINY, decoder_precision=decoder_precision))


def bert_mlm_step(bert, model, T):
    """loss and every parameter gradient (float64 arrays) of one masked-LM step of examples/bert.py on batch 2"""
    light.manual_seed(BERT_SEED)
    loss = bert.mlm_forward_backward(model, T.from_numpy(BERT_IDS, requires_grad=False))
    out = {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}
    out["loss"] = np.asarray(loss.item(), np.float64)
    return out


def bert_cpu_yardsticks(bert, decoder_precision="bf16"):
    """(parameter values, float32 CPU step, float64 CPU step of the same tape in the same bf16 mode)"""
    from common import float64_tape
    model = tiny_bert(bert, decoder_precision)
    values = {n: p.numpy().copy() for n, p in model.named_parameters()}
    cpu32 = bert_mlm_step(bert, model, CpuTensor)
    with float64_tape():
        ref_model = tiny_bert(bert, decoder_precision)
        ref_model.load_parameters({n: a.astype(np.float64) for n, a in values.items()})
        assert all(p.dtype == np.float64 for p in ref_model.parameters())
        ref64 = bert_mlm_step(bert, ref_model, CpuTensor)
    return values, cpu32, ref64
