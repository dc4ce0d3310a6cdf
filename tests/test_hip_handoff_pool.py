"""Every kernel family that folds across workgroups inside its launch (csrc/handoff.h), back to back in ONE process: each leaves
the shared ticket pool at zero for the next, different user.

The other tests check each family on its own.  Here every family runs at the smallest shape of its `*_cases.py` that takes its
split path (asserted through the family's `*_last_plan` where it has one), the whole sequence forwards, then in reverse order,
then forwards again.  A ticket that one family left non-zero makes the last workgroup of the next user of that word miss its
turn: its output is then not written, or folded from fewer partials.  Every output of the second and third pass must equal
the first pass bit for bit, and the first pass is within the family's own tolerance of the float64 numpy value (or equal to
it, for integers), computed here."""
import ctypes
import numpy as np
import pytest
import reduce_cases as RC
import argreduce_cases as AC
import batchnorm_cases as BC
import conv2d_cases as CC
import rowwise_cases as WC
from lightgrad_amd import CpuTensor
from common import rel_frobenius
from test_metrics_cpu import batch as top1_batch, restated as top1_restated, run as top1_run

pytestmark = pytest.mark.gpu

FLOOR = 1e-5                         # the rule of tests/common.py: within FLOOR of float64, or twice the float32 reference's distance


@pytest.fixture(scope="module")
def L(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    hiplib.lib()
    return hiplib


class Family(object):
    """run() -> {name: numpy array}; exact: {name: array} the outputs must equal; close: {name: (float64, bound)}"""

    def __init__(self, name, run, exact=None, close=None):
        self.name, self.run, self.exact, self.close = name, run, exact or {}, close or {}


def yardstick(ref64, base32):
    return ref64, max(FLOOR, 2 * rel_frobenius(base32, ref64))


def reduce_family(hip, L, case_name, family):
    c = RC.BY_NAME[case_name]
    flat, ref64, np32, _, _ = RC.real_inputs(case_name)
    src = hip.from_numpy(flat, requires_grad=False)
    plan = (ctypes.c_int32 * 6)()

    def run():
        out = hip.empty(c.kept_shape, requires_grad=False)
        L.check(L.lib().lg_reduce(L.RED_SUM, len(c.shape), L.i64(c.shape), src.ptr + 4 * c.offset, L.i64(c.strides), c.mask, out.ptr))
        L.check(L.lib().lg_reduce_last_plan(plan))
        assert plan[0] == RC.FAMILIES[family] and plan[1] > 1, (case_name, tuple(plan))
        assert (plan[2] >= 1) == (family == "rows_split"), (case_name, tuple(plan))
        return {"sum": out.numpy()}
    return Family("sum " + case_name, run, close={"sum": (ref64, RC.sum_bound(case_name))})


def argmax_family(hip, L):
    c = AC.BY_NAME["offset_3x20001"]
    view = next(iter(c.make().values()))
    base, shape, strides, offset = AC.layout(view)
    flat = hip.from_numpy(base, requires_grad=False)
    t = hip(flat.data, shape, strides, flat._offset + offset, np.float32, requires_grad=False)
    plan = (ctypes.c_int32 * 4)()

    def run():
        got = t.argmax(axis=c.axis)
        L.check(L.lib().lg_argreduce_last_plan(plan))
        assert plan[0] == AC.ROWS_SPLIT and plan[1] > 1, tuple(plan)
        return {"argmax": got.numpy()}
    return Family("argmax few long rows", run, exact={"argmax": AC.reference("argmax", view, c.axis)})


def top1_family(hip):
    logits, labels = top1_batch(257, 65, np.int32, -100)            # 65 workgroups: three first-level groups, the last one short

    def run():
        return {"counts": top1_run(hip, logits, labels, ignore_index=-100).numpy()}
    return Family("top1_count", run, exact={"counts": top1_restated(logits, labels, -100)})


def batchnorm_family(hip, i):
    from lightgrad_amd.autograd.hip import ops
    arrays = BC.draw(BC.CASES[i], 100 + i)
    f64, f32 = BC.direct(arrays, np.float64), BC.direct(arrays, np.float32)

    def run():
        got = BC.run_tape(hip, arrays)
        p = ops.batchnorm_last_plan()
        assert p["kernel"] == "bwd" and p["slices"] > 1, p
        return got
    return Family("batchnorm " + BC.IDS[i], run, close={n: yardstick(f64[n], f32[n]) for n in f64})


def conv_dw_family(hip, i):
    from lightgrad_amd.autograd.hip import ops
    case = CC.CASES[i]
    arrays = CC.draw(case, 100 + i)
    f64, cpu32 = CC.direct_float64(case, arrays), CC.run_tape(CpuTensor, case, arrays)

    def run():
        got = CC.run_tape(hip, case, arrays)
        p = ops.conv2d_last_plan()
        assert p["kernel"] is not None and p["dw_slices"] > 1, p
        return got
    return Family("conv2d dW " + CC.IDS[i], run, close={n: yardstick(f64[n], cpu32[n]) for n in f64})


def clip_family(hip, L):
    n = 1025                                                         # 257 float4: two workgroups
    host = np.random.RandomState(7).uniform(-1, 1, n).astype(np.float32)
    buf = hip.from_numpy(host, requires_grad=False)
    partial, ticket, out = hip._new_grad_norm_scratch()
    exact = np.sqrt(np.sum(host.astype(np.float64) ** 2))
    numpy32 = np.sqrt(np.sum(host * host, dtype=np.float32))
    bound = max(1e-6, 2 * abs(float(numpy32) - exact) / exact)       # test_hip_optim_recipe.py's rule for the norm launch

    def run():
        L.check(L.lib().lg_grad_norm_clip_f32(buf.ptr, n, 1.0, 0.5 * exact, partial.ptr, ticket.ptr, out.ptr))
        assert ticket.numpy()[0] == 0
        return {"norm": out.numpy()[:1].copy(), "coef": out.numpy()[1:].copy()}
    return Family("global-norm clip", run, close={"norm": (np.array([exact]), bound), "coef": (np.array([0.5 * exact / (exact + 1e-6)]), bound)})


def param_grads_family(hip, L):
    c = WC.PARAM_GRAD_BY_NAME["param_grads_64x96"]
    assert c.splits > 1
    g, xhat, _, _, dw, db = WC.param_grad_inputs(c.name)
    gb, hb = hip.from_numpy(g, requires_grad=False), hip.from_numpy(xhat, requires_grad=False)
    plan = (ctypes.c_int32 * 4)()

    def run():
        dwb, dbb = hip.empty((c.cols,), requires_grad=False), hip.empty((c.cols,), requires_grad=False)
        L.check(L.lib().lg_layernorm_param_grads_f32(gb.ptr, hb.ptr, dwb.ptr, dbb.ptr, c.rows, c.cols, 0, 0))
        L.check(L.lib().lg_rowwise_last_plan(plan))
        assert tuple(plan) == (WC.PARAM_GRADS, c.splits, c.chunk, 0), tuple(plan)
        return {"dw": dwb.numpy(), "db": dbb.numpy()}
    return Family("LayerNorm parameter gradients", run, exact={"dw": dw.astype(np.float32), "db": db.astype(np.float32)})


def cross_entropy_family(hip):
    from lightgrad_amd.autograd.hip import ops as H
    rng = np.random.RandomState(5)
    n, c = 5, 4096                                                   # the narrowest rows that take the launch with the mean inside
    logits, labels = rng.uniform(-8, 8, (n, c)).astype(np.float32), rng.randint(0, c, n).astype(np.int64)
    x = logits.astype(np.float64)
    x = x - x.max(1, keepdims=True)
    logp = x - np.log(np.exp(x).sum(1, keepdims=True))
    grad = np.exp(logp)
    grad[np.arange(n), labels] -= 1
    yb, lb = hip.from_numpy(logits), hip.from_numpy(labels, requires_grad=False)

    def run():
        loss, dlogits = H.cross_entropy_forward(yb, lb)
        return {"loss": loss.numpy().reshape(1), "dlogits": dlogits.numpy()}
    # test_hip_reduce.py::test_tickets_are_left_at_zero_for_the_split_k_consumers' bounds for this call
    return Family("cross_entropy with the mean", run, close={"loss": (-logp[np.arange(n), labels].mean().reshape(1), FLOOR),
                                                              "dlogits": (grad / n, FLOOR)})


def families(hip, L):
    return [reduce_family(hip, L, "split_1x8193", "rows_split"), reduce_family(hip, L, "tile_300x128_view", "cols_tile"),
            reduce_family(hip, L, "cols_200x8", "cols"), argmax_family(hip, L), top1_family(hip), batchnorm_family(hip, 6),
            batchnorm_family(hip, 7), conv_dw_family(hip, 2), clip_family(hip, L), param_grads_family(hip, L), cross_entropy_family(hip)]


def test_every_family_leaves_the_pool_at_zero_for_the_next(hip, L):
    fams = families(hip, L)
    first = [f.run() for f in fams]
    for order in (range(len(fams) - 1, -1, -1), range(len(fams))):
        for k in order:
            again = fams[k].run()
            assert sorted(again) == sorted(first[k]), fams[k].name
            for name, value in again.items():
                assert value.dtype == first[k][name].dtype and value.tobytes() == first[k][name].tobytes(), \
                    "%s %s: differs from its first run" % (fams[k].name, name)
    for f, got in zip(fams, first):
        assert set(f.exact) | set(f.close) == set(got), (f.name, sorted(got))
        for name, want in f.exact.items():
            np.testing.assert_array_equal(got[name], want, err_msg="%s %s" % (f.name, name))
        for name, (ref64, bound) in f.close.items():
            e = rel_frobenius(got[name], ref64)
            print("handoff-pool %-40s %-12s %.3g from float64 (bound %.3g)" % (f.name, name, e, bound))
            assert np.shape(got[name]) == np.shape(ref64) and e <= bound, (f.name, name, e, bound)
