"""Every writer of a parameter gradient under the optimizer update that rides in the backward kernels (optim.Adam.fuse_update_into_backward;
include/lghip.h: lg_adam_plan_* / lg_adam_epilogue_*).

The update of a parameter is applied by the kernel that OVERWRITES its gradient first in a step; a later write into that gradient
would change the gradient and not the update.  The contract says such a write raises.  Here it is checked writer by writer through
the C ABI (a refused call returns LG_EINVAL and writes nothing; the same call on the neighbouring gradients of the flat bucket goes
through), then on the tape with one parameter used twice (a square Linear applied twice, a penalty on a weight or a bias, a tied
embedding / decoder table, one LayerNorm applied twice, a deep stack whose weight gradients are queued): every optimizer form
against the CPU backend and a float64 run, and the fused update either bit-equal to the flat-bucket update launch or refused with
the contract's error.  Last, what the fused update needs around it: no data-parallel exchange after backward, lazy tensors that
read the old parameters, and a replayed graph at the bucket parity it was captured at."""
import ctypes
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from common import float64_tape
from tape_fuzz import compare

pytestmark = pytest.mark.gpu

CONTRACT = "again after its optimizer update was applied"
LR, B1, B2, EPS = 1e-2, 0.9, 0.999, 1e-3
LENS = (37, 1000, 4097)                    # odd lengths: the flat bucket's boundaries fall anywhere
OFFS = (0, 37, 1037, 5134)
STEPS_DONE = 2                             # the bias corrections of a step that is not the first
GM, GN, GK = 25, 40, 64                    # parameter 1's gradient dW = g^T @ x: [25, 40] = 1000 floats


def _i64(*v):
    return (ctypes.c_int64 * len(v))(*v)


class Bucket(object):
    """three parameters in flat buckets with armed plans (the layout of tensor.BackwardUpdate): p_in -> p_out, moments, gradient"""

    def __init__(self, hip, belief, seed=0):
        from lightgrad_amd.autograd.hip import lib as L
        self.L, self.lib, self.hip, self.belief = L, L.lib(), hip, belief
        rng = np.random.RandomState(seed)
        n = OFFS[-1]
        self.p0 = rng.uniform(-1, 1, n).astype(np.float32)
        self.m0 = rng.uniform(-0.1, 0.1, n).astype(np.float32)
        self.v0 = rng.uniform(0, 0.01, n).astype(np.float32)
        self.g0 = rng.uniform(-1, 1, n).astype(np.float32)
        self.p_in, self.m, self.v, self.g = (hip.from_numpy(a.copy(), requires_grad=False) for a in (self.p0, self.m0, self.v0, self.g0))
        self.p_out = hip.from_numpy(np.zeros(n, np.float32), requires_grad=False)
        self.steps = hip.from_numpy(np.array([STEPS_DONE, STEPS_DONE], np.int64), requires_grad=False)
        self.plans = []
        for i in range(3):
            a, b = OFFS[i], OFFS[i + 1]
            plan = ctypes.c_void_p()
            L.check(self.lib.lg_adam_plan_create(ctypes.byref(plan), self.p_in.ptr + 4 * a, self.p_out.ptr + 4 * a, self.m.ptr + 4 * a,
                                                 self.v.ptr + 4 * a, b - a, self.steps.ptr, self.steps.ptr + 8 if i == 0 else None,
                                                 3, i + 1, LR, B1, B2, EPS, 1.0, belief))
            self.plans.append(plan.value)
        for i in range(3):
            L.check(self.lib.lg_adam_epilogue_arm(self.g.ptr + 4 * OFFS[i], LENS[i], self.plans[i]))
        self.gx = hip.from_numpy(rng.uniform(-1, 1, (GK, GM)).astype(np.float32), requires_grad=False)
        self.xx = hip.from_numpy(rng.uniform(-1, 1, (GK, GN)).astype(np.float32), requires_grad=False)

    def grad_ptr(self, i, at=0):
        return self.g.ptr + 4 * (OFFS[i] + at)

    def gemm_dw1(self, accumulate):
        """dW of parameter 1 = g^T @ x, dense (ldc == N): takes parameter 1's plan when it overwrites"""
        return self.lib.lg_gemm_f32(1, 0, GM, GN, GK, self.gx.ptr, GM, 0, self.xx.ptr, GN, 0, self.grad_ptr(1), GN, 0, 1, accumulate)

    def finish(self):
        taken, here = ctypes.c_int(0), ctypes.c_int(0)
        self.L.check(self.lib.lg_adam_epilogue_finish(ctypes.byref(taken), ctypes.byref(here)))
        return taken.value, here.value

    def close(self):
        self.lib.lg_adam_epilogue_disarm()
        for plan in self.plans:
            self.L.check(self.lib.lg_adam_plan_destroy(plan))
        self.plans = []


def _np_adam(p, g, m, v, t, belief):
    """one step of optim.Adam / AdaBelief in float64 (the reference's expressions, optim.py: the fp32 scalars of the kernels)"""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    m = B1 * m + (1 - B1) * g
    s = g - m if belief else g
    v = B2 * v + (1 - B2) * s * s
    mh, vh = m / (1 - B1 ** t), v / (1 - B2 ** t)
    return p - LR * mh / (np.sqrt(vh) + EPS), m, v


# ---- every writer, through the C ABI ------------------------------------------------------------------------------------------
# A writer call is (name, fn(bucket, ptr, k) -> rc) writing k = ROWS * ROW floats from `ptr` (and nothing outside them).
ROWS, ROW = 3, 10
K = ROWS * ROW


def _operands(b):
    if not hasattr(b, "ops"):
        rng = np.random.RandomState(7)
        hip = b.hip
        b.ops = dict(src=hip.from_numpy(rng.uniform(-1, 1, (ROWS, ROW)).astype(np.float32), requires_grad=False),
                     xhat=hip.from_numpy(rng.uniform(-1, 1, (ROWS, K)).astype(np.float32), requires_grad=False),
                     gln=hip.from_numpy(rng.uniform(-1, 1, (ROWS, K)).astype(np.float32), requires_grad=False),
                     scratch=hip.from_numpy(np.zeros(K, np.float32), requires_grad=False),
                     ids=hip.from_numpy(np.array([2, 0, 2], np.int64), requires_grad=False),
                     wide=hip.from_numpy(rng.uniform(-1, 1, (ROWS, K)).astype(np.float32), requires_grad=False))
    return b.ops


def _w_ew(b, ptr, k):
    from lightgrad_amd.autograd.hip import lib as L
    o = _operands(b)
    return b.lib.lg_ew(L.EW_ADD, 1, _i64(k), ptr, _i64(1), None, None, ptr, _i64(1), o["src"].ptr, _i64(1), None, None, None, None, 0.0)


def _w_reduce_acc(b, ptr, k):
    from lightgrad_amd.autograd.hip import lib as L
    return b.lib.lg_reduce_acc(L.RED_SUM, 2, _i64(ROWS, k), _operands(b)["wide"].ptr, _i64(K, 1), 1, ptr, 1)


def _w_colsum(b, ptr, k):
    return b.lib.lg_gemm_group_colsum_f32(_operands(b)["wide"].ptr, K, ROWS, k, ptr, 1)


def _in_group(fn):
    def run(b, ptr, k):
        lib = b.lib
        b.L.check(lib.lg_gemm_group_begin())
        try:
            rc = fn(b, ptr, k)
        finally:
            b.L.check(lib.lg_gemm_group_end())
        b.L.check(lib.lg_gemm_group_flush())
        return rc
    return run


def _w_ln_dw(b, ptr, k):
    o = _operands(b)
    return b.lib.lg_layernorm_param_grads_f32(o["gln"].ptr, o["xhat"].ptr, ptr, o["scratch"].ptr, ROWS, k, 1, 1)


def _w_ln_db(b, ptr, k):
    o = _operands(b)
    return b.lib.lg_layernorm_param_grads_f32(o["gln"].ptr, o["xhat"].ptr, o["scratch"].ptr, ptr, ROWS, k, 1, 1)


def _w_scatter_rows(b, ptr, k):
    o = _operands(b)
    return b.lib.lg_scatter_add_rows_f32(o["src"].ptr, o["ids"].ptr, 8, ptr, 3, ROW, k // ROW)


def _w_scatter_axis(b, ptr, k):
    o = _operands(b)
    return b.lib.lg_scatter_add_axis_f32(ptr, 1, k // ROW, ROW, o["ids"].ptr, 8, 3, 0, o["src"].ptr)


def _w_put_axis(b, ptr, k):
    o = _operands(b)
    return b.lib.lg_put_axis(4, ptr, 1, k // ROW, ROW, o["ids"].ptr, 8, 3, 0, o["src"].ptr, 0)


def _w_copy(b, ptr, k):
    return b.lib.lg_copy_strided(4, 1, _i64(k), ptr, _i64(1), _operands(b)["wide"].ptr, _i64(1))


def _w_copy_transposed(b, ptr, k):
    # a 2-D view written column by column (the elementwise path of lg_copy_strided)
    return b.lib.lg_copy_strided(4, 2, _i64(ROW, k // ROW), ptr, _i64(1, ROW), _operands(b)["wide"].ptr, _i64(k // ROW, 1))


def _w_fill(b, ptr, k):
    return b.lib.lg_fill_strided(4, 1, _i64(k), ptr, _i64(1), int(np.float32(0.25).view(np.uint32)))


WRITERS = [("ew_add_inplace", _w_ew), ("reduce_acc", _w_reduce_acc), ("group_colsum", _w_colsum),
           ("group_colsum_queued", _in_group(_w_colsum)), ("layernorm_dw", _w_ln_dw), ("layernorm_db", _w_ln_db),
           ("layernorm_dw_queued", _in_group(_w_ln_dw)), ("layernorm_db_queued", _in_group(_w_ln_db)),
           ("scatter_add_rows", _w_scatter_rows), ("scatter_add_rows_queued", _in_group(_w_scatter_rows)),
           ("scatter_add_axis", _w_scatter_axis), ("put_axis", _w_put_axis), ("copy_strided", _w_copy),
           ("copy_strided_2d", _w_copy_transposed), ("fill_strided", _w_fill)]


@pytest.mark.parametrize("belief", [0, 1], ids=["adam", "adabelief"])
def test_every_writer_is_refused_after_the_gemm_applied_the_update(hip, belief):
    from lightgrad_amd.autograd.hip import lib as L
    b = Bucket(hip, belief)
    try:
        L.check(b.gemm_dw1(0))                             # overwrites parameter 1's gradient: takes its plan
        L.check(b.lib.lg_sync())
        p_after, g_after = b.p_out.numpy().copy(), b.g.numpy().copy()
        m_after, v_after = b.m.numpy().copy(), b.v.numpy().copy()
        a1, e1 = OFFS[1], OFFS[2]
        dw = (b.gx.numpy().astype(np.float64).T @ b.xx.numpy().astype(np.float64)).reshape(-1)
        np.testing.assert_allclose(g_after[a1:e1], dw, rtol=1e-5, atol=1e-5)
        want_p, _, _ = _np_adam(b.p0[a1:e1], g_after[a1:e1], b.m0[a1:e1], b.v0[a1:e1], STEPS_DONE * 3 + 2, belief)
        np.testing.assert_allclose(p_after[a1:e1], want_p, rtol=1e-6, atol=1e-4 * LR)
        refused = []
        for name, fn in WRITERS:
            for at in (0, 500, 1000 - K):                   # the start of the gradient, inside it, its end
                rc = fn(b, b.grad_ptr(1, at), K)
                msg = b.lib.lg_last_error().decode()
                if rc != -1:                                # LG_EINVAL
                    refused.append("%s@%d: rc %d" % (name, at, rc))
                elif CONTRACT not in msg:
                    refused.append("%s@%d: %s" % (name, at, msg))
        assert not refused, "writers that were not refused: %s" % refused
        L.check(b.lib.lg_sync())
        np.testing.assert_array_equal(b.p_out.numpy()[a1:e1], p_after[a1:e1])      # what the epilogue wrote, untouched
        np.testing.assert_array_equal(b.g.numpy()[a1:e1], g_after[a1:e1])          # and the gradient: refused calls write nothing
        np.testing.assert_array_equal(b.m.numpy()[a1:e1], m_after[a1:e1])
        np.testing.assert_array_equal(b.v.numpy()[a1:e1], v_after[a1:e1])
        # no false positives: the neighbours in the flat bucket, ending / starting at parameter 1's boundaries
        for name, fn in WRITERS:
            L.check(fn(b, b.grad_ptr(0, LENS[0] - K), K))
            L.check(fn(b, b.grad_ptr(2, 0), K))
        assert b.finish() == (1, 2)
    finally:
        b.close()


@pytest.mark.parametrize("belief", [0, 1], ids=["adam", "adabelief"])
@pytest.mark.parametrize("name,fn", WRITERS, ids=[w[0] for w in WRITERS])
def test_a_writer_before_an_accumulating_gemm_leaves_the_update_to_finish(hip, belief, name, fn):
    """the other order: the writer first, then the GEMM that ADDS (and so takes nothing) - finish() applies all three updates,
    bit for bit what the flat-bucket update launch computes from the same gradient"""
    from lightgrad_amd.autograd.hip import lib as L
    b = Bucket(hip, belief, seed=3)
    try:
        L.check(fn(b, b.grad_ptr(1, 500), K))
        L.check(b.gemm_dw1(1))
        assert b.finish() == (0, 3)
        L.check(b.lib.lg_sync())
        grad = b.g.numpy().copy()
        got_p, got_m, got_v = b.p_out.numpy().copy(), b.m.numpy().copy(), b.v.numpy().copy()
        assert int(b.steps.numpy()[1]) == STEPS_DONE + 1          # step_out of the first plan
    finally:
        b.close()
    # the same update through lg_adam_multi_dev_f32 on the same gradient
    p, m, v = (hip.from_numpy(a.copy(), requires_grad=False) for a in (b.p0, b.m0, b.v0))
    gt = hip.from_numpy(grad, requires_grad=False)
    step = hip.from_numpy(np.array([STEPS_DONE], np.int64), requires_grad=False)
    L.check(b.lib.lg_adam_multi_dev_f32(p.ptr, gt.ptr, m.ptr, v.ptr, 3, _i64(*OFFS), LR, B1, B2, EPS, step.ptr, 0, 1.0, belief))
    np.testing.assert_array_equal(got_p, p.numpy())
    np.testing.assert_array_equal(got_m, m.numpy())
    np.testing.assert_array_equal(got_v, v.numpy())
    for i in range(3):
        a, e = OFFS[i], OFFS[i + 1]
        want, _, _ = _np_adam(b.p0[a:e], grad[a:e], b.m0[a:e], b.v0[a:e], STEPS_DONE * 3 + i + 1, belief)
        np.testing.assert_array_less(np.abs(got_p[a:e] - want), 1e-6 * np.abs(want) + 1e-4 * LR, err_msg="parameter %d" % i)


def test_a_gemm_into_part_of_an_applied_gradient_is_refused(hip):
    """a second product into a sub-range of the gradient (not the same pointer) is a second writer too"""
    from lightgrad_amd.autograd.hip import lib as L
    b = Bucket(hip, 1)
    try:
        L.check(b.gemm_dw1(0))
        rc = b.lib.lg_gemm_f32(1, 0, 4, 8, GK, b.gx.ptr, GM, 0, b.xx.ptr, GN, 0, b.grad_ptr(1, 200), 8, 0, 1, 1)
        assert rc == -1 and CONTRACT in b.lib.lg_last_error().decode()
        L.check(b.lib.lg_gemm_f32(1, 0, 4, 8, GK, b.gx.ptr, GM, 0, b.xx.ptr, GN, 0, b.grad_ptr(2, 0), 8, 0, 1, 1))
        assert b.finish() == (1, 2)
    finally:
        b.close()


# ---- one parameter used twice, through the tape ---------------------------------------------------------------------------------
class Shared(light.nn.Module):
    """the scenarios: `kind` names how a parameter is used twice in one loss"""

    def __init__(self, kind):
        light.nn.Module.__init__(self)
        self.kind = kind
        if kind in ("square_twice_relu", "square_twice_tanh"):
            self.inp = light.nn.Linear(12, 48)
            self.sq = light.nn.Linear(48, 48)
            self.out = light.nn.Linear(48, 5)
        elif kind == "square_twice_head":
            self.inp = light.nn.Linear(12, 16)
            self.sq = light.nn.Linear(16, 16)             # skinny: its own head kernel and the riding head gradient
        elif kind in ("penalty_before", "penalty_after", "bias_penalty"):
            self.l1 = light.nn.Linear(12, 32)
            self.l2 = light.nn.Linear(32, 5)
        elif kind == "tied_table":
            self.emb = CpuTensor.from_numpy(np.random.uniform(-1, 1, (20, 16)).astype(np.float32))
            self.proj = light.nn.Linear(16, 16)
        elif kind == "layernorm_twice":
            self.l1 = light.nn.Linear(12, 32)
            self.ln = light.nn.LayerNorm(32)
            self.l2 = light.nn.Linear(32, 32)
            self.out = light.nn.Linear(32, 5)
        elif kind == "deep":
            self.inp = light.nn.Linear(12, 32)
            self.sq = light.nn.Linear(32, 32)
            self.mid = light.nn.ModuleList(*[light.nn.Linear(32, 32) for _ in range(4)])
            self.out = light.nn.Linear(32, 5)
        else:
            raise ValueError(kind)

    def forward(self, x, T):
        k = self.kind
        if k == "square_twice_relu":
            h = self.inp(x).relu()
            return self.out(self.sq(self.sq(h).relu()).relu())
        if k == "square_twice_tanh":
            h = self.inp(x).tanh()
            return self.out(self.sq(self.sq(h).tanh()).tanh())
        if k == "square_twice_head":
            return self.sq(self.sq(self.inp(x).relu()).relu())
        if k in ("penalty_before", "penalty_after", "bias_penalty"):
            return self.l2(self.l1(x).relu())
        if k == "tied_table":
            return self.proj(x).tanh() @ self.emb.transpose(1, 0)       # the decoder reads the embedding table
        if k == "layernorm_twice":
            h = self.ln(self.l1(x).tanh())
            return self.out(self.ln(self.l2(h).tanh()))
        h = self.inp(x).relu()
        h = self.sq(h).relu()
        for layer in self.mid:
            h = layer(h).tanh()
        h = self.sq(h).relu()
        return self.out(h)


SCENARIOS = ["square_twice_relu", "square_twice_tanh", "square_twice_head", "penalty_before", "penalty_after", "bias_penalty",
             "tied_table", "layernorm_twice", "deep"]
# What the update inside the backward kernels does with each, given the tape's backward order (reverse creation order, the
# operands of a node in the order they were given).  "refused": the kernel that reaches the gradient first OVERWRITES it and applies
# the update; the second use then writes into it and raises.  "accepted": the first write carries no update (an elementwise or
# reduction kernel, a LayerNorm / scatter job, a product that adds) - step() applies the update in its one launch, bit for bit
# the flat-bucket form.
FUSED_OUTCOME = {
    "square_twice_relu": "refused",        # the outer use's dW = g^T relu(h1) overwrites (GEMM epilogue); the inner use adds
    "square_twice_tanh": "refused",        # the same through materialised activations
    "square_twice_head": "refused",        # the outer use is a skinny head: its product overwrites dW, the inner use adds
    "penalty_before": "refused",           # `pen + data`: the data term's dW GEMM comes first and overwrites, the penalty adds
    "penalty_after": "accepted",           # `data + pen`: the penalty's gradient (elementwise) comes first, the GEMM adds into it
    "bias_penalty": "accepted",            # `data + pen(b)`: the same for the bias, the row sums add
    "tied_table": "accepted",              # the decoder's dE and the gather's scatter-add: neither is an overwriting dense product
    "layernorm_twice": "accepted",         # LayerNorm's parameter gradients carry no update
    "deep": "refused",                     # a product that takes a plan is never queued: it overwrites at once, the other use adds
}
X_ROWS = 33


def _inputs(kind):
    rng = np.random.RandomState(5)
    if kind == "tied_table":
        return rng.uniform(-1, 1, (X_ROWS, 16)).astype(np.float32), rng.randint(0, 20, X_ROWS).astype(np.int64)
    return rng.uniform(-1, 1, (X_ROWS, 12)).astype(np.float32), rng.uniform(-1, 1, (X_ROWS, 5 if kind != "square_twice_head" else 16)).astype(np.float32)


def run_shared(T, kind, form, steps=3, dtype=np.float32, made=None):
    """the scenario `kind` for `steps` Adam steps on tensor class T; form: "tape" (plain), "fused" (per-parameter kernel), "flat"
    (flat buckets, one update launch), "in_backward" (the update inside the backward kernels).  Returns [(label, array)]."""
    np.random.seed(11)
    model = Shared(kind)
    model.load_parameters([(n, p.numpy().astype(dtype)) for n, p in model.named_parameters()])
    x_np, t_np = _inputs(kind)
    if T is not CpuTensor:
        model.map_parameters(lambda p: p.hip())
    params = list(model.named_parameters())
    tensors = [p for _, p in params]
    if form == "tape" or T is CpuTensor:
        opt = light.optim.Adam(tensors, lr=LR, eps=EPS)
    elif form == "fused":
        opt = light.optim.Adam(tensors, lr=LR, eps=EPS, fused=True, device_step=True)
    else:
        from lightgrad_amd.dist import DataParallel, SingleProcess
        dp = DataParallel(tensors, SingleProcess(), flatten=True)
        opt = light.optim.Adam(tensors, lr=LR, eps=EPS, fused=True, device_step=True)
        dp.attach(opt)
        if form == "in_backward":
            opt.fuse_update_into_backward()
    if made is not None:
        made.append(opt)
    out = []
    x = T.from_numpy(x_np.astype(dtype), requires_grad=False)
    for s in range(steps):
        if kind == "tied_table":
            ids = T.from_numpy(t_np, requires_grad=False)
            h = model.emb[ids]                                            # embedding lookup: the gather
            y = model(h + x, T)                                           # ... and the decoder: x @ E^T
            loss = light.loss.cross_entropy(y, ids)
        else:
            y = model(x, T)
            target = T.from_numpy(t_np.astype(dtype), requires_grad=False)
            data = light.loss.mse(y, target)
            if kind == "penalty_before":
                w = model.l1.weight
                loss = (w * w).sum() * 0.01 + data
            elif kind == "penalty_after":
                w = model.l1.weight
                loss = data + (w * w).sum() * 0.01
            elif kind == "bias_penalty":
                loss = data + (model.l1.bias * model.l1.bias).sum() * 0.05
            else:
                loss = data
        opt.zero_grad()
        loss.backward()
        out.append(("s%d/loss" % s, np.array(loss.numpy(), np.float64)))
        for n, p in params:
            out.append(("s%d/grad/%s" % (s, n), np.array(p.grad.numpy(), np.float64)))
        opt.step()
        for n, p in params:
            out.append(("s%d/param/%s" % (s, n), np.array(p.numpy(), np.float64)))
    return out, opt


@pytest.mark.parametrize("kind", SCENARIOS)
def test_shared_parameters_every_form_matches_the_cpu_backend(hip, kind):
    ref, _ = run_shared(CpuTensor, kind, "tape")
    with float64_tape():
        ref64, _ = run_shared(CpuTensor, kind, "tape", dtype=np.float64)
    compare(ref64, ref, rtol=5e-3, atol=5e-4, what="%s cpu float32 vs float64" % kind)
    flat = None
    for form in ("tape", "fused", "flat"):
        got, _ = run_shared(hip, kind, form)
        compare(ref, got, what="%s %s" % (kind, form))
        compare(ref64, got, rtol=5e-3, atol=5e-4, what="%s %s vs float64" % (kind, form))
        if form == "flat":
            flat = got
    from lightgrad_amd.autograd.hip import HipError
    if FUSED_OUTCOME[kind] == "accepted":
        got, opt = run_shared(hip, kind, "in_backward")
        assert [l for l, _ in got] == [l for l, _ in flat]
        for (label, a), (_, b) in zip(flat, got):
            np.testing.assert_array_equal(b, a, err_msg="%s %s: the update inside the backward kernels vs the update launch" % (kind, label))
        return
    made = []
    with pytest.raises(HipError, match=CONTRACT):
        run_shared(hip, kind, "in_backward", steps=1, made=made)
    made[0]._backward_update.disarm()
    # the library is usable again: an unfused step of the same scenario gives the CPU backend's values
    again, _ = run_shared(hip, kind, "flat", steps=1)
    compare(ref[:len(again)], again, what="%s after the refusal" % kind)


# ---- around the fused update: data-parallel exchange, lazy readers, graph replay ----------------------------------------------
class TwoRanks(object):
    """a communicator of world size 2 whose exchange runs outside the optimizer (sync_gradients): the plain host-staged kind"""
    rank, world_size = 0, 2

    def allreduce_sum_(self, flat, forked=False):
        return flat

    def fork(self):
        pass

    def join(self):
        pass


def _linear_dp(comm):
    from lightgrad_amd.dist import DataParallel
    np.random.seed(4)
    lin = light.nn.Linear(24, 8)
    lin.map_parameters(lambda p: p.hip())
    dp = DataParallel(lin.parameters(), comm, broadcast_parameters=False, flatten=True)
    opt = light.optim.Adam(lin.parameters(), lr=LR, eps=EPS, fused=True, device_step=True)
    dp.attach(opt)
    return lin, dp, opt


def test_no_update_in_backward_when_the_gradients_are_exchanged_after_it(hip):
    from lightgrad_amd.dist import SingleProcess
    _, _, opt = _linear_dp(TwoRanks())
    with pytest.raises(AssertionError, match="exchanged first"):
        opt.fuse_update_into_backward()
    assert opt._backward_update is None
    lin, dp, opt = _linear_dp(SingleProcess())
    opt.fuse_update_into_backward()
    x = hip.from_numpy(np.random.RandomState(1).uniform(-1, 1, (16, 24)).astype(np.float32), requires_grad=False)
    loss = lin(x).tanh().sum()
    opt.zero_grad()
    loss.backward()
    dp.sync_gradients()
    opt.step()


@pytest.mark.parametrize("out_features", [8, 48], ids=["head_output", "gemm_output"])
def test_an_output_read_after_step_has_the_old_weights(hip, out_features):
    """y = model(x) before the step, first looked at after it: the reference computed it before the update"""
    from lightgrad_amd.dist import DataParallel, SingleProcess
    rng = np.random.RandomState(8)
    x_np = rng.uniform(-1, 1, (64, 32)).astype(np.float32)
    t_np = rng.uniform(-1, 1, (64, out_features)).astype(np.float32)

    def run(T):
        np.random.seed(6)
        # a skinny output layer is a lazy head product, a wide one without bias a lazy plain product: both read the weights later
        l1, l2 = light.nn.Linear(32, 64), light.nn.Linear(64, out_features, bias=out_features <= 16)
        params = list(l1.parameters()) + list(l2.parameters())
        if T is CpuTensor:
            opt = light.optim.Adam(params, lr=LR, eps=EPS)
        else:
            l1.map_parameters(lambda p: p.hip())
            l2.map_parameters(lambda p: p.hip())
            params = list(l1.parameters()) + list(l2.parameters())
            dp = DataParallel(params, SingleProcess(), flatten=True)
            opt = light.optim.Adam(params, lr=LR, eps=EPS, fused=True, device_step=True)
            dp.attach(opt)
            opt.fuse_update_into_backward()
        x, t = T.from_numpy(x_np, requires_grad=False), T.from_numpy(t_np, requires_grad=False)
        seen = []
        for _ in range(2):
            early = l2(l1(x).relu())                        # nobody reads it before the step
            loss = light.loss.mse(l2(l1(x).relu()), t)
            opt.zero_grad()
            loss.backward()
            opt.step()
            seen.append(early.numpy().copy())
        return seen
    for a, b in zip(run(CpuTensor), run(hip)):
        np.testing.assert_allclose(b, a, rtol=2e-5, atol=2e-5)


def test_a_graph_is_replayed_only_at_the_parity_it_was_captured_at(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    from lightgrad_amd.dist import SingleProcess
    lin, dp, opt = _linear_dp(SingleProcess())
    opt.fuse_update_into_backward()
    x = hip.from_numpy(np.random.RandomState(2).uniform(-1, 1, (16, 24)).astype(np.float32), requires_grad=False)

    def step():
        loss = lin(x).tanh().sum()
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss
    step()
    step()
    assert opt._backward_update.parity == 0
    graph = HipGraph()
    with graph.capture():
        step()
        step()
    opt.t -= 4
    graph.replay()                                          # at the parity of the capture: fine
    opt.on_graph_replay(2)
    step()                                                  # one eager step: parity 1
    before = [p.numpy().copy() for p in lin.parameters()]
    with pytest.raises(RuntimeError, match="parity 0"):
        graph.replay()
    for p, b in zip(lin.parameters(), before):
        np.testing.assert_array_equal(p.numpy(), b)
    step()                                                  # back at parity 0: the graph replays again
    graph.replay()
    opt.on_graph_replay(2)


@pytest.mark.parametrize("first_accumulates", [0, 1], ids=["overwrite_then_add", "add_then_add"])
def test_two_products_into_one_gradient_inside_a_pair_bracket(hip, first_accumulates):
    """[dW, dW, dx] in one bracket (the three-product launch of a head riding with the hidden layer) where both weight gradients
    are the SAME buffer - one weight used twice: the second must see the first's result, not race with it"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    rng = np.random.RandomState(9)
    M, N, Kd = 64, 64, 128
    g1, g2 = (rng.uniform(-1, 1, (Kd, M)).astype(np.float32) for _ in range(2))
    x1, x2 = (rng.uniform(-1, 1, (Kd, N)).astype(np.float32) for _ in range(2))
    gs, w = rng.uniform(-1, 1, (Kd, M)).astype(np.float32), rng.uniform(-1, 1, (M, N)).astype(np.float32)
    c0 = rng.uniform(-1, 1, (M, N)).astype(np.float32)
    t = {k: hip.from_numpy(v, requires_grad=False) for k, v in dict(g1=g1, g2=g2, x1=x1, x2=x2, gs=gs, w=w, c=c0).items()}
    dx = hip.from_numpy(np.zeros((Kd, N), np.float32), requires_grad=False)
    L.check(lib.lg_gemm_pair_begin())
    try:
        L.check(lib.lg_gemm_f32(1, 0, M, N, Kd, t["g1"].ptr, M, 0, t["x1"].ptr, N, 0, t["c"].ptr, N, 0, 1, first_accumulates))
        L.check(lib.lg_gemm_f32(1, 0, M, N, Kd, t["g2"].ptr, M, 0, t["x2"].ptr, N, 0, t["c"].ptr, N, 0, 1, 1))
        L.check(lib.lg_gemm_f32(0, 0, Kd, N, M, t["gs"].ptr, M, 0, t["w"].ptr, N, 0, dx.ptr, N, 0, 1, 0))
    finally:
        L.check(lib.lg_gemm_pair_end())
    f = lambda a: a.astype(np.float64)       # noqa: E731
    want = (f(c0) if first_accumulates else 0) + f(g1).T @ f(x1) + f(g2).T @ f(x2)
    np.testing.assert_allclose(t["c"].numpy(), want, rtol=1e-5, atol=1e-4)
    np.testing.assert_allclose(dx.numpy(), f(gs) @ f(w), rtol=1e-5, atol=1e-4)
