"""Dropout on the HIP backend (csrc/dropout.hip): bit equality with the CPU backend at every launch edge, the C ABI on flat
buffers, calls queued back to back, hipGraph replay (a fresh mask per replay from device-resident state), and the BERT example."""
import ctypes
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from test_dropout_cpu import BERT_IDS, build_bert

pytestmark = pytest.mark.gpu

SEEDS = (1234, (0x9E3779B9 << 32) | 0x7F4A7C15)          # the second one has a non-zero high word
LG_EINVAL = -1

# One thread takes four elements, a workgroup 1024; the arrival tickets are grouped by g workgroups, g the power of two with
# g * g >= workgroups, so g changes after 1, 4, 16, 64 and 256 workgroups: both sides of each of those sizes.
EDGES = [1, 3, 4, 5] + [1024 * 4**k + d for k in range(5) for d in (-1, 0, 1)] + [2**20 + 3]


SPECIAL = 128        # elements per mask that receive the special values (tensors of at least 2 * SPECIAL elements)


def special_values(n, rng, keeps):
    """random normal float32; mask d of `keeps` gets -0.0, an infinity and a NaN at a kept and at a dropped position each, inside
    elements [SPECIAL * d, SPECIAL * (d + 1))"""
    x = rng.standard_normal(n).astype(np.float32)
    if n >= len(keeps) * SPECIAL:
        for d, keep in enumerate(keeps):
            part = slice(SPECIAL * d, SPECIAL * (d + 1))
            kept, dropped = np.flatnonzero(keep[part]) + part.start, np.flatnonzero(~keep[part]) + part.start
            assert len(kept) >= 3 and len(dropped) >= 3
            x[kept[:3]] = x[dropped[:3]] = (-0.0, np.inf, np.nan)
    return x


def run(x, r, g, p):
    y = x.dropout(p) if r is None else x.dropout(p, residual=r)
    (y * g).backward(allow_fill=True)
    return y.numpy(), x.grad.numpy(), (None if r is None else r.grad.numpy())


@pytest.mark.parametrize("n", EDGES)
def test_bit_equality_with_the_cpu_backend(hip, n):
    rng = np.random.RandomState(n % 9973)
    for p in (0.1, 0.5):
        for seed in SEEDS:
            keeps = [lrandom.keep_mask(seed, d, min(n, 2 * SPECIAL), p) for d in (0, 1)]
            xa, ra, ga = special_values(n, rng, keeps), rng.standard_normal(n).astype(np.float32), special_values(n, rng, keeps)
            light.manual_seed(seed)
            results = {}
            for T in (CpuTensor, hip):
                out = []
                for residual in (False, True):
                    x, g = T.from_numpy(xa), T.from_numpy(ga, requires_grad=False)
                    r = T.from_numpy(ra) if residual else None
                    out.append(run(x, r, g, p))
                results[T] = out
            assert lrandom.get_state("cpu") == lrandom.get_state("hip") == (seed, 2)
            for (yc, dxc, drc), (yh, dxh, drh) in zip(results[CpuTensor], results[hip]):
                np.testing.assert_array_equal(yh, yc)
                np.testing.assert_array_equal(dxh, dxc)
                assert np.array_equal(np.signbit(yh), np.signbit(yc)) and np.array_equal(np.signbit(dxh), np.signbit(dxc))
                if drc is not None:
                    np.testing.assert_array_equal(drh, drc)
            if n >= 2 * SPECIAL:
                y = results[hip][0][0][:2 * SPECIAL]
                dropped_nan = np.isnan(xa[:2 * SPECIAL]) & ~keeps[0]
                assert dropped_nan.any() and np.all(y[dropped_nan] == 0) and not np.signbit(y[dropped_nan]).any()


def _state(L):
    seed, draws = ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert L.lg_rng_state(ctypes.byref(seed), ctypes.byref(draws)) == 0
    return seed.value, draws.value


@pytest.mark.parametrize("pad", [8, 3])          # 8: every pointer 16-byte aligned (float4 path); 3: not (scalar path)
@pytest.mark.parametrize("n", [0, 1, 5, 1024, 4099])
def test_c_abi_on_flat_buffers(hip, n, pad):
    from lightgrad_amd.autograd.hip import lib as hiplib
    L = hiplib.lib()
    rng = np.random.RandomState(n + pad)
    p, seed = 0.3, SEEDS[1]
    x, r, g = (rng.standard_normal(n).astype(np.float32) for _ in range(3))
    guard, mark = np.full(pad, np.nan, np.float32), np.full(pad, 7.25, np.float32)
    xin = hip.from_numpy(np.concatenate([guard, x, guard]))           # NaN guards: a read outside x shows in the result
    rin = hip.from_numpy(np.concatenate([guard, r, guard]))
    gin = hip.from_numpy(np.concatenate([guard, g, guard]))
    keep = lrandom.keep_mask(seed, 4, n, p)
    s = lrandom.scale(p)
    expect_y = np.where(keep, x * s, np.float32(0))
    expect = {"plain": expect_y, "residual": expect_y + r, "bwd": np.where(keep, g * s, np.float32(0))}

    def fresh():
        return hip.from_numpy(np.concatenate([mark, np.full(n, -3.0, np.float32), mark]))

    def at(t):
        return t.ptr + 4 * pad

    def check(buf, what):
        got = buf.numpy()
        np.testing.assert_array_equal(got[:pad], mark)
        np.testing.assert_array_equal(got[pad + n:], mark)
        np.testing.assert_array_equal(got[pad:pad + n], expect[what])

    base = hip.from_numpy(np.full(3, 99, np.uint64))
    for what, res in (("plain", None), ("residual", at(rin))):
        assert L.lg_rng_seed(seed) == 0
        for _ in range(4):                                                # four empty calls: draws = 4 (n == 0 advances too)
            assert L.lg_dropout_fwd_f32(at(xin), None, at(xin), 0, p, base.ptr + 8) == 0
        assert _state(L) == (seed, 4)
        y = fresh()
        assert L.lg_dropout_fwd_f32(at(xin), res, at(y), n, p, base.ptr + 8) == 0
        assert _state(L) == (seed, 5)
        np.testing.assert_array_equal(base.numpy(), [99, 4, 99])          # base_out holds the draws of before the call
        check(y, what)
        # in place: y == x
        xcopy = hip.from_numpy(np.concatenate([mark, x, mark]))
        assert L.lg_rng_seed(seed) == 0
        for _ in range(4):
            assert L.lg_dropout_fwd_f32(at(xin), None, at(xin), 0, p, base.ptr + 8) == 0
        assert L.lg_dropout_fwd_f32(at(xcopy), res, at(xcopy), n, p, base.ptr + 8) == 0
        check(xcopy, what)
    np.testing.assert_array_equal(xin.numpy()[pad:pad + n], x)           # the inputs are untouched
    dx = fresh()
    assert L.lg_dropout_bwd_f32(at(gin), at(dx), n, p, base.ptr + 8) == 0
    check(dx, "bwd")
    gcopy = hip.from_numpy(np.concatenate([mark, g, mark]))
    assert L.lg_dropout_bwd_f32(at(gcopy), at(gcopy), n, p, base.ptr + 8) == 0       # in place: dx == g
    check(gcopy, "bwd")
    assert _state(L) == (seed, 5)                                         # the backward draws nothing


def test_c_abi_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as hiplib
    L = hiplib.lib()
    a, b = hip.from_numpy(np.ones(8, np.float32)), hip.from_numpy(np.full(8, 5.0, np.float32))
    base = hip.from_numpy(np.zeros(1, np.uint64))
    assert L.lg_rng_seed(21) == 0
    assert L.lg_dropout_fwd_f32(a.ptr, None, b.ptr, 8, 0.5, base.ptr) == 0
    before = _state(L)
    assert before == (21, 1)
    bad_fwd = [(None, None, b.ptr, 8, 0.5, base.ptr), (a.ptr, None, None, 8, 0.5, base.ptr), (a.ptr, None, b.ptr, 8, 0.5, None),
               (a.ptr, None, b.ptr, -1, 0.5, base.ptr), (a.ptr, None, b.ptr, 8, 1.0, base.ptr), (a.ptr, None, b.ptr, 8, -0.25, base.ptr),
               (a.ptr, None, b.ptr, 8, float("nan"), base.ptr)]
    for args in bad_fwd:
        assert L.lg_dropout_fwd_f32(*args) == LG_EINVAL, args
        assert b"lg_dropout_fwd_f32" in L.lg_last_error()
    bad_bwd = [(None, b.ptr, 8, 0.5, base.ptr), (a.ptr, None, 8, 0.5, base.ptr), (a.ptr, b.ptr, 8, 0.5, None),
               (a.ptr, b.ptr, -1, 0.5, base.ptr), (a.ptr, b.ptr, 8, 1.0, base.ptr), (a.ptr, b.ptr, 8, -0.25, base.ptr)]
    for args in bad_bwd:
        assert L.lg_dropout_bwd_f32(*args) == LG_EINVAL, args
    assert L.lg_rng_state(None, None) == LG_EINVAL
    assert _state(L) == before
    y = b.numpy()
    assert set(np.unique(y)) <= {0.0, 2.0}                                # the refused calls wrote nothing


def test_tensor_level_checks_and_bookkeeping(hip):
    x = hip.from_numpy(np.ones((4, 4), np.float32))
    light.manual_seed(3)
    for bad in (1.0, -0.5):
        with pytest.raises(ValueError):
            x.dropout(bad)
    for dtype in (np.int32, np.float64):
        with pytest.raises(TypeError):
            hip.from_numpy(np.ones(4, dtype=dtype)).dropout(0.5)
    with pytest.raises(ValueError):
        x.dropout(0.5, residual=hip.from_numpy(np.ones(5, np.float32)))
    assert x.dropout(0.0) is x
    r = hip.from_numpy(np.full((4, 4), 2.0, np.float32))
    np.testing.assert_array_equal(x.dropout(0.0, residual=r).numpy(), np.full((4, 4), 3.0, np.float32))
    assert lrandom.get_state("hip") == (3, 0)
    with light.no_grad():
        y = x.dropout(0.5)
    assert y.ctx is None and lrandom.get_state("hip") == (3, 1)
    hip.from_numpy(np.ones((0, 3), np.float32)).dropout(0.5)
    assert lrandom.get_state("hip") == (3, 2)


def test_calls_back_to_back_use_consecutive_draws(hip):
    """eight calls of different sizes enqueued without a synchronisation in between: call k must see draws == k - a workgroup of
    call k that read `draws` after the kernel's own increment (or before call k - 1's) would show as another call's mask"""
    sizes = [70001, 5, 262145, 1024, 3, 1025, 16385, 40000]
    rng = np.random.RandomState(8)
    arrays = [rng.standard_normal(n).astype(np.float32) for n in sizes]
    seed = SEEDS[1]
    light.manual_seed(seed)
    tensors = [hip.from_numpy(a) for a in arrays]
    with light.no_grad():
        outs = [t.dropout(0.5) for t in tensors]                          # nothing here waits for the device
    got = [o.numpy() for o in outs]
    cpu = [CpuTensor.from_numpy(a).dropout(0.5).numpy() for a in arrays]
    for k, (h, c, a) in enumerate(zip(got, cpu, arrays)):
        np.testing.assert_array_equal(h, c, err_msg="call %d" % k)
        np.testing.assert_array_equal(h != 0, lrandom.keep_mask(seed, k, len(a), 0.5) & (a != 0))
    assert lrandom.get_state("hip") == (seed, 8)


def test_non_dense_input(hip):
    a = np.random.RandomState(12).standard_normal((37, 50)).astype(np.float32)
    g = np.random.RandomState(13).standard_normal((50, 37)).astype(np.float32)
    light.manual_seed(44)
    out = {}
    for T in (CpuTensor, hip):
        x = T.from_numpy(a)
        y = x.transpose(1, 0).dropout(0.5)
        (y * T.from_numpy(g, requires_grad=False)).backward(allow_fill=True)
        out[T] = (y.numpy(), x.grad.numpy())
    np.testing.assert_array_equal(out[hip][0], out[CpuTensor][0])
    np.testing.assert_array_equal(out[hip][1], out[CpuTensor][1])


def test_graph_replay_draws_a_fresh_mask(hip):
    from lightgrad_amd.autograd.hip import GraphedStep, HipGraph
    from lightgrad_amd.autograd.hip import lib as hiplib
    rng = np.random.RandomState(30)
    xa, ra, ga = (rng.standard_normal((33, 41)).astype(np.float32) for _ in range(3))
    seed = SEEDS[1]

    def make(T):
        x, r, g = T.from_numpy(xa), T.from_numpy(ra), T.from_numpy(ga, requires_grad=False)

        def step():
            y1 = x.dropout(0.3)
            y2 = y1.dropout(0.5, residual=r)
            x.zero_grad()
            r.zero_grad()
            (y2 * g).backward(allow_fill=True)
            return y1, y2, x.grad, r.grad
        return step

    cpu_step = make(CpuTensor)
    light.manual_seed(seed)
    expected = [[t.numpy().copy() for t in cpu_step()] for _ in range(3)]
    assert lrandom.get_state("cpu") == (seed, 6)

    step = GraphedStep(make(hip), warmup=1)
    step()                                                                # eager: pool, kernels
    for attempt in range(2):
        light.manual_seed(seed)                                           # also AFTER the capture: a replay reads the seed from memory
        replays = [[t.numpy() for t in step()] for _ in range(3)]        # (the first of these captures, then replays)
        for k in range(3):
            for got, want in zip(replays[k], expected[k]):
                np.testing.assert_array_equal(got, want, err_msg="attempt %d, replay %d" % (attempt, k))
        assert lrandom.get_state("hip") == (seed, 6)
    assert step._graph is not None and step._graph.kernel_count() > 0
    assert not np.array_equal(replays[0][0] != 0, replays[1][0] != 0)    # masks of different replays differ
    assert not np.array_equal(replays[1][1], replays[2][1])
    step.destroy()

    L = hiplib.lib()
    x = hip.from_numpy(xa)
    graph = HipGraph()
    with graph.capture():
        x.dropout(0.5)
        assert L.lg_rng_seed(1) == LG_EINVAL and b"capturing" in L.lg_last_error()
        s, d = ctypes.c_uint64(0), ctypes.c_uint64(0)
        assert L.lg_rng_state(ctypes.byref(s), ctypes.byref(d)) == LG_EINVAL
        with pytest.raises(hiplib.HipError):
            light.manual_seed(5)
    graph.destroy()
    light.manual_seed(seed)                                               # (the refused manual_seed had already seeded the CPU side)


BERT_LABELS = np.random.RandomState(5).randint(0, 50, (16,)).astype(np.int64)


def _bert_loss_and_grads(model, T):
    loss = light.loss.cross_entropy(model(T.from_numpy(BERT_IDS, requires_grad=False)).reshape(-1, 50),
                                    T.from_numpy(BERT_LABELS, requires_grad=False))
    for p in model.parameters():
        p.zero_grad()
    loss.backward()
    out = {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}
    out["loss"] = np.asarray(loss.item(), np.float64)
    return out


def test_bert_training_mode_against_float64(hip):
    """loss and every parameter gradient of the tiny-BERT in training mode (both probabilities 0.1): the masks of the three runs
    are identical by construction (same seed, same order of calls), so the float64 run of the same tape on the CPU backend is
    the yardstick - HIP within 1e-5 (relative Frobenius) of it, or no further than twice the float32 CPU backend.  The key
    projection's bias has a gradient of exactly zero in exact arithmetic (softmax ignores a per-query constant; dropout comes
    after it): there all three are rounding noise and are bounded as such, like tests/test_hip_bert.py does."""
    dropout = dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    cpu_model = build_bert(**dropout)
    values = {n: p.numpy() for n, p in cpu_model.named_parameters()}
    hip_model = build_bert(**dropout).map_parameters(lambda p: p.hip())
    seed = SEEDS[1]
    light.manual_seed(seed)
    cpu32 = _bert_loss_and_grads(cpu_model, CpuTensor)
    got = _bert_loss_and_grads(hip_model, hip)
    assert lrandom.get_state("cpu") == lrandom.get_state("hip") == (seed, 4)
    light.manual_seed(seed)
    with float64_tape():
        ref_model = build_bert(**dropout)
        ref_model.load_parameters({n: a.astype(np.float64) for n, a in values.items()})
        assert all(p.dtype == np.float64 for p in ref_model.parameters())
        ref64 = _bert_loss_and_grads(ref_model, CpuTensor)
    noise = [n for n in ref64 if n.endswith(".key.bias")]
    for n in noise:
        print("%-60s |hip| %.2e  |cpu32| %.2e  |float64| %.2e" % (n, np.abs(got[n]).max(), np.abs(cpu32[n]).max(), np.abs(ref64[n]).max()))
        assert np.abs(got[n]).max() < 1e-6 and np.abs(cpu32[n]).max() < 1e-6 and np.abs(ref64[n]).max() < 1e-12
    for n in ref64:
        print("%-60s hip %.2e  cpu32 %.2e" % (n, rel_frobenius(got[n], ref64[n]), rel_frobenius(cpu32[n], ref64[n])))
    rest = {n: a for n, a in ref64.items() if n not in noise}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, rest, what="tiny-BERT with dropout")


def test_bert_eval_mode_launches_what_the_plain_model_launches(hip):
    from lightgrad_amd.autograd.hip import HipGraph
    counts, logits = {}, {}
    ids = hip.from_numpy(BERT_IDS, requires_grad=False)
    labels = hip.from_numpy(BERT_LABELS, requires_grad=False)
    light.manual_seed(2)
    for name, kwargs in (("plain", {}), ("dropout", dict(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1))):
        model = build_bert(**kwargs).map_parameters(lambda p: p.hip())
        model.eval()

        def step():
            out = model(ids)
            loss = light.loss.cross_entropy(out.reshape(-1, 50), labels)
            for p in model.parameters():
                p.zero_grad()
            loss.backward()
            return out
        logits[name] = step().numpy()
        graph = HipGraph()
        with graph.capture():
            step()
        counts[name] = graph.kernel_count()
        graph.destroy()
    assert counts["dropout"] == counts["plain"] > 0, counts
    np.testing.assert_array_equal(logits["dropout"], logits["plain"])
    assert lrandom.get_state("hip") == (2, 0)                             # nothing drawn in eval()
