"""lg_sample_f32 (csrc/sample.hip) behind `HipTensor.sample`, and sampled decoding through examples/bert.py's `generate`.

The kernel holds every weight as an integer (floor(2^40 * w)), so its sums are exact and it has no rounding of its own beyond the
float32 weights: a token must lie in the row's acceptance band (tests/sample_cases.py: 1e-5 of cumulative probability around the
float64 definition) and must EQUAL the numpy backend's token wherever that band is one token.  L is the widest row the kernel
stages in LDS, found from lg_sample_last_plan; L + 1 takes the same passes from memory."""
import ctypes
import functools
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
import sample_cases as sc
import decode_cases as dc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
CASES = sc.cases(sc.WIDTHS + ("L", "L+1"))


def last_plan():
    plan = (ctypes.c_int32 * 4)()
    hiplib.check(hiplib.lib().lg_sample_last_plan(plan))
    return list(plan)


@functools.lru_cache(maxsize=None)
def lds_limit(hip):
    """L: the widest row lg_sample_f32 holds in LDS - a bisection over one-row calls, read from lg_sample_last_plan"""
    lo, hi = 1024, 1 << 17                           # kernel 0 at lo, kernel 1 at hi
    x = hip.from_numpy(np.zeros((1, hi), np.float32), requires_grad=False)
    out = hip.empty((1,), dtype=np.int64, requires_grad=False)
    base = hip.empty((1,), dtype=np.uint64, requires_grad=False)

    def kernel(cols):
        hiplib.check(hiplib.lib().lg_sample_f32(x.ptr, 1, cols, hi, 1.0, 0, 1.0, out.ptr, 8, base.ptr))
        return last_plan()[0]
    assert kernel(lo) == 0 and kernel(hi) == 1
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if kernel(mid) == 0 else (lo, mid)
    return lo


def width(hip, V):
    return lds_limit(hip) + (V == "L+1") if isinstance(V, str) else V


def seeded_at(hip, seed, call):
    """both generators seeded `seed`, about to make call number `call` (on the device: `call` zero-row calls, each one call)"""
    light.manual_seed(seed)
    lg_random._CpuGenerator.draws = call
    empty = hip.from_numpy(np.zeros((0, 3), np.float32), requires_grad=False)
    for _ in range(call):
        empty.sample()
    assert light.random.get_state("hip") == (seed, call)


def case_id(case):
    return sc.case_id((0, case[1], case[2])).replace("V0", "V%s" % case[0])


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_tokens_lie_in_the_band_and_equal_the_cpu_backend_where_it_is_one_token(hip, case):
    V, rows, parameters = width(hip, case[0]), case[1], case[2]
    x = sc.logits(V, rows)
    seeded_at(hip, sc.STREAM_SEED, sc.STREAM_CALL)
    got = hip.from_numpy(x, requires_grad=False).sample(*parameters)
    assert got.dtype == np.int64 and tuple(got.shape) == (rows,) and not got.requires_grad
    assert last_plan()[0] == (1 if case[0] == "L+1" else 0)
    want = CpuTensor.from_numpy(x, requires_grad=False).sample(*parameters).numpy()
    single = sc.assert_in_band(got.numpy(), V, rows, parameters, "HipTensor.sample")
    print("%s: %d of %d rows have a one-token band, %d tokens equal the numpy backend's" % (
        case_id(case), single.sum(), rows, (got.numpy() == want).sum()))
    np.testing.assert_array_equal(got.numpy()[single], want[single])


@pytest.mark.parametrize("V", [30522, "L+1"])
def test_two_runs_from_one_seed_give_the_same_bits(hip, V):
    x = hip.from_numpy(sc.logits(width(hip, V), 64), requires_grad=False)
    runs = []
    for _ in range(2):
        light.manual_seed(13)
        runs.append([x.sample(0.8, 50, 0.95).numpy(), x.sample(1.3, 0, 0.9).numpy(), x.sample().numpy()])
    for a, b in zip(*runs):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(runs[0][2], runs[0][1])


def test_every_call_advances_draws_by_one(hip):
    light.manual_seed(5)
    assert light.random.get_state("hip") == (5, 0)
    x = hip.from_numpy(sc.logits(257, 5), requires_grad=False)
    first = x.sample().numpy()
    assert light.random.get_state("hip") == (5, 1)
    x.sample(0.7, 40, 0.9)
    assert light.random.get_state("hip") == (5, 2)
    empty = hip.from_numpy(np.zeros((0, 9), np.float32), requires_grad=False).sample()
    assert tuple(empty.shape) == (0,) and light.random.get_state("hip") == (5, 3)         # a zero-row call is a call
    hip.from_numpy(sc.logits(33, 64), requires_grad=False).sample(dtype=np.int32)           # 64 workgroups: one advance
    assert light.random.get_state("hip") == (5, 4)
    light.manual_seed(5)
    np.testing.assert_array_equal(x.sample().numpy(), first)


@pytest.mark.parametrize("V", [2, 33, 4097, 30522])
def test_top_k_1_is_argmax_bit_for_bit(hip, V):
    x = sc.logits(V, 64)
    untied = (x == x.max(axis=1, keepdims=True)).sum(axis=1) == 1
    assert untied.sum() >= 32
    light.manual_seed(11)
    t = hip.from_numpy(x, requires_grad=False)
    got, want = t.sample(top_k=1), t.argmax(-1)
    assert got.dtype == want.dtype == np.int64
    np.testing.assert_array_equal(got.numpy()[untied], want.numpy()[untied])


def test_degenerate_rows_answer_argmax_and_raise_no_flag(hip):
    from test_sample_cpu import degenerate_rows
    x, degenerate = degenerate_rows()
    t = hip.from_numpy(x, requires_grad=False)
    want = t.argmax(-1).numpy()
    np.testing.assert_array_equal(want, np.argmax(x, axis=1))
    light.manual_seed(3)
    for parameters in ((1.0, 0, 1.0), (0.8, 5, 0.9), (2.0, 0, 0.99)):
        for _ in range(8):
            got = t.sample(*parameters, dtype=np.int32).numpy()
            np.testing.assert_array_equal(got[degenerate], want[degenerate])
            assert got[3] % 2 == 1, "a -inf logit was returned"
    HipDevice.synchronize()                          # no status flag was raised


def test_rows_at_the_lds_limit_and_one_beyond(hip):
    L = lds_limit(hip)
    print("the widest row held in LDS: %d floats" % L)
    assert L >= 30522
    for V, kernel in ((L, 0), (L + 1, 1)):
        hip.from_numpy(sc.logits(V, 1), requires_grad=False).sample(0.8, 50, 0.95)
        plan = last_plan()
        assert plan[0] == kernel and plan[1] == 1024 and plan[2] == 1 + 3 + 4 + 2 and plan[3] == 1 - kernel, plan      # max, top-k, W + top-p, scan
    hip.from_numpy(sc.logits(257, 5), requires_grad=False).sample()
    assert last_plan() == [0, 256, 3, 1]


def test_views_equal_the_dense_call(hip):
    x = sc.logits(4097, 5)
    parameters = (0.8, 50, 0.95)

    def tokens(t):
        light.manual_seed(17)
        return t.sample(*parameters, dtype=np.int32)
    dense = tokens(hip.from_numpy(x, requires_grad=False))
    assert dense.dtype == np.int32 and tuple(dense.shape) == (5,)
    lifted = tokens(hip.from_numpy(x.reshape(5, 1, 4097), requires_grad=False))
    assert tuple(lifted.shape) == (5, 1)
    np.testing.assert_array_equal(lifted.numpy().reshape(-1), dense.numpy())
    transposed = hip.from_numpy(np.ascontiguousarray(x.T), requires_grad=False).transpose(1, 0)         # the vocabulary strided
    np.testing.assert_array_equal(tokens(transposed).numpy(), dense.numpy())
    padded = np.zeros((5, 4097 + 6), np.float32)
    padded[:, 3:4100] = x
    pitched = hip.from_numpy(padded, requires_grad=False)[:, 3:4100]                    # a pitch of its own, rows off 16 bytes
    np.testing.assert_array_equal(tokens(pitched).numpy(), dense.numpy())
    single = tokens(hip.from_numpy(x[0], requires_grad=False))
    assert tuple(single.shape) == () and int(single.numpy()) == int(dense.numpy()[0])


@pytest.mark.parametrize("temperature", [1.0, 0.5])
def test_frequencies_follow_the_softmax(hip, temperature):
    """test_sample_cpu.py's frequency case on the device"""
    light.manual_seed(0)
    tokens = hip.from_numpy(np.tile(sc.FREQUENCY_ROW, (sc.FREQUENCY_ROWS, 1)), requires_grad=False).sample(temperature=temperature).numpy()
    counts, z = sc.frequency_z(tokens, temperature)
    print("temperature %g: counts %s, max |z| %.2f" % (temperature, counts.tolist(), np.abs(z).max()))
    assert counts[5] == 0 and counts.sum() == sc.FREQUENCY_ROWS
    assert np.abs(z).max() <= 4.0


def test_the_c_abi_refuses_bad_arguments_before_anything_is_launched(hip):
    lib = hiplib.lib()
    x = hip.from_numpy(sc.logits(33, 5), requires_grad=False)
    out = hip.empty((5,), dtype=np.int64, requires_grad=False)
    base = hip.empty((1,), dtype=np.uint64, requires_grad=False)
    good = dict(logits=x.ptr, rows=5, cols=33, row_pitch=33, temperature=1.0, top_k=0, top_p=1.0, out=out.ptr, out_itemsize=8, base_out=base.ptr)

    def call(**change):
        a = dict(good, **change)
        return lib.lg_sample_f32(a["logits"], a["rows"], a["cols"], a["row_pitch"], a["temperature"], a["top_k"], a["top_p"], a["out"],
                                 a["out_itemsize"], a["base_out"])
    light.manual_seed(2)
    assert light.random.get_state("hip") == (2, 0)
    for change in (dict(logits=None), dict(out=None), dict(base_out=None), dict(row_pitch=32), dict(rows=(1 << 24) + 1), dict(rows=-1),
                   dict(cols=0), dict(cols=1 << 31, row_pitch=1 << 31), dict(out_itemsize=2), dict(out_itemsize=16),
                   dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                   dict(top_k=-1), dict(top_p=0.0), dict(top_p=1.0000001), dict(top_p=float("nan"))):
        assert call(**change) == LG_EINVAL, change
        assert last_plan()[0] == -1
    assert light.random.get_state("hip") == (2, 0), "a refused call took a call of the stream"
    assert call() == 0 and last_plan()[0] == 0
    assert light.random.get_state("hip") == (2, 1)
    t = hip.from_numpy(sc.logits(33, 5), requires_grad=False)
    for bad in (dict(temperature=0.0), dict(top_k=-1), dict(top_p=0.0), dict(dtype=np.int16)):
        with pytest.raises(ValueError):
            t.sample(**bad)
    with pytest.raises(TypeError):
        hip.from_numpy(np.zeros((3, 4), np.int32), requires_grad=False).sample()
    with pytest.raises(ValueError):
        hip.from_numpy(np.zeros((3, 0), np.float32), requires_grad=False).sample()
    assert light.random.get_state("hip") == (2, 1)


def test_a_captured_sample_draws_fresh_numbers_at_every_replay(hip):
    V, rows, parameters, seed, first = 257, 64, (0.8, 50, 0.95), 19, 2
    x = sc.logits(V, rows)
    t = hip.from_numpy(x, requires_grad=False)
    t.sample(*parameters, dtype=np.int32)                                 # eager once: pool, kernel
    graph = HipGraph()
    with graph.capture():
        tokens = t.sample(*parameters, dtype=np.int32)
    assert graph.kernel_count() == 1
    seeded_at(hip, seed, first)                                           # after the capture: a replay reads the state from memory
    cpu = CpuTensor.from_numpy(x, requires_grad=False)
    seen = []
    for k in range(3):
        graph.replay()
        got = tokens.numpy().copy()
        want = cpu.sample(*parameters).numpy()
        band = sc.bands(V, parameters, seed, first + k)
        assert all(got[r] in band[r] for r in range(rows)), "replay %d" % k
        single = np.array([b.size == 1 for b in band])
        assert single.sum() >= 0.85 * rows
        np.testing.assert_array_equal(got[single], want[single], err_msg="replay %d" % k)
        seen.append(got)
    assert light.random.get_state("hip") == light.random.get_state("cpu") == (seed, first + 3)
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    graph.destroy()


def test_sampled_generation_eager_and_captured_agree_and_greedy_is_unchanged(hip):
    model = dc.make_model(hip)
    sampling = dict(temperature=0.8, top_k=40, top_p=0.95)
    new = 8

    def cache():
        return nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    light.manual_seed(23)
    eager = dc.greedy(hip, new=new, model=model, **sampling)
    assert light.random.get_state("hip") == (23, new)                     # one call per token
    light.manual_seed(23)
    sampled_graph = HipGraph()
    replayed = dc.greedy(hip, new=new, model=model, cache=cache(), graph=sampled_graph, **sampling)
    assert light.random.get_state("hip") == (23, new)
    np.testing.assert_array_equal(replayed, eager)
    light.manual_seed(24)
    assert not np.array_equal(dc.greedy(hip, new=new, model=model, **sampling), eager), "another seed gave the same continuation"
    assert eager.min() >= 0 and eager.max() < dc.CFG["vocab_size"]
    # without a temperature: the greedy ids of before, and one kernel more in the captured step (argmax + astype against sample)
    greedy_graph = HipGraph()
    greedy = dc.greedy(hip, new=new, model=model, cache=cache(), graph=greedy_graph)
    np.testing.assert_array_equal(greedy, dc.assert_margins_rule_out_ties()[:, :new])
    np.testing.assert_array_equal(dc.greedy(hip, new=new, model=model), greedy)
    print("kernels of one captured decode step: greedy %d, sampled %d" % (greedy_graph.kernel_count(), sampled_graph.kernel_count()))
    assert sampled_graph.kernel_count() == greedy_graph.kernel_count() - 1
    assert light.random.get_state("hip")[1] == new, "greedy decoding took a call of the stream"
    sampled_graph.destroy()
    greedy_graph.destroy()
