"""Continuous batching on the GPU: lg_attention_extend_counts_f32 (a token count per batch element, csrc/extend.hip),
lg_serve_commit_i32 (csrc/serve.hip) and what stands on them - `extend_attention(count=)`, `Tensor.serve_commit`,
nn.RequestPool, one mixed model step and `serve` of examples/bert.py, eager and captured.

"Bit for bit against the element alone": for every batch element r with n = count[r] > 0, its context rows < n, its rows < n of
the probabilities and BOTH caches equal those of lg_attention_extend_rows_f32 called through the C ABI at batch 1 with m = n on
copies of that element's operands.  Cache rows >= t_r and the token rows >= n hold NaN before either call: neither reaches
anything.  The numerics of the `_rows` entry are the ground of test_hip_ragged.py / test_hip_extend.py."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend
from test_hip_attention_masked import padding_mask
import test_hip_decode as hd
import test_hip_extend as he
import decode_cases as dc
import serve_cases as sc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
bits = hd.bits
QUIET = ("lg_last_error", "lg_malloc", "lg_free", "lg_pool_trim", "lg_pool_stats", "lg_memcpy_h2d", "lg_memcpy_h2d_async", "lg_memcpy_d2d",
         "lg_stream", "lg_device", "lg_device_info", "lg_device_count", "lg_init")


class Recorder:
    """the loaded library, noting every entry that is called (a lookup alone is none) but the allocator's, the uploads and the
    queries of QUIET; `reads` holds the byte count of every device-to-host copy"""
    def __init__(self, handle):
        self._handle, self.calls, self.reads = handle, [], []

    def __getattr__(self, name):
        entry = getattr(self._handle, name)
        if not name.startswith("lg_") or name in QUIET or name.endswith("_supported"):
            return entry

        def noted(*args):
            if name == "lg_memcpy_d2h":
                self.reads.append(int(args[2]))
            else:
                self.calls.append(name)
            return entry(*args)
        return noted

    def attention(self):
        return [c for c in self.calls if (c.startswith("lg_attention_") and c.endswith("_f32")) or c.endswith("_commit_i32")]


@pytest.fixture
def recorder(hip, monkeypatch):
    from lightgrad_amd.autograd.hip import lib as L
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


# ---- lg_attention_extend_counts_f32 -------------------------------------------------------------------------------------------

def operands(b, capacity, m, heads, d, ts, counts, seed=13):
    """test_hip_extend.operands with NaN in the cache rows >= t_r and in the token rows >= count[r] of element r"""
    k, v, q, kn, vn = he.operands(b, capacity, m, heads, d, seed=seed)
    for r, (t, n) in enumerate(zip(ts, counts)):
        k[r, t:], v[r, t:] = np.nan, np.nan
        if 0 <= n <= m:
            q[r, n:], kn[r, n:], vn[r, n:] = np.nan, np.nan, np.nan
    return k, v, q, kn, vn


def run_counts(hip, q, kn, vn, k, v, ts, counts, heads, mask, probs=True):
    """one launch of `extend_attention(count=)` on fresh device copies: (context, probs, k after, v after) as numpy"""
    d = q.shape[-1] // heads
    tk, tv = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
    tm = None if mask is None else hip.from_numpy(np.ascontiguousarray(mask), requires_grad=False)
    tq, tkn, tvn = (hip.from_numpy(np.ascontiguousarray(a), requires_grad=False) for a in (q, kn, vn))
    tpos = hip.from_numpy(np.asarray(ts, np.int32), requires_grad=False)
    extra = {} if counts is None else {"count": hip.from_numpy(np.asarray(counts, np.int32), requires_grad=False)}
    out = tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=probs, **extra)
    return out.numpy(), out.attention_probs.numpy() if probs else None, tk.numpy(), tv.numpy()


def rows_entry_alone(hip, q, kn, vn, k, v, t, heads, mask, scale=None):
    """lg_attention_extend_rows_f32 through the C ABI at batch 1 with m = the rows given: (context, probs, k after, v after)"""
    from lightgrad_amd.autograd.hip import lib as L
    n, width = q.shape[1], q.shape[2]
    capacity, d = k.shape[1], width // heads
    tq, tkn, tvn, tk, tv = (hip.from_numpy(np.ascontiguousarray(a), requires_grad=False) for a in (q, kn, vn, k, v))
    o = hip.from_numpy(np.full((1, n, width), he.SENTINEL, np.float32), requires_grad=False)
    p = hip.from_numpy(np.full((1, heads, n, capacity), he.SENTINEL, np.float32), requires_grad=False)
    pos = hip.from_numpy(np.array([t], np.int32), requires_grad=False)
    tm = None if mask is None else hip.from_numpy(np.ascontiguousarray(mask), requires_grad=False)
    rc = L.lib().lg_attention_extend_rows_f32(tq.ptr, width, n * width, tkn.ptr, width, n * width, tvn.ptr, width, n * width, tk.ptr, tv.ptr, width,
                                              capacity * width, pos.ptr, o.ptr, width, n * width, p.ptr, 1, heads, n, capacity, d,
                                              math.sqrt(d) ** -1 if scale is None else scale,
                                              None if tm is None else tm.ptr, 0)
    assert rc == 0, L.lib().lg_last_error()
    return o.numpy(), p.numpy(), tk.numpy(), tv.numpy()


def assert_elements_equal_their_runs_alone(hip, q, kn, vn, k, v, ts, counts, heads, what):
    b, capacity, m = k.shape[0], k.shape[1], q.shape[1]
    full = padding_mask(b, capacity)
    for tag, mask in (("nomask", None), ("mask", full)):
        got = run_counts(hip, q, kn, vn, k, v, ts, counts, heads, mask)
        for r, (t, n) in enumerate(zip(ts, counts)):
            label = "%s %s element %d (t = %d, n = %d)" % (what, tag, r, t, n)
            if n:
                alone = rows_entry_alone(hip, q[r:r + 1, :n], kn[r:r + 1, :n], vn[r:r + 1, :n], k[r:r + 1], v[r:r + 1], t, heads,
                                         None if mask is None else mask[r:r + 1])
                np.testing.assert_array_equal(bits(got[0][r:r + 1, :n]), bits(alone[0]), err_msg=label + ": context")
                np.testing.assert_array_equal(bits(got[1][r:r + 1, :, :n]), bits(alone[1]), err_msg=label + ": probs")
                np.testing.assert_array_equal(bits(got[2][r:r + 1]), bits(alone[2]), err_msg=label + ": k_cache")
                np.testing.assert_array_equal(bits(got[3][r:r + 1]), bits(alone[3]), err_msg=label + ": v_cache")
                assert np.isfinite(got[0][r, :n]).all() and np.isfinite(got[1][r, :, :n]).all(), label
                np.testing.assert_array_equal(bits(got[2][r, t:t + n]), bits(kn[r, :n]), err_msg=label + ": new K rows")
            # the rows that hold no token: +0.0, not -0.0, not what the buffer held
            assert (bits(got[0][r, n:]) == 0).all() and (bits(got[1][r, :, n:]) == 0).all(), label
            # every cache byte outside rows t .. t + n - 1 is the one it was
            for after, before in ((got[2], k), (got[3], v)):
                np.testing.assert_array_equal(bits(after[r, :t]), bits(before[r, :t]), err_msg=label)
                np.testing.assert_array_equal(bits(after[r, t + n:]), bits(before[r, t + n:]), err_msg=label)
                assert np.isnan(after[r, t + n:]).all(), label
    return got


COUNT_CASES = [((4, 2, 32), 17, 5, (8, 0, 16, 12), (1, 4, 0, 5)), ((4, 2, 32), 17, 5, (8, 0, 16, 12), (1, 4, 1, 5)),
               ((3, 2, 64), 160, 33, (127, 100, 0), (33, 32, 1)), ((2, 1, 32), 512, 64, (448, 511), (64, 1))]


@pytest.mark.parametrize("shape,capacity,m,ts,counts", COUNT_CASES, ids=["%dx%dx%d-cap%d-m%d-%s" % (c[0] + (c[1], c[2], "_".join(map(str, c[4])))) for c in COUNT_CASES])
def test_counted_elements_equal_the_rows_entry_alone_bit_for_bit(hip, shape, capacity, m, ts, counts):
    b, heads, d = shape
    k, v, q, kn, vn = operands(b, capacity, m, heads, d, ts, counts)
    assert_elements_equal_their_runs_alone(hip, q, kn, vn, k, v, ts, counts, heads, "counts %s cap %d m %d" % (shape, capacity, m))
    HipDevice.synchronize()                                               # no element raised the flag


def test_the_rows_entry_flags_the_decode_row_at_the_last_position(hip):
    """the second case's positions through today's per-row route: t = 16 with m = 5 rows does not fit 17 positions"""
    k, v, q, kn, vn = he.operands(4, 17, 5, 2, 32)
    with pytest.raises(IndexError):
        run_counts(hip, q, kn, vn, k, v, (8, 0, 16, 12), None, 2, None)               # (reported by its first read)
    HipDevice.synchronize()                                               # reported once


def test_a_count_of_m_everywhere_gives_the_rows_entrys_bits(hip, recorder):
    (b, heads, d), capacity, m, ts = (3, 2, 64), 512, 40, (100, 128, 300)
    k, v, q, kn, vn = operands(b, capacity, m, heads, d, ts, (m,) * b)
    mask = padding_mask(b, capacity)
    rows = run_counts(hip, q, kn, vn, k, v, ts, None, heads, mask)
    counted = run_counts(hip, q, kn, vn, k, v, ts, (m,) * b, heads, mask)
    assert recorder.attention() == ["lg_attention_extend_rows_f32", "lg_attention_extend_counts_f32"]
    for name, a, c in zip(("context", "probs", "k_cache", "v_cache"), rows, counted):
        np.testing.assert_array_equal(bits(a), bits(c), err_msg=name)
    # at batch 1 a count still takes the counts entry (one word of `pos`, one of `count`)
    run_counts(hip, q[:1], kn[:1], vn[:1], k[:1], v[:1], ts[:1], (m,), heads, None)
    assert recorder.attention()[-1] == "lg_attention_extend_counts_f32"


def test_permuting_the_counted_rows_permutes_the_results_and_two_runs_agree(hip):
    (b, heads, d), capacity, m, ts, counts = (4, 2, 64), 129, 33, (3, 96, 0, 64), (33, 1, 0, 32)
    k, v, q, kn, vn = operands(b, capacity, m, heads, d, ts, counts, seed=5)
    mask = padding_mask(b, capacity)
    first = run_counts(hip, q, kn, vn, k, v, ts, counts, heads, mask)
    again = run_counts(hip, q, kn, vn, k, v, ts, counts, heads, mask)
    perm = np.array([2, 0, 3, 1])
    moved = run_counts(hip, q[perm], kn[perm], vn[perm], k[perm], v[perm], np.array(ts)[perm], np.array(counts)[perm], heads, mask[perm])
    for name, a, c, p in zip(("context", "probs", "k_cache", "v_cache"), first, again, moved):
        np.testing.assert_array_equal(bits(a), bits(c), err_msg="two runs, %s" % name)
        np.testing.assert_array_equal(bits(a[perm]), bits(p), err_msg="permuted rows, %s" % name)


class CountsCall(he.Call):
    """test_hip_extend.Call's problem with a position and a count per batch element, through the counts entry"""
    def __init__(self, hip, ts, counts, **kw):
        he.Call.__init__(self, hip, b=len(ts), **kw)
        self.pos = hip.from_numpy(np.array(ts, np.int32), requires_grad=False)
        self.count = hip.from_numpy(np.array(counts, np.int32), requires_grad=False)
        args = {}
        for key, value in self.args.items():
            args[key] = self.pos.ptr if key == "pos" else value
            if key == "pos":
                args["count"] = self.count.ptr
        self.args = args

    def __call__(self, **override):
        return self.lib.lg_attention_extend_counts_f32(*dict(self.args, **override).values())


@pytest.mark.parametrize("bad", ["-1", "m + 1", "t + count = capacity + 1"])
def test_one_bad_count_is_reported_and_the_good_elements_are_computed(hip, bad):
    """capacity 8, m 3: element 1 is out of range, elements 0 and 2 are computed and equal their runs alone"""
    ts, counts = {"-1": ((2, 1, 6), (3, -1, 2)), "m + 1": ((2, 1, 6), (3, 4, 2)), "t + count = capacity + 1": ((2, 6, 6), (3, 3, 2))}[bad]
    call = CountsCall(hip, ts, counts)
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    o, p, k, v = (getattr(call, name).numpy() for name in ("o", "p", "k", "v"))
    q, kn, vn = call.q.numpy(), call.kn.numpy(), call.vn.numpy()
    for r in (0, 2):
        t, n = ts[r], counts[r]
        alone = rows_entry_alone(hip, q[r:r + 1, :n], kn[r:r + 1, :n], vn[r:r + 1, :n], call.host["k"][r:r + 1], call.host["v"][r:r + 1], t, 2, None,
                                 scale=call.args["scale"])
        np.testing.assert_array_equal(bits(o[r:r + 1, :n]), bits(alone[0]))
        np.testing.assert_array_equal(bits(p[r:r + 1, :, :n]), bits(alone[1]))
        np.testing.assert_array_equal(bits(k[r:r + 1]), bits(alone[2]))
        np.testing.assert_array_equal(bits(v[r:r + 1]), bits(alone[3]))
        assert np.isfinite(o[r, :n]).all() and not (o[r, :n] == he.SENTINEL).any() and (bits(o[r, n:]) == 0).all() and (bits(p[r, :, n:]) == 0).all()
    assert (o[1] == he.SENTINEL).all() and (p[1] == he.SENTINEL).all()
    np.testing.assert_array_equal(bits(k[1]), bits(call.host["k"][1]))
    np.testing.assert_array_equal(bits(v[1]), bits(call.host["v"][1]))


def test_counts_that_overlap_are_refused_and_nothing_is_launched(hip, recorder):
    call = CountsCall(hip, (1, 2, 3), (3, 0, 1))
    handle = recorder._handle
    entry = lambda **o: handle.lg_attention_extend_counts_f32(*dict(call.args, **o).values())      # noqa: E731
    for override, word in ((dict(count=call.args["k_cache"]), b"overlaps a cache"), (dict(count=call.args["v_cache"] + 64), b"overlaps a cache"),
                           (dict(count=call.args["pos"]), b"overlaps pos"), (dict(count=call.args["pos"] + 8), b"overlaps pos"),
                           (dict(count=None), b"non-NULL"), (dict(count=call.args["count"] + 2), b"aligned"), (dict(D=48), b"unsupported"),
                           (dict(pos=call.args["k_cache"]), b"overlaps a cache")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_attention_extend_counts_f32" in handle.lg_last_error(), override
    HipDevice.synchronize()
    assert call.untouched()
    # through the ops: a count that is pos, of another shape or dtype, or next to one position for the batch
    b, heads, d, capacity, m = 3, 2, 32, 16, 4
    k, v, q, kn, vn = he.operands(b, capacity, m, heads, d)
    tk, tv, tq, tkn, tvn = (hip.from_numpy(a, requires_grad=False) for a in (k, v, q, kn, vn))
    w = hip.from_numpy(np.zeros((64, 64), np.float32), requires_grad=False)
    bias = hip.from_numpy(np.zeros(64, np.float32), requires_grad=False)
    pos = hip.from_numpy(np.zeros(b, np.int32), requires_grad=False)
    one = hip.from_numpy(np.zeros(1, np.int32), requires_grad=False)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)          # noqa: E731
    del recorder.calls[:]
    for p, count in ((pos, pos), (pos, i32(b + 1)), (pos, i32(b, 1)), (pos, hip.from_numpy(np.zeros(b, np.int64), requires_grad=False)), (one, i32(b))):
        for op in ("extend_attention", "self_attention_extend"):
            with pytest.raises(AssertionError, match="count"), light.no_grad():
                if op.startswith("self"):
                    tq.self_attention_extend(w, bias, w, bias, w, bias, tk, tv, p, heads=heads, scale=0.2, count=count)
                else:
                    tq.extend_attention(tkn, tvn, tk, tv, p, heads=heads, scale=0.2, count=count)
    assert recorder.attention() == []
    np.testing.assert_array_equal(bits(tk.numpy()), bits(k))


# ---- serve_commit ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 5, 64, 65, 300, 1024])
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_serve_commit_against_the_loop_by_hand(hip, recorder, b, eos, strided):
    for waiting in (0, 2, 7, 400):
        for overflow in (False, True):
            state, nxt = sc.commit_state(b, waiting, seed=10 * b + waiting, eos=eos, overflow=overflow)
            want, flag = sc.commit_by_hand(state, nxt, 12, eos)
            del recorder.calls[:]
            tensors, error = sc.commit_on(hip, state, nxt, 12, eos, strided_out=strided)
            assert error is None and recorder.calls == ["lg_serve_commit_i32"]
            if flag:
                with pytest.raises(IndexError):
                    HipDevice.synchronize()
            HipDevice.synchronize()
            for name in sc.NAMES:
                np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg="%s (waiting %d, overflow %s)" % (name, waiting, overflow))
            if strided:
                wide, G = tensors["wide"].numpy(), state["out"].shape[1]
                assert (wide[:, :2] == -7).all() and (wide[:, 2 + G:] == -7).all()


def test_serve_commit_refusals_launch_nothing(hip, recorder):
    state, nxt = sc.commit_state(3, 2, seed=0)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("req", i32(4)), ("ids", i32(3, 5)), ("queue", i32(3)), ("out_len", i32(4)), ("last", i32(3, 1)), ("prompts", i32(5)),
                        ("pos", hip.from_numpy(np.zeros(3, np.int64), requires_grad=False)), ("count", "pos"), ("last", "req")):
        tensors = sc.upload(hip, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="serve_commit"):
            hip.from_numpy(nxt.copy(), requires_grad=False).serve_commit(*(tensors[k] for k in sc.NAMES), 12)
    assert recorder.calls == []
    # through the C ABI
    tensors = sc.upload(hip, state)
    t_nxt = hip.from_numpy(nxt.copy(), requires_grad=False)
    g = {k: t.ptr for k, t in tensors.items()}
    good = dict(nxt=t_nxt.ptr, np_=1, prompts=g["prompts"], pp=9, P=9, plen=g["prompt_len"], budget=g["budget"], out=g["out"], op=5, G=5,
                out_len=g["out_len"], queue=g["queue"], N=5, req=g["req"], pos=g["pos"], count=g["count"], ids=g["ids"], position_ids=g["position_ids"],
                last=g["last"], slots=3, m=4, capacity=12, eos=-1)
    handle = recorder._handle
    entry = lambda **o: handle.lg_serve_commit_i32(*dict(good, **o).values())                    # noqa: E731
    for override, word in ((dict(last=None), b"NULL"), (dict(count=g["pos"]), b"overlap"), (dict(ids=g["position_ids"] + 4), b"overlap"),
                           (dict(queue=g["req"] + 4), b"overlap"), (dict(op=4), b"pitch"), (dict(pp=8), b"pitch"), (dict(np_=0), b"pitch"),
                           (dict(pos=g["pos"] + 2), b"aligned"), (dict(slots=1025), b"unsupported"), (dict(m=0), b"unsupported"),
                           (dict(capacity=0), b"unsupported")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_serve_commit_i32" in handle.lg_last_error(), override
    assert entry(slots=0) == 0
    HipDevice.synchronize()
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)
    assert entry() == 0
    HipDevice.synchronize()
    want, _ = sc.commit_by_hand(state, nxt, 12, None)
    np.testing.assert_array_equal(tensors["ids"].numpy(), want["ids"])


# ---- one mixed model step -----------------------------------------------------------------------------------------------------

def test_one_mixed_step_on_hip_matches_each_sequence_alone(hip, recorder):
    ref64, cpu32 = sc.mixed_reference()
    got, cache = sc.mixed_step(hip)
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="mixed step on HipTensor")
    assert set(recorder.attention()) == {"lg_attention_extend_counts_f32"} and len(recorder.attention()) == 2 * 4
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])          # the caller moves the positions, not the forward


# ---- serve ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_on_hip_gives_each_request_its_own_continuation(hip, model, slots, chunk, captured):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    assert tuple(want_len) == sc.EMITTED
    graph = HipGraph() if captured else None
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, graph=graph)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
def test_serve_on_hip_with_a_budget_per_request(hip, model, captured):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGETS, None)
    graph = HipGraph() if captured else None
    out, out_len, stats = sc.run_serve(hip, 3, 4, model=model, budgets=sc.BUDGETS, eos=None, poll=1, graph=graph)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out_len, want_len)
    assert stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], sc.BUDGETS, 3, 4)
    if captured:
        graph.destroy()


def test_the_host_reads_the_poll_word_only_and_every_step_is_the_same_launches(hip, model, recorder):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    del recorder.calls[:], recorder.reads[:]
    (out, out_len), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4)
    steps = stats["steps"]
    assert steps % 4 == 0 and recorder.reads == [4] * (steps // 4)        # one int32 word per poll, nothing else
    np.testing.assert_array_equal(out.numpy(), want)
    calls = [c for c in recorder.calls if c != "lg_sync"]
    per_step, step = [], []
    for name in calls:
        step.append(name)
        if name == "lg_serve_commit_i32":
            per_step.append(step)
            step = []
    assert step == [] and len(per_step) == steps + 1                      # the admission commit, then a commit at the end of every step
    assert per_step[0] == ["lg_fill_strided", "lg_serve_commit_i32"]      # the pool sets the positions to 0, then the admissions
    assert all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the slots hold"
    assert per_step[1].count("lg_attention_extend_counts_f32") == sc.CFG["num_hidden_layers"] and not any("decode" in c for c in calls)
    print("launch entries of one serving step: %d" % len(per_step[1]))


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
def test_sampled_serving_on_hip_repeats_for_a_seed(hip, model, captured):
    options = dict(eos=86, temperature=0.9, top_k=20, top_p=0.95, poll=1)
    light.manual_seed(5)
    first = sc.run_serve(hip, 3, 4, model=model, **options)
    light.manual_seed(5)
    graph = HipGraph() if captured else None
    again = sc.run_serve(hip, 3, 4, model=model, graph=graph, **options)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    assert first[2]["steps"] == again[2]["steps"] and (first[1] >= 1).all()
    if captured:
        graph.destroy()


def test_a_single_request_on_hip_gives_generates_tokens(hip, model):
    prompt = sc.prompts()[2]
    today = dc.bert.generate(model, hip.from_numpy(prompt[None, :], requires_grad=False), sc.BUDGET).numpy()[0, len(prompt):]
    np.testing.assert_array_equal(today, sc.assert_margins_rule_out_ties()[2])
    (out, out_len), _ = dc.bert.serve(model, [prompt], sc.BUDGET, slots=1, chunk=16)
    np.testing.assert_array_equal(out.numpy()[0], today)
    assert out_len.numpy().tolist() == [sc.BUDGET]
