"""Token-packed serving steps on the GPU: lg_attention_extend_packed_f32 (csrc/extend.hip: the step's tokens of all slots in flat
(T, .) operands, `cu` says whose they are), lg_serve_commit_packed_i32 (csrc/serve_packed.hip) and what stands on them -
`extend_attention(cu=)`, `Tensor.serve_commit_packed`, one packed model step and `serve(token_budget=)` of examples/bert.py,
eager and captured.

"Bit for bit against the slot alone": for every slot s with n = cu[s + 1] - cu[s] > 0, its context rows, its rows of the
probabilities and BOTH of its caches equal those of lg_attention_extend_rows_f32 called through the C ABI at batch 1 with m = n on
copies of that slot's rows and caches.  Cache rows >= t_s and the token rows that belong to nobody hold NaN before either call:
neither reaches anything.  The numerics of the `_rows` entry are the ground of test_hip_ragged.py / test_hip_extend.py.

The launch shapes are the issue's, with two mends where its numbers contradict each other: its second set of slots owns
1 + 33 + 0 + 3 + 33 = 70 rows, which do not fit the 48 token rows it names - that set keeps every slot and runs with 80 token rows
(serve_packed_cases.PACKED_T); and m_max = 33 exceeds the first set's capacity of 17, which the entry refuses (m_max <= capacity) -
that set runs with m_max = 17."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend
from test_hip_attention_masked import padding_mask
from test_hip_serve import recorder, rows_entry_alone                     # noqa: F401 (a fixture)
import test_hip_extend as he
import test_serve_packed_cpu as cpu_side
import decode_cases as dc
import serve_cases as sc
import serve_packed_cases as pc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
HEADS = 2
bits = he.bits


# ---- lg_attention_extend_packed_f32 ---------------------------------------------------------------------------------------------

def operands(capacity, d, seed=13):
    """(k, v (slots, capacity, width), q, kn, vn (1, T, width), pos, cu) of a launch case: uniform(-1.5, 1.5) draws as
    test_hip_extend.operands, NaN in every cache row >= t and in every token row that belongs to nobody"""
    slots, T, width = pc.LAUNCH_CASES[capacity], pc.PACKED_T[capacity], HEADS * d
    rng = np.random.RandomState(seed)
    k, v = (rng.uniform(-1.5, 1.5, (len(slots), capacity, width)).astype(np.float32) for _ in range(2))
    q, kn, vn = (rng.uniform(-1.5, 1.5, (1, T, width)).astype(np.float32) for _ in range(3))
    cu = pc.cu_of(slots)
    for s, (t, _) in enumerate(slots):
        k[s, t:], v[s, t:] = np.nan, np.nan
    q[0, cu[-1]:], kn[0, cu[-1]:], vn[0, cu[-1]:] = np.nan, np.nan, np.nan
    return k, v, q, kn, vn, np.array([t for t, _ in slots], np.int32), cu


def m_max_of(capacity):
    """the issue's largest piece, 33 rows - within the cache: the entry takes 1 <= m_max <= capacity"""
    return min(pc.PACKED_M_MAX, capacity)


def run_packed(hip, q, kn, vn, k, v, pos, cu, mask, m_max="case", strided=False):
    """one launch of `extend_attention(cu=)` on fresh device copies: (context (1, T, width), probs (heads, T, capacity), k after,
    v after) as numpy.  strided: q, k_new and v_new are the thirds of ONE (1, T, 3 * width) buffer, read in place"""
    d = q.shape[-1] // HEADS
    m_max = m_max_of(k.shape[1]) if m_max == "case" else m_max
    tensor = lambda a: hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)      # noqa: E731
    tk, tv, tpos, tcu = tensor(k), tensor(v), tensor(pos), tensor(cu)
    tm = None if mask is None else tensor(mask)
    if strided:
        from lightgrad_amd.autograd.hip.ops import _idx_view
        width = q.shape[-1]
        qkv = tensor(np.concatenate([q, kn, vn], axis=-1))
        tq, tkn, tvn = (_idx_view(qkv, (slice(None), slice(None), slice(i * width, (i + 1) * width))) for i in range(3))
        assert tq._strides[1] == 3 * width
    else:
        tq, tkn, tvn = tensor(q), tensor(kn), tensor(vn)
    with light.no_grad():                                                 # (views of a tensor come with the tape's default flags)
        out = tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, scale=math.sqrt(d) ** -1, mask=tm, probs=True, cu=tcu, m_max=m_max)
    return out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()


_alone = {}


def slots_alone(hip, capacity, d, masked):
    """per slot with a row: what the `_rows` entry gives for it alone at batch 1 with m = n - computed once and left unchanged"""
    key = (capacity, d, masked)
    if key not in _alone:
        k, v, q, kn, vn, pos, cu = operands(capacity, d)
        mask = padding_mask(len(pos), capacity) if masked else None
        _alone[key] = {s: rows_entry_alone(hip, q[:, cu[s]:cu[s + 1]], kn[:, cu[s]:cu[s + 1]], vn[:, cu[s]:cu[s + 1]], k[s:s + 1], v[s:s + 1], int(pos[s]),
                                           HEADS, None if mask is None else mask[s:s + 1])
                       for s in range(len(pos)) if cu[s + 1] > cu[s]}
    return _alone[key]


def assert_slots_equal_their_runs_alone(hip, got, capacity, d, masked, what):
    k, v, q, kn, vn, pos, cu = operands(capacity, d)
    alone = slots_alone(hip, capacity, d, masked)
    for s, (t, n) in enumerate(pc.LAUNCH_CASES[capacity]):
        label = "%s slot %d (t = %d, n = %d, rows %d ..)" % (what, s, t, n, cu[s])
        lo, hi = cu[s], cu[s + 1]
        if n:
            np.testing.assert_array_equal(bits(got[0][:, lo:hi]), bits(alone[s][0]), err_msg=label + ": context")
            np.testing.assert_array_equal(bits(got[1][None, :, lo:hi]), bits(alone[s][1]), err_msg=label + ": probs")
            np.testing.assert_array_equal(bits(got[2][s:s + 1]), bits(alone[s][2]), err_msg=label + ": k_cache")
            np.testing.assert_array_equal(bits(got[3][s:s + 1]), bits(alone[s][3]), err_msg=label + ": v_cache")
            assert np.isfinite(got[0][0, lo:hi]).all() and np.isfinite(got[1][:, lo:hi]).all(), label
            np.testing.assert_array_equal(bits(got[2][s, t:t + n]), bits(kn[0, lo:hi]), err_msg=label + ": new K rows")
            # exact +0.0 beyond column t + i of row i
            for i in range(n):
                assert (bits(got[1][:, lo + i, t + i + 1:]) == 0).all(), label
        # every cache byte outside rows t .. t + n - 1 is the one it was
        for after, before in ((got[2], k), (got[3], v)):
            np.testing.assert_array_equal(bits(after[s, :t]), bits(before[s, :t]), err_msg=label)
            np.testing.assert_array_equal(bits(after[s, t + n:]), bits(before[s, t + n:]), err_msg=label)
            assert np.isnan(after[s, t + n:]).all(), label
    # the rows that belong to nobody: +0.0, not -0.0, not what the buffers held
    assert cu[-1] < got[0].shape[1] and (bits(got[0][0, cu[-1]:]) == 0).all() and (bits(got[1][:, cu[-1]:]) == 0).all(), what


@pytest.mark.parametrize("d", [32, 64])
@pytest.mark.parametrize("capacity", sorted(pc.LAUNCH_CASES))
def test_packed_slots_equal_the_rows_entry_alone_bit_for_bit(hip, recorder, capacity, d):
    k, v, q, kn, vn, pos, cu = operands(capacity, d)
    for masked in (False, True):
        mask = padding_mask(len(pos), capacity) if masked else None
        del recorder.calls[:]
        got = run_packed(hip, q, kn, vn, k, v, pos, cu, mask)
        assert recorder.attention() == ["lg_attention_extend_packed_f32"]
        assert_slots_equal_their_runs_alone(hip, got, capacity, d, masked, "cap %d D %d %s" % (capacity, d, "mask" if masked else "nomask"))
    HipDevice.synchronize()                                               # no slot raised the flag


@pytest.mark.parametrize("capacity,d", [(17, 32), (160, 64)])
def test_packed_rows_are_read_in_place_from_one_projection_buffer_and_m_max_changes_no_bit(hip, capacity, d):
    k, v, q, kn, vn, pos, cu = operands(capacity, d)
    mask = padding_mask(len(pos), capacity)
    got = run_packed(hip, q, kn, vn, k, v, pos, cu, mask, strided=True)
    assert_slots_equal_their_runs_alone(hip, got, capacity, d, True, "strided cap %d D %d" % (capacity, d))
    # one mask row for every slot, the default m_max = min(T, capacity) (a grid of more query blocks) and two runs: the same bits
    first = run_packed(hip, q, kn, vn, k, v, pos, cu, mask[:1], m_max=None)
    again = run_packed(hip, q, kn, vn, k, v, pos, cu, np.repeat(mask[:1], len(pos), axis=0))
    for name, a, c in zip(("context", "probs", "k_cache", "v_cache"), first, again):
        np.testing.assert_array_equal(bits(a), bits(c), err_msg=name)


class PackedCall(object):
    """the first launch case (capacity 17, D = 32) on the device through the C ABI, every argument replaceable; o and p hold a
    sentinel"""
    def __init__(self, hip, pos=None, cu=None):
        from lightgrad_amd.autograd.hip import lib as L
        self.lib, self.capacity, self.d = L.lib(), 17, 32
        self.T, width = pc.PACKED_T[17], HEADS * 32
        k, v, q, kn, vn, good_pos, good_cu = operands(17, 32)
        self.host = dict(k=k, v=v)
        self.k, self.v, self.q, self.kn, self.vn = (hip.from_numpy(a, requires_grad=False) for a in (k, v, q, kn, vn))
        self.pos = hip.from_numpy(np.asarray(good_pos if pos is None else pos, np.int32), requires_grad=False)
        self.cu = hip.from_numpy(np.asarray(good_cu if cu is None else cu, np.int32), requires_grad=False)
        self.o = hip.from_numpy(np.full((1, self.T, width), he.SENTINEL, np.float32), requires_grad=False)
        self.p = hip.from_numpy(np.full((HEADS, self.T, 17), he.SENTINEL, np.float32), requires_grad=False)
        self.args = dict(q=self.q.ptr, ldq=width, k_new=self.kn.ptr, ldk=width, v_new=self.vn.ptr, ldv=width, k_cache=self.k.ptr, v_cache=self.v.ptr,
                         ldc=width, sbc=17 * width, pos=self.pos.ptr, cu=self.cu.ptr, o=self.o.ptr, ldo=width, p=self.p.ptr, slots=4, heads=HEADS,
                         T=self.T, m_max=m_max_of(17), capacity=17, D=32, scale=math.sqrt(32) ** -1, mask=None, sbm=0)

    def __call__(self, **override):
        return self.lib.lg_attention_extend_packed_f32(*dict(self.args, **override).values())

    def results(self, T=None):
        """(o (T, width), p (heads, T, capacity) as a launch of T token rows lays it out, k, v)"""
        T = self.T if T is None else T
        return self.o.numpy()[0], self.p.numpy().reshape(-1)[:HEADS * T * 17].reshape(HEADS, T, 17), self.k.numpy(), self.v.numpy()

    def untouched(self):
        return ((self.o.numpy() == he.SENTINEL).all() and (self.p.numpy() == he.SENTINEL).all()
                and (bits(self.k.numpy()) == bits(self.host["k"])).all() and (bits(self.v.numpy()) == bits(self.host["v"])).all())


# what is wrong -> (pos, cu, arguments of the call, the slots that are bad, is the clearing slice bad?)
BAD_SLOTS = {"t + n > capacity": ((6, 0, 14, 13), None, {}, (3,), False),
             "decreasing cu": (None, (0, 1, 5, 4, 10), {}, (2, 3), False),       # slot 2 has n = -1; slot 3 would take rows 4 .. 9: 12 + 6 > 17
             "cu[slots] > T": (None, None, {"T": 8}, (3,), True),                # the launch is told of 8 token rows: rows 5 .. 9 leave them
             "n > m_max": (None, None, {"m_max": 4}, (3,), False)}


@pytest.mark.parametrize("bad", sorted(BAD_SLOTS))
def test_a_bad_slot_is_reported_writes_nothing_and_the_others_are_computed(hip, bad):
    pos, cu, override, bad_slots, clear_bad = BAD_SLOTS[bad]
    good = PackedCall(hip)
    assert good() == 0
    HipDevice.synchronize()
    want = good.results()
    call = PackedCall(hip, pos=pos, cu=cu)
    assert call(**override) == 0                                          # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    T = override.get("T", call.T)
    o, p, k, v = call.results(T)
    good_cu = pc.cu_of(pc.LAUNCH_CASES[17])
    for s in range(4):
        lo, hi = good_cu[s], good_cu[s + 1]
        if s in bad_slots:
            assert (o[lo:hi] == he.SENTINEL).all() and (p[:, lo:hi] == he.SENTINEL).all(), s
            np.testing.assert_array_equal(bits(k[s]), bits(call.host["k"][s]))
            np.testing.assert_array_equal(bits(v[s]), bits(call.host["v"][s]))
        else:
            np.testing.assert_array_equal(bits(o[lo:hi]), bits(want[0][lo:hi]))
            np.testing.assert_array_equal(bits(p[:, lo:hi]), bits(want[1][:, lo:hi]))
            np.testing.assert_array_equal(bits(k[s]), bits(want[2][s]))
            np.testing.assert_array_equal(bits(v[s]), bits(want[3][s]))
    whole = call.o.numpy()[0]
    if clear_bad:
        assert (whole[good_cu[-1]:] == he.SENTINEL).all() and (call.p.numpy().reshape(-1)[HEADS * T * 17:] == he.SENTINEL).all()
    else:
        assert (bits(o[good_cu[-1]:T]) == 0).all() and (bits(p[:, good_cu[-1]:]) == 0).all()


def test_packed_operands_that_overlap_are_refused_and_nothing_is_launched(hip, recorder):
    call = PackedCall(hip)
    handle = recorder._handle
    entry = lambda **o: handle.lg_attention_extend_packed_f32(*dict(call.args, **o).values())      # noqa: E731
    a = call.args
    for override, word in ((dict(cu=a["k_cache"]), b"overlaps a cache"), (dict(cu=a["v_cache"] + 64), b"overlaps a cache"), (dict(cu=a["pos"]), b"overlaps pos"),
                           (dict(cu=a["pos"] + 12), b"overlaps pos"), (dict(cu=a["q"] + 16), b"overlaps an operand"), (dict(cu=a["o"]), b"overlaps an operand"),
                           (dict(cu=a["p"] + 32), b"overlaps an operand"), (dict(cu=None), b"non-NULL"), (dict(cu=a["cu"] + 2), b"aligned"),
                           (dict(D=48), b"unsupported"), (dict(T=0), b"unsupported"), (dict(m_max=0), b"unsupported"), (dict(m_max=18), b"unsupported"),
                           (dict(pos=a["k_cache"]), b"overlaps a cache"), (dict(k_new=a["k_cache"]), b"overlap a cache"), (dict(ldq=66), b"pitches")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_attention_extend_packed_f32" in handle.lg_last_error(), override
    assert entry(slots=0) == 0
    HipDevice.synchronize()
    assert call.untouched()
    # through the ops: cu next to count, of another shape or dtype, next to (b, m) rows
    k, v, q, kn, vn, pos, cu = operands(17, 32)
    tensor = lambda x: hip.from_numpy(np.ascontiguousarray(x), requires_grad=False)      # noqa: E731
    tk, tv, tq, tkn, tvn, tpos, tcu = (tensor(x) for x in (k, v, q, kn, vn, pos, cu))
    w, bias = tensor(np.zeros((64, 64), np.float32)), tensor(np.zeros(64, np.float32))
    del recorder.calls[:]
    for kw in (dict(cu=tcu, count=tensor(np.zeros(4, np.int32))), dict(cu=tensor(np.zeros(4, np.int32))), dict(cu=tensor(np.zeros(5, np.int64))),
               dict(cu=tpos), dict(cu=tcu, m_max=18), dict(m_max=4)):
        for op in ("extend_attention", "self_attention_extend"):
            with pytest.raises(AssertionError, match="cu|m_max"), light.no_grad():
                if op.startswith("self"):
                    tq.self_attention_extend(w, bias, w, bias, w, bias, tk, tv, tpos, heads=HEADS, scale=0.2, **kw)
                else:
                    tq.extend_attention(tkn, tvn, tk, tv, tpos, heads=HEADS, scale=0.2, **kw)
    with pytest.raises(AssertionError, match="cu"), light.no_grad():
        tensor(np.zeros((2, 24, 64), np.float32)).extend_attention(tensor(np.zeros((2, 24, 64), np.float32)), tensor(np.zeros((2, 24, 64), np.float32)),
                                                                   tk, tv, tpos, heads=HEADS, scale=0.2, cu=tcu)
    assert recorder.attention() == []
    np.testing.assert_array_equal(bits(tk.numpy()), bits(k))


# ---- serve_commit_packed --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", pc.SLOTS)
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_serve_commit_packed_against_the_words_by_hand(hip, recorder, b, eos, strided):
    chunk = 4
    for T in pc.budgets_of(b, chunk):
        for waiting in (0, 2, b + 100):
            for overflow in (False, True):
                state, nxt = pc.packed_state(b, waiting, seed=10 * b + waiting, T=T, chunk=chunk, eos=eos, overflow=overflow)
                want, flag = pc.commit_packed_by_hand(state, nxt, 12, chunk, eos)
                del recorder.calls[:]
                tensors, error = pc.commit_on(hip, state, nxt, 12, chunk, eos, strided_out=strided)
                assert error is None and recorder.calls == ["lg_serve_commit_packed_i32"]
                if flag:
                    with pytest.raises(IndexError):
                        HipDevice.synchronize()
                HipDevice.synchronize()
                for name in pc.NAMES:
                    np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg="%s (T %d, waiting %d, overflow %s)" % (name, T, waiting, overflow))
                if strided:
                    wide, G = tensors["wide"].numpy(), state["out"].shape[1]
                    assert (wide[:, :2] == -7).all() and (wide[:, 2 + G:] == -7).all()


def test_the_budget_runs_out_inside_a_want_and_an_idle_slot_behind_a_full_buffer_is_clamped_on_hip(hip):
    state, nxt, T, chunk, capacity = pc.tight_state()
    want, flag = pc.commit_packed_by_hand(state, nxt, capacity, chunk, None)
    assert not flag and want["count"].tolist() == [1, 4, 1, 0] and want["last"].tolist() == [0, 4, 5, 5] and want["cu"][-1] == T
    tensors, _ = pc.commit_on(hip, state, nxt, capacity, chunk, None)
    HipDevice.synchronize()
    for name in pc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)


def test_serve_commit_packed_refusals_launch_nothing(hip, recorder):
    state, nxt = pc.packed_state(3, 2, seed=0, T=5)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("req", i32(4)), ("ids", i32(3, 5)), ("ids", i32(1, 2)), ("cu", i32(3)), ("position_ids", i32(1, 6)), ("queue", i32(3)),
                        ("cu", hip.from_numpy(np.zeros(4, np.int64), requires_grad=False)), ("count", "pos"), ("cu", "last")):
        tensors = pc.upload(hip, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="serve_commit_packed"):
            hip.from_numpy(nxt.copy(), requires_grad=False).serve_commit_packed(*(tensors[k] for k in pc.NAMES), 12, 4)
    assert recorder.calls == []
    # through the C ABI
    tensors = pc.upload(hip, state)
    t_nxt = hip.from_numpy(nxt.copy(), requires_grad=False)
    g = {k: t.ptr for k, t in tensors.items()}
    good = dict(nxt=t_nxt.ptr, np_=1, prompts=g["prompts"], pp=9, P=9, plen=g["prompt_len"], budget=g["budget"], out=g["out"], op=5, G=5,
                out_len=g["out_len"], queue=g["queue"], N=5, req=g["req"], pos=g["pos"], count=g["count"], cu=g["cu"], ids=g["ids"],
                position_ids=g["position_ids"], last=g["last"], slots=3, T=5, chunk=4, capacity=12, eos=-1)
    handle = recorder._handle
    entry = lambda **o: handle.lg_serve_commit_packed_i32(*dict(good, **o).values())             # noqa: E731
    for override, word in ((dict(cu=None), b"NULL"), (dict(cu=g["pos"]), b"overlap"), (dict(cu=g["last"] + 4), b"overlap"), (dict(ids=g["position_ids"] + 4), b"overlap"),
                           (dict(op=4), b"pitch"), (dict(pp=8), b"pitch"), (dict(cu=g["cu"] + 2), b"aligned"), (dict(slots=1025), b"unsupported"),
                           (dict(T=2), b"unsupported"), (dict(chunk=0), b"unsupported"), (dict(capacity=0), b"unsupported")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_serve_commit_packed_i32" in handle.lg_last_error(), override
    assert entry(slots=0, T=1) == 0
    HipDevice.synchronize()
    for name in pc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)
    assert entry() == 0
    HipDevice.synchronize()
    want, _ = pc.commit_packed_by_hand(state, nxt, 12, 4, None)
    np.testing.assert_array_equal(tensors["ids"].numpy(), want["ids"])
    np.testing.assert_array_equal(tensors["cu"].numpy(), want["cu"])


# ---- one packed model step ------------------------------------------------------------------------------------------------------

def test_one_packed_step_on_hip_matches_each_sequence_alone(hip, recorder):
    ref64, cpu32 = sc.mixed_reference()
    got, cache = cpu_side.packed_step(hip)
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="packed step on HipTensor")
    assert set(recorder.attention()) == {"lg_attention_extend_packed_f32"} and len(recorder.attention()) == 2 * 4
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])          # the caller moves the positions, not the forward


# ---- serve(token_budget=) -------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("run", range(len(pc.RUNS)), ids=["chunk%d-T%s" % (c, n) for c, n in zip((1, 4, 16, 16), ("slots", "slots+3", "slots+16", "slotsx16"))])
def test_packed_serve_on_hip_gives_each_request_its_own_continuation(hip, model, slots, run, captured):
    chunk, budget = pc.RUNS[run][0], pc.RUNS[run][1](slots)
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    assert tuple(want_len) == sc.EMITTED
    graph = HipGraph() if captured else None
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, graph=graph, token_budget=budget)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    lengths = [len(p) for p in sc.prompts()]
    assert stats["token_budget"] == budget and stats["steps"] == pc.simulate_packed(lengths, want_len, slots, chunk, budget)
    if budget == slots * chunk:                                           # the budget never binds: the schedule of the (slots, chunk) step
        assert stats["steps"] == sc.simulate(lengths, want_len, slots, chunk)
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


def test_the_host_reads_the_poll_word_only_and_every_packed_step_is_the_same_launches(hip, model, recorder):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    del recorder.calls[:], recorder.reads[:]
    (out, out_len), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4,
                                          token_budget=6)
    steps = stats["steps"]
    assert steps % 4 == 0 and recorder.reads == [4] * (steps // 4)        # one int32 word per poll, nothing else
    np.testing.assert_array_equal(out.numpy(), want)
    calls = [c for c in recorder.calls if c != "lg_sync"]
    per_step, step = [], []
    for name in calls:
        step.append(name)
        if name == "lg_serve_commit_packed_i32":
            per_step.append(step)
            step = []
    assert step == [] and len(per_step) == steps + 1                      # the admission commit, then a commit at the end of every step
    assert all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the slots hold"
    assert per_step[1].count("lg_attention_extend_packed_f32") == sc.CFG["num_hidden_layers"]
    assert not any("decode" in c or c in ("lg_attention_extend_counts_f32", "lg_serve_commit_i32") for c in calls)
    print("launch entries of one packed serving step: %d" % len(per_step[1]))


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
def test_sampled_packed_serving_on_hip_repeats_for_a_seed(hip, model, captured):
    options = dict(eos=86, temperature=0.9, top_k=20, top_p=0.95, poll=1, token_budget=6)
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
