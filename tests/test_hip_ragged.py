"""Ragged batches in the KV cache on the GPU: lg_attention_decode_rows_f32 / lg_attention_extend_rows_f32 (a position per batch
element, csrc/decode.hip and csrc/extend.hip), lg_decode_commit_i32 (csrc/commit.hip) and what stands on them - the ops with a
`pos` of shape (b,), nn.KVCache(per_row=True), the per-row cached forward of examples/bert.py and `generate(lengths=,
eos_token_id=)`, eager and captured.

"Bit for bit against the row alone": for every batch element r, the context, the probabilities and BOTH caches equal those of
the EXISTING one-word entry called at batch 1 with pos = t_r on copies of that element's operands; cache rows >= t_r hold NaN
before either call.  The numerics of the one-word entries are the ground of test_hip_decode.py / test_hip_extend.py."""
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
import ragged_cases as rc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
bits = hd.bits


class Recorder:
    """the loaded library, noting every attention launch entry and every commit that is called (a lookup alone is none)"""
    def __init__(self, handle):
        self._handle, self.calls = handle, []

    def __getattr__(self, name):
        entry = getattr(self._handle, name)
        if not ((name.startswith("lg_attention_") and name.endswith("_f32")) or name == "lg_decode_commit_i32"):
            return entry

        def noted(*args):
            self.calls.append(name)
            return entry(*args)
        return noted


@pytest.fixture
def recorder(hip, monkeypatch):
    from lightgrad_amd.autograd.hip import lib as L
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def with_nan_beyond(cache, ts, m=0):
    """a copy of (b, capacity, width) cache rows with NaN in the rows >= t_r of element r"""
    out = cache.copy()
    for r, t in enumerate(ts):
        out[r, t:] = np.nan
    return out


def run(hip, op, q, kn, vn, k, v, pos, heads, mask):
    """one launch of `decode_attention` / `extend_attention` on fresh device copies: (context, probs, k after, v after) as numpy"""
    d = q.shape[-1] // heads
    tk, tv = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
    tm = None if mask is None else hip.from_numpy(np.ascontiguousarray(mask), requires_grad=False)
    tq, tkn, tvn = (hip.from_numpy(np.ascontiguousarray(a), requires_grad=False) for a in (q, kn, vn))
    tpos = hip.from_numpy(np.asarray(pos, np.int32), requires_grad=False)
    out = getattr(tq, op)(tkn, tvn, tk, tv, tpos, heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=True)
    return out.numpy(), out.attention_probs.numpy(), tk.numpy(), tv.numpy()


def masks_of(b, capacity):
    full = padding_mask(b, capacity)
    return (("nomask", None), ("mask", full), ("shared-mask", np.ascontiguousarray(full[-1:])))


def assert_rows_equal_their_runs_alone(hip, op, q, kn, vn, k, v, ts, heads, what):
    b, capacity = k.shape[0], k.shape[1]
    m = q.shape[1]
    for tag, mask in masks_of(b, capacity):
        got = run(hip, op, q, kn, vn, k, v, ts, heads, mask)
        for r, t in enumerate(ts):
            row_mask = None if mask is None else mask[r:r + 1] if mask.shape[0] == b else mask
            alone = run(hip, op, q[r:r + 1], kn[r:r + 1], vn[r:r + 1], k[r:r + 1], v[r:r + 1], [t], heads, row_mask)
            for name, g, a in zip(("context", "probs", "k_cache", "v_cache"), got, alone):
                np.testing.assert_array_equal(bits(g[r:r + 1]), bits(a), err_msg="%s %s row %d (t = %d): %s" % (what, tag, r, t, name))
            assert np.isfinite(got[0][r]).all() and np.isfinite(got[1][r]).all(), (what, tag, r)
            # beyond each query's own diagonal: exact +0.0
            for i in range(m):
                assert (bits(got[1][r, :, i, t + i + 1:]) == 0).all(), (what, tag, r, i)
            np.testing.assert_array_equal(bits(got[2][r, t:t + m]), bits(kn[r]), err_msg="%s %s row %d: new K rows" % (what, tag, r))
            assert np.isnan(got[2][r, t + m:]).all() and np.isnan(got[3][r, t + m:]).all(), (what, tag, r)
    return got


DECODE_CASES = [((3, 2, 32), 64, (0, 33, 63)), ((3, 1, 64), 129, (17, 128, 0)), ((4, 2, 64), 512, (255, 256, 257, 511)),
                ((2, 2, 32), 512, (511, 31))]


@pytest.mark.parametrize("shape,capacity,ts", DECODE_CASES, ids=["%dx%dx%d-cap%d" % (c[0] + (c[1],)) for c in DECODE_CASES])
def test_decode_rows_equal_each_row_alone_bit_for_bit(hip, shape, capacity, ts):
    b, heads, d = shape
    k, v, q, kn, vn = hd.operands(b, capacity, heads, d, seed=13)
    k, v = with_nan_beyond(k, ts), with_nan_beyond(v, ts)
    assert_rows_equal_their_runs_alone(hip, "decode_attention", q, kn, vn, k, v, ts, heads, "decode %s cap %d" % (shape, capacity))


EXTEND_CASES = [((3, 2, 32), 129, 33, (0, 5, 96)), ((3, 2, 64), 512, 40, (100, 128, 300)), ((2, 1, 64), 64, 1, (0, 63))]


@pytest.mark.parametrize("shape,capacity,m,ts", EXTEND_CASES, ids=["%dx%dx%d-cap%d-m%d" % (c[0] + (c[1], c[2])) for c in EXTEND_CASES])
def test_extend_rows_equal_each_row_alone_bit_for_bit(hip, shape, capacity, m, ts):
    b, heads, d = shape
    k, v, q, kn, vn = he.operands(b, capacity, m, heads, d, seed=13)
    k, v = with_nan_beyond(k, ts), with_nan_beyond(v, ts)
    assert_rows_equal_their_runs_alone(hip, "extend_attention", q, kn, vn, k, v, ts, heads, "extend %s cap %d m %d" % (shape, capacity, m))


@pytest.mark.parametrize("op,m", [("decode_attention", 1), ("extend_attention", 1), ("extend_attention", 33)])
def test_permuting_the_rows_permutes_the_results_and_two_runs_agree(hip, op, m):
    b, heads, d, capacity, ts = 4, 2, 64, 129, (3, 96, 0, 64)
    k, v, q, kn, vn = he.operands(b, capacity, m, heads, d, seed=5)
    k, v = with_nan_beyond(k, ts), with_nan_beyond(v, ts)
    mask = padding_mask(b, capacity)
    first = run(hip, op, q, kn, vn, k, v, ts, heads, mask)
    again = run(hip, op, q, kn, vn, k, v, ts, heads, mask)
    perm = np.array([2, 0, 3, 1])
    moved = run(hip, op, q[perm], kn[perm], vn[perm], k[perm], v[perm], np.array(ts)[perm], heads, mask[perm])
    for name, a, c, p in zip(("context", "probs", "k_cache", "v_cache"), first, again, moved):
        np.testing.assert_array_equal(bits(a), bits(c), err_msg="%s: two runs, %s" % (op, name))
        np.testing.assert_array_equal(bits(a[perm]), bits(p), err_msg="%s: permuted rows, %s" % (op, name))


def test_self_attention_forms_take_a_position_per_row(hip, recorder):
    """`self_attention_decode` / `self_attention_extend` with pos (b,): the rows entry behind the projection launch; against
    `decode_attention` / `extend_attention` (the ground of the tests above) on projections made in float64 on the host"""
    b, heads, d, capacity, hidden = 3, 2, 32, 40, 64
    width = heads * d
    rng = np.random.RandomState(2)
    w = [rng.uniform(-0.3, 0.3, (width, hidden)).astype(np.float32) for _ in range(3)]
    bias = [rng.uniform(-0.3, 0.3, width).astype(np.float32) for _ in range(3)]
    params = [hip.from_numpy(a, requires_grad=False) for pair in zip(w, bias) for a in pair]
    for op, m, ts, entry in (("decode", 1, (0, 39, 17), "lg_attention_decode_rows_f32"), ("extend", 5, (0, 35, 17), "lg_attention_extend_rows_f32")):
        x = rng.uniform(-1, 1, (b, m, hidden)).astype(np.float32)
        k0, v0 = (rng.uniform(-1, 1, (b, capacity, width)).astype(np.float32) for _ in range(2))
        q, kn, vn = ((x.astype(np.float64) @ wi.astype(np.float64).T + bi).astype(np.float32) for wi, bi in zip(w, bias))
        pos = hip.from_numpy(np.array(ts, np.int32), requires_grad=False)
        tk, tv = hip.from_numpy(k0, requires_grad=False), hip.from_numpy(v0, requires_grad=False)
        del recorder.calls[:]
        with light.no_grad():
            one = getattr(hip.from_numpy(x, requires_grad=False), "self_attention_" + op)(*params, tk, tv, pos, heads=heads, scale=0.2)
        assert recorder.calls == [entry]
        tk2, tv2 = hip.from_numpy(k0, requires_grad=False), hip.from_numpy(v0, requires_grad=False)
        with light.no_grad():
            two = getattr(hip.from_numpy(q, requires_grad=False), op + "_attention")(
                hip.from_numpy(kn, requires_grad=False), hip.from_numpy(vn, requires_grad=False), tk2, tv2, pos, heads=heads, scale=0.2)
        for r, t in enumerate(ts):
            np.testing.assert_array_equal(tk.numpy()[r, :t], k0[r, :t])
            np.testing.assert_array_equal(tk.numpy()[r, t + m:], k0[r, t + m:])
            np.testing.assert_array_equal(tv.numpy()[r, t + m:], v0[r, t + m:])
        # a projection is 64 products of |x| <= 1 and |w| <= 0.3 summed in float32: at most 64 * 2^-24 * 19.2 = 7.4e-5 from the float64 sum
        np.testing.assert_allclose(one.numpy(), two.numpy(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(tk.numpy(), tk2.numpy(), rtol=0, atol=1e-4)
        np.testing.assert_allclose(tv.numpy(), tv2.numpy(), rtol=0, atol=1e-4)


def test_one_position_for_the_batch_and_batch_one_keep_the_old_entry(hip, recorder):
    k, v, q, kn, vn = hd.operands(2, 16, 2, 32)
    run(hip, "decode_attention", q, kn, vn, k, v, [3], 2, None)
    run(hip, "decode_attention", q[:1], kn[:1], vn[:1], k[:1], v[:1], [3], 2, None)
    run(hip, "decode_attention", q, kn, vn, k, v, [3, 4], 2, None)
    k, v, q, kn, vn = he.operands(2, 16, 3, 2, 32)
    run(hip, "extend_attention", q, kn, vn, k, v, [3], 2, None)
    run(hip, "extend_attention", q, kn, vn, k, v, [3, 4], 2, None)
    assert recorder.calls == ["lg_attention_decode_f32"] * 2 + ["lg_attention_decode_rows_f32", "lg_attention_extend_f32", "lg_attention_extend_rows_f32"]


# ---- one bad row, through the C ABI ---------------------------------------------------------------------------------------------

class DecodeRows(hd.Call):
    """test_hip_decode.Call's problem with a position per batch element, through the rows entry"""
    def __init__(self, hip, ts, **kw):
        hd.Call.__init__(self, hip, b=len(ts), **kw)
        self.pos = hip.from_numpy(np.array(ts, np.int32), requires_grad=False)
        self.args["pos"] = self.pos.ptr

    def __call__(self, **override):
        return self.lib.lg_attention_decode_rows_f32(*dict(self.args, **override).values())

    def alone(self, **override):
        return self.lib.lg_attention_decode_f32(*dict(self.args, batch=1, **override).values())


class ExtendRows(he.Call):
    def __init__(self, hip, ts, **kw):
        he.Call.__init__(self, hip, b=len(ts), **kw)
        self.pos = hip.from_numpy(np.array(ts, np.int32), requires_grad=False)
        self.args["pos"] = self.pos.ptr

    def __call__(self, **override):
        return self.lib.lg_attention_extend_rows_f32(*dict(self.args, **override).values())

    def alone(self, **override):
        return self.lib.lg_attention_extend_f32(*dict(self.args, batch=1, **override).values())


@pytest.mark.parametrize("kind", ["decode", "extend"])
def test_one_bad_row_is_reported_and_the_good_rows_are_computed(hip, kind):
    """decode: t = (5, capacity, -1); extend: t + m = capacity + 1 in one row, -1 in another.  The bounds path the existing tests
    walk (a status flag, nothing written), per row: row 0 equals its run alone, the bad rows keep every byte"""
    if kind == "decode":
        call, ref = DecodeRows(hip, (5, 8, -1)), DecodeRows(hip, (5, 5, 5))
    else:
        call, ref = ExtendRows(hip, (2, 6, -1)), ExtendRows(hip, (2, 2, 2))                 # capacity 8, m 3: 6 + 3 = capacity + 1
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert ref.alone() == 0                                               # the same operands (one seed), row 0 alone through the one-word entry
    HipDevice.synchronize()
    for name in ("o", "p", "k", "v"):
        got, want = getattr(call, name).numpy(), getattr(ref, name).numpy()
        np.testing.assert_array_equal(bits(got[0]), bits(want[0]), err_msg=name)
        assert not (got[0] == hd.SENTINEL).all()
    assert (call.o.numpy()[1:] == hd.SENTINEL).all() and (call.p.numpy()[1:] == hd.SENTINEL).all()
    np.testing.assert_array_equal(bits(call.k.numpy()[1:]), bits(call.host["k"][1:]))
    np.testing.assert_array_equal(bits(call.v.numpy()[1:]), bits(call.host["v"][1:]))


@pytest.mark.parametrize("kind", ["decode", "extend"])
def test_positions_that_overlap_a_cache_are_refused(hip, kind):
    call = DecodeRows(hip, (1, 2, 3)) if kind == "decode" else ExtendRows(hip, (1, 2, 3))
    for where in (call.args["k_cache"], call.args["v_cache"] + 64):
        assert call(pos=where) == LG_EINVAL
        assert b"overlaps a cache" in call.lib.lg_last_error() and b"_rows_f32" in call.lib.lg_last_error()
    assert call.alone(pos=call.args["k_cache"]) == LG_EINVAL               # the one-word entries refuse it as well
    assert call(D=48) == LG_EINVAL and b"_rows_f32" in call.lib.lg_last_error() and b"unsupported" in call.lib.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched()


@pytest.mark.parametrize("op", ["decode_attention", "extend_attention", "self_attention_decode", "self_attention_extend"])
def test_other_positions_are_refused_and_nothing_is_launched(hip, recorder, op):
    b, heads, d, capacity = 3, 2, 32, 16
    m = 1 if "decode" in op else 4
    k, v, q, kn, vn = he.operands(b, capacity, m, heads, d)
    tk, tv, tq, tkn, tvn = (hip.from_numpy(a, requires_grad=False) for a in (k, v, q, kn, vn))
    w = hip.from_numpy(np.zeros((64, 64), np.float32), requires_grad=False)
    bias = hip.from_numpy(np.zeros(64, np.float32), requires_grad=False)
    bad = [np.zeros(b + 1, np.int32), np.zeros((b, 1), np.int32), np.zeros(b, np.int64), np.zeros(2, np.int32)]
    for pos in bad:
        tpos = hip.from_numpy(pos, requires_grad=False)
        with pytest.raises(AssertionError, match="pos"), light.no_grad():
            if op.startswith("self"):
                getattr(tq, op)(w, bias, w, bias, w, bias, tk, tv, tpos, heads=heads, scale=0.2)
            else:
                getattr(tq, op)(tkn, tvn, tk, tv, tpos, heads=heads, scale=0.2)
    assert recorder.calls == []
    np.testing.assert_array_equal(bits(tk.numpy()), bits(k))


# ---- decode_commit ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 5, 300])
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_decode_commit_against_the_numpy_definition(hip, recorder, b, eos, strided):
    from lightgrad_amd.autograd.hip.ops import _idx_view
    rng = np.random.RandomState(10 * b + strided)
    columns = 9
    nxt = rng.randint(0, 6, (b, 1)).astype(np.int32)
    token = rng.randint(0, 6, (b, 1)).astype(np.int32)
    wide = rng.randint(0, 6, (b, columns + 5)).astype(np.int32)
    out_ids = wide[:, 2:2 + columns] if strided else wide[:, :columns].copy()
    pos = rng.randint(-1, columns - 1, b).astype(np.int32)
    done = (rng.uniform(size=b) < 0.3).astype(np.int32)
    nxt[0], done[0] = 3, 0                                                # a live row that draws id 3 ...
    if b > 1:
        nxt[1], done[1] = 3, 1                                            # ... a finished one that would ...
        pos[b - 1], done[b - 1] = columns - 1, 0                          # ... and a live row whose pos + 1 == columns: untouched, flag raised
    want = rc.commit_by_hand(nxt, token, out_ids, pos, done, eos)
    assert want[4] == (b > 1)
    t_nxt, t_token, t_pos, t_done = (hip.from_numpy(a, requires_grad=False) for a in (nxt, token, pos, done))
    t_wide = hip.from_numpy(wide if strided else np.ascontiguousarray(out_ids), requires_grad=False)
    t_out = _idx_view(t_wide, (slice(None), slice(2, 2 + columns))) if strided else t_wide
    assert t_nxt.decode_commit(t_token, t_out, t_pos, t_done, eos=eos) is None
    assert recorder.calls == ["lg_decode_commit_i32"]
    if b > 1:
        with pytest.raises(IndexError):
            HipDevice.synchronize()
    HipDevice.synchronize()
    got_wide = t_wide.numpy()
    got_out = got_wide[:, 2:2 + columns] if strided else got_wide
    for name, got, w in zip(("token", "out_ids", "pos", "done"), (t_token.numpy(), got_out, t_pos.numpy(), t_done.numpy()), want):
        np.testing.assert_array_equal(got, w, err_msg=name)
    if strided:                                                           # nothing beside the view was written
        np.testing.assert_array_equal(got_wide[:, :2], wide[:, :2])
        np.testing.assert_array_equal(got_wide[:, 2 + columns:], wide[:, 2 + columns:])
    # nxt of shape (b,) means the same
    t2 = [hip.from_numpy(a, requires_grad=False) for a in (nxt.reshape(b), token, np.ascontiguousarray(out_ids), pos, done)]
    t2[0].decode_commit(*t2[1:], eos=eos)
    if b > 1:
        with pytest.raises(IndexError):
            HipDevice.synchronize()
    np.testing.assert_array_equal(t2[3].numpy(), want[2])


def test_decode_commit_refusals_launch_nothing(hip, recorder):
    from lightgrad_amd.autograd.hip import lib as L
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)      # noqa: E731
    good = dict(nxt=i32(3, 1), token=i32(3, 1), out_ids=i32(3, 4), pos=i32(3), done=i32(3))
    for name, other in (("nxt", i32(4, 1)), ("token", i32(3)), ("out_ids", i32(4, 4)), ("pos", i32(3, 1)), ("done", i32(2)),
                        ("pos", hip.from_numpy(np.zeros(3, np.int64), requires_grad=False)), ("done", good["pos"]), ("token", good["nxt"])):
        args = dict(good, **{name: other})
        with pytest.raises(AssertionError, match="decode_commit"):
            args["nxt"].decode_commit(args["token"], args["out_ids"], args["pos"], args["done"])
    assert recorder.calls == []
    # through the C ABI: a NULL `done`, operands that overlap, a pitch below the columns
    lib, g = L.lib()._handle, {n: t.ptr for n, t in good.items()}
    entry = lambda **o: lib.lg_decode_commit_i32(*dict(dict(nxt=g["nxt"], np_=1, token=g["token"], out=g["out_ids"], op=4, cols=4, pos=g["pos"],      # noqa: E731
                                                           done=g["done"], b=3, eos=-1), **o).values())
    for override, word in ((dict(done=None), b"NULL"), (dict(done=g["pos"]), b"overlap"), (dict(token=g["out_ids"] + 4), b"overlap"),
                           (dict(op=3), b"pitch"), (dict(pos=g["pos"] + 2), b"aligned")):
        assert entry(**override) == LG_EINVAL and word in lib.lg_last_error() and b"lg_decode_commit_i32" in lib.lg_last_error(), override
    assert entry(b=0) == 0 and entry() == 0
    HipDevice.synchronize()
    assert good["pos"].numpy().tolist() == [1, 1, 1] and not good["done"].numpy().any()


# ---- the model ----------------------------------------------------------------------------------------------------------------

def test_teacher_forced_logits_of_a_ragged_batch_on_hip(hip, recorder):
    """tests/test_ragged_cpu.py's run on HipTensor against the same float64 yardstick of every sequence alone - through the rows
    entries: 2 layers x (6 decode steps + 1 append)"""
    ref64, cpu32 = rc.teacher_reference()
    got = rc.teacher_forced(hip)
    assert_as_close_to_float64_as_the_cpu_backend(rc.named(got), rc.named(cpu32), rc.named(ref64), floor=1e-5, what="per-row cache on HipTensor")
    assert recorder.calls.count("lg_attention_decode_rows_f32") == 2 * rc.FORCED and recorder.calls.count("lg_attention_extend_rows_f32") == 2
    assert "lg_attention_decode_f32" not in recorder.calls and "lg_attention_extend_f32" not in recorder.calls


def test_generate_on_hip_stops_a_row_at_its_eos_and_equals_the_float64_tokens(hip):
    tokens = rc.assert_margins_rule_out_ties()
    want, stop = rc.expected_ids(tokens)
    got, cache = rc.generate(hip)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cache.pos.numpy(), stop)                # row 0 frozen at its EOS column, the others moved on
    assert cache.lengths is None
    for chunk in (3,):
        np.testing.assert_array_equal(rc.generate(hip, prefill_chunk=chunk)[0], want)


def test_a_second_turn_with_lengths_on_hip(hip, recorder):
    """tests/test_ragged_cpu.py's second turn on HipTensor: ragged pieces appended with `generate(append=True, lengths=)` behind
    rows that stand at different positions, through the rows entry of the extend launch"""
    rc.second_turn(hip)
    assert recorder.calls.count("lg_attention_extend_rows_f32") == 2 and "lg_attention_extend_f32" not in recorder.calls
    assert "lg_attention_decode_f32" not in recorder.calls


def test_a_finished_row_is_left_alone_on_hip(hip):
    """as in test_ragged_cpu.py: row 0's cache rows and ids after 7 new tokens are bit for bit those after 8"""
    model = dc.make_model(hip, seed=rc.SEED)
    short, cache_short = rc.generate(hip, model=model, new=7)
    full, cache_full = rc.generate(hip, model=model, new=8)
    np.testing.assert_array_equal(full[0, :rc.S0 + 7], short[0])
    assert (full[0, 11:] == rc.PAD).all() and full[0, 10] == rc.EOS
    assert cache_short.pos.numpy()[0] == cache_full.pos.numpy()[0] == 10
    for layer in range(dc.CFG["num_hidden_layers"]):
        for a, b in ((cache_short.k[layer], cache_full.k[layer]), (cache_short.v[layer], cache_full.v[layer])):
            np.testing.assert_array_equal(bits(a.numpy()[0]), bits(b.numpy()[0]))


def test_uniform_lengths_through_the_per_row_path_give_todays_tokens_on_hip(hip):
    _, ids = dc.parameters()
    model = dc.make_model(hip)
    prompt = hip.from_numpy(ids[:, :dc.S0], requires_grad=False)
    today = dc.bert.generate(model, prompt, 6).numpy()
    np.testing.assert_array_equal(today[:, dc.S0:], dc.assert_margins_rule_out_ties()[:, :6])
    np.testing.assert_array_equal(dc.bert.generate(model, prompt, 6, lengths=[dc.S0] * dc.B).numpy(), today)
    np.testing.assert_array_equal(dc.bert.generate(model, prompt, 6, eos_token_id=100).numpy(), today)


def test_a_per_row_step_takes_the_rows_launch_twice_and_one_commit(hip, recorder):
    model = dc.make_model(hip, seed=rc.SEED)
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], rc.B, rc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    model(hip.from_numpy(rc.padded(rc.prompts()), requires_grad=False), cache=cache)
    cache.set_lengths(rc.LENGTHS)
    token = hip.from_numpy(np.full((rc.B, 1), 86, np.int32), requires_grad=False)
    out_ids = hip.from_numpy(np.zeros((rc.B, rc.CAPACITY), np.int32), requires_grad=False)
    done = hip.from_numpy(np.zeros(rc.B, np.int32), requires_grad=False)
    del recorder.calls[:]
    dc.bert.decode_step_rows(model, cache, token, out_ids, done, eos=rc.EOS)
    assert recorder.calls == ["lg_attention_decode_rows_f32"] * 2 + ["lg_decode_commit_i32"]
    np.testing.assert_array_equal(cache.pos.numpy(), np.array(rc.LENGTHS) + 1)


@pytest.mark.parametrize("sampled", [False, True], ids=["greedy", "sampled"])
def test_a_captured_per_row_step_replays_the_eager_run(hip, sampled):
    """eager and captured `generate(lengths=, eos_token_id=)` give the same bits, greedy and sampled; the captured per-row step
    has no more kernels than the captured uniform step of the same model (both counted here, no literal)"""
    model = dc.make_model(hip, seed=rc.SEED)
    options = dict(temperature=0.9, top_k=20, top_p=0.95) if sampled else {}
    eos = 86 if sampled else rc.EOS                                       # (the likeliest id: sampled rows stop at different steps)
    if sampled:
        light.manual_seed(5)
    eager, eager_cache = rc.generate(hip, model=model, eos=eos, **options)
    if sampled:
        light.manual_seed(5)
    graph = HipGraph()
    replayed, cache = rc.generate(hip, model=model, eos=eos, graph=graph, **options)
    np.testing.assert_array_equal(replayed, eager)
    np.testing.assert_array_equal(cache.pos.numpy(), eager_cache.pos.numpy())
    for layer in range(dc.CFG["num_hidden_layers"]):
        np.testing.assert_array_equal(bits(cache.k[layer].numpy()[:, :int(cache.pos.numpy().min())]),
                                      bits(eager_cache.k[layer].numpy()[:, :int(cache.pos.numpy().min())]))
    if not sampled:
        np.testing.assert_array_equal(replayed, rc.expected_ids(rc.assert_margins_rule_out_ties())[0])
    # the uniform step of the same model at the same batch
    if sampled:
        light.manual_seed(5)
    uniform = HipGraph()
    prompt = hip.from_numpy(rc.padded(rc.prompts(), fill=7), requires_grad=False)
    dc.bert.generate(model, prompt, rc.NEW, graph=uniform, **options)
    per_row, plain = graph.kernel_count(), uniform.kernel_count()
    print("kernels of one captured decode step (%s): per-row %d, uniform %d" % ("sampled" if sampled else "greedy", per_row, plain))
    assert 0 < per_row <= plain
    graph.destroy()
    uniform.destroy()
