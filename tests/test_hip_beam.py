"""Beam search on the GPU: lg_beam_step_f32 and lg_beam_reorder_f32 (csrc/beam.hip) against the numpy backend's definitions - every
integer operand byte for byte, the scores against the float64 definition -, their host refusals, and `generate(num_beams=w)` of
examples/bert.py on HipTensor, eager and captured, against the float64 reference beam search of beam_cases.py."""
import ctypes
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
import decode_cases as dc
import speculate_cases as sc
import beam_cases as bc
from test_hip_serve import Recorder

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
GOOD = tuple(k for k in bc.KINDS if not k.startswith("bad"))
BAD = tuple(k for k in bc.KINDS if k.startswith("bad"))
# groups per state: every kind occurs for b = 1 (one state each) and for b = 3 (three at a time, a flagged group among good ones)
KIND_SETS = {1: [(k,) for k in bc.KINDS], 3: [GOOD[0:3], GOOD[3:6], (GOOD[6], BAD[0], GOOD[0]), (BAD[1], GOOD[1], BAD[2])]}
MEASURED = {}                             # V -> the largest deviation of a score from the float64 definition, over this process


@pytest.fixture
def recorder(hip, monkeypatch):
    from lightgrad_amd.autograd.hip import lib as L
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


def synchronize(flagged):
    if flagged:
        with pytest.raises(IndexError):
            HipDevice.synchronize()
    HipDevice.synchronize()


# ---- beam_step --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 3])
@pytest.mark.parametrize("vocab", ["w", 101, 4099, 30522])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_beam_step_against_the_numpy_definition(hip, recorder, b, vocab, strided):
    for w in (1, 2, 4, 8):
        V = w if vocab == "w" else vocab
        for n, kinds in enumerate(KIND_SETS[b]):
            columns = (2, 7, 33, 64)[(n + w) % 4]
            what = "b %d, w %d, V %d, columns %d, %s" % (b, w, V, columns, kinds)
            state, logits, eos = bc.step_state(kinds, w, V, columns, seed=1000 * w + 10 * n + b)
            dev = bc.assert_margins_rule_out_ties(state, logits, w, what)
            eos = eos if n % 2 else None
            want, flagged = bc.step_on(CpuTensor, state, logits, w, eos, strided_out=strided)
            exact, _ = bc.step_by_hand_fast(state, logits, w, eos)
            del recorder.calls[:]
            tensors, error = bc.step_on(hip, state, logits, w, eos, strided_out=strided, three_d=bool(n % 2))
            assert error is None and recorder.calls == ["lg_beam_step_f32"], what
            synchronize(flagged is not None)
            for name in bc.NAMES[1:] + (("wide",) if strided else ()):
                np.testing.assert_array_equal(tensors[name].numpy(), want[name].numpy(), err_msg="%s (%s)" % (name, what))
            np.testing.assert_array_equal(tensors["logits"].numpy().reshape(logits.shape), logits)
            got = tensors["scores"].numpy().astype(np.float64)
            finite = np.isfinite(exact["scores64"])
            np.testing.assert_array_equal(got[~finite], exact["scores64"][~finite], err_msg=what)
            deviation = np.abs(got[finite] - exact["scores64"][finite])
            tol = 8 * dev + 2.0 ** -22 * np.maximum(1.0, np.abs(exact["scores64"][finite]))
            MEASURED[V] = max(MEASURED.get(V, 0.0), float(deviation.max()) if deviation.size else 0.0)
            print("%s: largest score deviation %.3g (dev32 %.3g, smallest bound %.3g)" % (what, deviation.max() if deviation.size else 0.0, dev, tol.min() if tol.size else 0.0))
            assert (deviation <= tol).all(), "%s: a score is %.3g from the float64 definition, bound %.3g" % (what, deviation.max(), tol[np.argmax(deviation - tol)])
    print("largest score deviation per V so far: %s" % MEASURED)


def test_two_launches_agree_bytewise_and_a_group_does_not_depend_on_its_neighbours(hip):
    for w, V in ((4, 101), (8, 30522), (2, 4099)):
        kinds = ("mixed", "ties_across", "done_top")
        state, logits, eos = bc.step_state(kinds, w, V, 33, seed=5 * w)
        first, _ = bc.step_on(hip, state, logits, w, eos)
        again, _ = bc.step_on(hip, state, logits, w, eos)
        # the outer groups change places: the middle one keeps its rows, its inputs and so its bytes
        order = np.concatenate([np.arange(2 * w, 3 * w), np.arange(w, 2 * w), np.arange(0, w)])
        moved_state = {k: (v if k == "stats" else v[order]) for k, v in state.items()}
        moved, _ = bc.step_on(hip, moved_state, logits[order], w, eos)
        HipDevice.synchronize()
        for name in bc.NAMES:
            a, c, m = first[name].numpy(), again[name].numpy(), moved[name].numpy()
            assert a.tobytes() == c.tobytes(), name
            if name != "stats":
                assert a[w:2 * w].tobytes() == m[w:2 * w].tobytes(), name
        # the planted cross-beam tie resolves by index: identical candidates, bit for bit
        s = first["scores"].numpy()
        assert s[w] == s[w + 1] and list(first["parent"].numpy()[w:w + 2]) == [w, w + 1]


def test_beam_step_refusals_launch_nothing(hip, recorder):
    state, logits, _ = bc.step_state(("mixed", "initial"), 2, 11, 8, seed=0)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    f32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.float32), requires_grad=False)      # noqa: E731
    call = lambda x, tensors, w=2, **kw: x.beam_step(*(tensors[k] for k in bc.NAMES), w, **kw)   # noqa: E731
    for name, other in (("scores", f32(3)), ("scores", i32(4)), ("parent", i32(4, 1)), ("token", i32(4)), ("out_ids", i32(3, 8)), ("pos", i32(5)),
                        ("done", f32(4)), ("stats", i32(3)), ("pos", "done"), ("parent", "pos")):
        tensors = bc.upload(hip, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="beam_step"):
            call(hip.from_numpy(logits.copy(), requires_grad=False), tensors)
    tensors = bc.upload(hip, state)
    for bad_logits, w in ((f32(3, 11), 2), (f32(4, 11), 3), (f32(4, 11), 0), (f32(4, 11), 9), (f32(4, 1), 2)):
        with pytest.raises(AssertionError, match="beam_step"):
            call(bad_logits, tensors, w)
    assert recorder.calls == []
    # through the C ABI
    t_logits = hip.from_numpy(logits.copy(), requires_grad=False)
    g = {k: t.ptr for k, t in tensors.items()}
    good = dict(logits=t_logits.ptr, lp=11, scores=g["scores"], parent=g["parent"], token=g["token"], out_ids=g["out_ids"], op=8, columns=8,
                pos=g["pos"], done=g["done"], stats=g["stats"], rows=4, vocab=11, w=2, eos=-1)
    handle = recorder._handle
    entry = lambda **o: handle.lg_beam_step_f32(*dict(good, **o).values())                     # noqa: E731
    for override, word in ((dict(stats=None), b"NULL"), (dict(logits=None), b"NULL"), (dict(pos=g["done"]), b"overlap"),
                           (dict(parent=g["pos"] + 4), b"overlap"), (dict(scores=t_logits.ptr + 8), b"overlap"), (dict(stats=g["done"] + 8), b"overlap"),
                           (dict(op=7), b"pitch"), (dict(lp=10), b"pitch"), (dict(pos=g["pos"] + 2), b"aligned"), (dict(w=0), b"num_beams"),
                           (dict(w=9), b"num_beams"), (dict(w=3), b"unsupported"), (dict(vocab=1, lp=1), b"unsupported"), (dict(columns=0), b"unsupported"),
                           (dict(rows=1 << 24), b"unsupported")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_beam_step_f32" in handle.lg_last_error(), override
    assert entry(rows=0) == 0
    HipDevice.synchronize()
    for name in bc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)
    assert entry() == 0
    HipDevice.synchronize()
    want, _ = bc.step_by_hand(state, logits, 2, None)
    for name in bc.NAMES[1:]:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)


# ---- beam_reorder -----------------------------------------------------------------------------------------------------------------------

def filled_cache(T, layers, rows, capacity, width, pos, w, seed):
    rng = np.random.RandomState(seed)
    cache = nn.KVCache(layers, rows, capacity, width, like=T.from_numpy(np.zeros(1, np.float32), requires_grad=False), per_row=True)
    arrays = [rng.standard_normal((rows, capacity, width)).astype(np.float32) for _ in range(2 * layers)]
    cache.k = [T.from_numpy(a.copy(), requires_grad=False) for a in arrays[:layers]]
    cache.v = [T.from_numpy(a.copy(), requires_grad=False) for a in arrays[layers:]]
    cache.set_lengths(pos)
    cache.num_beams = w
    return cache, arrays


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["identity", "swap", "cycle", "leader", "mixed"])
def test_reorder_against_the_numpy_take(hip, recorder, w, kind):
    for b in (1, 3):
        for capacity, width, layers in ((17, 64, 2), (17, 128, 1), (512, 64, 1), (512, 128, 2)):
            what = "b %d, capacity %d, width %d, layers %d" % (b, capacity, width, layers)
            rng = np.random.RandomState(capacity + width + b)
            pos = rng.randint(1, capacity + 1, b * w)                      # ragged
            pos[0] = capacity if b == 1 else 0
            parent = bc.parents(kind, b, w, seed=b + w)
            cache, arrays = filled_cache(hip, layers, b * w, capacity, width, pos, w, seed=w + b)
            del recorder.calls[:]
            assert cache.reorder(hip.from_numpy(parent, requires_grad=False)) is None
            assert recorder.calls == ["lg_beam_reorder_f32"], what
            HipDevice.synchronize()
            want = bc.reorder_by_take(arrays, parent, pos, w)
            for t, a in zip(cache.k + cache.v, want):                     # (what lies at or beyond a group's longest row: as it was)
                assert t.numpy().tobytes() == a.tobytes(), what
            np.testing.assert_array_equal(cache.pos.numpy(), pos)


def test_reorder_through_the_c_abi_pitches_sentinels_and_a_parent_outside_its_group(hip, recorder):
    w, b, capacity, width, pad = 4, 3, 9, 64, 8
    rows, ldc = b * w, width + pad
    rng = np.random.RandomState(3)
    arrays = [rng.standard_normal((rows, capacity, ldc)).astype(np.float32) for _ in range(3)]
    for a in arrays:
        a[:, :, width:] = -7.0                                             # the pitch padding
    pos = rng.randint(1, capacity, rows).astype(np.int32)
    tensors = [hip.from_numpy(a.copy(), requires_grad=False) for a in arrays]
    parent = bc.parents("cycle", b, w)
    t_parent, t_pos = hip.from_numpy(parent, requires_grad=False), hip.from_numpy(pos, requires_grad=False)
    handle = recorder._handle
    table = (ctypes.c_void_p * 3)(*[t.ptr for t in tensors])
    good = dict(tensors=table, n=3, ldc=ldc, sbc=capacity * ldc, capacity=capacity, width=width, parent=t_parent.ptr, pos=t_pos.ptr, rows=rows, w=w)
    entry = lambda **o: handle.lg_beam_reorder_f32(*dict(good, **o).values())                  # noqa: E731
    twice = (ctypes.c_void_p * 3)(tensors[0].ptr, tensors[1].ptr, tensors[0].ptr + 64)
    for override, word in ((dict(n=65), b"tensors"), (dict(w=0), b"num_beams"), (dict(w=9), b"num_beams"), (dict(w=5), b"unsupported"),
                           (dict(width=62), b"unsupported"), (dict(ldc=width - 4), b"pitch"), (dict(sbc=capacity * ldc - 4 * pad), b"pitch"),
                           (dict(ldc=ldc + 2), b"pitch"), (dict(parent=None), b"NULL"), (dict(pos=t_pos.ptr + 2), b"aligned"),
                           (dict(pos=t_parent.ptr + 4), b"overlap"), (dict(tensors=twice), b"overlap"), (dict(parent=tensors[1].ptr + 16), b"overlap"),
                           (dict(tensors=(ctypes.c_void_p * 3)(tensors[0].ptr, tensors[1].ptr + 4, tensors[2].ptr)), b"aligned")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_beam_reorder_f32" in handle.lg_last_error(), override
    assert entry(rows=0) == 0 and entry(n=0) == 0
    HipDevice.synchronize()
    for t, a in zip(tensors, arrays):
        assert t.numpy().tobytes() == a.tobytes()
    assert entry() == 0
    HipDevice.synchronize()
    for t, a, moved in zip(tensors, arrays, bc.reorder_by_take([a[:, :, :width] for a in arrays], parent, pos, w)):
        got = t.numpy()
        assert got[:, :, :width].tobytes() == np.ascontiguousarray(moved).tobytes()
        assert (got[:, :, width:] == -7.0).all()
        for lo in range(0, rows, w):
            L = pos[lo:lo + w].max()
            assert got[lo:lo + w, L:].tobytes() == a[lo:lo + w, L:].tobytes()      # sentinels at and beyond the longest row
    # one parent outside its group, once, with in-range memory: the flag, the group as it was, the others moved
    before = [t.numpy().copy() for t in tensors]
    outside = parent.copy()
    outside[w + 1] = 0
    assert handle.lg_beam_reorder_f32(table, 3, ldc, capacity * ldc, capacity, width, hip.from_numpy(outside, requires_grad=False).ptr, t_pos.ptr, rows, w) == 0
    synchronize(True)
    inside = outside.copy()
    inside[w:2 * w] = np.arange(w, 2 * w)
    for t, old, moved in zip(tensors, before, bc.reorder_by_take(before, inside, pos, w)):
        assert t.numpy()[w:2 * w].tobytes() == old[w:2 * w].tobytes() and t.numpy().tobytes() == moved.tobytes()


def test_kv_reorder_refusals_launch_nothing(hip, recorder):
    cache, _ = filled_cache(hip, 1, 4, 5, 64, [3, 3, 2, 2], 2, seed=0)
    parent = lambda *p: hip.from_numpy(np.array(p, np.int32), requires_grad=False)             # noqa: E731
    del recorder.calls[:]
    for bad in (lambda: cache.reorder(parent(0, 1, 2)), lambda: cache.reorder(parent(0, 1, 2, 3), 3), lambda: cache.reorder(parent(0, 1, 2, 3), 9),
                lambda: cache.reorder(hip.from_numpy(np.zeros(4, np.int64), requires_grad=False)), lambda: cache.reorder(cache.pos),
                lambda: hip.kv_reorder(cache.k + cache.k, parent(0, 1, 2, 3), cache.pos, 2)):
        with pytest.raises(AssertionError):
            bad()
    assert recorder.calls == []


# ---- generate(num_beams=w) --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=bc.SEED)


@pytest.mark.parametrize("w", [2, 4])
@pytest.mark.parametrize("eos", [None, bc.EOS, bc.EOS_ALL], ids=["budget", "eos", "eos-everywhere"])
def test_beam_search_on_hip_eager_and_captured(hip, model, w, eos):
    _, dev = bc.assert_reference_rules_out_ties(bc.SEED, w, eos)
    ids, beams, cache = bc.run(hip, bc.SEED, w, model=model, eos=eos, poll=1)
    bc.compare_with_reference(ids, beams, bc.SEED, w, eos, dev)
    _, _, scores = bc.expected(bc.SEED, w, eos)
    print("%d beams, eos %s: largest score deviation from the float64 reference %.3g (dev32 %.3g)" % (w, eos, np.abs(beams["scores"] - scores).max(), dev))
    graph = HipGraph()
    ids_g, beams_g, _ = bc.run(hip, bc.SEED, w, model=model, eos=eos, poll=1, graph=graph)
    print("kernels of one captured beam-search step (b * w = %d): %d" % (4 * w, graph.kernel_count()))
    assert graph.kernel_count() > 0
    graph.destroy()
    assert ids_g.tobytes() == ids.tobytes() and beams_g["scores"].tobytes() == beams["scores"].tobytes() and beams_g["steps"] == beams["steps"]
    results, _, _ = bc.beam_reference(bc.SEED, w, eos)
    for r, (p, (hyps, _)) in enumerate(zip(sc.prompts(bc.SEED), results)):
        for n, (tokens, _, _) in enumerate(hyps):
            used = len(p) + len(tokens)
            assert beams_g["sequences"][r, n, :used].tobytes() == beams["sequences"][r, n, :used].tobytes()
    assert cache.lengths is None


def test_every_step_is_the_decode_forward_one_beam_step_and_one_reorder_and_the_host_reads_the_poll_word(hip, model, recorder):
    w, eos, poll = 4, None, 3
    ps = sc.prompts(bc.SEED)
    lengths = [len(p) for p in ps]
    padded = np.zeros((4, max(lengths)), np.int32)
    for r, p in enumerate(ps):
        padded[r, :len(p)] = p
    ids = hip.from_numpy(padded, requires_grad=False)
    cache = nn.KVCache(bc.CFG["num_hidden_layers"], 4 * w, bc.CAPACITY, bc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    info = {}
    del recorder.calls[:], recorder.reads[:]
    out = dc.bert.generate(model, ids, bc.NEW, lengths=lengths, eos_token_id=eos, pad_token_id=bc.PAD, cache=cache, num_beams=w, poll=poll, beams=info)
    calls = [c for c in recorder.calls if c != "lg_sync"]
    steps = info["steps"]
    assert steps == bc.NEW - 1 and steps % poll == 0
    assert recorder.reads == [4] * (steps // poll)                         # one int32 word per poll, nothing else
    rows, _, _ = bc.expected(bc.SEED, w, eos)
    np.testing.assert_array_equal(out.numpy(), rows)
    assert calls.count("lg_beam_step_f32") == steps + 1 and calls.count("lg_beam_reorder_f32") == steps + 1      # (+ the first token, the broadcast)
    behind = calls[calls.index("lg_beam_step_f32") + 1:]
    per_step, step = [], []
    for name in behind:
        step.append(name)
        if name == "lg_beam_reorder_f32":
            per_step.append(step)
            step = []
    # (the first step also uploads the constants of a (b * w, 1) forward)
    assert len(per_step) == steps and all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the beams hold"
    del recorder.calls[:]
    import lightgrad_amd as light
    with light.no_grad():
        model(hip.from_numpy(np.zeros((4 * w, 1), np.int32), requires_grad=False), cache=cache)
    forward = [c for c in recorder.calls if c != "lg_sync"]
    assert per_step[1] == forward + ["lg_beam_step_f32", "lg_beam_reorder_f32"]
    assert forward.count("lg_attention_decode_rows_f32") == bc.CFG["num_hidden_layers"]
    print("launch entries of one beam-search step: %d (the decode forward: %d)" % (len(per_step[1]), len(forward)))


def test_generate_without_num_beams_on_hip_is_what_it_was(hip, recorder):
    want, _ = sc.expected(2)
    out, stats, cache = sc.run(hip, 2, None)
    np.testing.assert_array_equal(out, want)
    assert stats == {} and cache.lengths is not None and cache.num_beams == 1
    assert not any("beam" in c for c in recorder.calls) and recorder.calls.count("lg_decode_commit_i32") == sc.NEW
