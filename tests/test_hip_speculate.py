"""Speculative decoding by prompt lookup on the GPU: lg_speculate_commit_i32 (csrc/speculate.hip) byte for byte against the
numpy backend's definition on every operand, its host refusals, and `generate(speculate=k)` of examples/bert.py on HipTensor,
eager and captured - against the float64 greedy continuation of every prompt ALONE (speculate_cases.py)."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
import decode_cases as dc
import speculate_cases as sc
from test_hip_serve import Recorder

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
# (m, columns): every m at every width up to the model's 512 positions, and two widths beyond the 4096 columns staged in LDS
SIZES = [(m, columns) for m in (1, 2, 4, 8) for columns in (2, 7, 64, 512)] + [(4, 4100), (8, 4097)]


@pytest.fixture
def recorder(hip, monkeypatch):
    from lightgrad_amd.autograd.hip import lib as L
    rec = Recorder(L.lib())
    monkeypatch.setattr(L, "lib", lambda: rec)
    return rec


# ---- speculate_commit ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 3, 67])
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_speculate_commit_against_the_numpy_definition(hip, recorder, b, eos, strided):
    for m, columns in SIZES:
        for draft in sorted({0, m - 1}):
            for max_ngram, min_ngram in ((1, 1), (3, 1), (5, 5)):
                for overflow in (False, True):
                    what = "m %d, columns %d, draft %d, n-grams %d..%d, overflow %s" % (m, columns, draft, min_ngram, max_ngram, overflow)
                    state, tgt = sc.commit_state(b, m, columns, seed=1000 * b + 10 * m + columns, draft=draft, max_ngram=max_ngram,
                                                 min_ngram=min_ngram, eos=eos, overflow=overflow)
                    want, flagged = sc.commit_on(CpuTensor, state, tgt, draft, max_ngram, min_ngram, eos, strided_out=strided)
                    del recorder.calls[:]
                    tensors, error = sc.commit_on(hip, state, tgt, draft, max_ngram, min_ngram, eos, strided_out=strided)
                    assert error is None and recorder.calls == ["lg_speculate_commit_i32"], what
                    if flagged is not None:
                        with pytest.raises(IndexError):
                            HipDevice.synchronize()
                    HipDevice.synchronize()
                    for name in sc.NAMES + ("tgt",) + (("wide",) if strided else ()):
                        np.testing.assert_array_equal(tensors[name].numpy(), want[name].numpy(), err_msg="%s (%s)" % (name, what))


def test_two_launches_on_the_same_state_agree_and_rows_do_not_depend_on_their_neighbours(hip):
    b, m, columns = 67, 8, 512
    state, tgt = sc.commit_state(b, m, columns, seed=4, draft=7, eos=3)
    first, _ = sc.commit_on(hip, state, tgt, 7, 3, 1, 3)
    again, _ = sc.commit_on(hip, state, tgt, 7, 3, 1, 3)
    perm = np.random.RandomState(0).permutation(b)
    moved, _ = sc.commit_on(hip, {k: (v if k == "stats" else v[perm]) for k, v in state.items()}, tgt[perm], 7, 3, 1, 3)
    for name in sc.NAMES:
        np.testing.assert_array_equal(first[name].numpy(), again[name].numpy(), err_msg=name)
        np.testing.assert_array_equal(first[name].numpy() if name == "stats" else first[name].numpy()[perm], moved[name].numpy(), err_msg=name)


def test_speculate_commit_refusals_launch_nothing(hip, recorder):
    state, tgt = sc.commit_state(3, 4, 16, seed=0, draft=3)
    i32 = lambda *shape: hip.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("ids", i32(3, 5)), ("count", i32(4)), ("out_ids", i32(3)), ("pos", i32(3, 1)), ("stats", i32(2)),
                        ("pos", hip.from_numpy(np.zeros(3, np.int64), requires_grad=False)), ("count", "pos"), ("end", "done"), ("position_ids", "ids")):
        tensors = sc.upload(hip, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="speculate_commit"):
            hip.from_numpy(tgt.copy(), requires_grad=False).speculate_commit(*(tensors[k] for k in sc.NAMES), 3)
    tensors = sc.upload(hip, state)
    for bad in (dict(draft=4), dict(draft=-1), dict(draft=3, min_ngram=0), dict(draft=3, max_ngram=2, min_ngram=3)):
        with pytest.raises(AssertionError, match="speculate_commit"):
            hip.from_numpy(tgt.copy(), requires_grad=False).speculate_commit(*(tensors[k] for k in sc.NAMES), **bad)
    assert recorder.calls == []
    # through the C ABI
    t_tgt = hip.from_numpy(tgt.copy(), requires_grad=False)
    g = {k: t.ptr for k, t in tensors.items()}
    good = dict(tgt=t_tgt.ptr, ids=g["ids"], count=g["count"], position_ids=g["position_ids"], out_ids=g["out_ids"], pitch=16, columns=16, pos=g["pos"],
                end=g["end"], done=g["done"], stats=g["stats"], batch=3, m=4, draft=3, max_ngram=3, min_ngram=1, eos=-1)
    handle = recorder._handle
    entry = lambda **o: handle.lg_speculate_commit_i32(*dict(good, **o).values())                # noqa: E731
    for override, word in ((dict(stats=None), b"NULL"), (dict(tgt=None), b"NULL"), (dict(count=g["pos"]), b"overlap"),
                           (dict(ids=g["position_ids"] + 4), b"overlap"), (dict(stats=g["done"] + 4), b"overlap"), (dict(tgt=g["ids"]), b"overlap"),
                           (dict(end=g["out_ids"] + 64), b"overlap"), (dict(pitch=15), b"pitch"), (dict(pos=g["pos"] + 2), b"aligned"),
                           (dict(m=0), b"unsupported"), (dict(columns=0), b"unsupported"), (dict(batch=1 << 24), b"unsupported"),
                           (dict(draft=4), b"unsupported"), (dict(draft=-1), b"unsupported"), (dict(min_ngram=0), b"unsupported"),
                           (dict(max_ngram=2, min_ngram=3), b"unsupported")):
        assert entry(**override) == LG_EINVAL and word in handle.lg_last_error() and b"lg_speculate_commit_i32" in handle.lg_last_error(), override
    assert entry(batch=0) == 0
    HipDevice.synchronize()
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)
    assert entry() == 0
    HipDevice.synchronize()
    want, _ = sc.commit_by_hand(state, tgt, 3, 3, 1, None)
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)


# ---- generate(speculate=k) ----------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def models(hip):
    return {seed: dc.make_model(hip, seed=seed) for seed in sc.SEEDS}


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("eos", [None, sc.EOS], ids=["budget", "eos"])
@pytest.mark.parametrize("seed", sc.SEEDS)
def test_speculative_generate_on_hip_gives_each_prompt_its_own_continuation(hip, models, seed, eos, captured):
    sc.assert_margins_rule_out_ties(seed)
    want, per_k = sc.expected(seed, eos=eos)
    _, cpu_stats, _ = sc.run(CpuTensor, seed, 3, eos=eos, poll=1)
    graph = HipGraph() if captured else None
    kept = []
    out, stats, cache = sc.run(hip, seed, 3, model=models[seed], eos=eos, poll=1, graph=graph, tensors=kept)
    np.testing.assert_array_equal(out, want)
    assert stats == cpu_stats == {key: per_k[3][key] for key in ("steps", "drafted", "accepted")}
    assert cache.lengths is None
    if captured:
        print("kernels of one captured speculative step (b = 4, m = 4): %d" % graph.kernel_count())
        assert graph.kernel_count() > 0
        # past completion every count is 0: a replay changes nothing
        position = cache.pos.numpy().copy()
        for _ in range(2):
            graph.replay()
        np.testing.assert_array_equal(kept[0].numpy(), want)
        np.testing.assert_array_equal(cache.pos.numpy(), position)
        graph.destroy()


def test_the_host_reads_the_poll_word_only_and_every_step_is_the_same_launches(hip, models, recorder):
    want, per_k = sc.expected(3)
    model = models[3]
    ps = sc.prompts(3)
    padded = np.zeros((4, 9), np.int32)
    for r, p in enumerate(ps):
        padded[r, :len(p)] = p
    ids = hip.from_numpy(padded, requires_grad=False)
    del recorder.calls[:], recorder.reads[:]
    out = dc.bert.generate(model, ids, sc.NEW, lengths=[len(p) for p in ps], pad_token_id=sc.PAD, speculate=3, poll=4)
    steps = -(-per_k[3]["steps"] // 4) * 4
    assert recorder.reads == [4] * (steps // 4)                             # one int32 word per poll, nothing else
    np.testing.assert_array_equal(out.numpy(), want)
    calls = [c for c in recorder.calls if c != "lg_sync"]
    per_step, step = [], []
    for name in calls:
        step.append(name)
        if name == "lg_speculate_commit_i32":
            per_step.append(step)
            step = []
    assert step == [] and len(per_step) == steps + 1                        # the first commit, then a commit at the end of every step
    assert all(s == per_step[1] for s in per_step[2:]), "a step's launches depend on what the rows hold"
    assert per_step[1].count("lg_attention_extend_counts_f32") == sc.CFG["num_hidden_layers"] and not any("decode" in c for c in calls)
    print("launch entries of one speculative step: %d" % len(per_step[1]))


def test_sampled_speculative_runs_on_hip_repeat_for_a_seed_eager_and_captured(hip, models):
    options = dict(model=models[3], temperature=1.5, top_k=4, poll=1)
    light.manual_seed(11)
    first = sc.run(hip, 3, 3, **options)
    light.manual_seed(11)
    again = sc.run(hip, 3, 3, **options)
    light.manual_seed(11)
    graph = HipGraph()
    captured = sc.run(hip, 3, 3, graph=graph, **options)
    graph.destroy()
    for other in (again, captured):
        np.testing.assert_array_equal(first[0], other[0])
        assert first[1] == other[1]
    assert first[1]["drafted"] > 0 and (first[0][:, :2] != sc.PAD).all()


def test_generate_without_speculate_on_hip_is_what_it_was(hip, models, recorder):
    want, _ = sc.expected(2)
    out, stats, cache = sc.run(hip, 2, None, model=models[2])
    np.testing.assert_array_equal(out, want)
    assert stats == {} and cache.lengths is not None and "lg_speculate_commit_i32" not in recorder.calls
    assert recorder.calls.count("lg_decode_commit_i32") == sc.NEW
