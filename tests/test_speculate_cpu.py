"""Speculative decoding by prompt lookup without a device: `speculate_commit` as the numpy backend defines it against the steps
written out by hand (speculate_cases.py), and `generate(speculate=k)` of examples/bert.py on CpuTensor - against the float64
greedy continuation of every prompt ALONE, with the step counts of the schedule simulated over those reference tokens."""
import ctypes
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import lib as hiplib
from conftest import ROOT
import decode_cases as dc
import speculate_cases as sc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


# ---- speculate_commit: the definition -------------------------------------------------------------------------------------------

def assert_commit(T, state, tgt, draft, max_ngram, min_ngram, eos, strided=False, sync=None):
    want, flag = sc.commit_by_hand(state, tgt, draft, max_ngram, min_ngram, eos)
    tensors, error = sc.commit_on(T, state, tgt, draft, max_ngram, min_ngram, eos, strided_out=strided)
    if sync is not None:
        error = sync(flag) or error
    assert (error is not None) == flag
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    np.testing.assert_array_equal(tensors["tgt"].numpy(), tgt)
    if strided:                                                           # nothing beside the view was written
        wide, columns = tensors["wide"].numpy(), state["out_ids"].shape[1]
        assert (wide[:, :3] == -7).all() and (wide[:, 3 + columns:] == -7).all()
    return want


@pytest.mark.parametrize("b", [1, 3, 67])
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_speculate_commit_on_the_numpy_backend(b, eos, strided):
    for m in (1, 2, 4, 8):
        for columns in (2, 7, 64, 512):
            for draft in sorted({0, m - 1}):
                for max_ngram, min_ngram in ((1, 1), (3, 1), (5, 5)):
                    for overflow in (False, True):
                        state, tgt = sc.commit_state(b, m, columns, seed=1000 * b + 10 * m + columns, draft=draft, max_ngram=max_ngram,
                                                     min_ngram=min_ngram, eos=eos, overflow=overflow)
                        assert_commit(CpuTensor, state, tgt, draft, max_ngram, min_ngram, eos, strided)


def test_the_states_hold_what_they_are_meant_to():
    """by hand alone: every kind of row occurs in one state, and a flagged row keeps its bytes but the count"""
    b, m, columns, draft, eos = 67, 4, 64, 3, 3
    state, tgt = sc.commit_state(b, m, columns, seed=5, draft=draft, eos=eos, overflow=True)
    want, flag = sc.commit_by_hand(state, tgt, draft, 3, 1, eos)
    assert flag
    seen = set()
    for r in range(b):
        c, p, last = int(state["count"][r]), int(state["pos"][r]), int(state["end"][r])
        if state["done"][r]:
            seen.add("done")
            assert want["count"][r] == 0
        elif not (1 <= c <= m and p >= 0 and p + c <= last <= columns - 1):
            seen.add("out of bounds: %s" % ("count" if not 1 <= c <= m else "position" if p < 0 else "end" if last > columns - 1 else "room"))
            assert want["count"][r] == 0
            for name in ("ids", "position_ids", "out_ids", "pos", "end", "done"):
                np.testing.assert_array_equal(want[name][r], state[name][r], err_msg=name)
            continue
        else:
            a = 0
            while a < c - 1 and state["ids"][r, a + 1] == tgt[r, a]:
                a += 1
            e = int(want["pos"][r]) - p
            seen.add("count 1" if c == 1 else "full accept" if a == c - 1 else "full reject" if a == 0 else "partial accept")
            if e < a + 1:
                seen.add("eos inside the accepted run")
                assert want["done"][r] == 1 and tgt[r, e - 1] == eos and (want["out_ids"][r, p + e + 1:] >= sc.JUNK).all()
            elif want["done"][r]:
                seen.add("reaches end" if p + e == last else "eos")
            else:
                if last - (p + e) - 1 == 0:
                    seen.add("cap == 0")
                    assert want["count"][r] == 1
                if want["count"][r] > 1 and want["ids"][r, 0] >= 1000:
                    # built rows: the ids are unique but for what was planted
                    seq = want["out_ids"][r, :p + e + 1].tolist()
                    if seq[-1] >= 2000:
                        seen.add("two matches")
                        starts = [q for q in range(len(seq) - 3) if seq[q:q + 3] == seq[-3:]]
                        assert len(starts) == 2 and want["ids"][r, 1] == seq[starts[1] + 3] != seq[starts[0] + 3]
                    else:
                        seen.add("only a shorter match")
                        assert seq[-2:] not in [seq[q:q + 2] for q in range(len(seq) - 2)] and seq[:-1].count(seq[-1]) == 1
        np.testing.assert_array_equal(want["end"][r], state["end"][r])
    assert seen >= set(sc.KINDS[:-1]) | {"out of bounds: count", "out of bounds: position", "out of bounds: end", "out of bounds: room"}, seen
    assert want["stats"][0] - state["stats"][0] == ((want["done"] == 1) & (state["done"] == 0)).sum()


def test_a_step_by_hand():
    """three rows, m = 4: two of three drafts accepted; an end-of-sequence id as the first of two accepted drafts; a row that
    reaches its end"""
    st = dict(ids=np.array([[5, 6, 7, 8], [5, 18, 9, 0], [4, 3, 0, 0]], np.int32), count=np.array([4, 3, 2], np.int32),
              position_ids=np.zeros((3, 4), np.int32), pos=np.array([6, 2, 3], np.int32), end=np.array([15, 9, 5], np.int32),
              out_ids=np.array([[6, 7, 1, 6, 7, 2, 5] + [0] * 9, [1, 2, 5] + [0] * 13, [1, 2, 3, 4] + [0] * 12], np.int32),
              done=np.zeros(3, np.int32), stats=np.zeros(3, np.int32))
    tgt = np.array([[6, 7, 3, 3], [18, 9, 2, 2], [3, 8, 0, 0]], np.int32)
    tensors, error = sc.commit_on(CpuTensor, st, tgt, 3, 3, 1, 18)
    got = {k: tensors[k].numpy() for k in sc.NAMES}
    assert error is None
    assert got["out_ids"][0].tolist() == [6, 7, 1, 6, 7, 2, 5, 6, 7, 3] + [0] * 6 and got["pos"].tolist() == [9, 3, 5]
    # row 0: no 3-gram "6 7 3" before, no 2-gram "7 3", the 1-gram "3" neither: no drafts
    assert got["ids"][0].tolist() == [3, 0, 0, 0] and got["count"].tolist() == [1, 0, 0] and got["position_ids"][0].tolist() == [9, 0, 0, 0]
    assert got["out_ids"][1].tolist() == [1, 2, 5, 18] + [0] * 12 and got["out_ids"][2].tolist() == [1, 2, 3, 4, 3, 8] + [0] * 10
    assert got["done"].tolist() == [0, 1, 1] and got["stats"].tolist() == [2, 3 + 2 + 1, 2 + 2 + 1]
    # the same row with "3" as the model's token replaced by "2": the 3-gram "6 7 2" stands at columns 3 .. 5 and its continuation follows
    tgt[0, 2] = 2
    tensors, _ = sc.commit_on(CpuTensor, st, tgt, 3, 3, 1, 18)
    assert tensors["ids"].numpy()[0].tolist() == [2, 5, 6, 7] and tensors["position_ids"].numpy()[0].tolist() == [9, 10, 11, 12]
    # ... and with two drafts at most, and with 4-grams only ("5 6 7 2" stands nowhere else)
    assert sc.commit_on(CpuTensor, st, tgt, 2, 3, 1, 18)[0]["ids"].numpy()[0].tolist() == [2, 5, 6, 0]
    assert sc.commit_on(CpuTensor, st, tgt, 3, 4, 4, 18)[0]["count"].numpy()[0] == 1


def test_speculate_commit_refuses_other_operands():
    state, tgt = sc.commit_state(3, 4, 16, seed=0, draft=3)
    i32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    call = lambda t, tensors, draft=3, **kw: t.speculate_commit(*(tensors[k] for k in sc.NAMES), draft, **kw)     # noqa: E731
    for name, other in (("ids", i32(3, 5)), ("count", i32(4)), ("position_ids", i32(4, 4)), ("out_ids", i32(3)), ("pos", i32(3, 1)), ("end", i32(2)),
                        ("done", i32(4)), ("stats", i32(2)), ("pos", CpuTensor.from_numpy(np.zeros(3, np.int64), requires_grad=False)),
                        ("count", "pos"), ("end", "done"), ("position_ids", "ids")):
        tensors = sc.upload(CpuTensor, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="speculate_commit"):
            call(CpuTensor.from_numpy(tgt.copy(), requires_grad=False), tensors)
    tensors = sc.upload(CpuTensor, state)
    t_tgt = CpuTensor.from_numpy(tgt.copy(), requires_grad=False)
    for bad in (dict(draft=4), dict(draft=-1), dict(min_ngram=0), dict(max_ngram=2, min_ngram=3), dict(eos=1.5)):
        with pytest.raises(AssertionError, match="speculate_commit"):
            call(t_tgt, tensors, **bad)
    with pytest.raises(AssertionError, match="speculate_commit"):
        call(i32(3, 3), tensors)
    with pytest.raises(AssertionError, match="speculate_commit"):
        call(tensors["ids"], tensors)                                      # tgt overlaps ids
    for name in sc.NAMES:                                                  # nothing was written by any of them
        np.testing.assert_array_equal(tensors[name].numpy(), state[name], err_msg=name)


# ---- generate(speculate=k) ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", sc.SEEDS)
def test_the_references_rule_out_ties_and_their_schedules_hold_every_kind_of_step(seed):
    sc.assert_margins_rule_out_ties(seed)
    _, per_k = sc.expected(seed)
    plans = per_k[3]["plans"]
    print("seed %d, k = 3: steps per prompt %s" % (seed, [len(p) for p in plans]))
    assert all(11 <= len(p) <= 15 for p in plans) and sc.NEW - 1 == 23
    steps = [s for p in plans for s in p]
    assert (0, 0) in steps and (3, 3) in steps and (3, 0) in steps and any(d > 1 and 0 < a < d for d, a in steps), steps


@pytest.mark.parametrize("seed", sc.SEEDS)
@pytest.mark.parametrize("k", sc.KS)
def test_speculative_generate_gives_each_prompt_its_own_continuation(seed, k):
    sc.assert_margins_rule_out_ties(seed)
    want, per_k = sc.expected(seed)
    out, stats, cache = sc.run(CpuTensor, seed, k, poll=1)
    np.testing.assert_array_equal(out, want)
    assert stats == {key: per_k[k][key] for key in ("steps", "drafted", "accepted")}
    assert cache.lengths is None and cache.length == max(len(p) for p in sc.prompts(seed)) + sc.NEW - 1
    lengths = [len(p) for p in sc.prompts(seed)]
    np.testing.assert_array_equal(cache.pos.numpy(), np.array(lengths) + sc.NEW - 1)          # the position of each row's last token


def test_speculative_generate_stops_behind_the_end_of_sequence_id():
    tokens = sc.assert_margins_rule_out_ties(3)
    assert all(sc.EOS in t.tolist() for t in tokens)
    want, per_k = sc.expected(3, eos=sc.EOS)
    for r, (p, t) in enumerate(zip(sc.prompts(3), tokens)):
        n = t.tolist().index(sc.EOS) + 1
        assert n < sc.NEW and (want[r, len(p):len(p) + n] == t[:n]).all() and (want[r, len(p) + n:] == sc.PAD).all()
    for k in sc.KS:
        out, stats, _ = sc.run(CpuTensor, 3, k, eos=sc.EOS, poll=1)
        np.testing.assert_array_equal(out, want)
        assert stats == {key: per_k[k][key] for key in ("steps", "drafted", "accepted")}


def test_the_poll_interval_changes_the_steps_run_not_the_tokens():
    want, per_k = sc.expected(3, eos=sc.EOS)
    exact = per_k[3]["steps"]
    out, stats, _ = sc.run(CpuTensor, 3, 3, eos=sc.EOS, poll=4)
    np.testing.assert_array_equal(out, want)
    assert stats["steps"] == min(-(-exact // 4) * 4, sc.NEW - 1) and exact % 4 != 0          # steps behind the last finish change nothing
    assert (stats["drafted"], stats["accepted"]) == (per_k[3]["drafted"], per_k[3]["accepted"])


def test_a_ragged_batch_with_padding_behind_every_row():
    """two of the prompts in another order, in a wider right-padded array: `lengths` says what is real"""
    seed, k = 2, 3
    refs, ps = sc.assert_margins_rule_out_ties(seed), sc.prompts(seed)
    model = dc.make_model(CpuTensor, seed=seed)
    padded = np.full((2, 12), 77, np.int32)
    padded[0, :9], padded[1, :2] = ps[3], ps[1]
    out = dc.bert.generate(model, CpuTensor.from_numpy(padded, requires_grad=False), sc.NEW, lengths=[9, 2], speculate=k, pad_token_id=sc.PAD).numpy()
    assert out.shape == (2, 9 + sc.NEW)
    np.testing.assert_array_equal(out[0], np.concatenate([ps[3], refs[3]]))
    np.testing.assert_array_equal(out[1], np.concatenate([ps[1], refs[1], np.full(7, sc.PAD)]))


def test_a_second_turn_appends_behind_what_the_cache_holds():
    """the front of every prompt enters the cache by a prefill; the rest is appended by `generate(append=True, speculate=k)`"""
    seed, k = 3, 3
    refs, ps = sc.assert_margins_rule_out_ties(seed), sc.prompts(seed)
    model = dc.make_model(CpuTensor, seed=seed)
    front = [max(1, len(p) // 2) for p in ps]
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], 4, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    first = np.zeros((4, max(front)), np.int32)
    rest = np.zeros((4, max(len(p) - f for p, f in zip(ps, front))), np.int32)
    for r, (p, f) in enumerate(zip(ps, front)):
        first[r, :f], rest[r, :len(p) - f] = p[:f], p[f:]
    with light.no_grad():
        model.bert(CpuTensor.from_numpy(first, requires_grad=False), cache=cache)
    cache.set_lengths(front)
    stats = {}
    out = dc.bert.generate(model, CpuTensor.from_numpy(rest, requires_grad=False), sc.NEW, lengths=[len(p) - f for p, f in zip(ps, front)], cache=cache,
                           append=True, speculate=k, pad_token_id=sc.PAD, stats=stats, poll=1).numpy()
    assert out.shape == (4, rest.shape[1] + sc.NEW)
    for r, (p, f) in enumerate(zip(ps, front)):
        row = np.concatenate([p[f:], refs[r]])
        np.testing.assert_array_equal(out[r, :len(row)], row)
        assert (out[r, len(row):] == sc.PAD).all()
    _, per_k = sc.expected(seed)
    assert stats["steps"] == per_k[k]["steps"]                             # the lookup sees the whole sequence, the front included


def test_sampled_speculative_runs_repeat_for_a_seed_and_stay_within_the_filtered_support():
    seed, k, top_k = 3, 3, 4
    runs = []
    for _ in range(2):
        light.manual_seed(11)
        runs.append(sc.run(CpuTensor, seed, k, temperature=1.5, top_k=top_k, poll=1))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] and runs[0][1]["drafted"] > 0
    light.manual_seed(12)
    assert not np.array_equal(sc.run(CpuTensor, seed, k, temperature=1.5, top_k=top_k, poll=1)[0], runs[0][0])
    # every emitted token is one of the top_k of the float64 logits of its own prefix (1e-4: far above the float32 deviation
    # of 1.6e-6 that may reorder two logits, far below the logits' spread)
    model64 = dc.make_model(CpuTensor, np.float64, seed)
    for r, p in enumerate(sc.prompts(seed)):
        row = runs[0][0][r, :len(p) + sc.NEW]
        assert (row != sc.PAD).all()
        logits = dc.full_logits(model64, row[None, :])[0]
        for i in range(len(p), len(row)):
            kth = np.sort(logits[i - 1])[-top_k]
            assert logits[i - 1, row[i]] >= kth - 1e-4, (r, i)


def test_generate_without_speculate_is_what_it_was():
    """the same ragged batch through the per-row path of before: the same tokens, a host mirror that stays valid, no statistics"""
    want, _ = sc.expected(2)
    out, stats, cache = sc.run(CpuTensor, 2, None)
    np.testing.assert_array_equal(out, want)
    assert stats == {} and cache.lengths is not None
    np.testing.assert_array_equal(dc.greedy(CpuTensor), dc.assert_margins_rule_out_ties())
    model = dc.make_model(CpuTensor, seed=2)
    ids = CpuTensor.from_numpy(sc.prompts(2)[0][None, :], requires_grad=False)
    for bad in (dict(speculate=0), dict(speculate=2, min_ngram=0), dict(speculate=2, max_ngram=1, min_ngram=2), dict(speculate=2, poll=0)):
        with pytest.raises(AssertionError):
            dc.bert.generate(model, ids, 4, **bad)


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------

def test_header_and_prototypes_name_the_new_entry():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"int lg_speculate_commit_i32\((.*?)\);", text, re.S)
    assert decl is not None
    assert len(decl.group(1).split(",")) == 17 == len(hiplib.PROTOTYPES["lg_speculate_commit_i32"][1])
    assert "speculate.hip" in open(os.path.join(CSRC, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_speculate_kernel_uses_no_scratch(tmp_path):
    """csrc/speculate.hip compiled for the device only: one kernel, a private segment of 0 bytes, the staged sequence and the
    waves' words in LDS (4096 + 4 words)"""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "speculate.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "speculate.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    assert len(found) == 1 and "speculate_commit" in list(found)[0], sorted(found)
    for name, row in found.items():
        print("%-52s scratch %d vgprs %d sgprs %d lds %d" % ((name,) + row))
        assert row[0] == 0 and row[3] == 4 * (4096 + 4), (name, row)


def test_the_new_entry_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entry)
        assert handle.lg_speculate_commit_i32(None, None, None, None, None, 4, 4, None, None, None, None, 1, 2, 1, 3, 1, -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_speculate_commit_i32" in handle.lg_last_error()
