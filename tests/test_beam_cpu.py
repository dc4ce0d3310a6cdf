"""Beam search without a device: `beam_step` as the numpy backend defines it against the six points written out by hand
(beam_cases.py), nn.KVCache.reorder against `take`, `generate(num_beams=w)` of examples/bert.py on CpuTensor against a float64
reference beam search, and the two new entries of the C ABI."""
import ctypes
import os
import re
import shutil
import subprocess
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import lib as hiplib
from conftest import ROOT
import decode_cases as dc
import speculate_cases as sc
import beam_cases as bc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4
GOOD = tuple(k for k in bc.KINDS if not k.startswith("bad"))
BAD = tuple(k for k in bc.KINDS if k.startswith("bad"))


# ---- beam_step: the definition ----------------------------------------------------------------------------------------------------

def assert_step(T, state, logits, w, eos, strided=False, three_d=False):
    want, flag = bc.step_by_hand(state, logits, w, eos)
    tensors, error = bc.step_on(T, state, logits, w, eos, strided_out=strided, three_d=three_d)
    assert (error is not None) == flag
    for name in bc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    np.testing.assert_array_equal(tensors["logits"].numpy().reshape(logits.shape), logits)
    if strided:                                                           # nothing beside the view was written
        wide, columns = tensors["wide"].numpy(), state["out_ids"].shape[1]
        assert (wide[:, :3] == -7).all() and (wide[:, 3 + columns:] == -7).all()
    return want


@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_beam_step_on_the_numpy_backend(w, strided):
    for V in sorted({w, 101}):
        for columns in (2, 7, 64):
            for eos_on in (False, True):
                for kinds in (GOOD, GOOD[3:] + BAD, ("mixed",), ("initial", "bad_full", "eos")):
                    state, logits, eos = bc.step_state(kinds, w, V, columns, seed=100 * w + columns + V)
                    bc.assert_margins_rule_out_ties(state, logits, w, "w %d, V %d, columns %d" % (w, V, columns))
                    assert_step(CpuTensor, state, logits, w, eos if eos_on else None, strided, three_d=eos_on)


def test_a_step_written_out_for_two_beams_of_a_vocabulary_of_two():
    """by hand alone, with numbers: log-probabilities log(1/4), log(3/4) for the live beam, a done beam between its two continuations"""
    x = np.log(np.array([[1.0, 3.0], [5.0, 5.0]], np.float32))
    state = dict(scores=np.array([-1.0, -1.5], np.float32), parent=np.zeros(2, np.int32), token=np.array([[7], [9]], np.int32),
                 out_ids=np.array([[4, 5, 900, 900], [6, 9, 900, 900]], np.int32), pos=np.array([1, 1], np.int32), done=np.array([0, 1], np.int32),
                 stats=np.zeros(2, np.int32))
    for step in (bc.step_by_hand, bc.step_by_hand_fast):
        want, flag = step(state, x, 2, eos=1)
        assert not flag
        # candidates: (-1 + log 3/4 = -1.288, beam 0, token 1), (-1.5, beam 1 itself), (-1 + log 1/4 = -2.386, beam 0, token 0)
        np.testing.assert_array_equal(want["parent"], [0, 1])
        np.testing.assert_array_equal(want["out_ids"], [[4, 5, 1, 900], [6, 9, 900, 900]])
        np.testing.assert_array_equal(want["token"], [[1], [9]])
        np.testing.assert_array_equal(want["pos"], [2, 1])
        np.testing.assert_array_equal(want["done"], [1, 1])                    # token 1 is eos: the group has finished
        np.testing.assert_array_equal(want["stats"], [1, 0])
        np.testing.assert_allclose(want["scores"], [-1.0 + np.log(0.75), -1.5], rtol=1e-6)
    assert_step(CpuTensor, state, x, 2, 1)


def test_the_states_hold_what_they_are_meant_to():
    """by hand alone: every kind of group does what its name says"""
    w, V, columns = 4, 101, 16
    state, logits, eos = bc.step_state(bc.KINDS, w, V, columns, seed=7)
    want, flag = bc.step_by_hand(state, logits, w, eos)
    fast, flag_fast = bc.step_by_hand_fast(state, logits, w, eos)
    assert flag and flag_fast
    for name in bc.NAMES:
        np.testing.assert_array_equal(want[name], fast[name], err_msg=name)
    group = lambda kind: slice(bc.KINDS.index(kind) * w, bc.KINDS.index(kind) * w + w)            # noqa: E731
    lo = lambda kind: bc.KINDS.index(kind) * w                                                    # noqa: E731
    assert (want["parent"][group("initial")] == lo("initial")).all() and np.isfinite(want["scores"][group("initial")]).all()
    g = group("done_top")
    assert want["parent"][g][0] == lo("done_top") and want["done"][g][0] == 1 and want["scores"][g][0] == np.float32(-0.25)
    assert want["pos"][g][0] == state["pos"][g][0] and (want["out_ids"][g][0] == state["out_ids"][g][0]).all()
    for kind in ("all_done", "bad_negative", "bad_full", "bad_done_negative"):
        g = group(kind)
        for name in ("scores", "token", "out_ids", "pos", "done"):
            np.testing.assert_array_equal(want[name][g], state[name][g], err_msg="%s %s" % (kind, name))
        np.testing.assert_array_equal(want["parent"][g], np.arange(lo(kind), lo(kind) + w))
    g = group("ties_inside")
    first, second = want["token"][g][0, 0], want["token"][g][1, 0]
    assert logits[lo("ties_inside"), first] == logits[lo("ties_inside"), second] and first < second and (want["parent"][g][:2] == lo("ties_inside")).all()
    assert want["scores"][g][0] == want["scores"][g][1]
    g = group("ties_across")
    assert list(want["parent"][g][:2]) == [lo("ties_across"), lo("ties_across") + 1] and want["token"][g][0, 0] == want["token"][g][1, 0]
    assert want["scores"][g][0] == want["scores"][g][1]
    g = group("eos")
    assert want["token"][g][0, 0] == eos and want["done"][g][0] == 1 and want["done"][g][1:].sum() == 0
    g = group("mixed")
    assert want["done"][g].sum() <= 1 and (want["stats"] - state["stats"])[1] > 0


@pytest.mark.parametrize("kind", BAD)
def test_each_clause_of_the_bounds_check_keeps_the_group_and_raises(kind):
    for w in (1, 2, 8):
        state, logits, eos = bc.step_state(("mixed", kind, "initial"), w, 11, 5, seed=w)
        want = assert_step(CpuTensor, state, logits, w, eos)
        for name in ("scores", "token", "out_ids", "pos", "done"):
            np.testing.assert_array_equal(want[name][w:2 * w], state[name][w:2 * w], err_msg=name)
        assert (want["pos"][2 * w:] == state["pos"][2 * w:] + 1).all()             # the groups around it were committed


def test_beam_step_refuses_other_operands():
    state, logits, _ = bc.step_state(("mixed", "initial"), 2, 11, 8, seed=0)
    i32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    f32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.float32), requires_grad=False)      # noqa: E731
    call = lambda x, tensors, w=2, **kw: x.beam_step(*(tensors[k] for k in bc.NAMES), w, **kw)       # noqa: E731
    for name, other in (("scores", f32(3)), ("scores", i32(4)), ("parent", i32(4, 1)), ("token", i32(4)), ("out_ids", i32(3, 8)), ("pos", i32(5)),
                        ("done", f32(4)), ("stats", i32(3)), ("pos", "done"), ("parent", "pos")):
        tensors = bc.upload(CpuTensor, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="beam_step"):
            call(CpuTensor.from_numpy(logits.copy(), requires_grad=False), tensors)
    tensors = bc.upload(CpuTensor, state)
    for bad_logits, w in ((f32(4, 12, 1), 2), (f32(3, 11), 2), (f32(4, 11), 3), (f32(4, 11), 0), (f32(4, 11), 9), (f32(4, 1), 2),
                          (CpuTensor.from_numpy(np.zeros((4, 11)), requires_grad=False), 2)):
        with pytest.raises(AssertionError, match="beam_step"):
            call(bad_logits, tensors, w)
    with pytest.raises(AssertionError, match="beam_step"):
        call(f32(4, 11), tensors, eos=1.5)


# ---- KVCache.reorder --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [1, 2, 4, 8])
@pytest.mark.parametrize("kind", ["identity", "swap", "cycle", "leader", "mixed"])
def test_reorder_against_take(w, kind):
    b, layers, capacity, width = 3, 2, 17, 8
    rng = np.random.RandomState(w)
    cache = nn.KVCache(layers, b * w, capacity, width, per_row=True)
    before = [rng.standard_normal((b * w, capacity, width)).astype(np.float32) for _ in range(2 * layers)]
    for t, a in zip(cache.k + cache.v, before):
        t.data[...] = a
    pos = rng.randint(0, capacity + 1, b * w)
    pos[:w] = 0                                                            # a group with nothing to move
    cache.set_lengths(pos)
    parent = bc.parents(kind, b, w, seed=w)
    cache.num_beams = w
    assert cache.reorder(CpuTensor.from_numpy(parent, requires_grad=False)) is None
    want = bc.reorder_by_take(before, parent, pos, w)
    for t, a, old in zip(cache.k + cache.v, want, before):
        np.testing.assert_array_equal(t.numpy(), a)
        for lo in range(0, b * w, w):                                      # positions at and beyond the group's longest row: untouched
            L = pos[lo:lo + w].max()
            np.testing.assert_array_equal(t.numpy()[lo:lo + w, L:], old[lo:lo + w, L:])
    np.testing.assert_array_equal(cache.pos.numpy(), pos)


def test_reorder_refuses_what_it_cannot_do():
    cache = nn.KVCache(1, 4, 5, 8, per_row=True)
    for t in cache.k + cache.v:
        t.data[...] = np.random.RandomState(0).standard_normal(t.shape)
    cache.set_lengths([3, 3, 2, 2])
    before = [t.numpy().copy() for t in cache.k + cache.v]
    parent = lambda *p: CpuTensor.from_numpy(np.array(p, np.int32), requires_grad=False)         # noqa: E731
    with pytest.raises(IndexError):
        cache.reorder(parent(1, 0, 1, 3), 2)                               # row 2 names a row of the other group
    for t, old in zip(cache.k + cache.v, before):
        np.testing.assert_array_equal(t.numpy()[2:], old[2:])              # its group is as it was,
        np.testing.assert_array_equal(t.numpy()[0, :3], old[1, :3])        # the other one was moved
    for bad in (lambda: cache.reorder(parent(0, 1, 2), 2), lambda: cache.reorder(parent(0, 1, 2, 3), 3), lambda: cache.reorder(parent(0, 1, 2, 3), 9),
                lambda: nn.KVCache(1, 4, 5, 8).reorder(parent(0, 1, 2, 3))):
        with pytest.raises(AssertionError):
            bad()


# ---- generate(num_beams=w) --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("w", [1, 2, 4])
@pytest.mark.parametrize("eos", [None, bc.EOS, bc.EOS_ALL], ids=["budget", "eos", "eos-everywhere"])
def test_beam_search_on_the_numpy_backend_finds_the_reference_hypotheses(w, eos):
    seed = bc.SEED
    _, dev = bc.assert_reference_rules_out_ties(seed, w, eos)
    ids, beams, cache = bc.run(CpuTensor, seed, w, eos=eos, poll=1)
    bc.compare_with_reference(ids, beams, seed, w, eos, dev)
    assert cache.lengths is None and cache.num_beams == w
    results, _, _ = bc.beam_reference(seed, w, eos)
    finished = all(done for hyps, _ in results for _, _, done in hyps)
    if eos == bc.EOS and w > 1:
        assert any(done for hyps, _ in results for _, _, done in hyps) and not finished, "no beam finishes among live ones - pick other inputs"
        assert any(best != 0 for _, best in results), "the length penalty never prefers another beam than the first - pick other inputs"
    if eos == bc.EOS_ALL:
        assert finished and beams["steps"] < bc.NEW - 1, "the loop does not stop early - pick other inputs"
    else:
        assert beams["steps"] == bc.NEW - 1


def test_one_beam_is_greedy_decoding_and_more_beams_score_no_worse():
    seed = bc.SEED
    bc.assert_reference_rules_out_ties(seed, 1)                            # (one beam: the gap is the top-2 margin of greedy decoding)
    one, _, _ = bc.run(CpuTensor, seed, 1)
    out, _, _ = sc.run(CpuTensor, seed, None, new=bc.NEW)                                       # the per-row path of before
    np.testing.assert_array_equal(one[:, :out.shape[1]], np.where(out == sc.PAD, bc.PAD, out))
    results1, _, _ = bc.beam_reference(seed, 1)
    for w in (2, 4):
        results, _, _ = bc.beam_reference(seed, w)
        for (hyps, best), (hyps1, _) in zip(results, results1):
            assert hyps[best][1] >= hyps1[0][1]                            # same length, same penalty: the raw scores compare


def test_the_poll_interval_a_given_cache_and_pieces_change_nothing():
    seed, w = bc.SEED, 2
    want, beams, _ = bc.run(CpuTensor, seed, w, eos=bc.EOS, poll=1)
    for options in (dict(poll=4), dict(prefill_chunk=3), dict(length_penalty=1.0)):
        ids, other, _ = bc.run(CpuTensor, seed, w, eos=bc.EOS, **options)
        np.testing.assert_array_equal(ids, want)
        # (pieces round the prompt's keys and values differently: the scores move by float32 rounding, far below any gap)
        np.testing.assert_allclose(other["scores"], beams["scores"], rtol=0, atol=1e-5 if "prefill_chunk" in options else 0)
    # length_penalty = 0 ranks by the raw score: the first beam
    ids, other, _ = bc.run(CpuTensor, seed, w, eos=bc.EOS, length_penalty=0.0)
    ps = sc.prompts(seed)
    for r, p in enumerate(ps):
        np.testing.assert_array_equal(ids[r, :len(p) + 1], other["sequences"][r, 0, :len(p) + 1])


def test_generate_refuses_what_beams_do_not_support_and_is_what_it_was_without_them():
    model = dc.make_model(CpuTensor, seed=bc.SEED)
    ids = CpuTensor.from_numpy(sc.prompts(bc.SEED)[0][None, :], requires_grad=False)
    cache = nn.KVCache(bc.CFG["num_hidden_layers"], 2, bc.CAPACITY, bc.CFG["hidden_size"], per_row=True)
    for bad in (dict(num_beams=0), dict(num_beams=9), dict(num_beams=2, temperature=1.0), dict(num_beams=2, speculate=2),
                dict(num_beams=2, append=True, cache=cache), dict(num_beams=2, poll=0), dict(num_beams=2, length_penalty=-1.0),
                dict(num_beams=4, cache=cache)):
        with pytest.raises(AssertionError):
            dc.bert.generate(model, ids, 4, **bad)
    np.testing.assert_array_equal(dc.greedy(CpuTensor), dc.assert_margins_rule_out_ties())


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------------

NEW_ENTRIES = (("lg_beam_step_f32", 15), ("lg_beam_reorder_f32", 10))


def test_header_and_prototypes_name_the_new_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, count in NEW_ENTRIES:
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == count == len(hiplib.PROTOTYPES[name][1]), name
    assert "beam.hip" in open(os.path.join(CSRC, "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_beam_kernels_use_no_scratch(tmp_path):
    """csrc/beam.hip compiled for the device only: both kernels at every group size, a private segment of 0 bytes each"""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "beam.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "beam.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    assert len(found) == 8 and sum("beam_step" in n for n in found) == 4 and sum("beam_reorder" in n for n in found) == 4, sorted(found)
    for name, row in sorted(found.items()):
        print("%-52s scratch %d vgprs %d sgprs %d lds %d" % ((name,) + row))
        assert row[0] == 0, (name, row)
        assert row[3] == 0 if "reorder" in name else row[3] <= 1024, (name, row)


def test_the_new_entries_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entries)
        assert handle.lg_beam_step_f32(None, 4, None, None, None, None, 4, 4, None, None, None, 2, 4, 2, -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_beam_step_f32" in handle.lg_last_error()
        assert handle.lg_beam_reorder_f32(None, 1, 8, 40, 5, 8, None, None, 2, 2) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_beam_reorder_f32" in handle.lg_last_error()
