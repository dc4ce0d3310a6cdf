"""Continuous batching without a device: `serve_commit` as the numpy backend defines it, nn.RequestPool, one model step that
mixes a decoding, a prefilling and an idle sequence (`model(ids, cache=, append=True, count=)`, the composite definition) and
`serve` of examples/bert.py on CpuTensor - against each request's float64 greedy continuation ALONE (serve_cases.py)."""
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
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius, float64_tape
import decode_cases as dc
import serve_cases as sc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


# ---- serve_commit: the definition ---------------------------------------------------------------------------------------------

def assert_commit(T, state, nxt, capacity, eos, strided=False, sync=None):
    want, flag = sc.commit_by_hand(state, nxt, capacity, eos)
    tensors, error = sc.commit_on(T, state, nxt, capacity, eos, strided_out=strided)
    if sync is not None:
        error = sync(flag) or error
    assert (error is not None) == flag
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    if strided:                                                           # nothing beside the view was written
        wide, G = tensors["wide"].numpy(), state["out"].shape[1]
        assert (wide[:, :2] == -7).all() and (wide[:, 2 + G:] == -7).all()
    return want


@pytest.mark.parametrize("b", [1, 5, 64, 65, 300, 1024])
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_serve_commit_on_the_numpy_backend(b, eos, strided):
    for waiting in (0, 2, 7, 400):
        for overflow in (False, True):
            state, nxt = sc.commit_state(b, waiting, seed=10 * b + waiting, eos=eos, overflow=overflow)
            assert_commit(CpuTensor, state, nxt, 12, eos, strided)


def test_the_states_hold_what_they_are_meant_to():
    """by hand alone: every kind of slot occurs, and the queue is longer than, equal to and shorter than the free slots"""
    state, nxt = sc.commit_state(300, 400, seed=1, eos=3, overflow=True)
    want, flag = sc.commit_by_hand(state, nxt, 12, 3)
    assert flag and (want["count"] == 1).any() and (want["count"] > 1).any() and want["queue"][1] > 40 and (state["req"] < 0).sum() > 30
    assert (want["req"] >= 0).all() and want["queue"][0] < 700            # a long queue: every free slot is refilled in this commit
    classes = set()
    for waiting in range(0, 8):
        state, nxt = sc.commit_state(5, waiting, seed=3, eos=3)
        want, _ = sc.commit_by_hand(state, nxt, 12, 3)
        free_before = int((state["req"] < 0).sum()) + int(want["queue"][1])       # free slots, and slots freed by this commit
        assert int(want["queue"][1]) >= 1
        classes.add(np.sign(waiting - free_before))
        assert (want["req"] < 0).sum() == max(0, free_before - waiting)
        assert want["queue"][0] == state["queue"][0] + min(waiting, free_before)
    assert classes == {-1, 0, 1}


def test_a_freed_slot_is_refilled_by_the_same_commit_in_slot_order():
    """three slots: slot 0 ends by its budget, slot 1 is free, slot 2 draws EOS; two requests wait"""
    st = dict(prompts=np.arange(1, 26, dtype=np.int32).reshape(5, 5), prompt_len=np.array([2, 1, 3, 5, 2], np.int32),
              budget=np.array([1, 4, 4, 4, 4], np.int32), out=np.full((5, 4), 9, np.int32), out_len=np.array([0, 0, 1, 0, 0], np.int32),
              queue=np.array([3, 0], np.int32), req=np.array([0, -1, 2], np.int32), pos=np.array([0, 5, 3], np.int32),
              count=np.array([2, 0, 1], np.int32), ids=np.zeros((3, 2), np.int32), position_ids=np.zeros((3, 2), np.int32),
              last=np.zeros(3, np.int32))
    tensors, error = sc.commit_on(CpuTensor, st, np.array([40, 41, 18], np.int32), 8, 18)
    got = {k: tensors[k].numpy() for k in sc.NAMES}
    assert error is None
    assert got["req"].tolist() == [3, 4, -1] and got["queue"].tolist() == [5, 2]
    assert got["out"][0].tolist() == [40, 9, 9, 9] and got["out"][2].tolist() == [9, 18, 9, 9] and got["out_len"].tolist() == [1, 0, 2, 0, 0]
    assert got["ids"].tolist() == [[16, 17], [21, 22], [0, 0]] and got["position_ids"].tolist() == [[0, 1], [0, 1], [0, 0]]
    assert got["pos"].tolist() == [0, 0, 0] and got["count"].tolist() == [2, 2, 0] and got["last"].tolist() == [1, 3, 4]


def test_serve_commit_refuses_other_operands():
    state, nxt = sc.commit_state(3, 2, seed=0)
    i32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("req", i32(4)), ("ids", i32(3, 5)), ("queue", i32(3)), ("out_len", i32(4)), ("last", i32(3, 1)), ("prompts", i32(5)),
                        ("pos", CpuTensor.from_numpy(np.zeros(3, np.int64), requires_grad=False)), ("count", "pos")):
        tensors = sc.upload(CpuTensor, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="serve_commit"):
            CpuTensor.from_numpy(nxt.copy(), requires_grad=False).serve_commit(*(tensors[k] for k in sc.NAMES), 12)
    tensors = sc.upload(CpuTensor, state)
    with pytest.raises(AssertionError, match="serve_commit"):
        i32(4, 1).serve_commit(*(tensors[k] for k in sc.NAMES), 12)


# ---- nn.RequestPool -----------------------------------------------------------------------------------------------------------

def test_request_pool_holds_the_state_and_checks_the_capacity():
    cache = nn.KVCache(2, 3, 17, 64, per_row=True)
    rows = sc.prompts()
    pool = nn.RequestPool(cache, np.stack([np.pad(p, (0, 9 - len(p))) for p in rows]), [len(p) for p in rows], [6] * 7, 4, pad_token_id=sc.PAD)
    assert tuple(pool.ids.shape) == tuple(pool.position_ids.shape) == (3, 4) and tuple(pool.out.shape) == (7, 6) and (pool.out.numpy() == sc.PAD).all()
    assert pool.req.numpy().tolist() == [-1] * 3 and pool.queue.numpy().tolist() == [0, 0] and pool.pos is cache.pos and cache.lengths is None
    assert pool.max_steps == sum(-(-len(p) // 4) + 6 for p in rows)
    pool.admit()
    assert pool.req.numpy().tolist() == [0, 1, 2] and pool.count.numpy().tolist() == [4, 2, 4] and pool.queue.numpy().tolist() == [3, 0]
    assert pool.last.numpy().tolist() == [3, 5, 11] and pool.ids.numpy()[1].tolist() == rows[1].tolist() + [0, 0] and pool.finished() == 0
    with pytest.raises(AssertionError, match="per_row"):
        nn.RequestPool(nn.KVCache(2, 3, 17, 64), np.zeros((1, 3), np.int32), [3], [2], 4)
    with pytest.raises(AssertionError, match="does not fit"):
        nn.RequestPool(cache, np.zeros((1, 12), np.int32), [12], [7], 4)              # 12 + 7 - 1 = 18 > 17
    nn.RequestPool(cache, np.zeros((1, 12), np.int32), [12], [6], 4)                  # 17 fits: the last token is fed to nobody
    with pytest.raises(AssertionError, match="position embeddings"):
        nn.RequestPool(cache, np.zeros((1, 3), np.int32), [3], [2], 4, max_positions=16)


# ---- one mixed model step -----------------------------------------------------------------------------------------------------

def test_one_mixed_step_matches_each_sequence_alone():
    ref64, cpu32 = sc.mixed_reference()
    got, cache = sc.mixed_step(CpuTensor)
    assert [g.shape for g in got] == [r.shape for r in ref64]
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="mixed step on CpuTensor")


def test_one_mixed_step_in_float64_is_each_sequence_alone():
    ref64, _ = sc.mixed_reference()
    with float64_tape():
        got, _ = sc.mixed_step(CpuTensor, model=dc.make_model(CpuTensor, np.float64, sc.SEED), dtype=np.float64)
    for r, (_, n) in enumerate(sc.MIXED):
        if n:
            assert got[r].dtype == np.float64 and rel_frobenius(got[r], ref64[r]) < 1e-13, r


def test_a_count_of_m_everywhere_is_the_call_without_count_and_misuse_is_refused():
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    ids = CpuTensor.from_numpy(np.array([[3, 4, 5], [6, 7, 8]], np.int32), requires_grad=False)
    outs = []
    for count in (None, CpuTensor.from_numpy(np.array([3, 3], np.int32), requires_grad=False)):
        cache = nn.KVCache(2, 2, 17, 64, like=model.cls.predictions.bias, per_row=True)
        cache.set_lengths([2, 5])
        outs.append(model(ids, cache=cache, append=True, **({} if count is None else {"count": count})).numpy().copy())
    np.testing.assert_array_equal(outs[0], outs[1])
    with pytest.raises(AssertionError, match="per_row"):
        model(ids, cache=nn.KVCache(2, 2, 17, 64, like=model.cls.predictions.bias), append=True, count=count)
    with pytest.raises(AssertionError, match="append"):
        model(ids, cache=cache, count=count)
    with pytest.raises(AssertionError, match="no room"):
        cache.set_lengths([2, 15])
        model(ids, cache=cache, append=True, count=count)


# ---- serve --------------------------------------------------------------------------------------------------------------------

def test_the_references_take_both_stops():
    tokens = sc.assert_margins_rule_out_ties()
    want, out_len = sc.expected(tokens, sc.BUDGET, sc.EOS)
    assert tuple(out_len) == sc.EMITTED


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_gives_each_request_its_own_continuation(slots, chunk):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, poll=1)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)


def test_serve_with_a_budget_per_request_and_in_float64():
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGETS, None)
    assert tuple(want_len) == sc.BUDGETS
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, budgets=sc.BUDGETS, eos=None, poll=1)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out_len, want_len)
    assert stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], sc.BUDGETS, 3, 4)
    with float64_tape():
        out, out_len, _ = sc.run_serve(CpuTensor, 3, 4, model=dc.make_model(CpuTensor, np.float64, sc.SEED), budgets=sc.BUDGETS, eos=None)
    np.testing.assert_array_equal(out, want)


def test_the_poll_interval_changes_the_steps_run_not_the_tokens():
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    exact = sc.simulate([len(p) for p in sc.prompts()], want_len, 3, 4)
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, poll=8)
    np.testing.assert_array_equal(out, want)
    assert stats["steps"] == -(-exact // 8) * 8                          # idle steps behind the last finish change nothing


def test_sampled_serving_repeats_for_a_seed():
    runs = []
    for _ in range(2):
        light.manual_seed(5)
        runs.append(sc.run_serve(CpuTensor, 3, 4, eos=86, temperature=0.9, top_k=20, top_p=0.95, poll=1))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2]["steps"] == runs[1][2]["steps"] and (runs[0][1] >= 1).all()


def test_a_single_request_gives_generates_tokens():
    prompt = sc.prompts()[2]
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    today = dc.bert.generate(model, CpuTensor.from_numpy(prompt[None, :], requires_grad=False), sc.BUDGET).numpy()[0, len(prompt):]
    (out, out_len), stats = dc.bert.serve(model, [prompt], sc.BUDGET, slots=1, chunk=16)
    np.testing.assert_array_equal(out.numpy()[0], today)
    assert out_len.numpy().tolist() == [sc.BUDGET]
    # right-padded ids with lengths= mean the same
    (out2, _), _ = dc.bert.serve(model, np.pad(prompt, (0, 3))[None, :], sc.BUDGET, slots=1, chunk=16, lengths=[len(prompt)])
    np.testing.assert_array_equal(out2.numpy(), out.numpy())


# ---- the C ABI without a device -----------------------------------------------------------------------------------------------

NEW_ENTRIES = (("lg_attention_extend_counts_f32", 27), ("lg_serve_commit_i32", 23))


def test_header_and_prototypes_name_the_new_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRIES:
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name
    # the `_counts` entry takes the `_rows` entry's arguments and one pointer behind `pos`
    rows, counts = hiplib.PROTOTYPES["lg_attention_extend_rows_f32"][1], hiplib.PROTOTYPES["lg_attention_extend_counts_f32"][1]
    assert counts[:14] == rows[:14] and counts[14] is ctypes.c_void_p and counts[15:] == rows[14:]
    assert "serve.hip" in open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_serve_kernel_uses_no_scratch(tmp_path):
    """csrc/serve.hip compiled for the device only: one kernel, a private segment of 0 bytes, the four slot arrays and the wave
    totals in LDS (4 x 1024 + 2 x 16 words)"""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "serve.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "serve.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    assert len(found) == 1 and "serve_commit" in list(found)[0], sorted(found)
    for name, row in found.items():
        print("%-52s scratch %d vgprs %d sgprs %d lds %d" % ((name,) + row))
        assert row[0] == 0 and row[3] == 4 * (4 * 1024 + 2 * 16), (name, row)


def test_new_entries_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entries)
        assert handle.lg_attention_extend_counts_f32(None, 0, 0, None, 0, 0, None, 0, 0, None, None, 64, 0, None, None, None, 0, 0, None, 1, 1, 1, 8, 64,
                                                     1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_attention_extend_counts_f32" in handle.lg_last_error()
        assert handle.lg_serve_commit_i32(None, 1, None, 4, 4, None, None, None, 4, 4, None, None, 1, None, None, None, None, None, None, 1, 1, 8,
                                          -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_serve_commit_i32" in handle.lg_last_error()
