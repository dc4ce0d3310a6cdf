"""Token-packed serving steps without a device: `serve_commit_packed` as the numpy backend defines it against the words written
out by hand (serve_packed_cases.py), nn.RequestPool(token_budget=), the composite definition of a packed model step
(`model(ids, cache=, append=True, cu=, token_positions=)`) and `serve(token_budget=)` of examples/bert.py on CpuTensor - against
each request's float64 greedy continuation ALONE (serve_cases.py)."""
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
import serve_packed_cases as pc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


# ---- serve_commit_packed: the definition ----------------------------------------------------------------------------------------

def assert_commit(T, state, nxt, capacity, chunk, eos, strided=False):
    want, flag = pc.commit_packed_by_hand(state, nxt, capacity, chunk, eos)
    tensors, error = pc.commit_on(T, state, nxt, capacity, chunk, eos, strided_out=strided)
    assert (error is not None) == flag
    for name in pc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    if strided:                                                           # nothing beside the view was written
        wide, G = tensors["wide"].numpy(), state["out"].shape[1]
        assert (wide[:, :2] == -7).all() and (wide[:, 2 + G:] == -7).all()
    return want


@pytest.mark.parametrize("b", pc.SLOTS)
@pytest.mark.parametrize("eos", [None, 3])
@pytest.mark.parametrize("strided", [False, True], ids=["dense", "strided-out"])
def test_serve_commit_packed_on_the_numpy_backend(b, eos, strided):
    chunk = 4
    for T in pc.budgets_of(b, chunk):
        for waiting in (0, 2, b + 100):
            for overflow in (False, True):
                state, nxt = pc.packed_state(b, waiting, seed=10 * b + waiting, T=T, chunk=chunk, eos=eos, overflow=overflow)
                assert_commit(CpuTensor, state, nxt, 12, chunk, eos, strided)


def test_the_packed_states_hold_what_they_are_meant_to():
    """by hand alone: with T = slots the budget binds (a prefilling slot is granted less than it wants, some nothing), with
    T = slots * chunk it never does and the grants are serve_commit's counts; cu is the running sum of the counts"""
    b, chunk = 200, 4
    state, nxt = pc.packed_state(b, 300, seed=1, T=b, chunk=chunk, eos=3, overflow=True)
    tight, flag = pc.commit_packed_by_hand(state, nxt, 12, chunk, 3)
    loose_state, _ = pc.packed_state(b, 300, seed=1, T=b * chunk, chunk=chunk, eos=3, overflow=True)
    loose, _ = pc.commit_packed_by_hand(loose_state, nxt, 12, chunk, 3)
    rows_state, _ = sc.commit_state(b, 300, 1, m=chunk, capacity=12, eos=3, overflow=True)
    rows, rows_flag = sc.commit_by_hand(rows_state, nxt, 12, 3)
    assert flag and rows_flag
    np.testing.assert_array_equal(loose["count"], rows["count"])
    np.testing.assert_array_equal(loose["req"], rows["req"])
    np.testing.assert_array_equal(loose["out"], rows["out"])
    for r, (c, k) in enumerate(zip(loose["count"], rows["ids"])):
        np.testing.assert_array_equal(loose["ids"][0, loose["cu"][r]:loose["cu"][r] + c], k[:c])
    assert (tight["count"] < loose["count"]).any() and ((tight["count"] == 0) & (loose["count"] > 1) & (tight["req"] >= 0)).any()
    assert tight["cu"][-1] == min(b, loose["cu"][-1]) == b                # a full buffer: the rows granted are min(T, the rows wanted)
    for st in (tight, loose):
        np.testing.assert_array_equal(st["cu"], np.concatenate([[0], np.cumsum(st["count"])]))
        assert (st["ids"][0, st["cu"][-1]:] == 0).all() and (st["position_ids"][0, st["cu"][-1]:] == 0).all()


def test_the_budget_runs_out_inside_a_want_and_an_idle_slot_behind_a_full_buffer_is_clamped():
    state, nxt, T, chunk, capacity = pc.tight_state()
    want = assert_commit(CpuTensor, state, nxt, capacity, chunk, None)
    assert want["count"].tolist() == [1, 4, 1, 0] and want["cu"].tolist() == [0, 1, 5, 6, 6] and want["last"].tolist() == [0, 4, 5, 5]
    assert want["ids"][0].tolist() == [50, 17, 18, 19, 20, 29] and want["position_ids"][0].tolist() == [3, 4, 5, 6, 7, 4]
    assert want["pos"].tolist() == [3, 4, 4, 0] and want["req"].tolist() == [0, 1, 2, -1] and want["out"][0].tolist() == [sc.PAD, 50, sc.PAD, sc.PAD]
    # the slot that was granted 1 of 4 goes on behind it, the one granted nothing asks again: a second commit on the result
    second = {k: v.copy() for k, v in want.items()}
    second["pos"][1], second["count"][1] = 8, 4                            # slot 1 ends its prompt: it decodes from now on
    after = assert_commit(CpuTensor, second, nxt, capacity, chunk, None)
    assert after["pos"][2] == 5 and after["count"][2] == 4 and after["ids"][0, after["cu"][2]:after["cu"][3]].tolist() == [30, 31, 32, 33]


def test_serve_commit_packed_refuses_other_operands():
    state, nxt = pc.packed_state(3, 2, seed=0, T=5)
    i32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.int32), requires_grad=False)        # noqa: E731
    for name, other in (("req", i32(4)), ("ids", i32(3, 5)), ("ids", i32(1, 2)), ("cu", i32(3)), ("position_ids", i32(1, 6)), ("queue", i32(3)),
                        ("last", i32(3, 1)), ("cu", CpuTensor.from_numpy(np.zeros(4, np.int64), requires_grad=False)), ("count", "pos"), ("cu", "last")):
        tensors = pc.upload(CpuTensor, state)
        tensors[name] = tensors[other] if isinstance(other, str) else other
        with pytest.raises(AssertionError, match="serve_commit_packed"):
            CpuTensor.from_numpy(nxt.copy(), requires_grad=False).serve_commit_packed(*(tensors[k] for k in pc.NAMES), 12, 4)
    tensors = pc.upload(CpuTensor, state)
    with pytest.raises(AssertionError, match="chunk"):
        CpuTensor.from_numpy(nxt.copy(), requires_grad=False).serve_commit_packed(*(tensors[k] for k in pc.NAMES), 12, 0)


# ---- nn.RequestPool(token_budget=) ----------------------------------------------------------------------------------------------

def test_request_pool_with_a_token_budget_holds_the_packed_state():
    cache = nn.KVCache(2, 3, 17, 64, per_row=True)
    rows = sc.prompts()
    padded, lengths = np.stack([np.pad(p, (0, 9 - len(p))) for p in rows]), [len(p) for p in rows]
    pool = nn.RequestPool(cache, padded, lengths, [6] * 7, 4, pad_token_id=sc.PAD, token_budget=7)
    assert tuple(pool.ids.shape) == tuple(pool.position_ids.shape) == (1, 7) and tuple(pool.cu.shape) == (4,) and pool.token_budget == 7
    assert tuple(pool.count.shape) == (3,) and pool.max_steps == sum(len(p) + 6 for p in rows)
    pool.admit()
    # prompts of 5, 2 and 7 tokens in pieces of 4 under 7 rows: 4, 2, and 1 of the third slot's 4
    assert pool.req.numpy().tolist() == [0, 1, 2] and pool.count.numpy().tolist() == [4, 2, 1] and pool.cu.numpy().tolist() == [0, 4, 6, 7]
    assert pool.last.numpy().tolist() == [3, 5, 6] and pool.ids.numpy()[0].tolist() == rows[0][:4].tolist() + rows[1].tolist() + rows[2][:1].tolist()
    assert pool.position_ids.numpy()[0].tolist() == [0, 1, 2, 3, 0, 1, 0] and pool.finished() == 0
    plain = nn.RequestPool(cache, padded, lengths, [6] * 7, 4, pad_token_id=sc.PAD)
    assert plain.cu is None and plain.token_budget is None and tuple(plain.ids.shape) == (3, 4)
    with pytest.raises(AssertionError, match="token_budget"):
        nn.RequestPool(cache, padded, lengths, [6] * 7, 4, token_budget=2)


# ---- one packed model step ------------------------------------------------------------------------------------------------------

def packed_step(T, model=None, dtype=np.float32, rows=12):
    """the logits of ONE `model(ids, cache=, append=True, cu=, token_positions=)` call on tensor class T per slot of
    serve_cases.MIXED, the step's 10 tokens packed into `rows` token rows; the tokens in front of the step enter the cache through
    packed calls too, one slot at a time"""
    seqs, b = sc.mixed_sequences(), len(sc.MIXED)
    model = dc.make_model(T, dtype, sc.SEED) if model is None else model
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], b, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    tensor = lambda a: T.from_numpy(np.ascontiguousarray(a, np.int32), requires_grad=False)          # noqa: E731
    for r, (t, n) in enumerate(sc.MIXED):
        if t:
            cu = np.array([0] * (r + 1) + [t] * (b - r), np.int32)
            model(tensor(seqs[r][None, :t]), cache=cache, append=True, cu=tensor(cu), token_positions=tensor(np.arange(t)[None, :]))
            count = np.zeros(b, np.int32)
            count[r] = t
            cache.advance(tensor(count))
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])
    ids, positions, cu = np.full((1, rows), 7, np.int32), np.zeros((1, rows), np.int32), pc.cu_of(sc.MIXED)
    for r, (t, n) in enumerate(sc.MIXED):
        ids[0, cu[r]:cu[r + 1]], positions[0, cu[r]:cu[r + 1]] = seqs[r][t:], t + np.arange(n)
    logits = model(tensor(ids), cache=cache, append=True, cu=tensor(cu), token_positions=tensor(positions))
    assert tuple(logits.shape) == (1, rows, sc.CFG["vocab_size"]) and logits.ctx is None          # outside the tape
    logits = logits.numpy()
    return [logits[0, cu[r]:cu[r + 1]].copy() for r in range(b)], cache


def test_one_packed_step_matches_each_sequence_alone():
    ref64, cpu32 = sc.mixed_reference()
    got, cache = packed_step(CpuTensor)
    assert [g.shape for g in got] == [r.shape for r in ref64]
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="packed step on CpuTensor")
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])          # the caller moves the positions, not the forward


def test_one_packed_step_in_float64_is_each_sequence_alone():
    ref64, _ = sc.mixed_reference()
    with float64_tape():
        got, _ = packed_step(CpuTensor, model=dc.make_model(CpuTensor, np.float64, sc.SEED), dtype=np.float64)
    for r, (_, n) in enumerate(sc.MIXED):
        if n:
            assert got[r].dtype == np.float64 and rel_frobenius(got[r], ref64[r]) < 1e-13, r


def test_the_packed_context_of_unowned_rows_is_zero_and_misuse_is_refused():
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    layer = model.bert.encoder.layer[0].attention.self
    cache = nn.KVCache(2, 2, 17, 64, like=model.cls.predictions.bias, per_row=True)
    cache.set_lengths([2, 5])
    i32 = lambda a: CpuTensor.from_numpy(np.asarray(a, np.int32), requires_grad=False)             # noqa: E731
    hidden = CpuTensor.from_numpy(np.random.RandomState(0).randn(1, 6, 64).astype(np.float32), requires_grad=False)
    with light.no_grad():
        context, _ = layer(hidden, cache=cache, index=0, append=True, cu=i32([0, 3, 4]))
    context = context.numpy()
    assert (context[0, 4:] == 0).all() and np.abs(context[0, :4]).min() > 0
    ids, positions = i32([[3, 4, 5, 6, 7, 8]]), i32([[2, 3, 4, 5, 0, 0]])
    with pytest.raises(AssertionError, match="exclude"):
        model(ids, cache=cache, append=True, cu=i32([0, 3, 4]), count=i32([3, 1]), token_positions=positions)
    with pytest.raises(AssertionError, match="append"):
        model(ids, cache=cache, cu=i32([0, 3, 4]))
    with pytest.raises(AssertionError, match="slots"):
        model(ids, cache=cache, append=True, cu=i32([0, 3, 4, 4]), token_positions=positions)
    with pytest.raises(AssertionError, match="token_positions"):
        model(ids, cache=cache, append=True, cu=i32([0, 3, 4]))
    with pytest.raises(AssertionError, match="no room"):
        cache.set_lengths([2, 15])
        model(ids, cache=cache, append=True, cu=i32([0, 3, 6]), token_positions=positions)


# ---- serve(token_budget=) -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("run", range(len(pc.RUNS)), ids=["chunk%d-T%s" % (c, n) for c, n in zip((1, 4, 16, 16), ("slots", "slots+3", "slots+16", "slotsx16"))])
def test_packed_serve_gives_each_request_its_own_continuation(slots, run):
    chunk, budget = pc.RUNS[run][0], pc.RUNS[run][1](slots)
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, poll=1, token_budget=budget)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    lengths = [len(p) for p in sc.prompts()]
    assert stats["token_budget"] == budget and stats["steps"] == pc.simulate_packed(lengths, want_len, slots, chunk, budget)
    if budget == slots * chunk:                                           # the budget never binds: the schedule of the (slots, chunk) step
        assert stats["steps"] == sc.simulate(lengths, want_len, slots, chunk)


def test_the_budget_changes_the_schedule_not_the_tokens():
    """by hand alone: with 7 slots and T = 7 the packed schedule takes more steps than the unpacked one at chunk 4"""
    lengths = [len(p) for p in sc.prompts()]
    assert pc.simulate_packed(lengths, sc.EMITTED, 7, 4, 7) > sc.simulate(lengths, sc.EMITTED, 7, 4) == pc.simulate_packed(lengths, sc.EMITTED, 7, 4, 28)


def test_packed_serve_with_a_budget_per_request_and_in_float64():
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGETS, None)
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, budgets=sc.BUDGETS, eos=None, poll=1, token_budget=6)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out_len, want_len)
    assert stats["steps"] == pc.simulate_packed([len(p) for p in sc.prompts()], sc.BUDGETS, 3, 4, 6)
    with float64_tape():
        out, out_len, _ = sc.run_serve(CpuTensor, 3, 4, model=dc.make_model(CpuTensor, np.float64, sc.SEED), budgets=sc.BUDGETS, eos=None, token_budget=6)
    np.testing.assert_array_equal(out, want)
    with pytest.raises(AssertionError, match="token_budget"):
        sc.run_serve(CpuTensor, 3, 4, token_budget=2)


def test_sampled_packed_serving_repeats_for_a_seed():
    runs = []
    for _ in range(2):
        light.manual_seed(5)
        runs.append(sc.run_serve(CpuTensor, 3, 4, eos=86, temperature=0.9, top_k=20, top_p=0.95, poll=1, token_budget=6))
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    assert runs[0][2]["steps"] == runs[1][2]["steps"] and (runs[0][1] >= 1).all()


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------

NEW_ENTRIES = (("lg_attention_extend_packed_f32", 24), ("lg_serve_commit_packed_i32", 25))


def test_header_and_prototypes_name_the_packed_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRIES:
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name
    # the packed commit takes the commit's arguments with `cu` behind `count` and {T, chunk} in place of m
    rows, packed = hiplib.PROTOTYPES["lg_serve_commit_i32"][1], hiplib.PROTOTYPES["lg_serve_commit_packed_i32"][1]
    assert packed[:16] == rows[:16] and packed[16] is ctypes.c_void_p and packed[17:20] == rows[16:19] and len(packed) == len(rows) + 2
    assert "serve_packed.hip" in open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_packed_commit_kernel_uses_no_scratch(tmp_path):
    """csrc/serve_packed.hip compiled for the device only: one kernel, a private segment of 0 bytes, cu and the three slot arrays
    and five rows of wave totals in LDS"""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "serve_packed.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "serve_packed.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    assert len(found) == 1 and "serve_commit_packed" in list(found)[0], sorted(found)
    for name, row in found.items():
        print("%-52s scratch %d vgprs %d sgprs %d lds %d" % ((name,) + row))
        words = 1025 + 3 * 1024 + 5 * 16
        assert row[0] == 0 and 4 * words <= row[3] < 4 * words + 64, (name, row)        # (the arrays are padded to their alignment)


def test_packed_entries_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entries)
        assert handle.lg_attention_extend_packed_f32(None, 64, None, 64, None, 64, None, None, 64, 0, None, None, None, 64, None, 1, 1, 4, 1, 8, 64,
                                                     1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_attention_extend_packed_f32" in handle.lg_last_error()
        assert handle.lg_serve_commit_packed_i32(None, 1, None, 4, 4, None, None, None, 4, 4, None, None, 1, None, None, None, None, None, None, None,
                                                 1, 2, 1, 8, -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_serve_commit_packed_i32" in handle.lg_last_error()
