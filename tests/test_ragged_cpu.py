"""Ragged batches in the KV cache without a device: nn.KVCache(per_row=True), `decode_commit` as the numpy backend defines it,
the per-row composite of examples/bert.py on CpuTensor (float32 and a float64 tape), `generate(lengths=, eos_token_id=)`, the
host half of the three new entries of the C ABI and the resources of the commit kernel.

The yardsticks are float64 runs of every sequence ALONE (tests/ragged_cases.py): a sequence of a ragged batch must decode as
it does at batch 1.  Greedy tokens of this model depend little on the input, so the teacher-forced logits carry the weight: a
wrong position shows there.  hipcc cross-compiles without a GPU."""
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
from common import assert_as_close_to_float64_as_the_cpu_backend, float64_tape, rel_frobenius
import decode_cases as dc
import ragged_cases as rc

HIPCC = "/opt/rocm/bin/hipcc"
CSRC = os.path.join(ROOT, "lightgrad_amd", "csrc")
LG_ENOTINIT = -4


# ---- the cache ----------------------------------------------------------------------------------------------------------------

def test_kv_cache_with_a_position_per_row():
    like = CpuTensor.from_numpy(np.zeros(3, np.float32))
    cache = nn.KVCache(2, 3, 9, 8, like=like, per_row=True)
    assert cache.per_row and isinstance(cache.pos, CpuTensor) and cache.pos.dtype == np.int32 and tuple(cache.pos.shape) == (3,)
    assert not cache.pos.requires_grad and cache.length == 0 and cache.lengths.tolist() == [0, 0, 0]
    storage = cache.pos.numpy()
    cache.set_lengths([4, 0, 6])
    assert cache.pos.numpy().tolist() == [4, 0, 6] and cache.lengths.tolist() == [4, 0, 6] and cache.length == 6
    cache.advance()
    assert cache.pos.numpy().tolist() == [5, 1, 7] and cache.lengths.tolist() == [5, 1, 7] and cache.length == 7
    cache.advance(np.array([0, 2, 1]))
    assert cache.pos.numpy().tolist() == [5, 3, 8] and cache.lengths.tolist() == [5, 3, 8]
    cache.advance(CpuTensor.from_numpy(np.array([1, 0, 0], np.int32), requires_grad=False))
    assert cache.pos.numpy().tolist() == [6, 3, 8] and cache.lengths.tolist() == [6, 3, 8]
    assert cache.pos.numpy() is storage                                   # in place: a captured step sees it
    ids = cache.positions(3)
    assert tuple(ids.shape) == (3, 3) and ids.dtype == np.int32 and not ids.requires_grad
    np.testing.assert_array_equal(ids.numpy(), [[6, 7, 8], [3, 4, 5], [8, 9, 10]])
    cache.committed(2)
    assert cache.lengths.tolist() == [8, 5, 10] and cache.length == 10       # (the host follows what a commit did on the device)
    cache.committed(1, eos=True)
    assert cache.lengths is None and cache.length == 11                       # only the device knows which rows moved
    cache.reset()
    assert cache.pos.numpy().tolist() == [0, 0, 0] and cache.lengths.tolist() == [0, 0, 0] and cache.length == 0
    for bad in ([1, 2], [1, 2, 10], [-1, 0, 0]):
        with pytest.raises(AssertionError):
            cache.set_lengths(bad)
    # without per_row nothing changed
    plain = nn.KVCache(2, 3, 9, 8, like=like)
    assert not plain.per_row and tuple(plain.pos.shape) == (1,) and plain.lengths is None and tuple(plain.positions(2).shape) == (2,)
    with pytest.raises(AssertionError):
        plain.set_lengths([1, 2, 3])


# ---- decode_commit: the definition ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("b", [1, 5, 300])
@pytest.mark.parametrize("eos", [None, 3, -1])
def test_decode_commit_on_the_numpy_backend(b, eos):
    rng = np.random.RandomState(b)
    columns = 9
    nxt = rng.randint(0, 6, (b, 1)).astype(np.int32)
    token = rng.randint(0, 6, (b, 1)).astype(np.int32)
    out_ids = rng.randint(0, 6, (b, columns)).astype(np.int32)
    pos = rng.randint(-1, columns - 1, b).astype(np.int32)                # every p = pos + 1 is a column
    done = (rng.uniform(size=b) < 0.3).astype(np.int32)
    nxt[0], done[0] = 3, 0                                                # a live row that draws id 3 ...
    if b > 1:
        nxt[1], done[1] = 3, 1                                            # ... and a finished one that would
    want = rc.commit_by_hand(nxt, token, out_ids, pos, done, eos)
    assert not want[4] and want[3][0] == (1 if eos == 3 else 0) and want[2][0] == pos[0] + 1
    t = [CpuTensor.from_numpy(a.copy(), requires_grad=False) for a in (nxt, token, out_ids, pos, done)]
    assert t[0].decode_commit(*t[1:], eos=eos) is None
    for got, w in zip(t[1:], want):
        np.testing.assert_array_equal(got.numpy(), w)
    if b > 1:
        assert want[2][1] == pos[1] and want[1][1, pos[1] + 1] == out_ids[1, pos[1] + 1]          # the finished row kept its bytes
    # nxt of shape (b,) means the same; a row at the last column is left untouched, the others are committed, and the call raises
    pos2 = pos.copy()
    pos2[0], done2 = columns - 1, done.copy()
    done2[0] = 0
    want = rc.commit_by_hand(nxt, token, out_ids, pos2, done2, eos)
    assert want[4]
    t = [CpuTensor.from_numpy(a.copy(), requires_grad=False) for a in (nxt.reshape(b), token, out_ids, pos2, done2)]
    with pytest.raises(IndexError):
        t[0].decode_commit(*t[1:], eos=eos)
    for got, w in zip(t[1:], want):
        np.testing.assert_array_equal(got.numpy(), w)


def test_decode_commit_refuses_other_operands():
    i32 = lambda *shape: CpuTensor.from_numpy(np.zeros(shape, np.int32), requires_grad=False)      # noqa: E731
    good = dict(nxt=i32(3, 1), token=i32(3, 1), out_ids=i32(3, 4), pos=i32(3), done=i32(3))
    for name, other in (("nxt", i32(4, 1)), ("token", i32(3)), ("out_ids", i32(4, 4)), ("pos", i32(3, 1)), ("done", i32(2)),
                        ("pos", CpuTensor.from_numpy(np.zeros(3, np.int64), requires_grad=False))):
        args = dict(good, **{name: other})
        with pytest.raises(AssertionError, match="decode_commit"):
            args["nxt"].decode_commit(args["token"], args["out_ids"], args["pos"], args["done"])


# ---- the model ----------------------------------------------------------------------------------------------------------------

def test_teacher_forced_logits_of_a_ragged_batch_match_each_sequence_alone():
    """prompts of 5, 2 and 7 tokens into one per-row cache, 6 given tokens per row one step at a time, then second pieces of 3, 1
    and 2 tokens in one append: every logit row against the float64 full forward of that sequence alone"""
    ref64, cpu32 = rc.teacher_reference()
    got = rc.teacher_forced(CpuTensor)
    assert [g.shape for g in got] == [r.shape for r in ref64]
    assert_as_close_to_float64_as_the_cpu_backend(rc.named(got), rc.named(cpu32), rc.named(ref64), floor=1e-5, what="per-row cache on CpuTensor")


def test_teacher_forced_in_float64_is_each_sequence_alone():
    ref64, _ = rc.teacher_reference()
    with float64_tape():
        got = rc.teacher_forced(CpuTensor, model=dc.make_model(CpuTensor, np.float64, rc.SEED), dtype=np.float64)
    for r in range(rc.B):
        assert got[r].dtype == np.float64 and rel_frobenius(got[r], ref64[r]) < 1e-13, r


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["float32", "float64"])
def test_generate_stops_a_row_at_its_eos_and_equals_the_float64_tokens(dtype):
    """the issue's example: sequence 0 draws token 18 as its 6th, the others never.  First, on the references alone: no step of
    any sequence is a near-tie (margin >= 100 x the float32 deviation)"""
    tokens = rc.assert_margins_rule_out_ties()
    assert [t.tolist() for t in tokens] == [[86, 86, 86, 86, 86, 18, 86, 86], [86] * 8, [86] * 8]
    want, stop = rc.expected_ids(tokens)
    assert stop.tolist() == [10, 9, 14]                                    # row 0 frozen at its EOS column, the others at their last token's
    if dtype == np.float64:
        with float64_tape():
            got, cache = rc.generate(CpuTensor, model=dc.make_model(CpuTensor, np.float64, rc.SEED), dtype=np.float64)
    else:
        got, cache = rc.generate(CpuTensor)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(cache.pos.numpy(), stop)
    assert cache.lengths is None                                           # where the rows stopped is the device's knowledge


def test_a_finished_row_is_left_alone():
    """row 0 draws its EOS as its 6th new token; the step after that feeds it (position 10, the row's last cache row).  Row 0's
    cache rows and its row of the ids after 7 new tokens are, bit for bit, those after 8: the step after it finished recomputes it
    at its frozen position and writes the same bits"""
    short, cache_short = rc.generate(CpuTensor, new=7)
    full, cache_full = rc.generate(CpuTensor, new=8)
    np.testing.assert_array_equal(full[0, :rc.S0 + 7], short[0])
    assert (full[0, rc.S0 + 7:] == rc.PAD).all() and (full[0, 11:] == rc.PAD).all() and full[0, 10] == rc.EOS
    assert cache_short.pos.numpy()[0] == cache_full.pos.numpy()[0] == 10
    for layer in range(dc.CFG["num_hidden_layers"]):
        for a, b in ((cache_short.k[layer], cache_full.k[layer]), (cache_short.v[layer], cache_full.v[layer])):
            np.testing.assert_array_equal(a.numpy()[0].view(np.uint32), b.numpy()[0].view(np.uint32))


def test_uniform_lengths_through_the_per_row_path_give_todays_tokens():
    """decode_cases' own prompts (equal lengths): `generate(lengths=)` and `generate(eos_token_id=)` with an id that never comes
    against `generate` as it was"""
    _, ids = dc.parameters()
    model = dc.make_model(CpuTensor)
    prompt = CpuTensor.from_numpy(ids[:, :dc.S0], requires_grad=False)
    today = dc.bert.generate(model, prompt, 6).numpy()
    np.testing.assert_array_equal(today[:, dc.S0:], dc.assert_margins_rule_out_ties()[:, :6])
    np.testing.assert_array_equal(dc.bert.generate(model, prompt, 6, lengths=[dc.S0] * dc.B).numpy(), today)
    assert 100 not in today
    np.testing.assert_array_equal(dc.bert.generate(model, prompt, 6, eos_token_id=100).numpy(), today)


def test_chunked_prefill_and_a_second_turn_with_lengths():
    """prefill_chunk= gives the tokens of the one-piece prefill; append=True appends ragged pieces behind rows that stopped at
    different positions, and the continuation is each sequence's own (float64, alone)"""
    tokens = rc.assert_margins_rule_out_ties()
    want, _ = rc.expected_ids(tokens)
    for chunk in (1, 3, 7):
        np.testing.assert_array_equal(rc.generate(CpuTensor, prefill_chunk=chunk)[0], want)
    # a second turn: 4 new tokens without EOS, then the last of them and 2 / 0 / 1 given tokens appended, 2 more new tokens
    model, cache, turn = rc.second_turn(CpuTensor)
    with pytest.raises(AssertionError, match="do not fit"):
        dc.bert.generate(model, turn, 9, lengths=rc.TURN_LENGTHS, cache=cache, append=True)


def test_generate_with_lengths_checks_its_arguments():
    model = dc.make_model(CpuTensor, seed=rc.SEED)
    ids = CpuTensor.from_numpy(rc.padded(rc.prompts()), requires_grad=False)
    with pytest.raises(AssertionError, match="lengths"):
        dc.bert.generate(model, ids, 2, lengths=[5, 2])
    with pytest.raises(AssertionError, match="lengths"):
        dc.bert.generate(model, ids, 2, lengths=[5, 0, 7])
    with pytest.raises(AssertionError, match="per_row"):
        dc.bert.generate(model, ids, 2, lengths=rc.LENGTHS, cache=nn.KVCache(2, 3, 17, 64, like=model.cls.predictions.bias))
    with pytest.raises(AssertionError, match="mask"):
        dc.bert.generate(model, ids, 2, lengths=rc.LENGTHS, attention_mask=CpuTensor.from_numpy(np.ones((3, 7), np.float32), requires_grad=False))


# ---- the C ABI without a device ---------------------------------------------------------------------------------------------

NEW_ENTRIES = (("lg_attention_decode_rows_f32", 21), ("lg_attention_extend_rows_f32", 26), ("lg_decode_commit_i32", 10))


def test_header_and_prototypes_name_the_new_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRIES:
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name
    # the `_rows` entries take the argument lists of the one-word entries
    for name in ("lg_attention_decode", "lg_attention_extend"):
        assert hiplib.PROTOTYPES[name + "_rows_f32"] == hiplib.PROTOTYPES[name + "_f32"]


def test_new_entries_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entries)
        assert handle.lg_attention_decode_rows_f32(None, 0, None, 0, None, 0, None, None, 64, 0, None, None, 0, None, 1, 1, 8, 64, 1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_attention_decode_rows_f32" in handle.lg_last_error()
        assert handle.lg_attention_extend_rows_f32(None, 0, 0, None, 0, 0, None, 0, 0, None, None, 64, 0, None, None, 0, 0, None, 1, 1, 1, 8, 64, 1.0,
                                                   None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_attention_extend_rows_f32" in handle.lg_last_error()
        assert handle.lg_decode_commit_i32(None, 1, None, None, 4, 4, None, None, 1, -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_decode_commit_i32" in handle.lg_last_error()


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="no hipcc")
@pytest.mark.timeout(600)
def test_commit_kernel_uses_no_scratch(tmp_path):
    """csrc/commit.hip compiled for the device only: one kernel, a private segment of 0 bytes, no LDS"""
    shutil.copytree(CSRC, tmp_path / "pkg" / "csrc", ignore=shutil.ignore_patterns("*.o", "*.so"))
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")     # the sources include ../../include/lghip.h
    out = tmp_path / "commit.s"
    r = subprocess.run([HIPCC, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-S", "--cuda-device-only",
                        "-o", str(out), "commit.hip"], cwd=str(tmp_path / "pkg" / "csrc"), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S):
        field = lambda key: int(re.search(r"\.amdhsa_%s (\d+)" % key, body).group(1))        # noqa: E731
        found[name] = (field("private_segment_fixed_size"), field("next_free_vgpr"), field("next_free_sgpr"), field("group_segment_fixed_size"))
    assert len(found) == 1 and "decode_commit" in list(found)[0], sorted(found)
    for name, row in found.items():
        print("%-52s scratch %d vgprs %d sgprs %d lds %d" % ((name,) + row))
        assert row[0] == 0 and row[3] == 0, (name, row)
