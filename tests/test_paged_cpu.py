"""The paged key / value cache without a device: nn.PagedKVCache, `serve_commit_paged` as the numpy backend defines it against the
words written out by hand (paged_cases.py), the composite definition of a model step against a paged cache
(`model(ids, cache=paged, append=True, count=)`) and the paged `serve` of examples/bert.py on CpuTensor - with a generous and a
tight pool, with and without a shared prefix - against each request's float64 greedy continuation ALONE."""
import ctypes
import os
import re
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.hip import lib as hiplib
from conftest import ROOT
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius, float64_tape
import decode_cases as dc
import serve_cases as sc
import paged_cases as pg

LG_ENOTINIT = -4


# ---- nn.PagedKVCache ------------------------------------------------------------------------------------------------------------

def test_paged_cache_holds_pools_tables_and_a_stack():
    cache = nn.PagedKVCache(2, 3, 10, 4, 64, 6)
    assert len(cache.k) == len(cache.v) == 2 and all(tuple(t.shape) == (10, 4, 64) and t.dtype == np.float32 for t in cache.k + cache.v)
    assert tuple(cache.block_table.shape) == (3, 6) and (cache.block_table.numpy() == -1).all() and cache.block_table.dtype == np.int32
    assert cache.held.numpy().tolist() == [0, 0, 0] and cache.pos.numpy().tolist() == [0, 0, 0] and cache.per_row and cache.batch == 3
    assert cache.capacity == 24 and cache.block_size == 4 and cache.max_blocks == 6 and cache.num_blocks == 10
    assert cache.free.numpy().tolist() == [10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0]            # the top is word 10: block 0 is popped first
    assert cache.positions(3).numpy().tolist() == [[0, 1, 2]] * 3
    cache.block_table[:] = CpuTensor.from_numpy(np.ones((3, 6), np.int32), requires_grad=False)
    cache.reset(prefix_blocks=2)
    assert cache.free.numpy()[:9].tolist() == [8, 9, 8, 7, 6, 5, 4, 3, 2] and (cache.block_table.numpy() == -1).all()
    like = CpuTensor.from_numpy(np.zeros(1, np.float64), requires_grad=False)
    assert nn.PagedKVCache(1, 1, 2, 128, 64, 4, like=like).k[0].dtype == np.float64
    for bad in (dict(block_size=3), dict(block_size=2), dict(block_size=256), dict(block_size=128, max_blocks=5)):
        with pytest.raises(AssertionError, match="PagedKVCache"):
            nn.PagedKVCache(**dict(dict(layers=1, slots=1, num_blocks=4, block_size=4, width=64, max_blocks=4), **bad))
    with pytest.raises(NotImplementedError, match="PagedKVCache"):
        cache.reorder(None)


# ---- serve_commit_paged: the definition -----------------------------------------------------------------------------------------

def assert_commit_matches(state, nxt, prefix_blocks, eos, expect_flag=False):
    want, flag = pg.commit_by_hand(state, nxt, 4, prefix_blocks, eos)
    tensors, error = pg.commit_on(CpuTensor, state, nxt, 4, prefix_blocks, eos)
    assert flag == expect_flag and (error is not None) == expect_flag
    for name in pg.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)
    return want


@pytest.mark.parametrize("b", (1, 3, 7, 64, 65, 70, 1024))
@pytest.mark.parametrize("eos", (None, 3))
@pytest.mark.parametrize("prefix_blocks", (0, 2))
@pytest.mark.parametrize("spare", (0, 2, 40))
def test_serve_commit_paged_on_the_numpy_backend(b, eos, prefix_blocks, spare):
    for shift in range(7 if b < 7 else 1):           # every kind of slot comes first once
        state, nxt = pg.commit_state(b + shift, 4, 11 * b + shift, prefix_blocks, spare, eos=eos)
        state = {k: (v[shift:] if k in ("req", "pos", "count", "ids", "position_ids", "last", "block_table", "held") else v) for k, v in state.items()}
        assert_commit_matches(state, nxt[shift:], prefix_blocks, eos)


def test_a_release_and_an_admission_in_one_commit_reuse_the_blocks():
    """7 slots, nothing spare: slots 3 and 4 (budget, eos) and whoever else draws its last token end, push their blocks, and the
    free slots pop exactly those"""
    state, nxt = pg.commit_state(7, 4, 5, 0, 0, eos=3)
    assert state["free"][0] == 0
    want = assert_commit_matches(state, nxt, 0, 3)
    ended = [s for s in range(7) if state["req"][s] >= 0 and want["req"][s] != state["req"][s]]
    assert {3, 4} <= set(ended)
    released = [e for s in ended for e in state["block_table"][s, :state["held"][s]].tolist()]
    assert want["queue"][1] == len(ended) and want["queue"][0] > state["queue"][0]             # somebody was admitted
    admitted = [s for s in range(7) if want["req"][s] >= state["queue"][0]]
    taken = [e for s in admitted for e in want["block_table"][s, :want["held"][s]].tolist()]
    assert admitted and set(taken) <= set(released) and len(set(taken)) == len(taken)
    assert want["free"][0] == len(released) - len(taken)
    # the first admitted slot pops from the top: the LAST block pushed
    assert want["block_table"][admitted[0], 0] == released[-1]


def test_a_request_that_does_not_fit_stops_the_admission_and_is_not_overtaken():
    state, nxt = pg.dry_pool_state()
    want = assert_commit_matches(state, nxt, 0, None)
    assert want["req"].tolist() == [0, -1, -1] and want["queue"].tolist() == [1, 0] and want["free"][0] == 2
    assert want["block_table"][0].tolist() == [2, -1, -1] and want["held"].tolist() == [1, 0, 0] and want["count"].tolist() == [3, 0, 0]
    # with one more block the second fits, and the third behind it
    state["free"][:] = [4, 4, 0, 2, 1, 0]
    want = assert_commit_matches(state, nxt, 0, None)
    assert want["req"].tolist() == [0, 1, -1] and want["free"][0] == 0 and want["block_table"][1].tolist() == [2, 0, 4]


@pytest.mark.parametrize("b", (1, 3, 7))
@pytest.mark.parametrize("eos", (None, 3))
def test_with_no_prefix_and_blocks_for_everybody_the_commit_writes_what_serve_commit_writes(b, eos):
    state, nxt = pg.commit_state(b, 4, 3 * b, 0, 7 * 6)
    plain = {k: state[k] for k in sc.NAMES}
    want, flag = sc.commit_by_hand(plain, nxt, 24, eos)
    tensors, error = pg.commit_on(CpuTensor, state, nxt, 4, 0, eos)
    assert not flag and error is None
    for name in sc.NAMES:
        np.testing.assert_array_equal(tensors[name].numpy(), want[name], err_msg=name)


def test_serve_commit_paged_checks_its_bounds():
    base, nxt = pg.commit_state(7, 4, 5, 0, 3, eos=3)
    for change in ("held", "entry", "stack", "need"):
        state = {k: v.copy() for k, v in base.items()}
        if change == "held":
            state["held"][3] = 7                     # the slot whose budget ends names more blocks than a table has
        elif change == "entry":
            state["block_table"][4, 1] = len(state["free"]) - 1          # the slot that draws eos releases a block the pool has not
        elif change == "stack":
            state["free"][0] = len(state["free"])
        else:
            state["budget"][state["queue"][0]] = 30  # the head of the queue needs more blocks than a table has
        want = assert_commit_matches(state, nxt, 0, 3, expect_flag=True)
        if change in ("held", "entry"):
            s = 3 if change == "held" else 4
            assert want["count"][s] == 0 and want["req"][s] == state["req"][s] and (want["block_table"][s] == state["block_table"][s]).all()
            clean, _ = pg.commit_by_hand(base, nxt, 4, 0, 3)                                      # the slots in front are committed as without it
            assert (want["req"][:s] == clean["req"][:s]).all() and (want["count"][:s] == clean["count"][:s]).all() and (want["count"][:s] > 0).any()


def test_serve_commit_paged_refuses_other_operands():
    state, nxt = pg.commit_state(3, 2, 1, 0, 4)
    i32 = lambda a: CpuTensor.from_numpy(np.asarray(a, np.int32), requires_grad=False)             # noqa: E731
    tensors = sc.upload(CpuTensor, state)
    for block_size, prefix in ((3, 0), (256, 0), (4, 9)):
        with pytest.raises(AssertionError, match="serve_commit_paged"):
            i32(nxt).serve_commit_paged(*(tensors[k] for k in pg.NAMES), block_size, prefix)
    for name, value in (("held", np.zeros(4, np.int32)), ("block_table", np.zeros((2, 6), np.int32)), ("free", np.zeros(5, np.float32))):
        with pytest.raises(AssertionError, match="serve_commit_paged"):
            i32(nxt).serve_commit_paged(*(dict(tensors, **{name: CpuTensor.from_numpy(value, requires_grad=False)})[k] for k in pg.NAMES), 4, 0)
    with pytest.raises(AssertionError, match="overlap"):
        i32(nxt).serve_commit_paged(*(dict(tensors, held=tensors["count"])[k] for k in pg.NAMES), 4, 0)


# ---- nn.RequestPool over a paged cache ------------------------------------------------------------------------------------------

def test_request_pool_dispatches_to_the_paged_commit_and_checks_the_reservations():
    rows = sc.prompts()
    padded, lengths = np.stack([np.pad(p, (0, 9 - len(p))) for p in rows]), [len(p) for p in rows]
    cache = nn.PagedKVCache(2, 3, 8, 4, 64, 6)
    pool = nn.RequestPool(cache, padded, lengths, [6] * 7, 4, pad_token_id=sc.PAD)
    assert pool.paged and pool.cu is None and tuple(pool.ids.shape) == (3, 4)
    pool.admit()
    # needs of 3, 2 and 3 blocks: the third does not fit the 8 - 5 = 3 ... it does; block 0 goes first
    assert pool.req.numpy().tolist() == [0, 1, 2] and cache.held.numpy().tolist() == [3, 2, 3] and cache.free.numpy()[0] == 0
    assert cache.block_table.numpy()[:, :3].tolist() == [[0, 1, 2], [3, 4, -1], [5, 6, 7]]
    with pytest.raises(AssertionError, match="PagedKVCache"):
        nn.RequestPool(cache, padded, lengths, [6] * 7, 4, token_budget=7)
    with pytest.raises(AssertionError, match="PagedKVCache"):           # 9 + 16 - 1 positions: 6 blocks fit a table, not a pool of 5
        nn.RequestPool(nn.PagedKVCache(2, 3, 5, 4, 64, 6), padded, lengths, [16] * 7, 4)
    with pytest.raises(AssertionError, match="does not fit"):           # ... and 7 blocks no table of 6: the capacity
        nn.RequestPool(nn.PagedKVCache(2, 3, 9, 4, 64, 6), padded, lengths, [20] * 7, 4)
    with pytest.raises(AssertionError, match="prefix"):                 # a prompt of 1 token behind a prefix of 4
        nn.RequestPool(cache, padded, lengths, [6] * 7, 4, prefix_blocks=1)
    with pytest.raises(AssertionError, match="prefix_blocks"):
        nn.RequestPool(nn.KVCache(2, 3, 17, 64, per_row=True), padded, lengths, [6] * 7, 4, prefix_blocks=1)


# ---- one model step against a paged cache ---------------------------------------------------------------------------------------

def test_one_paged_step_matches_each_sequence_alone():
    ref64, cpu32 = sc.mixed_reference()
    got, cache = pg.mixed_step(CpuTensor)
    assert [g.shape for g in got] == [r.shape for r in ref64]
    assert_as_close_to_float64_as_the_cpu_backend(sc.named(got), sc.named(cpu32), sc.named(ref64), floor=1e-5, what="paged step on CpuTensor")
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])          # the caller moves the positions, not the forward
    # the step's rows went where the tables say, and a block no table names was not touched
    named = {e for row in pg.MIXED_TABLES for e in row if e >= 0}
    assert named == set(range(16))
    k = cache.k[0].numpy().reshape(16 * 4, -1)
    for r, (t, n) in enumerate(sc.MIXED):
        rows = [pg.MIXED_TABLES[r][j // 4] * 4 + j % 4 for j in range(t + n)]
        assert np.abs(k[rows]).min(axis=1).max() > 0 or t + n == 0


def test_one_paged_step_in_float64_is_each_sequence_alone():
    ref64, _ = sc.mixed_reference()
    with float64_tape():
        got, _ = pg.mixed_step(CpuTensor, model=dc.make_model(CpuTensor, np.float64, sc.SEED), dtype=np.float64)
    for r, (_, n) in enumerate(sc.MIXED):
        if n:
            assert got[r].dtype == np.float64 and rel_frobenius(got[r], ref64[r]) < 1e-13, r


def test_misuse_of_a_paged_cache_is_refused():
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    cache = nn.PagedKVCache(2, 2, 8, 4, 64, 4, like=model.cls.predictions.bias)
    i32 = lambda a: CpuTensor.from_numpy(np.asarray(a, np.int32), requires_grad=False)             # noqa: E731
    ids = i32([[3, 4, 5], [6, 7, 8]])
    with pytest.raises(AssertionError, match="PagedKVCache"):           # the prompt / one-token decode route
        model(ids[:, :1], cache=cache)
    with pytest.raises(AssertionError, match="PagedKVCache"):           # append without a count
        model(ids, cache=cache, append=True)
    with pytest.raises(AssertionError, match="PagedKVCache"):           # token-packed rows
        model(i32([[3, 4, 5]]), cache=cache, append=True, cu=i32([0, 2, 3]), token_positions=i32([[0, 1, 0]]))
    with pytest.raises(AssertionError, match="PagedKVCache"):
        pg.bert.generate(model, ids, 2, cache=cache)
    with pytest.raises(IndexError, match="table"):                      # a slot reaches a block its table does not name
        model(ids, cache=cache, append=True, count=i32([3, 0]))
    with pytest.raises(AssertionError, match="token_budget"):
        pg.run_serve(CpuTensor, 3, 4, 12, token_budget=6)
    with pytest.raises(AssertionError, match="shared_prefix"):          # the prompts do not begin alike
        pg.run_serve(CpuTensor, 3, 4, 12, shared_prefix=1)
    with pytest.raises(AssertionError, match="shared_prefix"):
        sc.run_serve(CpuTensor, 3, 4, shared_prefix=4)


# ---- serve over a paged cache ---------------------------------------------------------------------------------------------------

def test_a_tight_pool_takes_more_steps_by_hand():
    """the schedule alone: with more than one slot a pool of the largest need plus one block runs fewer requests at once.  (With
    ONE slot a single request runs at a time whatever the pool holds: the two schedules are the same, and that is asserted.)"""
    rows, lengths = sc.prompts(), [len(p) for p in sc.prompts()]
    tight = pg.tight_blocks(rows, sc.BUDGET)
    assert tight == 5
    for chunk in sc.CHUNKS:
        plain = [sc.simulate(lengths, sc.EMITTED, slots, chunk) for slots in sc.SLOTS]
        generous = [pg.simulate(lengths, sc.EMITTED, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, slots * pg.MAX_BLOCKS) for slots in sc.SLOTS]
        few = [pg.simulate(lengths, sc.EMITTED, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, tight) for slots in sc.SLOTS]
        assert generous == plain and few[0] == generous[0] and few[1] > generous[1] and few[2] > generous[2], (chunk, plain, generous, few)


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_paged_serve_gives_each_request_its_own_continuation(slots, chunk):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    lengths, steps = [len(p) for p in sc.prompts()], []
    for num_blocks in (slots * pg.MAX_BLOCKS, pg.tight_blocks(sc.prompts(), sc.BUDGET)):
        out, out_len, stats, cache = pg.run_serve(CpuTensor, slots, chunk, num_blocks, poll=1)
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        assert stats["prefix_blocks"] == 0 and stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks)
        pg.assert_no_block_leaked(cache)
        steps.append(stats["steps"])
    assert steps[0] == sc.simulate(lengths, want_len, slots, chunk)          # a generous pool: the schedule of the unpaged serve
    assert steps[1] > steps[0] or slots == 1


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_paged_serve_with_a_shared_prefix(slots, chunk):
    rows = pg.prefixed_prompts()
    want, want_len = sc.expected(pg.assert_prefixed_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    lengths, steps = [len(p) for p in rows], []
    for num_blocks in (2 + slots * pg.MAX_BLOCKS, pg.tight_blocks(rows, sc.BUDGET, 2)):
        out, out_len, stats, cache = pg.run_serve(CpuTensor, slots, chunk, num_blocks, rows=rows, poll=1, shared_prefix=pg.PREFIX)
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        assert stats["prefix_blocks"] == 2 and stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks, 2)
        pg.assert_no_block_leaked(cache, 2)
        steps.append(stats["steps"])
    assert steps[1] > steps[0] or slots == 1
    if (slots, chunk) == (3, 4):
        # the same prompts without the declaration: the same tokens, the prefix recomputed by every request - more steps at a piece of 4
        out, out_len, stats, cache = pg.run_serve(CpuTensor, slots, chunk, slots * pg.MAX_BLOCKS, rows=rows, poll=1)
        np.testing.assert_array_equal(out, want)
        assert stats["prefix_blocks"] == 0 and stats["steps"] > steps[0]
        pg.assert_no_block_leaked(cache)


def test_paged_serve_with_a_budget_per_request_and_in_float64():
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGETS, None)
    tight = pg.tight_blocks(sc.prompts(), sc.BUDGETS)
    out, out_len, stats, cache = pg.run_serve(CpuTensor, 3, 4, tight, budgets=sc.BUDGETS, eos=None, poll=1)
    np.testing.assert_array_equal(out, want)
    np.testing.assert_array_equal(out_len, want_len)
    assert stats["steps"] == pg.simulate([len(p) for p in sc.prompts()], sc.BUDGETS, sc.BUDGETS, 3, 4, pg.BLOCK, tight)
    pg.assert_no_block_leaked(cache)
    with float64_tape():
        out, out_len, _, cache = pg.run_serve(CpuTensor, 3, 4, tight, model=dc.make_model(CpuTensor, np.float64, sc.SEED), budgets=sc.BUDGETS, eos=None)
    np.testing.assert_array_equal(out, want)
    pg.assert_no_block_leaked(cache)
    # num_blocks= makes the cache: tables as long as the longest request needs
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    (out, out_len), stats = pg.bert.serve(model, sc.prompts(), sc.BUDGETS, slots=3, chunk=4, pad_token_id=sc.PAD, num_blocks=9, block_size=8)
    np.testing.assert_array_equal(out.numpy(), want)
    assert stats["num_blocks"] == 9 and stats["block_size"] == 8 and stats["prefix_blocks"] == 0


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------

NEW_ENTRIES = (("lg_attention_extend_paged_f32", 29), ("lg_serve_commit_paged_i32", 29))


def test_header_prototypes_and_makefile_name_the_paged_entries():
    text = open(os.path.join(ROOT, "include", "lghip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, n_args in NEW_ENTRIES:
        decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
        assert decl is not None, name
        assert len(decl.group(1).split(",")) == n_args == len(hiplib.PROTOTYPES[name][1]), name
    # the paged commit takes the commit's arguments up to `last`, then the table, held and the stack
    rows, paged = hiplib.PROTOTYPES["lg_serve_commit_i32"][1], hiplib.PROTOTYPES["lg_serve_commit_paged_i32"][1]
    assert paged[:19] == rows[:19] and paged[19:22] == [ctypes.c_void_p] * 3 and paged[-1] is ctypes.c_int32
    makefile = open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()
    assert " paged.hip" in makefile and "serve_paged.hip" in makefile


def test_paged_entries_on_the_uninitialised_library():
    handle = hiplib.load_library()
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entries)
        assert handle.lg_attention_extend_paged_f32(None, 64, 0, None, 64, 0, None, 64, 0, None, None, 64, None, None, None, None, 64, 0, None,
                                                    1, 1, 4, 2, 4, 2, 64, 1.0, None, 0) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_attention_extend_paged_f32" in handle.lg_last_error()
        assert handle.lg_serve_commit_paged_i32(None, 1, None, 4, 4, None, None, None, 4, 4, None, None, 1, None, None, None, None, None, None,
                                                None, None, None, 1, 1, 2, 4, 2, 0, -1) == LG_ENOTINIT
        assert b"lg_init" in handle.lg_last_error() and b"lg_serve_commit_paged_i32" in handle.lg_last_error()
