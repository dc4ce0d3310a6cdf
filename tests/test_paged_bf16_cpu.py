"""A bfloat16 key / value cache on the numpy backend, the definition: nn.PagedKVCache(kv_dtype="bf16") holds `light.bf16_bits` of
every key and value in int16 pools, and every key and value is attended to as r(.) of what the projection produced (r =
`bf16_round_array`) - whichever step, chunk or shared prefix brought it in.  So `serve` still gives each request the continuation
it has ALONE, that of the model with r behind its key and value projections (paged_bf16_cases.rounded_reference, a float64 full
recompute per token).  Tokens are NOT compared with the float32 cache's: rounding moves logits by about as much as the top-2
margin.  (That int16 pools without the keyword are refused is an assertion of the HipTensor ops: test_hip_paged_bf16.py.)"""
import ctypes
import math
import os
import re
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.cpu.ops import bf16_round_array
from lightgrad_amd.autograd.hip import lib as hiplib
from conftest import ROOT
import decode_cases as dc
import serve_cases as sc
import paged_cases as pg
import paged_bf16_cases as pb


# ---- the definitions ------------------------------------------------------------------------------------------------------------

def test_bits_and_widen_against_words_written_out_by_hand():
    values, words = pb.special_values()
    got = light.bf16_bits(values)
    assert got.dtype == np.int16 and got.shape == values.shape
    np.testing.assert_array_equal(got.view(np.uint16), words.view(np.uint16))
    wide = light.bf16_widen(words)
    assert wide.dtype == np.float32
    np.testing.assert_array_equal(wide.view(np.uint32), words.view(np.uint16).astype(np.uint32) << 16)
    # a NaN stays a NaN, whatever its low half held
    nan = np.isnan(values)
    assert nan.sum() == 3 and np.isnan(wide[nan]).all() and not np.isnan(wide[~nan]).any()
    # r of the same values, where they are numbers: the definition that was there before
    np.testing.assert_array_equal(wide[~nan].view(np.uint32), bf16_round_array(values[~nan]).view(np.uint32))
    # float64 goes through float32, as in r
    np.testing.assert_array_equal(light.bf16_bits(values[~nan].astype(np.float64)), words[~nan])
    with pytest.raises(AssertionError, match="int16"):
        light.bf16_widen(values)


def test_widen_of_bits_is_the_rounding_on_random_values():
    rng = np.random.RandomState(0)
    x = (rng.standard_normal(100000) * np.exp(rng.uniform(-20, 20, 100000))).astype(np.float32)
    assert np.isfinite(x).all() and (np.abs(x[x != 0]) > 1e-30).all()                        # normal numbers only
    np.testing.assert_array_equal(light.bf16_widen(light.bf16_bits(x)).view(np.uint32), bf16_round_array(x).view(np.uint32))
    # and every word is within half a bfloat16 step of its value
    assert (np.abs(light.bf16_widen(light.bf16_bits(x)).astype(np.float64) - x) <= np.abs(x.astype(np.float64)) * 2.0 ** -8).all()


# ---- the composite --------------------------------------------------------------------------------------------------------------

TABLES = ((5, 1, 8, 3), (2, 9, -1, -1), (7, 0, 6, -1))          # B = 4, a pool of 10 blocks: non-monotone, interleaved; block 4 is nobody's
STEP = ((6, 3), (0, 4), (9, 0))                                  # (position, count): a seam inside a block, an empty slot, an idle slot


def _step_operands(dtype):
    rng = np.random.RandomState(5)
    model = dc.make_model(CpuTensor, dtype, sc.SEED)
    attention = model.bert.encoder.layer[0].attention.self
    hidden = rng.standard_normal((3, 4, 64)).astype(dtype)
    pools = [light.bf16_bits(rng.standard_normal((10, 4, 64)).astype(np.float32)) for _ in range(2)]
    mask = np.ones((3, 16), np.float32)
    mask[0, 2] = mask[1, 1] = 0
    return attention, hidden, pools, mask.astype(dtype)


def _run_step(attention, hidden, pools, mask, kv_dtype, dtype):
    T = CpuTensor
    tensor = lambda a: T.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    cache = nn.PagedKVCache(1, 3, 10, 4, 64, 4, like=tensor(np.zeros(1, dtype)), kv_dtype=kv_dtype)
    assert cache.kv_dtype == kv_dtype
    cache.k[0][:], cache.v[0][:] = tensor(pools[0]), tensor(pools[1])
    cache.block_table[:] = tensor(np.array(TABLES, np.int32))
    cache.pos[:] = tensor(np.array([t for t, _ in STEP], np.int32))
    with light.no_grad():
        context, probs = attention._paged_composite(tensor(hidden), tensor(mask), cache, 0, tensor(np.array([n for _, n in STEP], np.int32)))
    return context.numpy().copy(), probs.numpy().copy(), cache.k[0].numpy().copy(), cache.v[0].numpy().copy()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_step_on_int16_pools_is_the_float_step_on_rounded_keys_and_widened_pools(dtype):
    def run():
        attention, hidden, pools, mask = _step_operands(dtype)
        got = _run_step(attention, hidden, pools, mask, "bf16", dtype)
        # the float composite as it was, given r(k), r(v) by the projections and the widened pools
        attention.key, attention.value = pb.RoundedProjection(attention.key), pb.RoundedProjection(attention.value)
        want = _run_step(attention, hidden, [light.bf16_widen(p).astype(dtype) for p in pools], mask, None, dtype)
        return got, want, pools
    if dtype == np.float64:
        with dc.float64_tape():
            got, want, pools = run()
    else:
        got, want, pools = run()
    assert got[0].dtype == want[0].dtype == dtype and got[2].dtype == np.int16 and want[2].dtype == dtype
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert np.abs(got[0][0, :3]).min() > 0 and (got[0][2] == 0).all()
    written = np.zeros((10, 4), bool)
    for r, (t, n) in enumerate(STEP):
        for j in range(t, t + n):
            written[TABLES[r][j // 4], j % 4] = True
    assert written.sum() == 7
    for after, float_after, before in zip(got[2:], want[2:], pools):
        np.testing.assert_array_equal(after[~written], before[~written])                       # nothing else is touched
        np.testing.assert_array_equal(after[written], light.bf16_bits(float_after[written]))   # the new rows hold bits(.)
        np.testing.assert_array_equal(light.bf16_widen(after[written]).astype(dtype), float_after[written])
        assert (after[written] != before[written]).any()


# ---- serve ----------------------------------------------------------------------------------------------------------------------

def test_the_rounded_references_rule_out_ties_and_differ_from_nothing_by_chance():
    tokens = pb.assert_rounded_margins_rule_out_ties()
    assert len(tokens) == 7 and all(len(t) == sc.BUDGET for t in tokens)
    want, want_len = sc.expected(tokens, sc.BUDGET, sc.EOS)
    assert want_len.min() < sc.BUDGET and want_len.max() == sc.BUDGET          # both stops occur


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
@pytest.mark.parametrize("shared", [0, pg.PREFIX])
def test_bf16_serve_gives_each_request_its_own_rounded_continuation(slots, chunk, shared):
    rows = pg.prefixed_prompts()
    want, want_len = sc.expected(pb.assert_rounded_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    F = 2 if shared else 0
    lengths, steps = [len(p) for p in rows], []
    for num_blocks in (F + slots * pg.MAX_BLOCKS, pg.tight_blocks(rows, sc.BUDGET, F)):
        out, out_len, stats, cache = pb.run_serve(CpuTensor, slots, chunk, num_blocks, poll=1, **({"shared_prefix": shared} if shared else {}))
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        assert stats["prefix_blocks"] == F and stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks, F)
        pg.assert_no_block_leaked(cache, F)
        float_cache = nn.PagedKVCache(dc.CFG["num_hidden_layers"], slots, num_blocks, pg.BLOCK, dc.CFG["hidden_size"], pg.MAX_BLOCKS)
        assert float_cache.kv_dtype is None and 2 * cache.pool_bytes() == float_cache.pool_bytes()
        steps.append(stats["steps"])
    assert steps[1] > steps[0] or slots == 1


def test_bf16_serve_makes_its_own_cache_and_runs_in_float64():
    rows = pg.prefixed_prompts()
    want, want_len = sc.expected(pb.assert_rounded_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    (out, out_len), stats = pg.bert.serve(model, rows, sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, num_blocks=9, block_size=8,
                                          kv_dtype="bf16")
    np.testing.assert_array_equal(out.numpy(), want)
    np.testing.assert_array_equal(out_len.numpy(), want_len)
    assert stats["kv_dtype"] == "bf16" and stats["pool_bytes"] == 2 * 2 * 9 * 8 * 64 * 2
    # the float32 cache reports its form too
    (_, _), stats = pg.bert.serve(model, rows, sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, num_blocks=9, block_size=8)
    assert stats["kv_dtype"] is None and stats["pool_bytes"] == 2 * 2 * 9 * 8 * 64 * 4
    with dc.float64_tape():
        out, out_len, _, cache = pb.run_serve(CpuTensor, 3, 4, pg.tight_blocks(rows, sc.BUDGET), model=dc.make_model(CpuTensor, np.float64, sc.SEED))
    np.testing.assert_array_equal(out, want)
    pg.assert_no_block_leaked(cache)


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_misuse_of_a_bf16_cache_is_refused_by_name():
    model = dc.make_model(CpuTensor, seed=sc.SEED)
    like = model.cls.predictions.bias
    cache = nn.PagedKVCache(2, 2, 8, 4, 64, 4, like=like, kv_dtype="bf16")
    i32 = lambda a: CpuTensor.from_numpy(np.asarray(a, np.int32), requires_grad=False)             # noqa: E731
    ids = i32([[3, 4, 5], [6, 7, 8]])
    with pytest.raises(AssertionError, match="kv_dtype.*(paged|num_blocks)"):                      # kv_dtype= without paging
        pg.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, kv_dtype="bf16")
    with pytest.raises(AssertionError, match="kv_dtype"):                                          # ... and with a float32 paged cache
        pg.bert.serve(model, sc.prompts(), sc.BUDGET, slots=2, chunk=4, kv_dtype="bf16", cache=nn.PagedKVCache(2, 2, 8, 4, 64, 4, like=like))
    with pytest.raises(AssertionError, match="bf16"):
        nn.PagedKVCache(2, 2, 8, 4, 64, 4, like=like, kv_dtype="fp8")
    with pytest.raises(AssertionError, match="bf16.*float32 nn.KVCache"):
        pg.bert.generate(model, ids, 2, cache=cache)
    with pytest.raises(NotImplementedError, match="bf16.*float32 nn.KVCache"):
        cache.reorder(i32([0, 1]))
    with pytest.raises(AssertionError, match="token_budget.*bf16.*float32 nn.KVCache"):
        pb.run_serve(CpuTensor, 3, 4, 12, token_budget=6)
    with pytest.raises(AssertionError, match="token_budget.*bf16.*float32 nn.KVCache"):
        nn.RequestPool(nn.PagedKVCache(2, 3, 12, 4, 64, 6, kv_dtype="bf16"), np.ones((2, 3), np.int32), [3, 3], [2, 2], 4, token_budget=6)
    with pytest.raises(AssertionError, match="bf16.*float32 nn.KVCache"):                          # the prompt / one-token decode route
        model(ids[:, :1], cache=cache)
    with pytest.raises(AssertionError, match="bf16.*float32 nn.KVCache"):                          # token-packed rows
        model(i32([[3, 4, 5]]), cache=cache, append=True, cu=i32([0, 2, 3]), token_positions=i32([[0, 1, 0]]))
    assert math.isclose(cache.pool_bytes(), 2 * 2 * 8 * 4 * 64 * 2)


# ---- the C ABI without a device -------------------------------------------------------------------------------------------------

def test_header_prototype_and_makefile_name_the_bf16_entry():
    name = "lg_attention_extend_paged_bf16_f32"
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lghip.h")).read(), flags=re.S)
    decl = re.search(r"int %s\((.*?)\);" % name, text, re.S)
    assert decl is not None
    # the paged entry's argument list, with uint16_t pools
    paged = re.search(r"int lg_attention_extend_paged_f32\((.*?)\);", text, re.S).group(1)
    squeeze = lambda t: re.sub(r"\s+", " ", t).strip()                                            # noqa: E731
    assert squeeze(decl.group(1)) == squeeze(paged).replace("float* k_pool, float* v_pool", "uint16_t* k_pool, uint16_t* v_pool")
    assert hiplib.PROTOTYPES[name] == hiplib.PROTOTYPES["lg_attention_extend_paged_f32"] and len(hiplib.PROTOTYPES[name][1]) == 29
    makefile = open(os.path.join(ROOT, "lightgrad_amd", "csrc", "Makefile")).read()
    assert " paged_bf16.hip" in makefile and " paged.hip" in makefile
    handle = hiplib.load_library()                                                                # every declared symbol is there
    n = ctypes.c_int(0)
    handle.lg_device_count(ctypes.byref(n))
    if n.value == 0:                        # (with a GPU the library of this process may be initialised: the gpu tests cover the entry)
        assert handle.lg_attention_extend_paged_bf16_f32(None, 64, 0, None, 64, 0, None, 64, 0, None, None, 64, None, None, None, None, 64, 0, None,
                                                         1, 1, 4, 2, 4, 2, 64, 1.0, None, 0) == -4
        assert b"lg_init" in handle.lg_last_error() and name.encode() in handle.lg_last_error()
