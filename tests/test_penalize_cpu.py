"""Per-request penalties on the numpy backend: `random.penalty_table`, the definition `random.penalize_logits` behind
`CpuTensor.penalize_rows`, `nn.RequestPool(penalties=)` and `serve(repetition_penalty=, presence_penalty=, frequency_penalty=,
min_new_tokens=)` - every request's tokens are those of its run ALONE through the definition with its own history
(penalty_cases.reference), whatever slots, chunk, token budget, paging and the shared prefix are."""
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import paged_bf16_cases as pb
import paged_cases as pg
import penalty_cases as pc
import serve_cases as sc
import serve_packed_cases as spc


def tensor(a):
    return CpuTensor.from_numpy(np.array(a, copy=True, order="C"), requires_grad=False)      # a copy: the op writes in place


def tensors(case):
    """(logits, the six integer operands) of a case as CpuTensors"""
    return tensor(case["logits"]), [tensor(case[k]) for k in ("table", "index", "prompts", "prompt_len", "out", "out_len")]


# ---- the table ------------------------------------------------------------------------------------------------------------------

def test_penalty_table_against_words_written_out_by_hand():
    table = lg_random.penalty_table([1.0, 1.5, 0.5], [0.0, -2.0, 0.5], [0.0, 0.25, -0.0], [0, 7, 2 ** 31 - 1])
    assert table.dtype == np.int32 and table.shape == (3, 4)
    u = table.view(np.uint32).tolist()
    # float32: 1.0 = 0x3F800000, 1.5 = 0x3FC00000, 0.5 = 0x3F000000, -2.0 = 0xC0000000, 0.25 = 0x3E800000, -0.0 = 0x80000000
    assert u == [[0x3F800000, 0, 0, 0], [0x3FC00000, 0xC0000000, 0x3E800000, 7], [0x3F000000, 0x3F000000, 0x80000000, 0x7FFFFFFF]]
    # the float32 value IS the parameter
    assert lg_random.penalty_table(1.3).view(np.uint32)[0, 0] == np.float32(1.3).view(np.uint32)
    # scalars broadcast; the neutral row
    np.testing.assert_array_equal(lg_random.penalty_table(1.3, [0.5, 0.6], 0.25, 2), lg_random.penalty_table([1.3, 1.3], [0.5, 0.6], [0.25, 0.25], [2, 2]))
    assert lg_random.penalty_table().view(np.uint32).tolist() == [[0x3F800000, 0, 0, 0]]
    # the sampling table is a table of its own and has not moved: words 6 and 7 stay 0
    assert lg_random.sampling_table(0.9, 20, 0.95, 7).shape == (1, 8) and (lg_random.sampling_table(0.9, 20, 0.95, 7)[:, 6:] == 0).all()


@pytest.mark.parametrize("bad", [dict(repetition_penalty=0.0), dict(repetition_penalty=-0.0), dict(repetition_penalty=-1.3), dict(repetition_penalty=float("inf")),
                                 dict(repetition_penalty=float("nan")), dict(repetition_penalty=1e39), dict(repetition_penalty=1e-46),
                                 dict(presence_penalty=float("inf")), dict(presence_penalty=float("nan")), dict(presence_penalty=-1e39),
                                 dict(frequency_penalty=float("-inf")), dict(frequency_penalty=float("nan")), dict(frequency_penalty=1e39),
                                 dict(min_new_tokens=-1), dict(min_new_tokens=2 ** 31), dict(min_new_tokens=1.5),
                                 dict(repetition_penalty=[1.0, 2.0], min_new_tokens=[1, 2, 3]), dict(presence_penalty=[]), dict(frequency_penalty=[[0.5]])], ids=str)
def test_penalty_table_refuses_each_bad_entry(bad):
    with pytest.raises(ValueError):
        lg_random.penalty_table(**bad)
    if all(np.ndim(v) == 0 for v in bad.values()):                          # ... and as the last entry behind two good ones
        with pytest.raises(ValueError):
            lg_random.penalty_table(**{k: [1, 1, v] for k, v in bad.items()})


# ---- the definition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nine_rows_against_the_loop_over_the_elements(dtype):
    case = dict(pc.nine_rows(), logits=pc.nine_rows()["logits"].astype(dtype))
    for eos in (None, pc.NINE_EOS, 0, pc.V - 1):
        want, want_bad = pc.by_hand(case, eos)
        y, bad = lg_random.penalize_logits(**case, eos=eos)
        assert bad.tolist() == want_bad.tolist() == pc.NINE_BAD and pc.same_bits(y, want), eos
    y, _ = lg_random.penalize_logits(**case, eos=pc.NINE_EOS)
    x = case["logits"]
    real = dtype
    rho, alpha, beta = (real(np.float32(v)) for v in (1.2, 0.7, 0.35))
    assert np.isnan(y[0]).all() and pc.same_bits(y[6], x[6])                # the free row and the row beyond the table: as they came
    # request 3, row 2: the specials at ids of the prompt alone ...
    want = [x[2, 10] * rho, x[2, 11] / rho, real(0.0), real(-0.0), real(np.inf), real(-np.inf)]
    assert pc.same_bits(y[2, 10:16], np.array(want, dtype)) and np.isnan(y[2, 16])
    # ... and at ids of the tokens: 20 and 21 also stand in the prompt, and are changed ONCE by step 3; 22 .. 25 occur twice
    want = [(x[2, 20] * rho - beta * real(1)) - alpha, (x[2, 21] / rho - beta * real(1)) - alpha, (real(0.0) - beta * real(2)) - alpha,
            (real(-0.0) - beta * real(2)) - alpha, real(np.inf), real(-np.inf)]
    assert pc.same_bits(y[2, 20:26], np.array(want, dtype)) and np.isnan(y[2, 26])
    # every other logit of the row is untouched
    rest = np.setdiff1d(np.arange(pc.V), np.r_[10:17, 20:27])
    assert pc.same_bits(y[2, rest], x[2, rest])
    # request 0 (rows 1 and 7): eos inside the history, g = 2 < 4; request 4 (row 8): outside, g = 1 < 3, nothing else moves
    assert y[1, pc.NINE_EOS] == y[7, pc.NINE_EOS] == y[8, pc.NINE_EOS] == -np.inf
    rest = np.setdiff1d(np.arange(pc.V), [pc.NINE_EOS])
    assert pc.same_bits(y[8, rest], x[8, rest])
    without, _ = lg_random.penalize_logits(**case)
    assert np.isfinite(without[[1, 7, 8], pc.NINE_EOS]).all() and pc.same_bits(without[8], x[8])
    # request 2 (row 5): one id, seven times in the history, four of them tokens - changed once
    assert pc.same_bits(y[5, 7:8], np.array([((x[5, 7] * real(np.float32(1.5)) if x[5, 7] < 0 else x[5, 7] / real(np.float32(1.5)))
                                              - real(np.float32(0.3)) * real(4)) - real(np.float32(0.2))], dtype))
    # request 1 (row 4): g = 0 - the repetition penalty on its prompt alone
    assert sorted(np.flatnonzero(y[4] != x[4]).tolist()) == [1, 2, 3]


@pytest.mark.parametrize("L", pc.EDGES)
def test_every_history_length_against_the_loop_over_the_elements(L):
    case = pc.edge(L)
    assert case["prompt_len"][0] + case["out_len"][0] == L and case["prompts"].shape[1] + case["out"].shape[1] == max(L, 2)
    want, _ = pc.by_hand(case)
    y, bad = lg_random.penalize_logits(**case)
    assert not bad.any() and pc.same_bits(y, want)
    history = [np.r_[case["prompts"][i], case["out"][i, :case["out_len"][i]]] for i in (0, 1)]
    assert np.unique(history[0]).size == L and np.unique(history[1]).size <= 7
    assert (y[0] != case["logits"][0]).sum() == L and (L < 4096 or np.unique(case["out"][1], return_counts=True)[1].max() >= 200)


def test_the_neutral_row_is_the_identity_bit_for_bit():
    case = dict(pc.nine_rows(), table=np.repeat(lg_random.penalty_table(), 5, axis=0))
    for eos in (None, pc.NINE_EOS):                                        # min_new = 0: eos is never touched
        y, bad = lg_random.penalize_logits(**case, eos=eos)
        assert bad.tolist() == pc.NINE_BAD and pc.same_bits(y, case["logits"])


@pytest.mark.parametrize("what", sorted(pc.bad_causes()))
def test_each_bad_row_cause_leaves_its_row_untouched_and_the_rest_is_computed(what):
    good = pc.nine_rows()
    case = pc.changed(good, pc.bad_causes()[what])
    want, _ = lg_random.penalize_logits(**good, eos=pc.NINE_EOS)
    y, bad = lg_random.penalize_logits(**case, eos=pc.NINE_EOS)
    assert bad.tolist() == [r in (4, 6) for r in range(9)]
    assert pc.same_bits(y[4], good["logits"][4]) and pc.same_bits(np.delete(y, 4, axis=0), np.delete(want, 4, axis=0))
    # the op: in place, the good rows finished, then IndexError
    logits, operands = tensors(case)
    with pytest.raises(IndexError):
        logits.penalize_rows(*operands, eos=pc.NINE_EOS)
    assert pc.same_bits(logits.numpy(), y)


def test_penalize_logits_refuses_other_operands():
    case = pc.nine_rows()
    for eos in (-1, pc.V, 1.5):
        with pytest.raises(ValueError):
            lg_random.penalize_logits(**case, eos=eos)
    for bad in (dict(logits=case["logits"].astype(np.float16)), dict(logits=case["logits"][0]), dict(table=case["table"][:, :3]), dict(index=case["index"][:8]),
                dict(prompt_len=case["prompt_len"][:4]), dict(out=case["out"][:4]), dict(prompts=case["prompts"][0])):
        with pytest.raises(ValueError):
            lg_random.penalize_logits(**dict(case, **bad))


# ---- the op ---------------------------------------------------------------------------------------------------------------------

def test_penalize_rows_is_in_place_and_returns_its_tensor():
    case = pc.changed(pc.nine_rows(), dict(index=(6, 2)))                  # no bad row
    want, bad = lg_random.penalize_logits(**case, eos=pc.NINE_EOS)
    assert not bad.any()
    logits, operands = tensors(case)
    assert logits.penalize_rows(*operands, eos=pc.NINE_EOS) is logits and pc.same_bits(logits.numpy(), want)
    # (rows, 1, V), and rows of a wider tensor: the bytes between the rows are unchanged
    wide = np.full((9, 1, pc.V + 6), -7.0, np.float32)
    wide[:, 0, 3:3 + pc.V] = case["logits"]
    t = tensor(wide)
    view = CpuTensor.from_numpy(t.data[:, :, 3:3 + pc.V], requires_grad=False)
    assert view.penalize_rows(*operands, eos=pc.NINE_EOS) is view
    assert pc.same_bits(t.numpy()[:, 0, 3:3 + pc.V], want) and (t.numpy()[:, 0, :3] == -7).all() and (t.numpy()[:, 0, 3 + pc.V:] == -7).all()
    # float64 logits - the float64 tapes of the tests - in float64
    t = tensor(case["logits"].astype(np.float64))
    t.penalize_rows(*operands, eos=pc.NINE_EOS)
    assert pc.same_bits(t.numpy(), lg_random.penalize_logits(**dict(case, logits=case["logits"].astype(np.float64)), eos=pc.NINE_EOS)[0])
    # a tensor that requires a gradient is refused, and so are other operands
    with pytest.raises(AssertionError, match="gradient"):
        CpuTensor.from_numpy(case["logits"].copy(), requires_grad=True).penalize_rows(*operands)
    logits = tensor(case["logits"])
    names = ("table", "index", "prompts", "prompt_len", "out", "out_len")
    for bad in (dict(table=tensor(np.zeros((5, 8), np.int32))), dict(table=tensor(case["table"].astype(np.int64))), dict(index=tensor(case["index"][:8])),
                dict(prompts=tensor(case["prompts"][:4])), dict(out_len=tensor(case["out_len"].astype(np.int64))), dict(eos=pc.V), dict(eos=-1)):
        with pytest.raises(ValueError):
            logits.penalize_rows(**dict(dict(zip(names, operands)), **bad))
    for shape in ((9, 2, pc.V), (pc.V,)):
        with pytest.raises(ValueError):
            tensor(np.zeros(shape, np.float32)).penalize_rows(*operands)
    with pytest.raises(ValueError):
        tensor(np.zeros((9, pc.V), np.int32)).penalize_rows(*operands)
    # a history wider than the launch keeps in LDS is refused by name, with the numbers, on this backend too
    wide = list(operands)
    wide[2], wide[4] = tensor(np.zeros((5, 4000), np.int32)), tensor(np.zeros((5, 97), np.int32))
    with pytest.raises(AssertionError, match=r"4000 \+ 97"):
        logits.penalize_rows(*wide)
    assert pc.same_bits(logits.numpy(), case["logits"])


# ---- the pool -------------------------------------------------------------------------------------------------------------------

def pool_arguments(model, slots=3):
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], slots, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    rows = sc.prompts()
    padded = np.zeros((7, max(map(len, rows))), np.int32)
    for r, p in enumerate(rows):
        padded[r, :len(p)] = p
    return cache, padded, [len(p) for p in rows], [sc.BUDGET] * 7, 4


@pytest.fixture(scope="module")
def model():
    return dc.make_model(CpuTensor, seed=sc.SEED)


def test_request_pool_uploads_the_table_once_and_refuses_others(model):
    arguments = pool_arguments(model)
    pool = nn.RequestPool(*arguments, penalties=pc.table())
    assert isinstance(pool.penalties, CpuTensor) and pool.penalties.dtype == np.int32 and pool.sampling is None
    np.testing.assert_array_equal(pool.penalties.numpy(), pc.table())
    assert nn.RequestPool(*arguments).penalties is None
    for bad in (pc.table()[:6], pc.table().astype(np.int64), pc.table()[:, :3], np.zeros((7, 8), np.int32)):
        with pytest.raises(AssertionError, match="penalties"):
            nn.RequestPool(*arguments, penalties=bad)
    # P + G <= 4096: asserted with the numbers
    cache, padded, lengths, budgets, chunk = arguments
    long = nn.KVCache(1, 1, 8192, 8, like=model.cls.predictions.bias, per_row=True)
    wide = np.zeros((1, 4000), np.int32)
    with pytest.raises(AssertionError, match=r"4000 \+ 97"):
        nn.RequestPool(long, wide, [4000], [97], 4, penalties=lg_random.penalty_table(1.3))
    assert nn.RequestPool(long, wide, [4000], [96], 4, penalties=lg_random.penalty_table(1.3)).penalties is not None
    assert nn.RequestPool(long, wide, [4000], [97], 4).penalties is None


# ---- serve ----------------------------------------------------------------------------------------------------------------------

def test_the_references_have_no_near_tie_and_the_penalties_change_the_tokens():
    plain = sc.greedy_reference()[0]
    tokens = pc.reference("greedy")                                        # asserts the rule over all 42 steps, prints d
    changed = [r for r in range(7) if tokens[r].tolist() != plain[r].tolist()]
    print("greedy under penalties: %s, changed requests %s" % ([t.tolist() for t in tokens], changed))
    assert changed == [1, 2, 3, 4, 6] and tokens[1].tolist() == [86, 18, 10, 41, 90, 86]
    # min_new moves request 3's first token off the end-of-sequence id and request 6's stop from its fifth to its sixth token
    assert plain[3][0] == pc.EOS and tokens[3][0] != pc.EOS and pc.EOS not in tokens[3][:2].tolist()
    assert plain[6].tolist().index(pc.EOS) == 4 and tokens[6].tolist().index(pc.EOS) == 5
    for mode in pc.MODES:
        want, want_len = pc.expected(mode)
        print("%s: emitted %s" % (mode, want_len.tolist()))
        assert (want_len == pc.BUDGET).any() and (want_len < pc.BUDGET).any()        # both kinds of stop occur
    assert [t.tolist() for t in pc.reference("sampled")] != [t.tolist() for t in tokens]
    pc.reference("greedy", True)                                           # the prefixed prompts of the shared-prefix run, greedy


@pytest.mark.parametrize("mode", pc.MODES)
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_gives_each_request_the_tokens_of_its_run_alone(model, slots, chunk, mode):
    want, want_len = pc.expected(mode)
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, **pc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True and stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)
    assert stats.get("per_request_sampling") is (True if mode == "sampled" else None)


@pytest.mark.parametrize("mode", pc.MODES)
def test_serve_on_the_other_routes(model, mode):
    want, want_len = pc.expected(mode)
    lengths = [len(p) for p in sc.prompts()]
    # token-packed
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, token_budget=6, **pc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True and stats["steps"] == spc.simulate_packed(lengths, want_len, 3, 4, 6)
    # paged
    out, out_len, stats, cache = pg.run_serve(CpuTensor, 3, 4, 3 * pg.MAX_BLOCKS, model=model, poll=1, **pc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True
    pg.assert_no_block_leaked(cache)


@pytest.mark.parametrize("shared", [0, pg.PREFIX])
def test_serve_paged_with_and_without_a_shared_prefix(model, shared):
    """the prefixed prompts, greedy (their sampled run has a near-tie under the rule and is not used)"""
    want, want_len = pc.expected("greedy", True)
    F = 2 if shared else 0
    out, out_len, stats, cache = pg.run_serve(CpuTensor, 3, 4, F + 3 * pg.MAX_BLOCKS, model=model, poll=1, rows=pg.prefixed_prompts(),
                                              **pc.options("greedy", **({"shared_prefix": shared} if shared else {})))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["penalties"] is True and stats["prefix_blocks"] == F
    pg.assert_no_block_leaked(cache, F)


def test_the_bf16_route_gives_the_same_tokens_on_another_schedule(model):
    """its logits are the rounded model's: no reference equality, but schedule independence"""
    for mode in pc.MODES:
        runs = [pb.run_serve(CpuTensor, slots, chunk, slots * pg.MAX_BLOCKS, model=model, rows=sc.prompts(), poll=1, **pc.options(mode))
                for slots, chunk in ((3, 4), (7, 16))]
        np.testing.assert_array_equal(runs[0][1], runs[1][1])
        np.testing.assert_array_equal(runs[0][0], runs[1][0])
        assert runs[0][2]["penalties"] is True and not np.array_equal(runs[0][0], sc.expected(sc.greedy_reference()[0], sc.BUDGET, sc.EOS)[0])


def test_neutral_keywords_build_no_table_and_give_the_parents_tokens(model, monkeypatch):
    called = []
    op = CpuTensor.penalize_rows
    monkeypatch.setattr(CpuTensor, "penalize_rows", lambda self, *a, **kw: (called.append(1), op(self, *a, **kw))[1])
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    for neutral in (dict(), dict(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0),
                    dict(repetition_penalty=[1.0] * 7, presence_penalty=[0] * 7, min_new_tokens=[0] * 7)):
        out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, **neutral)
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(out_len, want_len)
        assert "penalties" not in stats and called == []
    # one keyword alone takes the route; a scalar broadcasts
    first = sc.run_serve(CpuTensor, 3, 4, model=model, repetition_penalty=1.3)
    assert first[2]["penalties"] is True and len(called) == first[2]["steps"]
    again = sc.run_serve(CpuTensor, 7, 16, model=model, repetition_penalty=[1.3] * 7)
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[0][1], pc.expected("greedy")[0][1])          # request 1 of the parameter set has exactly these
    # the global temperature= route takes the launch too; min_new_tokens without eos_token_id is accepted and does nothing
    del called[:]
    light.manual_seed(5)
    _, _, stats = sc.run_serve(CpuTensor, 3, 4, model=model, temperature=0.9, top_k=20, top_p=0.95, frequency_penalty=0.3)
    assert stats["penalties"] is True and len(called) == stats["steps"] and light.random.get_state("cpu") == (5, stats["steps"])
    a = sc.run_serve(CpuTensor, 3, 4, model=model, eos=None, min_new_tokens=4)
    b = sc.run_serve(CpuTensor, 3, 4, model=model, eos=None)
    np.testing.assert_array_equal(a[0], b[0])
    assert a[2]["penalties"] is True
    for bad in (dict(repetition_penalty=[1.3] * 6), dict(repetition_penalty=0.0), dict(presence_penalty=float("nan")), dict(min_new_tokens=-1)):
        with pytest.raises((AssertionError, ValueError)):
            sc.run_serve(CpuTensor, 3, 4, model=model, **bad)
