"""`random.token_logprobs_rows` - the float64 definition of per-token log-probabilities and top-n alternatives -,
`CpuTensor.logprob_rows`, `nn.RequestPool(logprobs=)` and `serve(logprobs=)` on the numpy backend.

The definition is held against a plain loop over the elements and against values worked out by hand; `serve` against the float64
run of every request ALONE (tests/logprob_cases.py): `top_ids` equal, the values within 200 x the float32 deviation, the fills
bit for bit - whatever slots, chunk, token_budget and paging are."""
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import logprob_cases as lc
import paged_cases as pg
import penalty_cases as pc
import sample_rows_cases as rc
import serve_cases as sc

NAMES = ("token", "want", "index", "counter")


def cpu(a):
    return CpuTensor.from_numpy(np.array(a), requires_grad=False)


def one_row(x, token, k, n_max=lc.N_MAX):
    """(logprob, top_ids (n_max,), top_logprob (n_max,)) of the definition for one row, in float64"""
    out = lc.fills(1, 1, n_max, np.float64)
    bad = lg_random.token_logprobs_rows(np.asarray(x, np.float32)[None, :], [token], [k], [0], [0], *out)
    assert not bad.any()
    return out[0][0, 0], out[1][0, 0], out[2][0, 0]


# ---- the definition -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 5, 101])
def test_the_definition_is_the_plain_loop(V):
    case = lc.nine_rows(V)
    got, want = lc.defined(case), lc.by_hand(case)
    assert not got[3].any() and not want[3].any()
    np.testing.assert_array_equal(got[1], want[1])
    for a, b in ((got[0], want[0]), (got[2], want[2])):
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b))
        np.testing.assert_allclose(a[~np.isnan(a)], b[~np.isnan(b)], rtol=0, atol=1e-12)
    # the float32 outputs of a pool are the float64 ones rounded once
    f32 = lc.defined(case, np.float32)
    assert lc.same_bits(f32[0], got[0].astype(np.float32)) and lc.same_bits(f32[2], got[2].astype(np.float32)) and (f32[1] == got[1]).all()


@pytest.mark.parametrize("V", [1, 2, 5, 101])
def test_an_all_equal_row(V):
    logprob, ids, top = one_row(np.full(V, -3.5), V - 1, 8)
    k = min(8, V)
    assert ids.tolist() == list(range(k)) + [-1] * (8 - k)
    np.testing.assert_allclose(top[:k], -np.log(V), rtol=0, atol=1e-15)
    assert logprob == top[0] and (top[k:] == 0).all() and not np.signbit(top[k:]).any()


def test_small_rows_by_hand():
    # V = 1: the only token is certain
    logprob, ids, top = one_row([7.0], 0, 3)
    assert logprob == 0 and ids.tolist() == [0] + [-1] * 7 and top[0] == 0
    # V = 2: log-probabilities of a logistic
    logprob, ids, top = one_row([0.0, np.log(3.0)], 0, 2)
    np.testing.assert_allclose([logprob, top[0], top[1]], [np.log(0.25), np.log(0.75), np.log(0.25)], rtol=0, atol=1e-7)
    assert ids[:2].tolist() == [1, 0]
    # -0.0 next to +0.0: equal values, the lower index first - whichever of the two it is
    for row in ([-1.0, -0.0, 0.0, -2.0, 0.0], [-1.0, 0.0, -0.0, -2.0, -0.0]):
        assert one_row(row, 0, 4)[1][:4].tolist() == [1, 2, 4, 0]
    # -inf entries: log-probability -inf, behind every finite value, lower index first among themselves; chosen: -inf
    logprob, ids, top = one_row([-np.inf, 1.0, -np.inf, 1.0], 2, 4)
    assert logprob == -np.inf and ids[:4].tolist() == [1, 3, 0, 2] and top[2] == -np.inf and top[3] == -np.inf
    np.testing.assert_allclose(top[:2], np.log(0.5), rtol=0, atol=1e-15)
    # V < k: the entries behind V keep their fill
    logprob, ids, top = one_row([0.5, 2.5, 1.5], 1, 8)
    assert ids.tolist() == [1, 2, 0, -1, -1, -1, -1, -1] and (top[3:] == 0).all() and logprob == top[0]
    # k = 0: the token's only
    logprob, ids, top = one_row([0.5, 2.5, 1.5], 2, 0)
    assert (ids == -1).all() and (top == 0).all() and logprob == one_row([0.5, 2.5, 1.5], 2, 3)[2][1]


def test_degenerate_and_skipped_rows():
    for row in ([1.0, np.nan, 2.0], [1.0, np.inf, 2.0], [-np.inf] * 3):
        logprob, ids, top = one_row(row, 0, 2)
        assert np.isnan(logprob) and ids.tolist() == [-1] * 8 and np.isnan(top[:2]).all() and (top[2:] == 0).all()
    case = lc.nine_rows()
    logprob, ids, top, bad = lc.defined(case)
    assert not bad.any() and np.isnan(case["logits"][0]).all() and np.isnan(case["logits"][2]).all()
    assert (logprob[3] == 0).all() and (ids[3] == -1).all() and (top[3] == 0).all()          # request 3 wants nothing: row 2 is skipped
    assert np.isnan(logprob[6, 2]) and np.isnan(top[6, 2, :5]).all() and (top[6, 2, 5:] == 0).all()
    assert logprob[1, 3] == -np.inf and ids[1, 3, :2].tolist() == [99, 100]                 # row 4: -0.0 at 99 in front of +0.0 at 100
    assert (logprob != 0).sum() == 7                                                          # one cell per live row, nothing else


@pytest.mark.parametrize("what", sorted(lc.bad_causes()))
def test_each_kind_of_bad_row(what):
    good = lc.nine_rows()
    case = lc.changed(good, lc.bad_causes()[what])
    want = lc.defined(good, np.float32)
    got = lc.fills(8)
    bad = lg_random.token_logprobs_rows(case["logits"], case["token"], case["want"], case["index"], case["counter"], *got)
    assert bad.tolist() == [r == 8 for r in range(9)]
    assert got[0][4, 1] == 0 and (got[1][4] == -1).all() and (got[2][4] == 0).all()          # nothing of the bad row's request is written ...
    keep = np.arange(8) != 4
    assert all(lc.same_bits(a[keep], b[keep]) for a, b in zip(got, want[:3]))                  # ... and the others are
    # the op: IndexError after the others are written
    outs = [cpu(a) for a in lc.fills(8)]
    with pytest.raises(IndexError, match=r"\[8\]"):
        cpu(case["logits"]).logprob_rows(*(cpu(case[k]) for k in NAMES), *outs)
    assert all(lc.same_bits(t.data, a) for t, a in zip(outs, got))


def test_the_op_on_cpu_tensors():
    case = lc.nine_rows()
    want = lc.defined(case, np.float32)
    for shape in ((9, 101), (9, 1, 101)):
        outs = [cpu(a) for a in lc.fills(8)]
        assert cpu(case["logits"].reshape(shape)).logprob_rows(cpu(case["token"].reshape(shape[:-1])), *(cpu(case[k]) for k in NAMES[1:]), *outs) is None
        assert all(lc.same_bits(t.data, a) for t, a in zip(outs, want[:3]))
    outs = [cpu(a) for a in lc.fills(8)]
    operands = {k: cpu(case[k]) for k in NAMES}
    for wrong in (dict(token=cpu(case["token"].astype(np.int64))), dict(want=cpu(case["want"][:7])), dict(index=cpu(case["index"][:8])),
                  dict(counter=cpu(case["counter"].astype(np.int64)))):
        with pytest.raises(ValueError):
            cpu(case["logits"]).logprob_rows(*dict(operands, **wrong).values(), *outs)
    with pytest.raises(ValueError):
        cpu(case["logits"]).logprob_rows(*operands.values(), outs[0], outs[1], cpu(np.zeros((8, 4, 8))))          # float64 scores
    with pytest.raises(ValueError):
        cpu(case["logits"]).logprob_rows(*operands.values(), *[cpu(a) for a in lc.fills(8, n_max=9)])
    assert all(lc.same_bits(t.data, a) for t, a in zip(outs, lc.fills(8)))
    with pytest.raises(ValueError):
        lg_random.logprob_want(9, 7)
    with pytest.raises(ValueError):
        lg_random.logprob_want([1, 2], 7)
    assert lg_random.logprob_want(lc.MIXED, 7).tolist() == [3, 0, 8, -1, 3, 8, -1] and lg_random.logprob_want(2, 3).tolist() == [2, 2, 2]


# ---- RequestPool ----------------------------------------------------------------------------------------------------------------

def test_request_pool_holds_the_outputs_with_their_fills():
    rows = sc.prompts()
    padded, lengths = np.stack([np.pad(p, (0, 9 - len(p))) for p in rows]), [len(p) for p in rows]
    cache = nn.KVCache(2, 3, sc.CAPACITY, 64, per_row=True)
    pool = nn.RequestPool(cache, padded, lengths, sc.BUDGETS, 4, logprobs=[3, 0, 5, -1, 3, 5, -1])
    assert pool.logprobs.numpy().tolist() == [3, 0, 5, -1, 3, 5, -1] and pool.logprobs.dtype == np.int32
    assert pool.logprob.shape == (7, 6) and pool.top_ids.shape == (7, 6, 5) and pool.top_logprob.shape == (7, 6, 5)
    assert pool.logprob.dtype == np.float32 and pool.top_ids.dtype == np.int32 and pool.top_logprob.dtype == np.float32
    assert lc.same_bits(pool.logprob.numpy(), np.zeros((7, 6), np.float32)) and (pool.top_ids.numpy() == -1).all() and \
        lc.same_bits(pool.top_logprob.numpy(), np.zeros((7, 6, 5), np.float32))
    assert nn.RequestPool(cache, padded, lengths, sc.BUDGETS, 4, logprobs=[0] * 7).top_ids.shape == (7, 6, 1)        # n = max(want, 1)
    plain = nn.RequestPool(cache, padded, lengths, sc.BUDGETS, 4)
    assert plain.logprobs is None and plain.logprob is None and plain.top_ids is None and plain.top_logprob is None
    for wrong in ([3] * 6, [9] * 7, [-2] * 7):
        with pytest.raises(ValueError):
            nn.RequestPool(cache, padded, lengths, sc.BUDGETS, 4, logprobs=wrong)


# ---- serve ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return dc.make_model(CpuTensor, seed=sc.SEED)


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_scores_each_request_as_its_run_alone(model, slots, chunk):
    tokens = sc.assert_margins_rule_out_ties()
    want, want_len = sc.expected(tokens, sc.BUDGET, sc.EOS)
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, logprobs=3)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert all(isinstance(t, CpuTensor) for t in stats["logprobs"].values()) and sorted(stats["logprobs"]) == ["token", "top", "top_ids"]
    assert stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)
    lc.assert_matches(lc.read_back(stats), lc.reference(3))


@pytest.mark.parametrize("route", ["plain", "token_budget", "num_blocks"])
def test_serve_with_a_want_per_request_on_every_route(model, route):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    if route == "num_blocks":
        out, out_len, stats, cache = pg.run_serve(CpuTensor, 3, 4, 3 * pg.MAX_BLOCKS, model=model, poll=1, logprobs=list(lc.MIXED))
        pg.assert_no_block_leaked(cache)
    else:
        out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, logprobs=list(lc.MIXED), **({"token_budget": 6} if route == "token_budget" else {}))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    got = lc.read_back(stats)
    assert got["top_ids"].shape == (7, 6, 8)
    lc.assert_matches(got, lc.reference(lc.MIXED))
    assert (got["token"][[3, 6]] == 0).all() and (got["top_ids"][[1, 3, 6]] == -1).all() and (got["top_ids"][0, :, 3:] == -1).all()


def test_serve_with_logprobs_zero_and_a_budget_per_request(model):
    """no eos: every request runs to its own budget; columns behind it hold the fills"""
    tokens = sc.assert_margins_rule_out_ties()
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, budgets=sc.BUDGETS, eos=None, poll=1, logprobs=0)
    np.testing.assert_array_equal(out_len, sc.BUDGETS)
    got = lc.read_back(stats)
    ref = lc.reference(0)
    assert got["top_ids"].shape == (7, 6, 1) and (got["top_ids"] == -1).all() and (got["top"] == 0).all()
    for r, budget in enumerate(sc.BUDGETS):
        full = lc.from_logits([lc.forwards()[0][r]], [tokens[r]], [budget], np.array([0]), 100, lc.forwards()[2])[0][0]
        assert np.abs(got["token"][r, :budget] - full[:budget]).max() <= ref[4] and (got["token"][r, budget:] == 0).all()


def test_serve_with_penalties_scores_the_penalised_logits(model):
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, logprobs=list(lc.MIXED), **pc.options("greedy"))
    np.testing.assert_array_equal(out, pc.expected("greedy")[0])
    d = pc.near_ties("greedy")[0]
    lc.assert_matches(lc.read_back(stats), lc.alone(model, out, out_len, lc.want_of(lc.MIXED), d, penalties=pc.table()))


def test_serve_with_per_request_sampling_scores_the_logits_in_front_of_the_temperature(model):
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, logprobs=list(lc.MIXED), **rc.options())
    np.testing.assert_array_equal(out, rc.expected()[0])
    d = rc.near_ties(rc.BASE)[0]
    got = lc.read_back(stats)
    lc.assert_matches(got, lc.alone(model, out, out_len, lc.want_of(lc.MIXED), d))
    sampled = [(r, g) for r in (0, 2, 4, 5) for g in range(out_len[r]) if got["top_ids"][r, g, 0] != out[r, g]]
    print("sampled tokens that are not their step's most likely id:", sampled)


def test_without_logprobs_nothing_is_built(model):
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1)
    assert "logprobs" not in stats
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, logprobs=None)
    assert "logprobs" not in stats
    with pytest.raises(ValueError):
        sc.run_serve(CpuTensor, 3, 4, model=model, logprobs=9)
    with pytest.raises(ValueError):
        sc.run_serve(CpuTensor, 3, 4, model=model, logprobs=[3] * 6)
