"""lg_logprob_rows_f32 (csrc/logprob.hip) behind `HipTensor.logprob_rows`, and per-token log-probabilities through
examples/bert.py's `serve(logprobs=)`.

The launch is held against the float64 definition (`random.token_logprobs_rows`): the ids of the alternatives equal - they are
ordered by the float32 logits themselves, which both sides read -, the values within the project's 1e-5 max(1, |want|), -inf and
NaN exact; and against itself bit for bit: its sum of exponentials is a sum of integers, so neither the run, nor the place of a
row in the launch, nor the rows next to it may change a bit.  `serve` is held against the float64 run of every request ALONE
(tests/logprob_cases.py) within the bounds of the numpy backend's test."""
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import random as lg_random
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
from test_hip_sample_rows import steps_of
import decode_cases as dc
import logprob_cases as lc
import paged_bf16_cases as pb
import paged_cases as pg
import serve_cases as sc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
NAMES = ("token", "want", "index", "counter")
LIMIT = lg_random.LOGPROB_LDS_COLS
WIDTHS = (1, 2, 63, 64, 65, 101, 257, 4099, 30522, LIMIT, LIMIT + 1)


def up(hip, a, dtype=None):
    return hip.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)


def launch(hip, case, rows=slice(None), start=None, n_max=lc.N_MAX, shape=None):
    """one `logprob_rows` over the rows given, from `start` (default: the fills): the three outputs as numpy, after a
    synchronisation that the caller's bad rows make raise"""
    logits, token, index = case["logits"][rows], case["token"][rows], case["index"][rows]
    outs = [up(hip, a) for a in (lc.fills(len(case["want"]), n_max=n_max) if start is None else start)]
    x = up(hip, logits if shape is None else logits.reshape(shape))
    assert x.logprob_rows(up(hip, token), up(hip, case["want"]), up(hip, index), up(hip, case["counter"]), *outs) is None
    HipDevice.synchronize()
    return [t.numpy() for t in outs]


# ---- against the float64 definition ---------------------------------------------------------------------------------------------

def test_the_lds_limit_is_the_kernel_s(hip):
    assert hiplib.lib().lg_logprob_lds_cols() == LIMIT


@pytest.mark.parametrize("V", WIDTHS)
def test_nine_rows_of_every_kind_at_every_width(hip, V):
    case = lc.nine_rows(V)
    lc.assert_close_to_definition(launch(hip, case), case)


@pytest.mark.parametrize("rows", range(1, 10))
def test_launches_of_one_to_nine_rows(hip, rows):
    case = lc.nine_rows()
    part = dict(case, logits=case["logits"][:rows], token=case["token"][:rows], index=case["index"][:rows])
    lc.assert_close_to_definition(launch(hip, part), part)


@pytest.mark.parametrize("n_max", [1, 3])
def test_fewer_columns_of_alternatives(hip, n_max):
    case = lc.changed(lc.nine_rows(257), {})
    case["want"] = np.minimum(case["want"], n_max)
    lc.assert_close_to_definition(launch(hip, case, n_max=n_max), case, n_max=n_max)


def test_large_logits_and_a_wide_range(hip):
    """(x - m) - log S has no cancellation: logits around 1e4 and a range of hundreds keep the relative 1e-5"""
    rng = np.random.RandomState(3)
    x = (1e4 + 200 * rng.standard_normal((8, 4099))).astype(np.float32)
    x[4:] = (-1e4 + 5 * rng.standard_normal((4, 4099))).astype(np.float32)
    case = dict(logits=x, token=rng.randint(0, 4099, 8).astype(np.int32), want=np.full(8, 8, np.int32), index=np.arange(8, dtype=np.int32),
                counter=np.array(lc.COUNTER, np.int32))
    lc.assert_close_to_definition(launch(hip, case), case)


def test_a_middle_axis_and_rows_of_a_wider_tensor(hip):
    case = lc.nine_rows()
    want = launch(hip, case)
    got = launch(hip, case, shape=(9, 1, 101))
    assert all(lc.same_bits(a, b) for a, b in zip(got, want))
    wide = np.full((9, 101 + 6), np.nan, np.float32)
    wide[:, 3:104] = case["logits"]
    from lightgrad_amd.autograd.hip.ops import _idx_view
    t = up(hip, wide)
    outs = [up(hip, a) for a in lc.fills(8)]
    with light.no_grad():
        view = _idx_view(t, (slice(None), slice(3, 104)))                 # rows off 16 bytes, a pitch of its own
        view.logprob_rows(*(up(hip, case[k]) for k in NAMES), *outs)
    HipDevice.synchronize()
    assert all(lc.same_bits(o.numpy(), b) for o, b in zip(outs, want))
    assert lc.same_bits(t.numpy(), wide)                                  # the logits are only read
    with pytest.raises(TypeError):
        up(hip, case["logits"].astype(np.float64)).logprob_rows(*(up(hip, case[k]) for k in NAMES), *outs)
    with pytest.raises(AssertionError, match="dense"), light.no_grad():
        up(hip, case["logits"]).logprob_rows(*(up(hip, case[k]) for k in NAMES), _idx_view(up(hip, np.zeros((8, 8), np.float32)), (slice(None), slice(0, 4))),
                                             outs[1], outs[2])
    with pytest.raises(ValueError):
        up(hip, case["logits"]).logprob_rows(*(up(hip, case[k]) for k in NAMES), outs[0], outs[1], up(hip, np.zeros((8, 4, 8), np.float64)))


# ---- bit for bit ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [101, 30522, LIMIT + 1])
def test_the_launch_agrees_with_itself_bit_for_bit(hip, V):
    case = lc.changed(lc.nine_rows(V), {})
    case["token"][8] = int(np.argsort(-case["logits"][8], kind="stable")[0])           # row 8 (1 id): its token is the most likely one
    case["token"][1] = int(np.argsort(-case["logits"][1], kind="stable")[2])
    case["want"][0] = 3                                                                 # row 1: its token is the third alternative
    first = launch(hip, case)
    logprob, ids, top = first
    # the token's log-probability is the alternative's where the token is one
    hits = 0
    for r, i in enumerate(case["index"].tolist()):
        g = case["counter"][i] if i >= 0 else 0
        for k in np.flatnonzero(ids[i, g] == case["token"][r]) if i >= 0 and case["want"][i] > 0 else []:
            assert lc.same_bits(logprob[i, g:g + 1], top[i, g, k:k + 1]), (r, k)
            hits += 1
    assert hits >= 2
    # two runs agree
    assert all(lc.same_bits(a, b) for a, b in zip(launch(hip, case), first))
    # permuting the rows permutes nothing of the result: every row writes the cell of its request
    order = np.random.RandomState(V).permutation(9)
    assert all(lc.same_bits(a, b) for a, b in zip(launch(hip, case, rows=order), first))
    # each row is what a launch of that row alone gives
    alone = lc.fills(8)
    for r in range(9):
        alone = launch(hip, case, rows=slice(r, r + 1), start=alone)
    assert all(lc.same_bits(a, b) for a, b in zip(alone, first))


def test_fills_and_skipped_rows_keep_their_bytes(hip):
    """from outputs full of a pattern: only the cells the definition writes change"""
    case = lc.nine_rows()
    pattern = (np.full((8, lc.G), -7.5, np.float32), np.full((8, lc.G, lc.N_MAX), 12345, np.int32), np.full((8, lc.G, lc.N_MAX), np.float32(2.0 ** -130)))
    got = launch(hip, case, start=pattern)
    from_fills = launch(hip, case)
    _, ids, top, _ = lc.defined(case)
    written = (ids >= 0) | np.isnan(top)
    cell = np.zeros((8, lc.G), bool)
    cell[[0, 6, 1, 2, 7, 5, 4], [0, 2, 3, 1, 1, 3, 0]] = True            # the seven live rows' (request, column)
    for have, start, fresh, where in zip(got, pattern, from_fills, (cell, written, written)):
        assert lc.same_bits(have[~where], start[~where]) and lc.same_bits(have[where], fresh[where])


# ---- bad rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("what", sorted(lc.bad_causes()))
def test_a_bad_row_raises_the_flag_writes_nothing_and_the_others_are_right(hip, what):
    good = lc.nine_rows()
    case = lc.changed(good, lc.bad_causes()[what])
    assert lc.defined(case)[3].tolist() == [r == 8 for r in range(9)]
    outs = [up(hip, a) for a in lc.fills(8)]
    up(hip, case["logits"]).logprob_rows(*(up(hip, case[k]) for k in NAMES), *outs)
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    got = [t.numpy() for t in outs]
    lc.assert_close_to_definition(got, case)
    assert (got[0][4] == 0).all() and (got[1][4] == -1).all() and (got[2][4] == 0).all()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------

def test_the_c_abi_refuses_bad_arguments_before_anything_is_launched(hip):
    lib = hiplib.lib()
    case = lc.nine_rows()
    x = up(hip, case["logits"])
    t = {k: up(hip, case[k]) for k in NAMES}
    outs = [up(hip, a) for a in lc.fills(8)]
    good = dict(logits=x.ptr, rows=9, cols=101, row_pitch=101, token=t["token"].ptr, want=t["want"].ptr, n=8, index=t["index"].ptr, counter=t["counter"].ptr,
                logprob=outs[0].ptr, G=lc.G, top_ids=outs[1].ptr, top_logprob=outs[2].ptr, n_max=lc.N_MAX)

    def call(**change):
        return lib.lg_logprob_rows_f32(*dict(good, **change).values())
    pointers = ("logits", "token", "want", "index", "counter", "logprob", "top_ids", "top_logprob")
    refused = [{k: None} for k in pointers] + [{k: good[k] + 2} for k in pointers] + [
        dict(rows=-1), dict(rows=65536), dict(cols=0), dict(cols=1 << 31, row_pitch=1 << 31), dict(row_pitch=100), dict(n=0), dict(n=-3), dict(G=0), dict(G=-1),
        dict(n_max=0), dict(n_max=9), dict(n_max=-1),
        # an output that shares bytes with what the launch reads, or with another output
        dict(logprob=x.ptr), dict(logprob=x.ptr + 4 * (9 * 101 - 1)), dict(top_ids=t["token"].ptr), dict(top_logprob=t["want"].ptr), dict(top_ids=t["index"].ptr),
        dict(logprob=t["counter"].ptr), dict(top_ids=outs[0].ptr), dict(top_logprob=outs[1].ptr + 4 * (8 * lc.G * lc.N_MAX - 1)), dict(top_logprob=outs[0].ptr + 4)]
    for change in refused:
        assert call(**change) == LG_EINVAL and b"lg_logprob_rows_f32" in lib.lg_last_error(), change
    HipDevice.synchronize()
    assert all(lc.same_bits(o.numpy(), a) for o, a in zip(outs, lc.fills(8))), "a refused call wrote"
    assert call(rows=0, logits=None, cols=0) == 0                         # no rows: LG_OK before anything else
    assert all(lc.same_bits(o.numpy(), a) for o, a in zip(outs, lc.fills(8)))
    assert call() == 0
    HipDevice.synchronize()
    lc.assert_close_to_definition([o.numpy() for o in outs], case)


# ---- serve ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


def run_route(hip, model, route, graph, **options):
    if route == "plain":
        return sc.run_serve(hip, 3, 4, model=model, poll=1, graph=graph, **options)
    if route == "token_budget":
        return sc.run_serve(hip, 3, 4, model=model, poll=1, graph=graph, token_budget=6, **options)
    run = pg.run_serve if route == "num_blocks" else pb.run_serve
    out, out_len, stats, cache = run(hip, 3, 4, 3 * pg.MAX_BLOCKS, model=model, poll=1, graph=graph, rows=sc.prompts(), **options)
    pg.assert_no_block_leaked(cache)
    return out, out_len, stats


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("route", ["plain", "token_budget", "num_blocks", "bf16"])
def test_serve_on_hip_scores_each_request_as_its_run_alone(hip, model, route, captured):
    rounded = route == "bf16"
    tokens = pb.assert_rounded_margins_rule_out_ties(False) if rounded else sc.assert_margins_rule_out_ties()
    want, want_len = sc.expected(tokens, sc.BUDGET, sc.EOS)
    graph = HipGraph() if captured else None
    out, out_len, stats = run_route(hip, model, route, graph, logprobs=list(lc.MIXED))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert all(isinstance(t, hip) for t in stats["logprobs"].values())
    lc.assert_matches(lc.read_back(stats), lc.reference(lc.MIXED, rounded))
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


@pytest.mark.parametrize("slots,chunk", [(1, 16), (7, 1)])
def test_serve_on_hip_at_the_edges_of_the_schedule(hip, model, slots, chunk):
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, logprobs=3)
    np.testing.assert_array_equal(out, want)
    lc.assert_matches(lc.read_back(stats), lc.reference(3))


def test_kernel_counts_of_the_captured_step_and_the_host_reads_the_poll_word_only(hip, model, recorder):
    def serve(graph=None, **options):
        cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
        del recorder.calls[:], recorder.reads[:]
        (out, _), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4,
                                        graph=graph, **options)
        return out, stats, list(recorder.calls), list(recorder.reads)
    out, stats, calls, reads = serve(logprobs=3)
    assert stats["steps"] % 4 == 0 and reads == [4] * (stats["steps"] // 4)          # one int32 word per poll, nothing else
    new, plain = steps_of(calls), steps_of(serve()[2])
    assert all(s == new[1] for s in new[2:]), "a step's launches depend on what the slots hold"
    assert "lg_logprob_rows_f32" not in plain[1] and new[1].count("lg_logprob_rows_f32") == 1
    at = new[1].index("lg_logprob_rows_f32")
    assert new[1][:at] + new[1][at + 1:] == plain[1] and plain[1] == steps_of(serve(logprobs=None)[2])[1]
    print("the step behind its head: %s" % new[1][at - 2:])
    assert new[1][at + 1:] == ["lg_serve_commit_i32"]                     # behind the draw, in front of the commit
    graphs = [HipGraph() for _ in range(2)]
    stats = [serve(graph=g, **o)[1] for g, o in zip(graphs, ({}, dict(logprobs=3)))]
    counts = [g.kernel_count() for g in graphs]
    print("kernels of the captured step %d, with logprobs=3 %d" % tuple(counts))
    assert counts[1] == counts[0] + 1 and "logprobs" not in stats[0]
    lc.assert_matches(lc.read_back(stats[1]), lc.reference(3))
    for g in graphs:
        g.destroy()
