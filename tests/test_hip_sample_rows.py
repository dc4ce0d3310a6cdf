"""lg_sample_rows_f32 (csrc/sample_rows.hip) behind `HipTensor.sample_rows`, and per-request sampling through examples/bert.py's
`serve(..., seeds=)`.

The launch runs the row body of lg_sample_f32 (csrc/sample_body.h) and only fetches (inv_T, top_k, top_p, the Philox counter and
key) from elsewhere, so wherever the two are handed equal values their tokens are EQUAL - no band: row g of the call with draws
== 0 of a stream seeded s takes the counter (g, 0) and the key s, which is what a table row with the seed s and the counter g
takes.  Against the float64 definition (`random.sample_tokens_rows`) a token lies in the row's acceptance band
(tests/sample_cases.py) and equals it where the band is one token.  `serve` is held against the float64 run of every request
ALONE (tests/sample_rows_cases.py), whose near-ties are ruled out from the references alone."""
import ctypes
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from test_hip_sample import lds_limit, last_plan
from test_hip_serve import recorder                                       # noqa: F401 (a fixture)
from test_sample_cpu import degenerate_rows
from test_sample_rows_cpu import bad_tables
import decode_cases as dc
import paged_bf16_cases as pb
import paged_cases as pg
import sample_cases as smp
import sample_rows_cases as rc
import serve_cases as sc
import serve_packed_cases as pc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
SEEDS, COUNTERS = (7, 2 ** 63 + 5), (0, 3)


def up(hip, a, dtype=None):
    return hip.from_numpy(np.ascontiguousarray(a, dtype), requires_grad=False)


def width(hip, V):
    return lds_limit(hip) + (V == "L+1") if isinstance(V, str) else V


# ---- bit for bit against lg_sample_f32 --------------------------------------------------------------------------------------------

# every width with int32 tokens; int64 tokens and a pitch of its own at one width per kernel and thread count
BITWISE = [(V, "int32") for V in (1, 2, 33, 257, 4097, 30522, "L", "L+1")] + [(V, form) for form in ("int64", "pitched") for V in (33, 30522, "L+1")]


@pytest.mark.parametrize("V,form", BITWISE, ids=["V%s-%s" % c for c in BITWISE])
def test_tokens_equal_the_global_launch_given_the_same_numbers(hip, V, form):
    V, kernel = width(hip, V), 1 if V == "L+1" else 0
    x = smp.logits(V, 2)
    dtype = np.int64 if form == "int64" else np.int32
    if form == "pitched":
        wide = np.zeros((2, V + 6), np.float32)
        wide[:, 3:3 + V] = x
        device = up(hip, wide)[:, 3:3 + V]                               # a pitch of its own, rows off 16 bytes
    else:
        device = up(hip, x)
    pairs = [(i, g) for i in range(len(smp.PARAMETERS)) for g in COUNTERS]                  # a table row per (parameters, g)
    t, k, p = zip(*[smp.PARAMETERS[i] for i, _ in pairs])
    counter = up(hip, [g for _, g in pairs], np.int32)
    for seed in SEEDS:
        table = up(hip, lg_random.sampling_table(t, k, p, seed))
        got = np.stack([device.sample_rows(table, up(hip, [j, j], np.int32), counter, dtype=dtype).numpy() for j in range(len(pairs))])
        assert got.dtype == dtype and got.shape == (len(pairs), 2) and last_plan() == [kernel, 256 if V <= 8192 else 1024, 10, 1 if kernel == 0 and V >= 7 else 0]
        for r in range(2):
            copies = up(hip, np.repeat(x[r:r + 1], max(COUNTERS) + 1, axis=0))            # row g of call 0 draws the number of counter g
            for i, parameters in enumerate(smp.PARAMETERS):
                light.manual_seed(seed)
                want = copies.sample(*parameters, dtype=dtype).numpy()
                for g in COUNTERS:
                    assert got[pairs.index((i, g)), r] == want[g], "V %d, %s, seed %d, g %d, row %d" % (V, parameters, seed, g, r)


# ---- one launch, every kind of row ------------------------------------------------------------------------------------------------

def test_nine_rows_against_the_definition(hip):
    V, n = 257, 5
    x = smp.logits(V, 9).copy()
    x[0] = np.nan                                                         # the free row: never read
    x[3] = x[2]                                                           # rows 2 and 3 share table row 3 and its counter
    index = np.array([n if i == "n" else i for i in rc.INDEX], np.int32)
    t, k, p = zip(*smp.PARAMETERS[:n])
    seeds = [11, 2 ** 64 - 1, 2 ** 32, 5, 2 ** 63]
    table, counter = lg_random.sampling_table(t, k, p, seeds), np.array([2, 0, 7, 1, 40], np.int32)
    want, bad = lg_random.sample_tokens_rows(x, table, index, counter)
    assert bad.tolist() == [False] * 6 + [True] + [False] * 2
    light.manual_seed(9)
    got = up(hip, x).sample_rows(up(hip, table), up(hip, index), up(hip, counter))
    with pytest.raises(IndexError):
        HipDevice.synchronize()                                           # the row beyond the table raised the flag ...
    HipDevice.synchronize()
    got = got.numpy()                                                     # ... and every other row was computed
    assert got.dtype == np.int32 and got[0] == 0 and got[6] == 0 and got[2] == got[3]
    singles = 0
    for r, i in enumerate(index):
        if 0 <= i < n:
            band = smp.acceptable(x[r], rc.uniform(seeds[i], int(counter[i])), *smp.PARAMETERS[i])
            assert got[r] in band, (r, int(got[r]), band[:8].tolist())
            if band.size == 1:
                singles += 1
                assert got[r] == want[r], (r, int(got[r]), int(want[r]))
    print("%d of 7 drawn rows have a one-token band; tokens %s, the definition's %s" % (singles, got.tolist(), want.tolist()))
    assert singles == 7                                                   # (from the float64 definition alone: every band is one token)
    assert light.random.get_state("hip") == (9, 0)


def test_greedy_rows_answer_argmax_on_degenerate_rows_too(hip):
    x, _ = degenerate_rows()
    x = np.concatenate([x, smp.logits(33, 8)[4:]])                        # ... and on ordinary ones, ties included
    t = up(hip, x)
    table = up(hip, lg_random.sampling_table([0, 0.8], [0, 5], [1.0, 0.9], [1, 2]))
    want = t.argmax(-1).numpy()
    np.testing.assert_array_equal(want, np.argmax(x, axis=1))
    got = t.sample_rows(table, up(hip, np.zeros(8), np.int32), up(hip, [3, 0], np.int32), dtype=np.int64).numpy()
    np.testing.assert_array_equal(got, want)
    for g in range(4):                                                    # a sampled row over a degenerate row: its argmax, never a -inf logit
        got = t.sample_rows(table, up(hip, np.ones(8), np.int32), up(hip, [0, g], np.int32)).numpy()
        np.testing.assert_array_equal(got[:3], want[:3])
        assert got[3] % 2 == 1
    wide = smp.logits(lds_limit(hip) + 1, 2)                              # the memory kernel
    got = up(hip, wide).sample_rows(table, up(hip, [0, 0], np.int32), up(hip, [0, 0], np.int32)).numpy()
    np.testing.assert_array_equal(got, np.argmax(wide, axis=1))
    HipDevice.synchronize()                                               # no status flag was raised


@pytest.mark.parametrize("what", sorted(bad_tables()))
def test_a_bad_table_row_answers_0_raises_the_flag_and_the_others_are_computed(hip, what):
    x = smp.logits(33, 4).copy()
    x[1] = np.nan                                                         # the bad row returns before any load of its logits
    table, counter = bad_tables()[what]
    index = np.array([0, 1, 2, 0], np.int32)
    want, bad = lg_random.sample_tokens_rows(x, table, index, counter)
    assert bad.tolist() == [False, True, False, False]
    got = up(hip, x).sample_rows(up(hip, table), up(hip, index), up(hip, counter))
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    got = got.numpy()
    assert got[1] == 0
    for r in (0, 3):                                                      # (0.9, 20, 0.95) at g = 0
        assert got[r] in smp.acceptable(x[r], rc.uniform(1, 0), 0.9, 20, 0.95)
    assert got[2] == want[2] == np.argmax(x[2])                           # the greedy row


def test_the_c_abi_refuses_bad_arguments_before_anything_is_launched(hip):
    lib = hiplib.lib()
    x = up(hip, smp.logits(33, 5))
    table, index, counter = up(hip, lg_random.sampling_table([1.0, 0.0])), up(hip, [0, 1, -1, 0, 1], np.int32), up(hip, [0, 2], np.int32)
    out = hip.from_numpy(np.full(6, -7, np.int64), requires_grad=False)
    good = dict(logits=x.ptr, rows=5, cols=33, row_pitch=33, table=table.ptr, n=2, index=index.ptr, counter=counter.ptr, out=out.ptr, out_itemsize=8)

    def call(**change):
        return lib.lg_sample_rows_f32(*dict(good, **change).values())
    light.manual_seed(2)
    refused = [dict(logits=None), dict(table=None), dict(index=None), dict(counter=None), dict(out=None),
               dict(logits=x.ptr + 2), dict(table=table.ptr + 4), dict(table=table.ptr + 8), dict(index=index.ptr + 1), dict(counter=counter.ptr + 2),
               dict(out=out.ptr + 4), dict(out=out.ptr + 2, out_itemsize=4),
               dict(rows=-1), dict(rows=(1 << 24) + 1), dict(cols=0), dict(cols=1 << 31, row_pitch=1 << 31), dict(row_pitch=32), dict(n=0), dict(n=-3),
               dict(out_itemsize=2), dict(out_itemsize=16), dict(out_itemsize=0),
               dict(out=x.ptr), dict(out=x.ptr + 4 * (4 * 33 + 32), out_itemsize=4), dict(out=table.ptr), dict(out=table.ptr + 56),
               dict(out=index.ptr, out_itemsize=4), dict(out=counter.ptr, rows=1), dict(out=counter.ptr + 4, rows=1, out_itemsize=4)]
    for change in refused:
        assert call(**change) == LG_EINVAL and b"lg_sample_rows_f32" in lib.lg_last_error(), change
        assert last_plan()[0] == -1
    HipDevice.synchronize()
    assert (out.numpy() == -7).all(), "a refused call wrote tokens"
    assert call(rows=0) == 0 and last_plan()[0] == -1                     # no rows: nothing is launched
    assert call() == 0 and last_plan() == [0, 256, 10, 1]
    assert (out.numpy()[:5] >= 0).all() and out.numpy()[2] == 0 and out.numpy()[5] == -7
    assert light.random.get_state("hip") == (2, 0)
    # through the op
    with pytest.raises(TypeError):
        up(hip, np.zeros((5, 33), np.int32)).sample_rows(table, index, counter)
    for bad in (dict(table=up(hip, np.zeros((2, 7)), np.int32)), dict(index=up(hip, np.zeros(4), np.int32)), dict(counter=up(hip, np.zeros(3), np.int32)),
                dict(counter=up(hip, np.zeros(2), np.int64)), dict(dtype=np.int16)):
        with pytest.raises(ValueError):
            x.sample_rows(**dict(dict(table=table, index=index, counter=counter), **bad))
    empty = up(hip, np.zeros((0, 33), np.float32)).sample_rows(table, up(hip, np.zeros(0), np.int32), counter)
    assert tuple(empty.shape) == (0,) and empty.dtype == np.int32


# ---- serve ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model(hip):
    return dc.make_model(hip, seed=sc.SEED)


def run_route(hip, route, slots, chunk, model, **options):
    """(out, out_len, stats, the steps of the schedule by hand) of the per-request run over one of the three routes"""
    want_len = rc.expected()[1]
    lengths = [len(p) for p in sc.prompts()]
    if route == "packed":
        out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, token_budget=slots + 3, **rc.options(), **options)
        return out, out_len, stats, pc.simulate_packed(lengths, want_len, slots, chunk, slots + 3)
    if route == "paged":
        out, out_len, stats, cache = pg.run_serve(hip, slots, chunk, slots * pg.MAX_BLOCKS, model=model, poll=1, **rc.options(), **options)
        pg.assert_no_block_leaked(cache)
        return out, out_len, stats, pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, slots * pg.MAX_BLOCKS)
    out, out_len, stats = sc.run_serve(hip, slots, chunk, model=model, poll=1, **rc.options(), **options)
    return out, out_len, stats, sc.simulate(lengths, want_len, slots, chunk)


@pytest.mark.parametrize("captured", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("route", ["plain", "packed", "paged"])
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_on_hip_gives_each_request_the_tokens_of_its_run_alone(hip, model, slots, chunk, route, captured):
    want, want_len = rc.expected()
    light.manual_seed(77)
    graph = HipGraph() if captured else None
    out, out_len, stats, steps = run_route(hip, route, slots, chunk, model, graph=graph)
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True and stats["steps"] == steps
    assert light.random.get_state("hip") == (77, 0), "the per-request route read or advanced the generator"
    if captured:
        assert graph.kernel_count() > 0
        graph.destroy()


def test_seeds_none_is_the_seed_of_the_device_generator(hip, model):
    want, want_len = rc.expected()
    light.manual_seed(rc.BASE)
    out, out_len, stats = sc.run_serve(hip, 3, 4, model=model, **dict(rc.options(), seeds=None))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True and light.random.get_state("hip") == (rc.BASE, 0)


def test_the_bf16_paged_route_agrees_with_the_numpy_backend_schedule_for_schedule(hip, model):
    """its logits are the rounded model's: no reference equality, but the tokens of CpuTensor's run of the same schedule"""
    for slots, chunk in ((3, 4), (7, 16)):
        runs = [pb.run_serve(T, slots, chunk, slots * pg.MAX_BLOCKS, model=m, rows=sc.prompts(), poll=1, **rc.options())
                for T, m in ((hip, model), (CpuTensor, None))]
        np.testing.assert_array_equal(runs[0][1], runs[1][1])
        np.testing.assert_array_equal(runs[0][0], runs[1][0])
        assert runs[0][2]["steps"] == runs[1][2]["steps"] and runs[0][2]["per_request_sampling"] is True


def steps_of(calls, commit="lg_serve_commit_i32"):
    per_step, step = [], []
    for name in calls:
        if name != "lg_sync" and not name.startswith("lg_graph_"):
            step.append(name)
            if name == commit:
                per_step.append(step)
                step = []
    assert step == []
    return per_step


def test_the_host_reads_the_poll_word_only_and_the_step_is_the_sampled_step_with_one_name_exchanged(hip, model, recorder):
    want, want_len = rc.expected()

    def serve(graph=None, **options):
        cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
        del recorder.calls[:], recorder.reads[:]
        (out, _), stats = dc.bert.serve(model, sc.prompts(), sc.BUDGET, slots=3, chunk=4, eos_token_id=sc.EOS, pad_token_id=sc.PAD, cache=cache, poll=4,
                                        graph=graph, **options)
        return out, stats["steps"], list(recorder.calls), list(recorder.reads)
    light.manual_seed(rc.BASE)
    out, steps, calls, reads = serve(**rc.options())
    assert steps % 4 == 0 and reads == [4] * (steps // 4)                 # one int32 word per poll, nothing else: not even the seed
    np.testing.assert_array_equal(out.numpy(), want)
    new = steps_of(calls)
    assert len(new) == steps + 1 and all(s == new[1] for s in new[2:]), "a step's launches depend on what the slots hold"
    _, old_steps, calls, _ = serve(temperature=0.9, top_k=20, top_p=0.95)
    old = steps_of(calls)
    assert new[0] == old[0] and new[1] == ["lg_sample_rows_f32" if c == "lg_sample_f32" else c for c in old[1]]
    assert new[1].count("lg_sample_rows_f32") == 1 and old[1].count("lg_sample_f32") == 1 and "lg_sample_f32" not in new[1]
    assert light.random.get_state("hip") == (rc.BASE, old_steps)          # only the old route took calls of the stream
    # the same under capture: the entries recorded for the one captured step, and the kernels of the graph
    graphs = HipGraph(), HipGraph()
    captured_new = steps_of(serve(graph=graphs[0], **rc.options())[2])
    captured_old = steps_of(serve(graph=graphs[1], temperature=0.9, top_k=20, top_p=0.95)[2])
    assert captured_new[2] == new[1] and captured_old[2] == old[1] and len(captured_new) == 3
    print("launch entries of one serving step: %d; kernels of the captured step: %d per request, %d with one parameter set" % (
        len(new[1]), graphs[0].kernel_count(), graphs[1].kernel_count()))
    assert graphs[0].kernel_count() == graphs[1].kernel_count()
    for g in graphs:
        g.destroy()
