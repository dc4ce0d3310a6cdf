"""Per-request sampling on the numpy backend: `random.sampling_table`, the definition `random.sample_tokens_rows` behind
`CpuTensor.sample_rows`, and `serve(..., seeds=)` - every request under parameters and a random stream of its own, so that its
tokens are those of its run ALONE (sample_rows_cases.reference) whatever slots, chunk, token budget, paging and the order of the
queue are, with the backend's generator neither read by a step nor advanced."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import paged_cases as pg
import sample_cases as smp
import sample_rows_cases as rc
import serve_cases as sc
import serve_packed_cases as pc
from test_sample_cpu import degenerate_rows


def tensor(a):
    return CpuTensor.from_numpy(np.ascontiguousarray(a), requires_grad=False)


def i32(a):
    return tensor(np.asarray(a, np.int32))


# ---- the table ------------------------------------------------------------------------------------------------------------------

def test_sampling_table_against_words_written_out_by_hand():
    table = lg_random.sampling_table([0, 1.0, 0.5], [0, 7, 40], [1.0, 0.95, 0.5], [0, 2 ** 64 - 1, 2 ** 63 + 5])
    assert table.dtype == np.int32 and table.shape == (3, 8)
    u = table.view(np.uint32).tolist()
    # 1.0 = 0x3FF0000000000000, 0.95 = 0x3FEE666666666666, 0.5 = 0x3FE0000000000000; float32 1.0 = 0x3F800000, 2.0 = 0x40000000
    assert u[0] == [0, 0, 0, 0x3FF00000, 0, 0, 0, 0]                       # temperature 0: +0.0, GREEDY
    assert u[1] == [0x3F800000, 7, 0x66666666, 0x3FEE6666, 0xFFFFFFFF, 0xFFFFFFFF, 0, 0]
    assert u[2] == [0x40000000, 40, 0, 0x3FE00000, 5, 0x80000000, 0, 0]
    # inv_T is float32(1 / float64(T)), the value `sample_tokens` uses
    assert lg_random.sampling_table(0.7).view(np.uint32)[0, 0] == np.float32(1.0 / np.float64(0.7)).view(np.uint32)
    # scalars broadcast
    np.testing.assert_array_equal(lg_random.sampling_table(0.9, 20, 0.95, [3, 4]), lg_random.sampling_table([0.9, 0.9], [20, 20], [0.95, 0.95], [3, 4]))
    assert lg_random.sampling_table().shape == (1, 8)


@pytest.mark.parametrize("bad", [dict(temperature=-1.0), dict(temperature=-0.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
                                 dict(top_k=-1), dict(top_k=2 ** 31), dict(top_p=0.0), dict(top_p=1.5),
                                 dict(top_p=float("nan")), dict(seeds=-1), dict(seeds=2 ** 64), dict(temperature=[1.0, 2.0], seeds=[1, 2, 3]),
                                 dict(temperature=[]), dict(temperature=[[1.0]])], ids=str)
def test_sampling_table_refuses_each_bad_entry(bad):
    with pytest.raises(ValueError):
        lg_random.sampling_table(**bad)
    if all(np.ndim(v) == 0 for v in bad.values()):                          # ... and as the last entry behind two good ones
        with pytest.raises(ValueError):
            lg_random.sampling_table(**{k: [1, 1, v] for k, v in bad.items()})


# ---- the definition -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", [1, 2, 33, 257])
def test_rows_equal_sample_tokens_of_the_request_alone(V):
    seeds = [7, 2 ** 63 + 5, 0, 2 ** 64 - 1, 11, 12]
    t, k, p = zip(*smp.PARAMETERS)
    table = lg_random.sampling_table(t, k, p, seeds)
    x = smp.logits(V, 6)
    for g in (0, 1, 5):
        tokens, bad = lg_random.sample_tokens_rows(x, table, np.arange(6), np.full(6, g))
        assert tokens.dtype == np.int64 and not bad.any()
        for i in range(6):
            want = lg_random.sample_tokens(seeds[i], 0, np.repeat(x[i:i + 1], g + 1, axis=0), *smp.PARAMETERS[i])[g]
            assert tokens[i] == want, (V, g, i)
    # a row's answer depends on its table row and counter alone: permuted rows, a counter per table row
    order = np.array([4, 0, 5, 5, 2, 1])
    counter = np.array([0, 3, 1, 9, 2, 5])
    tokens, _ = lg_random.sample_tokens_rows(x, table, order, counter)
    for r, i in enumerate(order):
        want = lg_random.sample_tokens(seeds[i], 0, np.repeat(x[r:r + 1], counter[i] + 1, axis=0), *smp.PARAMETERS[i])[counter[i]]
        assert tokens[r] == want


def test_the_uniform_of_a_row_is_the_gth_number_of_its_own_stream():
    for seed in (0, 7, 2 ** 64 - 1):
        u = lg_random.sample_uniforms(seed, 0, 9)
        assert [lg_random._row_uniform(seed, g) for g in range(9)] == u.tolist()


def test_a_free_row_over_nan_answers_0_and_greedy_rows_answer_argmax():
    x, _ = degenerate_rows()
    table = lg_random.sampling_table([0, 0.8], [0, 5], [1.0, 0.9], [1, 2])
    # greedy over every degenerate row (and the one that is not) equals argmax
    got = tensor(x).sample_rows(i32(table), i32([0, 0, 0, 0]), i32([0, 4]))
    assert got.dtype == np.int32 and tuple(got.shape) == (4,) and not got.requires_grad
    np.testing.assert_array_equal(got.numpy(), np.argmax(x, axis=1))
    assert got.numpy()[:3].tolist() == [16, 7, 0]
    # a sampled row over a degenerate row answers argmax too, and never a -inf logit
    for g in range(8):
        sampled = tensor(x).sample_rows(i32(table), i32([1, 1, 1, 1]), i32([0, g]), dtype=np.int64).numpy()
        assert sampled.dtype == np.int64
        np.testing.assert_array_equal(sampled[:3], np.argmax(x, axis=1)[:3])
        assert sampled[3] % 2 == 1
    # i < 0: 0, whatever the row holds
    nan = np.full((3, 33), np.nan, np.float32)
    nan[1] = x[3]
    got = tensor(nan.reshape(3, 1, 33)).sample_rows(i32(table), i32([-1, 0, -5]), i32([0, 0])).numpy()
    assert got.shape == (3, 1) and got.reshape(-1).tolist() == [0, int(np.argmax(x[3])), 0]


def bad_tables():
    """{what: (table (3, 8), counter (3,), index of the bad row's table row)}: table row 1 is the bad one"""
    good = lg_random.sampling_table([0.9, 0.8, 0], [20, 0, 0], [0.95, 1.0, 1.0], [1, 2, 3])
    cases = {}

    def case(what, word=None, value=None, counter=(0, 2, 1)):
        t = good.copy()
        if word is not None:
            t.view(np.uint32)[1, word] = value
        cases[what] = (t, np.array(counter, np.int32))
    case("g < 0", counter=(0, -1, 1))
    case("top_k < 0", 1, 0xFFFFFFFF)
    case("top_p = 0", 3, 0)
    case("top_p > 1", 3, 0x3FF00001)
    case("top_p NaN", 3, 0x7FF80000)
    case("top_p < 0", 3, 0xBFE00000)
    case("inv_T < 0", 0, 0xBF800000)
    case("inv_T = -0.0", 0, 0x80000000)
    case("inv_T NaN", 0, 0x7FC00000)
    case("inv_T inf", 0, 0x7F800000)
    return cases


@pytest.mark.parametrize("what", sorted(bad_tables()) + ["i >= n"])
def test_a_bad_row_answers_0_raises_and_the_other_rows_are_answered(what):
    x = smp.logits(33, 4)
    table, counter = bad_tables().get(what, bad_tables()["g < 0"])
    index = np.array([0, 1, 2, 0], np.int32)
    if what == "i >= n":
        table, counter = bad_tables()["g < 0"][0], np.array([0, 2, 1], np.int32)
        index[1] = 3
    tokens, bad = lg_random.sample_tokens_rows(x, table, index, counter)
    assert bad.tolist() == [False, True, False, False] and tokens[1] == 0
    good = lg_random.sampling_table([0.9, 0.8, 0], [20, 0, 0], [0.95, 1.0, 1.0], [1, 2, 3])
    want, none = lg_random.sample_tokens_rows(x[[0, 2, 3]], good, index[[0, 2, 3]], np.array([0, 2, 1]))
    assert not none.any()
    np.testing.assert_array_equal(tokens[[0, 2, 3]], want)
    with pytest.raises(IndexError) as raised:
        tensor(x).sample_rows(i32(table), i32(index), i32(counter))
    np.testing.assert_array_equal(raised.value.tokens.numpy(), tokens)          # every other row was answered


def test_sample_rows_refuses_other_operands():
    x, table = tensor(smp.logits(33, 4)), i32(lg_random.sampling_table([1.0, 0.5]))
    index, counter = i32([0, 1, 0, -1]), i32([0, 0])
    assert tuple(x.sample_rows(table, index, counter).shape) == (4,)
    for bad in (dict(table=tensor(np.zeros((2, 8), np.int64))), dict(table=i32(np.zeros((2, 7)))), dict(table=i32(np.zeros((0, 8)))),
                dict(index=i32([0, 1, 0])), dict(index=tensor(np.zeros(4, np.int64))), dict(counter=i32([0, 0, 0])),
                dict(counter=tensor(np.zeros(2, np.float32))), dict(dtype=np.int16)):
        with pytest.raises(ValueError):
            x.sample_rows(**dict(dict(table=table, index=index, counter=counter), **bad))
    for logits in (np.zeros((4, 2, 33), np.float32), np.zeros(33, np.float32), np.zeros((4, 0), np.float32), np.zeros((4, 33), np.int32)):
        with pytest.raises(ValueError):
            tensor(logits).sample_rows(table, index, counter)


# ---- serve ----------------------------------------------------------------------------------------------------------------------

def test_the_reference_has_no_near_tie_and_its_base_is_the_first_that_has_none():
    tokens = rc.reference()                                                # asserts the condition over all 42 steps, prints d
    for base in range(rc.BASE):
        assert rc.near_ties(base)[1], "base %d has no near-tie either: BASE is not the first" % base
    want, want_len = rc.expected()
    print("reference tokens: %s, emitted %s" % ([t.tolist() for t in tokens], want_len.tolist()))
    greedy, sampled = [r for r, p in enumerate(rc.PARAMETERS) if p[0] == 0], [r for r, p in enumerate(rc.PARAMETERS) if p[0] != 0]
    assert any(want_len[r] < sc.BUDGET for r in greedy) or any(want_len[r] < sc.BUDGET for r in sampled)      # a stop by EOS ...
    assert (want_len == sc.BUDGET).any() and (want_len < sc.BUDGET).any()                                       # ... and by the budget
    # each request alone is ONE call of the existing definition: asserted here through `serve` itself
    for r in (1, 3, 4):
        t, k, p = rc.PARAMETERS[r]
        out, out_len, _ = run(1, 16, rows=[sc.prompts()[r]], temperature=t, top_k=k, top_p=p, seeds=[rc.BASE + r])
        assert out_len.tolist() == [want_len[r]]
        np.testing.assert_array_equal(out[0], want[r])


def run(slots, chunk, rows=None, model=None, T=CpuTensor, **options):
    """serve_cases.run_serve over `rows` (default: the seven prompts)"""
    import lightgrad_amd.nn as nn
    model = dc.make_model(T, seed=sc.SEED) if model is None else model
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], slots, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    (out, out_len), stats = dc.bert.serve(model, sc.prompts() if rows is None else rows, sc.BUDGET, slots=slots, chunk=chunk, eos_token_id=sc.EOS,
                                          pad_token_id=sc.PAD, cache=cache, **options)
    return out.numpy().copy(), out_len.numpy().copy(), stats


@pytest.fixture(scope="module")
def model():
    return dc.make_model(CpuTensor, seed=sc.SEED)


@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_gives_each_request_the_tokens_of_its_run_alone(model, slots, chunk):
    want, want_len = rc.expected()
    lengths = [len(p) for p in sc.prompts()]
    light.manual_seed(77)
    lg_random._CpuGenerator.draws = 5
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, **rc.options())
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True and stats["steps"] == sc.simulate(lengths, want_len, slots, chunk)
    assert light.random.get_state("cpu") == (77, 5), "the per-request route read or advanced the generator"
    # token-packed
    budget = slots + 3
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, token_budget=budget, **rc.options())
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True and stats["steps"] == pc.simulate_packed(lengths, want_len, slots, chunk, budget)
    # paged, the generous pool
    num_blocks = slots * pg.MAX_BLOCKS
    out, out_len, stats, cache = pg.run_serve(CpuTensor, slots, chunk, num_blocks, model=model, poll=1, **rc.options())
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True
    assert stats["steps"] == pg.simulate(lengths, want_len, [sc.BUDGET] * 7, slots, chunk, pg.BLOCK, num_blocks) == sc.simulate(lengths, want_len, slots, chunk)
    pg.assert_no_block_leaked(cache)
    assert light.random.get_state("cpu") == (77, 5)


def test_the_queue_reversed_gives_every_request_the_same_tokens(model):
    want, want_len = rc.expected()
    t, k, p = rc.columns()
    out, out_len, _ = run(3, 4, rows=sc.prompts()[::-1], model=model, poll=1, temperature=t[::-1], top_k=k[::-1], top_p=p[::-1], seeds=rc.seeds()[::-1])
    np.testing.assert_array_equal(out_len[::-1], want_len)
    np.testing.assert_array_equal(out[::-1], want)


def test_seeds_none_is_the_generators_seed_and_an_int_counts_up(model):
    want, want_len = rc.expected()
    light.manual_seed(rc.BASE)
    options = rc.options()
    options["seeds"] = None
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, **options)
    np.testing.assert_array_equal(out, want)
    assert stats["per_request_sampling"] is True and light.random.get_state("cpu") == (rc.BASE, 0)
    out, _, _ = sc.run_serve(CpuTensor, 3, 4, model=model, **dict(rc.options(), seeds=rc.seeds()))
    np.testing.assert_array_equal(out, want)
    light.manual_seed(rc.BASE + 1)
    other, _, _ = sc.run_serve(CpuTensor, 3, 4, model=model, **options)
    assert not np.array_equal(other, want), "another seed gave the same tokens"
    np.testing.assert_array_equal(other[[0, 5]], want[[0, 5]])               # ... but for the greedy requests


def test_scalars_broadcast_and_a_float_temperature_alone_takes_the_old_route(model, monkeypatch):
    called = []
    for name in ("sample", "sample_rows"):
        op = getattr(CpuTensor, name)
        monkeypatch.setattr(CpuTensor, name, lambda self, *a, _op=op, _name=name, **kw: (called.append(_name), _op(self, *a, **kw))[1])
    light.manual_seed(5)
    _, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, eos=86, temperature=0.9, top_k=20, top_p=0.95, poll=1)
    assert set(called) == {"sample"} and "per_request_sampling" not in stats
    assert light.random.get_state("cpu") == (5, stats["steps"])               # one call of the global stream per step, as before
    del called[:]
    first = sc.run_serve(CpuTensor, 3, 4, model=model, temperature=0.9, top_k=20, top_p=0.95, seeds=4)
    assert set(called) == {"sample_rows"} and first[2]["per_request_sampling"] is True
    again = sc.run_serve(CpuTensor, 7, 16, model=model, temperature=[0.9] * 7, top_k=20, top_p=[0.95] * 7, seeds=[4 + r for r in range(7)])
    np.testing.assert_array_equal(first[0], again[0])
    np.testing.assert_array_equal(first[1], again[1])
    del called[:]
    sc.run_serve(CpuTensor, 3, 4, model=model)                               # greedy: neither
    assert called == []
    for bad in (dict(temperature=[0.9] * 6), dict(temperature=0.9, seeds=[1, 2]), dict(seeds=3), dict(temperature=0.9, top_k=[1, 2])):
        with pytest.raises((AssertionError, ValueError)):
            sc.run_serve(CpuTensor, 3, 4, model=model, **bad)


def test_request_pool_uploads_the_table_once(model):
    import lightgrad_amd.nn as nn
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    rows = sc.prompts()
    padded = np.zeros((7, max(map(len, rows))), np.int32)
    for r, p in enumerate(rows):
        padded[r, :len(p)] = p
    lengths = [len(p) for p in rows]
    pool = nn.RequestPool(cache, padded, lengths, [sc.BUDGET] * 7, 4, sampling=rc.table())
    assert isinstance(pool.sampling, CpuTensor) and pool.sampling.dtype == np.int32
    np.testing.assert_array_equal(pool.sampling.numpy(), rc.table())
    assert nn.RequestPool(cache, padded, lengths, [sc.BUDGET] * 7, 4).sampling is None
    for bad in (rc.table()[:6], rc.table().astype(np.int64), rc.table()[:, :7]):
        with pytest.raises(AssertionError, match="sampling"):
            nn.RequestPool(cache, padded, lengths, [sc.BUDGET] * 7, 4, sampling=bad)
