"""Guided decoding on the numpy backend: the automata of `light.guide` and its four builders against the plain statement of each,
the layout of `compile_guides`, the definition `guide.guide_logits` behind `CpuTensor.guide_rows`, `nn.RequestPool(guide=)` and
`serve(guide=)` - every request's tokens are those of its run ALONE through the definition in the state its own automaton reaches
(guide_cases.reference), whatever slots, chunk, token budget, paging and the shared prefix are."""
import itertools
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
from lightgrad_amd import guide as lg_guide
import decode_cases as dc
import guide_cases as gc
import paged_bf16_cases as pb
import paged_cases as pg
import penalty_cases as pc
import serve_cases as sc
import serve_packed_cases as spc


def tensor(a):
    return CpuTensor.from_numpy(np.array(a, copy=True, order="C"), requires_grad=False)      # a copy: the op writes in place


def tensors(case):
    """(logits, the seven integer operands) of a case as CpuTensors"""
    return tensor(case["logits"]), [tensor(case[k]) for k in gc.NAMES]


# ---- the builders against brute force -------------------------------------------------------------------------------------------

SMALL = 6
EVERY = [seq for n in range(5) for seq in itertools.product(range(SMALL), repeat=n)]        # all 1555 sequences up to length 4


def occurs(seq, seqs):
    return any(seq[k:k + len(s)] == tuple(s) for s in seqs for k in range(len(seq) - len(s) + 1))


def test_light_guide_is_exported():
    assert light.guide is lg_guide


def test_allow_only_against_its_statement():
    a = lg_guide.allow_only(SMALL, [1, 4, 4, 5])
    for seq in EVERY:
        inside = all(v in (1, 4, 5) for v in seq)
        assert (a.walk(seq) >= 0) == inside and a.accepts(seq) == inside, seq


@pytest.mark.parametrize("seqs", [[[2]], [[2], [0, 1]], [[0, 1, 0]], [[0, 0], [0, 1, 2], [3]], [[1, 2, 1, 2]], [[0, 1], [1, 0], [0, 1, 0, 1]], [[1, 1, 1], [1, 1]]], ids=str)
def test_ban_sequences_against_its_statement(seqs):
    a = lg_guide.ban_sequences(SMALL, seqs)
    assert all(a.accepting)
    for seq in EVERY:
        free = not occurs(seq, seqs)
        assert (a.walk(seq) >= 0) == free and a.accepts(seq) == free, seq


@pytest.mark.parametrize("seqs", [[[2]], [[0, 1, 2], [0, 1, 3, 4], [0, 5]], [[1], [1, 1], [1, 1, 1, 1]], [[3, 3], [3, 3]]], ids=str)
def test_one_of_against_its_statement(seqs):
    a = lg_guide.one_of(SMALL, seqs)
    for seq in EVERY:
        prefix = any(tuple(s[:len(seq)]) == seq for s in seqs)
        assert (a.walk(seq) >= 0) == prefix and a.accepts(seq) == (list(seq) in seqs), seq


@pytest.mark.parametrize("seqs", [[[2]], [[0, 1]], [[0, 0], [0, 1, 2]], [[1, 2, 1]], [[4], [0, 1, 0, 1]], [[1, 1, 1], [1, 1]]], ids=str)
def test_stop_after_against_its_statement(seqs):
    a = lg_guide.stop_after(SMALL, seqs)
    assert all(a.accepting)
    for seq in EVERY:
        # free until a sequence is complete, nothing behind it: no proper prefix may end with one
        valid = not any(occurs(seq[:n], seqs) for n in range(len(seq)))
        assert (a.walk(seq) >= 0) == valid and a.accepts(seq) == valid, seq
        if valid and occurs(seq, seqs):
            assert all(a.step(a.walk(seq), v) < 0 for v in range(SMALL))


def test_the_automaton_by_hand_and_what_it_refuses():
    a = lg_guide.TokenAutomaton(5)
    s = a.add_state(accepting=True)
    a.add(0, [1, 2], s), a.add_default(s, 0), a.forbid(s, [4])
    assert len(a) == 2 and a.walk([]) == 0 and a.walk([1]) == s and a.walk([0]) == -1 and a.walk([2, 3, 1]) == s and a.walk([2, 4]) == -1
    assert a.accepts([1]) and not a.accepts([]) and not a.accepts([1, 0]) and not a.accepts([3]) and a.walk([5]) == -1 and a.walk([-1]) == -1
    for bad in (lambda: a.add(0, [5], 0), lambda: a.add(0, [-1], 0), lambda: a.add(2, [1], 0), lambda: a.add(0, [1], 2), lambda: a.add_default(0, -1),
                lambda: lg_guide.TokenAutomaton(0), lambda: lg_guide.one_of(5, [[]]), lambda: lg_guide.ban_sequences(5, []), lambda: lg_guide.stop_after(5, [[5]]),
                lambda: lg_guide.allow_only(5, [])):
        with pytest.raises(ValueError):
            bad()


# ---- compile_guides ---------------------------------------------------------------------------------------------------------------

def bits_of(allow, V):
    return np.unpackbits(np.ascontiguousarray(allow).view(np.uint8), bitorder="little").reshape(allow.shape[0], -1)


@pytest.mark.parametrize("V", [6, 32, 33, 101])
def test_compile_guides_layout(V):
    eos = 4
    shared = lg_guide.ban_sequences(V, [[2], [0, 1]])
    trie = lg_guide.one_of(V, [[0, 1], [0, 1, 3], [5]])
    only = lg_guide.allow_only(V, [3])
    tables = lg_guide.compile_guides([shared, None, trie, shared, only, trie], 6, eos)
    allow, states, edges, start = tables
    W = -(-V // 32)
    S = len(shared) + len(trie) + len(only)
    assert all(a.dtype == np.int32 for a in tables) and allow.shape == (S, W) and states.shape == (S, 4) and edges.shape[1] == 2 and tables.vocab_size == V
    # shared objects are laid out once, in the order of their first use; an unguided request has no start
    assert start.tolist() == [0, -1, len(shared), 0, len(shared) + len(trie), len(shared)]
    bits = bits_of(allow, V)
    assert bits.shape[1] == 32 * W and not bits[:, V:].any()                                 # the tail bits are zero
    for a, base in ((shared, 0), (trie, len(shared)), (only, len(shared) + len(trie))):
        for s in range(len(a)):
            row, (default, first, count, forced) = bits[base + s], states[base + s].tolist()
            assert bool(row[eos]) == a.accepting[s]                                          # the eos bit IS the accepting flag
            for v in range(V):
                if v != eos:
                    assert bool(row[v]) == (a.step(s, v) >= 0), (s, v)
            own = edges[first:first + count]
            assert (np.diff(own[:, 0]) > 0).all()                                            # sorted by id within a state
            for v in range(V):
                t = a.step(s, v)
                if t >= 0:
                    hit = own[own[:, 0] == v]
                    assert (int(hit[0, 1]) if len(hit) else default) == base + t, (s, v)
            assert forced == (int(np.flatnonzero(row)[0]) if row.sum() == 1 else -1)
    # the forced ids: the ends of the trie that nothing follows force eos; `only` allows 3 and eos: not forced
    ends = [len(shared) + trie.walk(seq) for seq in ([0, 1, 3], [5])]
    assert states[ends, 3].tolist() == [eos, eos] and states[len(shared) + trie.walk([0, 1]), 3] == -1 and states[-1, 3] == -1
    assert states[len(shared) + trie.walk([0]), 3] == 1                                      # one way on, and no end here
    # no S x V table: the exceptions are the transitions alone
    assert edges.shape[0] <= sum(len(e) for a in (shared, trie, only) for e in a.edges)
    # None and nothing but None build nothing; one automaton stands for all
    assert lg_guide.compile_guides(None, 3, eos) is None and lg_guide.compile_guides([None] * 3, 3, eos) is None
    assert lg_guide.compile_guides(only, 3, eos).start.tolist() == [0, 0, 0]
    free = lg_guide.TokenAutomaton(V, accepting=True)
    free.add_default(0, 0)
    assert lg_guide.compile_guides([None, free], 2, None).edges.tolist() == [[0, 0]]         # no exception anywhere: the dummy row


def test_compile_guides_refuses_by_name():
    V = 20
    with pytest.raises(ValueError, match="vocab_size = 21, not V = 20"):
        lg_guide.compile_guides([lg_guide.allow_only(V, [1]), lg_guide.allow_only(V + 1, [1])], 2, 3)
    with pytest.raises(ValueError, match="vocab_size = 20, not V = 30"):
        lg_guide.compile_guides(lg_guide.allow_only(V, [1]), 2, 3, vocab_size=30)
    # a dead end: with eos=None every accepting state without transitions is one
    for a in (lg_guide.one_of(V, [[1, 2]]), lg_guide.stop_after(V, [[4]])):
        assert lg_guide.needs_eos(a) and lg_guide.compile_guides(a, 1, 3) is not None
        with pytest.raises(ValueError, match="dead end"):
            lg_guide.compile_guides(a, 1, None)
    assert not lg_guide.needs_eos(lg_guide.ban_sequences(V, [[1]])) and lg_guide.compile_guides(lg_guide.ban_sequences(V, [[1]]), 1, None) is not None
    # with an eos: a reachable state that is not accepting and allows nothing
    dead = lg_guide.TokenAutomaton(V)
    dead.add(0, [1], dead.add_state())
    with pytest.raises(ValueError, match="state 1 of automaton 0 is a dead end"):
        lg_guide.compile_guides(dead, 1, 3)
    dead.add_state()                                                                         # an unreachable one is none
    dead.accepting[1] = True
    assert lg_guide.compile_guides(dead, 1, 3) is not None
    for bad in (dict(guides=[None], n=2), dict(guides=["a"], n=1), dict(guides=dead, n=1, eos=V), dict(guides=dead, n=1, eos=-1)):
        with pytest.raises(ValueError):
            lg_guide.compile_guides(**dict(dict(eos=3), **bad))


# ---- the definition ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("V", gc.WIDTHS)
def test_every_kernel_case_against_the_loop_over_the_elements(V):
    case = gc.kernel_case(V)
    want, want_state = gc.by_hand(case)
    y, state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert not bad.any() and gc.same_words(y, want) and state.tolist() == want_state.tolist()
    assert state[:, 0].tolist() == case["reached"].tolist() and state[:, 1].tolist() == case["out_len"].tolist()
    # the specials at allowed ids keep their bytes; the forced rows hold +0.0 and -inf alone
    words = case["allow"].view(np.uint32)
    for r, i in enumerate(case["index"].tolist()):
        q = int(state[i, 0])
        allowed = np.array([(int(words[q, v >> 5]) >> (v & 31)) & 1 for v in range(V)], bool)
        if allowed.sum() == 1:
            assert y[r, allowed].view(np.uint32).tolist() == [0] and (y[r, ~allowed] == -np.inf).all()
        else:
            assert gc.same_words(y[r, allowed], case["logits"][r, allowed]) and (y[r, ~allowed] == -np.inf).all()
    # a second call on the result changes nothing
    again, state2, bad2 = lg_guide.guide_logits(**dict(gc.operands(case), logits=y, state=state))
    assert not bad2.any() and gc.same_words(again, y) and state2.tolist() == state.tolist()
    # float64 logits by the same steps
    with np.errstate(invalid="ignore"):                                     # (widening a signalling NaN)
        y64, state64, _ = lg_guide.guide_logits(**dict(gc.operands(case), logits=case["logits"].astype(np.float64)))
    assert state64.tolist() == state.tolist() and gc.same_words(y64[np.isfinite(y)], y[np.isfinite(y)].astype(np.float64)) and ((y64 == -np.inf) == (y == -np.inf)).all()


def nine_expected(case):
    """(y, state, bad) of the definition, with what the docstring of nine_rows says checked by hand"""
    y, state, bad = lg_guide.guide_logits(**gc.operands(case))
    x, V = case["logits"], case["logits"].shape[1]
    with np.errstate(invalid="ignore"):
        masked = (y == -np.inf) & ~(x == -np.inf)                            # (an allowed -inf of the input is not the guide's)
    kept = lambda r, ids: sorted(np.flatnonzero(~masked[r]).tolist()) == sorted(ids)        # noqa: E731
    assert np.isnan(y[0]).all() and np.isnan(y[5]).all() and gc.same_words(y[6], x[6])
    assert kept(1, [0, 31, 32, 33, 64, V - 1, gc.NINE_EOS])
    assert kept(2, sorted(set(range(V)) - {30, 21})) and kept(7, sorted(set(range(V)) - {30}))      # 20 stored: 21 is banned now; behind 50: not
    assert kept(3, [gc.NINE_EOS]) and y[3, gc.NINE_EOS] == 0 and not np.signbit(y[3, gc.NINE_EOS])
    assert kept(4, sorted(set(range(V)) - {9})) and kept(8, list(range(V)))                         # 40 stored: 41 completes, and is allowed
    return y, state, bad


def test_nine_rows_of_every_kind():
    case = gc.nine_rows()
    y, state, bad = nine_expected(case)
    assert bad.tolist() == gc.NINE_BAD
    assert state[:, 1].tolist() == [0, 2, 0, 1, 3, 4, 1, 0] and state[2].tolist() == [-1, 0] and state[7].tolist() == case["state"][7].tolist()
    assert state[3, 0] != state[4, 0] and case["state"][3, 0] == case["state"][4, 0]              # one automaton, two requests, two states
    assert gc.same_words(y[2, 8:16], gc.specials()) and y[2, 21] == -np.inf
    assert gc.same_words(y[4, 2:9], gc.specials()[:7]) and y[4, 9] == -np.inf


@pytest.mark.parametrize("what", sorted(gc.bad_causes()))
def test_each_bad_row_cause_leaves_row_and_state_untouched_and_the_rest_is_computed(what):
    good = gc.changed(gc.nine_rows(), dict(index=(6, gc.SPARE_REQUEST)))
    case = gc.changed(good, gc.bad_causes()[what])
    want, want_state, none = lg_guide.guide_logits(**gc.operands(good))
    assert not none.any()
    y, state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert bad.tolist() == [r == gc.BAD_ROW for r in range(9)], what
    assert gc.same_words(y[gc.BAD_ROW], good["logits"][gc.BAD_ROW]) and gc.same_words(np.delete(y, gc.BAD_ROW, axis=0), np.delete(want, gc.BAD_ROW, axis=0))
    assert state[gc.BAD_REQUEST].tolist() == case["state"][gc.BAD_REQUEST].tolist()
    assert np.delete(state, gc.BAD_REQUEST, axis=0).tolist() == np.delete(want_state, gc.BAD_REQUEST, axis=0).tolist()
    # the op: in place, the good rows finished, then IndexError
    logits, operands = tensors(case)
    with pytest.raises(IndexError):
        logits.guide_rows(*operands)
    assert gc.same_words(logits.numpy(), y) and operands[-1].numpy().tolist() == state.tolist()


# ---- the op -----------------------------------------------------------------------------------------------------------------------

def test_guide_rows_is_in_place_and_returns_its_tensor():
    case = gc.changed(gc.nine_rows(), dict(index=(6, gc.SPARE_REQUEST)))
    want, want_state, bad = lg_guide.guide_logits(**gc.operands(case))
    assert not bad.any()
    logits, operands = tensors(case)
    assert logits.guide_rows(*operands) is logits and gc.same_words(logits.numpy(), want) and operands[-1].numpy().tolist() == want_state.tolist()
    assert logits.guide_rows(*operands) is logits and gc.same_words(logits.numpy(), want) and operands[-1].numpy().tolist() == want_state.tolist()
    # (rows, 1, V), and rows of a wider tensor: the bytes between the rows are unchanged
    V = want.shape[1]
    wide = np.full((9, 1, V + 6), -7.0, np.float32)
    wide[:, 0, 3:3 + V] = case["logits"]
    t = tensor(wide)
    view = CpuTensor.from_numpy(t.data[:, :, 3:3 + V], requires_grad=False)
    assert view.guide_rows(*tensors(case)[1]) is view
    assert gc.same_words(t.numpy()[:, 0, 3:3 + V], want) and (t.numpy()[:, 0, :3] == -7).all() and (t.numpy()[:, 0, 3 + V:] == -7).all()
    # float64 logits - the float64 tapes of the tests - in float64
    with np.errstate(invalid="ignore"):                                     # (widening a signalling NaN)
        wide = case["logits"].astype(np.float64)
    t = tensor(wide)
    t.guide_rows(*tensors(case)[1])
    assert gc.same_words(t.numpy(), lg_guide.guide_logits(**dict(gc.operands(case), logits=wide))[0])
    # a tensor that requires a gradient is refused, and so are other operands
    operands = tensors(case)[1]
    with pytest.raises(AssertionError, match="gradient"):
        CpuTensor.from_numpy(case["logits"].copy(), requires_grad=True).guide_rows(*operands)
    logits = tensor(case["logits"])
    for bad in (dict(allow=tensor(case["allow"][:, :3])), dict(allow=tensor(case["allow"].astype(np.int64))), dict(states=tensor(case["states"][:, :3])),
                dict(states=tensor(case["states"][:-1])), dict(edges=tensor(case["edges"][:, :1])), dict(index=tensor(case["index"][:8])),
                dict(out=tensor(case["out"][:7])), dict(out_len=tensor(case["out_len"].astype(np.int64))), dict(state=tensor(case["state"][:, :1])),
                dict(state=tensor(case["state"][:7]))):
        with pytest.raises(ValueError):
            logits.guide_rows(**dict(dict(zip(gc.NAMES, operands)), **bad))
    for shape in ((9, 2, V), (V,)):
        with pytest.raises(ValueError):
            tensor(np.zeros(shape, np.float32)).guide_rows(*operands)
    with pytest.raises(ValueError):
        tensor(np.zeros((9, V), np.int32)).guide_rows(*operands)
    assert gc.same_words(logits.numpy(), case["logits"]) and operands[-1].numpy().tolist() == case["state"].tolist()


# ---- the pool ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def model():
    return dc.make_model(CpuTensor, seed=sc.SEED)


def test_request_pool_uploads_the_tables_once_and_refuses_others(model):
    cache = nn.KVCache(sc.CFG["num_hidden_layers"], 3, sc.CAPACITY, sc.CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    rows = sc.prompts()
    padded = np.zeros((7, max(map(len, rows))), np.int32)
    for r, p in enumerate(rows):
        padded[r, :len(p)] = p
    arguments = (cache, padded, [len(p) for p in rows], [sc.BUDGET] * 7, 4)
    tables = lg_guide.compile_guides(gc.guides("greedy"), 7, gc.EOS)
    pool = nn.RequestPool(*arguments, guide=tuple(tables))
    assert len(pool.guide) == 3 and all(isinstance(t, CpuTensor) and t.dtype == np.int32 for t in pool.guide + (pool.guide_state,))
    for t, a in zip(pool.guide, tables):
        np.testing.assert_array_equal(t.numpy(), a)
    assert pool.guide_state.numpy().tolist() == [[s, 0] for s in tables.start.tolist()] and tables.start[0] == -1 and tables.start[1] == tables.start[6]
    plain = nn.RequestPool(*arguments)
    assert plain.guide is None and plain.guide_state is None
    allow, states, edges, start = tables
    for bad in ((allow, states, edges, start[:6]), (allow.astype(np.int64), states, edges, start), (allow, states[:, :3], edges, start),
                (allow, states, edges, np.full(7, len(states), np.int32)), (allow, states, edges[:, :1], start)):
        with pytest.raises(AssertionError, match="guide"):
            nn.RequestPool(*arguments, guide=bad)


# ---- serve ------------------------------------------------------------------------------------------------------------------------

def test_the_references_have_no_near_tie_and_the_guides_bind():
    for mode in gc.MODES + (gc.COMBINED,):
        tokens, plain = gc.reference(mode), gc.unguided(mode)                # asserts the rules over every step, prints d
        want, want_len = gc.expected(mode)
        print("%s: %s" % (mode, [t.tolist() for t in tokens]))
        gc.assert_consequences(mode, want, want_len)
        cut = sc.expected(plain, gc.BUDGET, gc.EOS)
        for r in range(1, 7):                                               # every guided request: the constraint binds
            assert want[r, :want_len[r]].tolist() != cut[0][r, :cut[1][r]].tolist(), (mode, r)
        np.testing.assert_array_equal(want[0], cut[0][0])                   # the unguided request: the plain run's tokens
        assert (want_len == gc.BUDGET).any() and (want_len < gc.BUDGET).any()
        # one of the three sequences, then the end
        assert want[3, :want_len[3]].tolist() in [list(s) + [gc.EOS] for s in gc.ONE_OF]
        # the cycle: halves alternate, and no end in front of four tokens
        body = [v for v in want[4, :want_len[4]].tolist() if v != gc.EOS]
        assert len(body) >= 4 and all((v < 50) == (j % 2 == 0) for j, v in enumerate(body))
        assert all(v in gc.ALLOWED + (gc.EOS,) for r in (1, 6) for v in want[r, :want_len[r]].tolist())
    gc.reference("greedy", True)                                            # the prefixed prompts of the shared-prefix run, greedy


@pytest.mark.parametrize("mode", gc.MODES)
@pytest.mark.parametrize("slots", sc.SLOTS)
@pytest.mark.parametrize("chunk", sc.CHUNKS)
def test_serve_gives_each_request_the_tokens_of_its_run_alone(model, slots, chunk, mode):
    want, want_len = gc.expected(mode)
    out, out_len, stats = sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, **gc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    gc.assert_consequences(mode, out, out_len)
    assert stats["guide"] is True and stats["steps"] == sc.simulate([len(p) for p in sc.prompts()], want_len, slots, chunk)


@pytest.mark.parametrize("mode", gc.MODES)
def test_serve_token_packed(model, mode):
    want, want_len = gc.expected(mode)
    out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, poll=1, token_budget=6, **gc.options(mode))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["guide"] is True and stats["steps"] == spc.simulate_packed([len(p) for p in sc.prompts()], want_len, 3, 4, 6)


def test_serve_paged_with_a_shared_prefix(model):
    want, want_len = gc.expected("greedy", True)
    out, out_len, stats, cache = pg.run_serve(CpuTensor, 3, 4, 2 + 3 * pg.MAX_BLOCKS, model=model, poll=1, rows=pg.prefixed_prompts(),
                                              **gc.options("greedy", shared_prefix=pg.PREFIX))
    np.testing.assert_array_equal(out_len, want_len)
    np.testing.assert_array_equal(out, want)
    assert stats["guide"] is True and stats["prefix_blocks"] == 2
    pg.assert_no_block_leaked(cache, 2)


def test_the_bf16_route_walks_and_accepts(model):
    """its logits are the rounded model's: no reference equality, but the consequences of the contract and schedule independence"""
    runs = [pb.run_serve(CpuTensor, slots, chunk, slots * pg.MAX_BLOCKS, model=model, rows=sc.prompts(), poll=1, **gc.options("sampled"))
            for slots, chunk in ((3, 4), (7, 16))]
    np.testing.assert_array_equal(runs[0][1], runs[1][1])
    np.testing.assert_array_equal(runs[0][0], runs[1][0])
    gc.assert_consequences("sampled", runs[0][0], runs[0][1])
    assert runs[0][2]["guide"] is True


def test_guide_none_builds_nothing_and_one_automaton_stands_for_all(model, monkeypatch):
    called = []
    op = CpuTensor.guide_rows
    monkeypatch.setattr(CpuTensor, "guide_rows", lambda self, *a, **kw: (called.append(1), op(self, *a, **kw))[1])
    want, want_len = sc.expected(sc.assert_margins_rule_out_ties(), sc.BUDGET, sc.EOS)
    for nothing in (dict(), dict(guide=None), dict(guide=[None] * 7)):
        out, out_len, stats = sc.run_serve(CpuTensor, 3, 4, model=model, **nothing)
        np.testing.assert_array_equal(out, want)
        np.testing.assert_array_equal(out_len, want_len)
        assert "guide" not in stats and called == []
    only = lg_guide.allow_only(gc.VOCAB, gc.ALLOWED)
    first = sc.run_serve(CpuTensor, 3, 4, model=model, guide=only)
    assert first[2]["guide"] is True and len(called) == first[2]["steps"]
    again = sc.run_serve(CpuTensor, 7, 16, model=model, guide=[only] * 7)
    np.testing.assert_array_equal(first[0], again[0])
    assert all(v in gc.ALLOWED + (gc.EOS,) for r in range(7) for v in first[0][r, :first[1][r]].tolist())
    # refused by name: another vocabulary, an automaton that needs an end without eos_token_id, a wrong number of entries
    with pytest.raises(AssertionError, match="vocabulary of 102 ids"):
        sc.run_serve(CpuTensor, 3, 4, model=model, guide=lg_guide.allow_only(gc.VOCAB + 1, [1]))
    with pytest.raises(AssertionError, match="needs eos_token_id"):
        sc.run_serve(CpuTensor, 3, 4, model=model, eos=None, guide=lg_guide.one_of(gc.VOCAB, gc.ONE_OF))
    with pytest.raises(AssertionError, match="one entry per request"):
        sc.run_serve(CpuTensor, 3, 4, model=model, guide=[only] * 6)
    assert sc.run_serve(CpuTensor, 3, 4, model=model, eos=None, guide=only)[2]["guide"] is True
    with pytest.raises(TypeError):
        dc.bert.generate(model, tensor(sc.prompts()[0][None, :]), 2, guide=only)


def test_penalties_sampling_logprobs_and_guides_together(model):
    """one combined run: a forced token has the log-probability 0.0, no alternative with a finite score is a masked id, and a
    min_new_tokens beyond a `one_of` sequence still ends it"""
    options = gc.options(gc.COMBINED, logprobs=3)
    options["min_new_tokens"] = [6 if r == 3 else p[3] for r, p in enumerate(pc.PARAMETERS)]       # request 3: longer than any of its sequences
    want, want_len = gc.expected(gc.COMBINED)
    assert pc.PARAMETERS[3][3] <= 2, "the reference was computed under a min_new_tokens that never holds the end back"
    runs = [sc.run_serve(CpuTensor, slots, chunk, model=model, poll=1, **options) for slots, chunk in ((3, 4), (7, 16))]
    for out, out_len, stats in runs:
        np.testing.assert_array_equal(out_len, want_len)
        np.testing.assert_array_equal(out, want)
        gc.assert_consequences(gc.COMBINED, out, out_len)
    out, out_len, stats = runs[0]
    assert out[3, :out_len[3]].tolist() in [list(s) + [gc.EOS] for s in gc.ONE_OF] and out_len[3] < 6
    scores, best, best_scores = (stats["logprobs"][k].numpy() for k in ("token", "top_ids", "top"))
    forced = 0
    for r, a in enumerate(gc.guides(gc.COMBINED)):
        for g in range(out_len[r]):
            if a is None:
                continue
            s = a.walk(out[r, :g])
            allowed = {v for v in range(gc.VOCAB) if v != gc.EOS and a.step(s, v) >= 0} | ({gc.EOS} if a.accepting[s] else set())
            assert out[r, g] in allowed
            if len(allowed) == 1:
                forced += 1
                assert scores[r, g] == 0.0 and not np.signbit(scores[r, g]), (r, g, scores[r, g])
            for v, score in zip(best[r, g], best_scores[r, g]):
                assert v < 0 or not np.isfinite(score) or v in allowed, (r, g, v, score)
    assert forced >= 2                                                      # the end of the `one_of` sequence, and the stop
