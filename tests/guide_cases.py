"""What test_guide_cpu.py and test_hip_guide.py share: the cases of `guide_rows` - hand-built tables at every word edge of the
bitset, nine rows of every kind, one change per bad cause - and the run of `serve(guide=)` over the seven prompts of serve_cases
with its reference: each request ALONE by a full float64 recompute per token, the float64 logits passed through the definition
(`guide.guide_logits`) in the state its own automaton reaches on its own tokens, in the manner of penalty_cases.forwards.  Computed
once per process and never changed afterwards.  No tests of its own.

The guides, one per request: None, `allow_only` of 20 ids, `ban_sequences` of one id and one bigram, `one_of` three sequences of
different lengths that share a prefix, the hand-built cycle (ids below 50, then ids from 50 on, accepting after four tokens, by
default transitions), `stop_after` one id, and the SAME object as the second.  The cycle and `stop_after` stand in the other order
than one would list them: request 4 alone emits one token and the end-of-sequence id, so a stop id taken from its tokens would not
change them; request 5 emits six.  The banned and the stop ids come from the unguided reference's own tokens of that mode, so that
the constraint binds.

Near-ties are ruled out from the references alone, over all 42 steps of a run, on the guided float64 logits with the -inf entries
set aside.  d is the largest deviation of the float32 full forward's last-row logits from float64 over those steps; the guide moves
no allowed logit (a forced one becomes exactly +0.0 next to nothing but -inf), so the rules are the project's own:
  * a greedy step needs a top-2 margin of the allowed logits >= 100 d (a single allowed id has no second);
  * a sampled step needs a one-token band under sample_cases.acceptable with eps = max(1e-5, 400 d inv_T) (an id at -inf has the
    weight 0 and is in no band);
  * with top-k on and more than k allowed ids, the gap between the k-th and the (k + 1)-th largest allowed logit must be >= 100 d.
The combined run adds penalties in front (penalty_cases.PARAMETERS) and takes their factor lam = max(rho, 1 / rho) into each rule.
`reference(mode)` asserts this; no step is left out."""
import functools
import numpy as np
from lightgrad_amd import CpuTensor
from lightgrad_amd import guide as lg_guide
from lightgrad_amd import random as lg_random
import decode_cases as dc
import paged_cases as pg
import penalty_cases as pc
import sample_cases as smp
import sample_rows_cases as rc
import serve_cases as sc

BUDGET, EOS = sc.BUDGET, sc.EOS
VOCAB = sc.CFG["vocab_size"]
BASE = 1
MODES = ("greedy", "sampled")
COMBINED = "combined"                         # penalties + per-request sampling + guides
ONE_OF = ((5, 9, 2), (5, 9, 40, 41), (5, 77))
ALLOWED = tuple(range(3, VOCAB, 5))           # 20 ids
NAMES = ("allow", "states", "edges", "index", "out", "out_len", "state")


def same_words(got, want):
    """equal bit for bit as unsigned words, NaN payloads and the sign of zero included"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    word = {4: np.uint32, 8: np.uint64}[want.dtype.itemsize]
    return got.dtype == want.dtype and got.shape == want.shape and bool((got.view(word) == want.view(word)).all())


def changed(case, change):
    case = {k: v.copy() for k, v in case.items()}
    for name, (at, value) in change.items():
        case[name][at] = value
    return case


def frozen(case):
    for a in case.values():
        a.setflags(write=False)
    return case


# ---- serve ------------------------------------------------------------------------------------------------------------------------

def cycle():
    """ids below 50, then ids from 50 on, and so on; accepting once four tokens are stored: states 0 .. 3 count them, 4 and 5 are
    the cycle.  Every transition is a default; the other half of the vocabulary is forbidden"""
    a = lg_guide.TokenAutomaton(VOCAB)
    for s in range(1, 6):
        a.add_state(accepting=s >= 4)
    for s in range(6):
        a.add_default(s, s + 1 if s < 5 else 4)
        a.forbid(s, range(50, VOCAB) if s % 2 == 0 else range(50))
    return a


def unguided(mode):
    """the reference tokens of the run without guides: the constraint is built from them"""
    if mode == "greedy":
        return sc.greedy_reference()[0]
    if mode == "sampled":
        return rc.reference()
    return pc.reference("sampled")


@functools.lru_cache(maxsize=None)
def guides(mode):
    """the seven entries of `serve(guide=)` for a mode"""
    plain = [t.tolist() for t in unguided(mode)]
    shared = lg_guide.allow_only(VOCAB, ALLOWED)
    ban = lg_guide.ban_sequences(VOCAB, [[plain[2][4]], plain[2][:2]])
    stop = lg_guide.stop_after(VOCAB, [[plain[5][2]]])
    return (None, shared, ban, lg_guide.one_of(VOCAB, ONE_OF), cycle(), stop, shared)


def sampling(mode, r):
    return (0, 0, 1) if mode == "greedy" else rc.PARAMETERS[r]


def options(mode, **more):
    """the keywords of `serve` for a mode"""
    base = {} if mode == "greedy" else rc.options(BASE)
    if mode == COMBINED:
        base = pc.options("sampled")
    return dict(base, guide=list(guides(mode)), **more)


@functools.lru_cache(maxsize=None)
def own_tables(mode, r):
    return lg_guide.compile_guides([guides(mode)[r]], 1, EOS, vocab_size=VOCAB)


def guided(y, mode, r, tokens):
    """the float64 logits y of request r behind `tokens`, through the definition in the state its automaton reaches on them"""
    tables = own_tables(mode, r)
    if tables is None:
        return y
    out = np.zeros((1, BUDGET), np.int32)
    out[0, :len(tokens)] = tokens
    z, state, bad = lg_guide.guide_logits(y[None, :], tables.allow, tables.states, tables.edges, [0], out, [len(tokens)], [[tables.start[0], 0]])
    assert not bad.any() and state[0, 1] == len(tokens)
    return z[0]


@functools.lru_cache(maxsize=None)
def forwards(mode, prefixed=False):
    """per request the steps (guided float64 last-row logits, |float32 - float64| of the logits in front of everything, token) of
    its run alone"""
    model64, model32 = pc.models()
    runs = []
    for r, prompt in enumerate(pg.prefixed_prompts() if prefixed else sc.prompts()):
        t, k, p = sampling(mode, r)
        seq, steps, tokens = prompt[None, :].copy(), [], []
        for g in range(BUDGET):
            l64, l32 = dc.full_logits(model64, seq)[0, -1], dc.full_logits(model32, seq)[0, -1]
            y = guided(pc.penalised(l64, r, prompt, tokens) if mode == COMBINED else l64, mode, r, tokens)
            if t == 0:
                token = int(np.argmax(y))
            else:
                token = int(lg_random.sample_tokens(BASE + r, 0, np.repeat(y[None, :], g + 1, axis=0), t, k, p)[g])
            steps.append((y, float(np.abs(l32.astype(np.float64) - l64).max()), token))
            tokens.append(token)
            seq = np.concatenate([seq, np.array([[token]], np.int32)], axis=1)
            if token == EOS:
                break                                                   # the request has ended: nothing behind it is drawn
        runs.append(steps)
    return runs


def near_ties(mode, prefixed=False):
    """(d, the steps (request, g, why) that the rules of the module text do not rule out)"""
    runs = forwards(mode, prefixed)
    d = max(dev for steps in runs for _, dev, _ in steps)
    failed = []
    for r, steps in enumerate(runs):
        t, k, p = sampling(mode, r)
        lam = max(float(np.float32(pc.PARAMETERS[r][0])), 1.0 / float(np.float32(pc.PARAMETERS[r][0]))) if mode == COMBINED else 1.0
        for g, (y, _, token) in enumerate(steps):
            top = np.sort(y[np.isfinite(y)])
            if t == 0:
                if top.size > 1 and not top[-1] - top[-2] >= 100 * lam * d:
                    failed.append((r, g, "top-2 margin %.3g" % (top[-1] - top[-2])))
                continue
            inv_t = float(np.float32(1.0 / np.float64(t)))
            band = smp.acceptable(y, rc.uniform(BASE + r, g), t, k, p, eps=max(1e-5, 400 * lam * d * inv_t))
            if band.tolist() != [token]:
                failed.append((r, g, "band %s around token %d" % (band[:6].tolist(), token)))
            if 1 <= k < top.size and not top[-k] - top[-k - 1] >= 100 * lam * d:
                failed.append((r, g, "top-k gap %.3g" % (top[-k] - top[-k - 1])))
    return d, failed


@functools.lru_cache(maxsize=None)
def reference(mode, prefixed=False):
    """[tokens] per request - up to BUDGET of them, the last one EOS if the request ended by it - with the condition of the module
    text asserted over every step"""
    d, failed = near_ties(mode, prefixed)
    print("guide reference (%s%s): float32 deviation d = %.3g" % (mode, ", prefixed prompts" if prefixed else "", d))
    assert not failed, "%s%s: near-ties (request, step, why): %s" % (mode, " prefixed" if prefixed else "", failed)
    tokens = [np.array([token for _, _, token in steps], np.int32) for steps in forwards(mode, prefixed)]
    for t in tokens:
        t.setflags(write=False)
    return tokens


def expected(mode, prefixed=False):
    """(out, out_len) that the references imply under BUDGET and EOS"""
    return sc.expected(reference(mode, prefixed), BUDGET, EOS)


def assert_consequences(mode, out, out_len):
    """what the contract implies for any run, whatever its logits: every request's tokens walk its automaton, and one that ended
    with EOS ended in an accepting state"""
    for r, a in enumerate(guides(mode)):
        tokens = out[r, :out_len[r]].tolist()
        if a is None:
            continue
        ended = bool(tokens) and tokens[-1] == EOS
        body = tokens[:-1] if ended else tokens
        assert a.walk(body) >= 0, "request %d: %s leaves its automaton" % (r, tokens)
        assert not ended or a.accepts(body), "request %d ended in a state that is not accepting: %s" % (r, tokens)
        assert ended or len(tokens) == BUDGET, "request %d stopped without EOS in front of its budget: %s" % (r, tokens)


# ---- the op: hand-built tables at every word edge ---------------------------------------------------------------------------------

WIDTHS = (1, 31, 32, 33, 64, 101, 1027, 4096, 30522)
G_COLUMNS = 8
PAD_IDS = (-5, 2 ** 31 - 1, -(2 ** 31), 1 << 20)     # what lies in `out` in front of k and behind g: never read


def specials():
    """NaNs with payloads (a quiet and a signalling one, one of them negative), both zeros, both infinities, subnormals"""
    return np.array([0x7FC12345, 0xFFA00001, 0x80000000, 0x00000000, 0x7F800000, 0xFF800000, 0x00000001, 0x807FFFFF], np.uint32).view(np.float32)


def hand_states(V):
    """six states written out by hand, as (bits (V,) bool, default, [(id, target)] sorted):
      0  allows everything, no exception, default 1
      1  allows nothing but one id (forced), one exception: it
      2  allows only id 0 (forced); its exception leads on
      3  allows only id V - 1 (forced); no exception: its default leads on
      4  alternating words (the ids of every second 32-bit word), two exceptions: its first and its last allowed id
      5  allows everything, min(17, V) exceptions spread over the vocabulary with id 0 the first and V - 1 the last, default 0"""
    every = np.ones(V, bool)
    one = lambda v: np.arange(V) == v                                              # noqa: E731
    words = (np.arange(V) >> 5) % 2 == 0
    ends = sorted({int(np.flatnonzero(words)[0]), int(np.flatnonzero(words)[-1])})
    spread = sorted({int(v) for v in np.linspace(0, V - 1, min(17, V)).round()})
    return [(every, 1, []), (one(V // 2), -1, [(V // 2, 2)]), (one(0), -1, [(0, 3)]), (one(V - 1), 4, []),
            (words, 5, [(v, k % 2 * 5) for k, v in enumerate(ends)]), (every, 0, [(v, k % 6) for k, v in enumerate(spread)])]


def hand_tables(V):
    """(allow, states, edges) of hand_states(V), laid out without `compile_guides`"""
    W = -(-V // 32)
    hand = hand_states(V)
    allow, states, edges = np.zeros((len(hand), W), np.uint32), np.zeros((len(hand), 4), np.int32), []
    for s, (bits, default, own) in enumerate(hand):
        padded = np.zeros(W * 32, bool)
        padded[:V] = bits
        allow[s] = np.packbits(padded, bitorder="little").view("<u4")
        states[s] = (default, len(edges), len(own), int(np.flatnonzero(bits)[0]) if bits.sum() == 1 else -1)
        edges += own
    return allow.view(np.int32), states, np.array(edges, np.int32).reshape(-1, 2)


def hand_step(V, q, v):
    """the state behind id v in state q of hand_states(V), by a look through the list"""
    bits, default, own = hand_states(V)[q]
    assert bits[v]
    return dict(own).get(v, default)


# (start state, what the catch-up absorbs: the first or the last exception's id, or an id that takes the default), tokens absorbed before
ROWS = ((0, (), 0), (0, ("miss",), 2), (1, ("first",), 0), (2, ("first", "miss", "miss"), 1), (3, ("miss",), 0), (4, ("first",), 3), (4, ("last",), 0),
        (4, ("miss", "miss", "first"), 0), (5, ("first",), 1), (5, ("last",), 0), (5, ("miss", "last", "first"), 2), (5, (), 4), (1, (), 0), (3, (), 5))


@functools.lru_cache(maxsize=None)
def kernel_case(V):
    """{name: array}: one launch over hand_tables(V), a row per entry of ROWS and a request per row (in another order), catch-ups
    of 0, 1 and 3 tokens that hit the first and the last exception of a list and miss into the default - where a state has no such
    id (a vocabulary of one), whatever it allows -, and the state each request must reach"""
    allow, states, edges = hand_tables(V)
    n = len(ROWS)
    rng = np.random.RandomState(V)
    x = (3 * rng.standard_normal((n, V))).astype(np.float32)
    for r in range(n):
        at = (np.arange(8) * 5 + r) % V
        x[r, at] = specials()[:at.size]
    out = np.resize(np.array(PAD_IDS, np.int64), (n, G_COLUMNS)).astype(np.int32)
    out_len, state, reached = np.zeros(n, np.int32), np.zeros((n, 2), np.int32), np.zeros(n, np.int32)
    index = ((np.arange(n) * 5 + 3) % n).astype(np.int32)                    # row r names request index[r]: a permutation
    for r, (q, picks, k) in enumerate(ROWS):
        i = int(index[r])
        state[i] = (q, k)
        for j, pick in enumerate(picks):
            bits, default, own = hand_states(V)[q]
            ids = [v for v, _ in own]
            misses = [v for v in np.flatnonzero(bits)[:40].tolist() if v not in ids]
            v = ids[0] if pick == "first" and ids else ids[-1] if pick == "last" and ids else misses[0] if misses else int(np.flatnonzero(bits)[0])
            out[i, k + j] = v
            q = hand_step(V, q, v)
            if q < 0:
                raise AssertionError("ROWS walks into a default of -1")
        out_len[i], reached[i] = k + len(picks), q
    return frozen(dict(logits=x, allow=allow, states=states, edges=edges, index=index, out=out, out_len=out_len, state=state, reached=reached))


def operands(case):
    return {k: case[k] for k in ("logits",) + NAMES}


def by_hand(case):
    """the definition as a plain loop over the elements of a case whose rows are all good: (y, state)"""
    x, V = case["logits"], case["logits"].shape[1]
    y, state = x.copy(), case["state"].copy()
    words = case["allow"].view(np.uint32)
    for r, i in enumerate(case["index"].tolist()):
        q, k = case["state"][i].tolist()
        g = int(case["out_len"][i])
        for j in range(k, g):
            v = int(case["out"][i, j])
            default, first, count = case["states"][q, :3].tolist()
            q = dict(case["edges"][first:first + count].tolist()).get(v, default)
        state[i] = (q, g)
        for v in range(V):
            if not (int(words[q, v >> 5]) >> (v & 31)) & 1:
                y[r, v] = -np.inf
        if case["states"][q, 3] >= 0:
            y[r, case["states"][q, 3]] = 0.0
    return y, state


# ---- the op: nine rows of every kind ------------------------------------------------------------------------------------------------

NINE_EOS = 18
NINE_BAD = [False] * 6 + [True] + [False] * 2
BAD_ROW, BAD_REQUEST, SPARE_REQUEST = 4, 1, 7


def hand_automaton(V):
    """state 0: id 3 stays, everything else goes to state 1; state 1: id 5 stays, id 9 is forbidden, everything else goes back"""
    a = lg_guide.TokenAutomaton(V, accepting=True)
    a.add_state(True)
    a.add_default(0, 1), a.add(0, [3], 0)
    a.add_default(1, 0), a.add(1, [5], 1), a.forbid(1, [9])
    return a


@functools.lru_cache(maxsize=None)
def nine_rows(V=101):
    """{name: array} of one launch over index = (-1, 0, 3, 5, 1, 2, "N", 4, 6) with N = 8 requests, compiled by `compile_guides`:
      row 0        free, its logits all NaN
      row 1        request 0: `allow_only`, nothing stored yet
      rows 2, 7    requests 3 and 4 share ONE automaton (`ban_sequences` of an id and a bigram): request 3 has stored the bigram's
                   first id (its second is banned now), request 4 catches up over three tokens
      row 3        request 5: `one_of`, its sequence complete - the end-of-sequence id is forced
      row 4        request 1: hand_automaton, tokens 3 (its exception) and 8 (its default) to catch up with
      row 5        request 2: unguided (q = -1), its logits all NaN - unread
      row 6        beyond the table
      row 8        request 6: `stop_after`, one token in front of the stop id absorbed earlier (k = 1 = g: nothing to catch up)
    Request 7 is guided and held by no row."""
    n, G = 8, 7
    shared = lg_guide.ban_sequences(V, [[30], [20, 21]])
    entries = [lg_guide.allow_only(V, [0, 31, 32, 33, 64, V - 1]), hand_automaton(V), None, shared, shared,
               lg_guide.one_of(V, [[5, 9], [5, 9, 2, 4]]), lg_guide.stop_after(V, [[40, 41]]), lg_guide.allow_only(V, [7])]
    tables = lg_guide.compile_guides(entries, n, NINE_EOS)
    rng = np.random.RandomState(9)
    x = (3 * rng.standard_normal((9, V))).astype(np.float32)
    x[0], x[5] = np.nan, np.nan
    x[2, 8:16], x[4, 2:10] = specials(), specials()
    out = np.resize(np.array(PAD_IDS, np.int64), (n, G)).astype(np.int32)
    stored = {0: [], 1: [3, 8], 2: [11, 12], 3: [20], 4: [20, 20, 50], 5: [5, 9, 2, 4], 6: [40], 7: []}
    out_len = np.zeros(n, np.int32)
    for i, tokens in stored.items():
        out[i, :len(tokens)], out_len[i] = tokens, len(tokens)
    state = np.stack([tables.start, np.zeros(n, np.int32)], axis=1)
    state[6] = (entries[6].walk([40]) + tables.start[6], 1)
    index = np.array([-1, 0, 3, 5, 1, 2, n, 4, 6], np.int32)
    return frozen(dict(logits=x, allow=tables.allow, states=tables.states, edges=tables.edges, index=index, out=out, out_len=out_len, state=state))


def bad_causes(V=101):
    """{what: a change of nine_rows() that makes row 4 (request 1, hand_automaton) - and nothing else - bad}"""
    case = nine_rows(V)
    S, E, G = case["states"].shape[0], case["edges"].shape[0], case["out"].shape[1]
    q0 = int(case["state"][BAD_REQUEST, 0])                                   # hand_automaton's state 0; its state 1 follows it
    first = int(case["states"][q0, 1])
    assert case["states"][q0, 2] == 1 and case["edges"][first].tolist() == [3, q0] and case["states"][q0, 0] == q0 + 1
    return {"i >= N": dict(index=(BAD_ROW, 8)), "g > G": dict(out_len=(BAD_REQUEST, G + 1)), "g < 0": dict(out_len=(BAD_REQUEST, -1)),
            "q >= S": dict(state=((BAD_REQUEST, 0), S)), "q < -1": dict(state=((BAD_REQUEST, 0), -2)),
            "k > g": dict(state=((BAD_REQUEST, 1), 3)), "k < 0": dict(state=((BAD_REQUEST, 1), -1)),
            "token = V": dict(out=((BAD_REQUEST, 1), V)), "token < 0": dict(out=((BAD_REQUEST, 0), -1)),
            "token whose bit is clear": dict(out=((BAD_REQUEST, slice(0, 2)), [8, 9])),
            "exception target = S": dict(edges=((first, 1), S)), "exception target < 0": dict(edges=((first, 1), -1)),
            "default of -1 taken": dict(states=((q0, 0), -1)),
            "exceptions behind E": dict(states=((q0, 1), E)), "exceptions in front of 0": dict(states=((q0, 1), -1)),
            "forced id = V": dict(states=((q0 + 1, 3), V)), "forced id whose bit is clear": dict(states=((q0 + 1, 3), 9))}
