"""Guided decoding: deterministic automata over token ids that restrict what a request of `serve` may generate.

A `TokenAutomaton` advances with every token a request stores; the logits of the ids its state does not allow go to -inf in
front of the draw.  Allowed-token sets, banned ids and banned sequences, "answer with one of these sequences" and stop sequences
are four builders on top of it (`allow_only`, `ban_sequences`, `one_of`, `stop_after`).  `compile_guides` lays any number of
automata out as three int32 tables for the device; `guide_logits` is the definition of `Tensor.guide_rows` and the numpy
backend.  Pure numpy; csrc/guide.hip restates `guide_logits` in one launch."""
import numpy as np

STATE_WORDS = 4                                           # a row of `states`: default next state, first exception, exceptions, forced id


class TokenAutomaton(object):
    """A DFA over the ids 0 .. vocab_size - 1.  State 0 exists from the start and is the start state.  In state s an id with a
    transition of its own (`add`) goes where that says; any other id goes to the state's default (`add_default`) if it has one;
    an id with neither - or one that `forbid` names - is NOT ALLOWED in s.  Accepting states are those a request may end in."""

    def __init__(self, vocab_size: int, accepting: bool = False):
        if int(vocab_size) != vocab_size or vocab_size < 1:
            raise ValueError("TokenAutomaton: vocab_size is an int >= 1 (got %r)" % (vocab_size,))
        self.vocab_size = int(vocab_size)
        self.accepting, self.default, self.edges = [], [], []
        self.add_state(accepting)

    def __len__(self):
        return len(self.accepting)

    def add_state(self, accepting: bool = False) -> int:
        self.accepting.append(bool(accepting))
        self.default.append(-1)
        self.edges.append({})
        return len(self.accepting) - 1

    def _state(self, s, what="state"):
        if int(s) != s or not 0 <= s < len(self):
            raise ValueError("TokenAutomaton: %s %r is none of the %d states" % (what, s, len(self)))
        return int(s)

    def _ids(self, ids):
        ids = np.asarray(ids).reshape(-1)
        if ids.size and (not np.issubdtype(ids.dtype, np.integer) or ids.min() < 0 or ids.max() >= self.vocab_size):
            raise ValueError("TokenAutomaton: ids are ints in 0 .. %d (got %s)" % (self.vocab_size - 1, ids[:8].tolist()))
        return ids.tolist()

    def add(self, s, ids, t) -> None:
        """the ids listed go from s to t"""
        s, t = self._state(s), self._state(t, "target")
        for v in self._ids(ids):
            self.edges[s][v] = t

    def forbid(self, s, ids) -> None:
        """the ids listed are not allowed in s, whatever its default"""
        s = self._state(s)
        for v in self._ids(ids):
            self.edges[s][v] = -1

    def add_default(self, s, t) -> None:
        """every id without a transition of its own goes from s to t"""
        self.default[self._state(s)] = self._state(t, "target")

    def step(self, s: int, v: int) -> int:
        """the state behind id v in state s, or -1 if v is not allowed there"""
        if not 0 <= v < self.vocab_size:
            return -1
        return self.edges[s].get(int(v), self.default[s])

    def walk(self, ids) -> int:
        """the state the ids lead to from the start, or -1 if one of them is not allowed where it stands"""
        s = 0
        for v in np.asarray(ids, np.int64).reshape(-1).tolist():
            s = self.step(s, v)
            if s < 0:
                return -1
        return s

    def accepts(self, ids) -> bool:
        s = self.walk(ids)
        return s >= 0 and self.accepting[s]


def _sequences(V, seqs, name):
    out = []
    for seq in seqs:
        seq = tuple(int(v) for v in (np.asarray(seq).reshape(-1).tolist()))
        if not seq or min(seq) < 0 or max(seq) >= V:
            raise ValueError("%s: every sequence has at least one id, each in 0 .. %d (got %s)" % (name, V - 1, list(seq)))
        out.append(seq)
    if not out:
        raise ValueError("%s: at least one sequence" % name)
    return out


def allow_only(V, ids) -> TokenAutomaton:
    """one accepting state that loops on `ids`: nothing else is ever allowed"""
    a = TokenAutomaton(V, accepting=True)
    ids = np.unique(np.asarray(ids).reshape(-1))
    if ids.size == 0:
        raise ValueError("allow_only: at least one id")
    a.add(0, ids, 0)
    return a


def _aho_corasick(V, seqs, name, stop):
    """the automaton whose states are the proper prefixes of `seqs` that end in none of them (the longest suffix of the history
    that still matters); an id that would complete a sequence is forbidden (stop=False) or leads to one final state (stop=True)"""
    seqs = _sequences(V, seqs, name)
    whole = set(seqs)
    ends = lambda w: any(w[k:] in whole for k in range(len(w)))                     # noqa: E731
    prefixes = sorted({seq[:k] for seq in seqs for k in range(len(seq))} - {()}, key=lambda w: (len(w), w))
    nodes = [()] + [w for w in prefixes if not ends(w)]
    number = {w: s for s, w in enumerate(nodes)}
    alphabet = sorted({v for seq in seqs for v in seq})
    a = TokenAutomaton(V, accepting=True)
    for _ in nodes[1:]:
        a.add_state(True)
    final = a.add_state(True) if stop else -1
    for w, s in number.items():
        a.add_default(s, 0)
        for v in alphabet:
            u = w + (v,)
            if ends(u):
                a.add(s, [v], final) if stop else a.forbid(s, [v])
                continue
            while u not in number:
                u = u[1:]
            if number[u]:
                a.add(s, [v], number[u])
    return a


def ban_sequences(V, seqs) -> TokenAutomaton:
    """none of `seqs` (single ids are sequences of length 1) ever occurs in what the request generates: the last id of a banned
    sequence is not allowed in the state that has matched the rest of it.  Every state is accepting"""
    return _aho_corasick(V, seqs, "ban_sequences", stop=False)


def stop_after(V, seqs) -> TokenAutomaton:
    """generation is free until one of `seqs` is complete; the state behind it is accepting and allows nothing else (the request
    must end).  The other states are accepting too"""
    return _aho_corasick(V, seqs, "stop_after", stop=True)


def one_of(V, seqs) -> TokenAutomaton:
    """the request emits one of `seqs` and then must end: a trie whose only accepting states are the ends of the sequences"""
    a = TokenAutomaton(V)
    for seq in _sequences(V, seqs, "one_of"):
        s = 0
        for v in seq:
            t = a.edges[s].get(v, -1)
            if t < 0:
                t = a.add_state()
                a.add(s, [v], t)
            s = t
        a.accepting[s] = True
    return a


class GuideTables(object):
    """what `compile_guides` returns: allow (S, W), states (S, 4), edges (E, 2), start (n,), all int32, and vocab_size"""

    def __init__(self, allow, states, edges, start, vocab_size):
        self.allow, self.states, self.edges, self.start, self.vocab_size = allow, states, edges, start, vocab_size

    def __iter__(self):
        return iter((self.allow, self.states, self.edges, self.start))


def compile_guides(guides, n: int, eos=None, vocab_size=None):
    """The device tables of n requests' guides.  guides: None (None is returned: nothing to build), one TokenAutomaton for every
    request, or a sequence of n entries that may include None.  Automata that are the same object are laid out once; states are
    numbered globally, automaton after automaton in the order of their first use.  Returns GuideTables:
      allow  int32 (S, W), W = ceil(V / 32): bit v % 32 of word v // 32 says that id v is allowed in the state.  With eos given
             the eos bit IS the state's accepting flag, whatever transitions name eos; the bits at and behind V are 0.
      states int32 (S, 4): the default next state or -1, the offset of the state's first exception in `edges`, the number of its
             exceptions, and the FORCED id - the one id the state allows when it allows exactly one, else -1.
      edges  int32 (E, 2): (id, next state), sorted by id within a state; one dummy row (0, 0) when there are none.
      start  int32 (n,): the global start state of the request's automaton, or -1 for an unguided request.
    Refused by name: an automaton whose vocab_size is not V (vocab_size=, default: the first automaton's), and a state that can
    be reached from its start and allows no id at all after the eos rule - a dead end: the request could neither go on nor end."""
    if guides is None:
        return None
    if isinstance(guides, TokenAutomaton):
        guides = [guides] * n
    guides = list(guides)
    if len(guides) != n or not all(g is None or isinstance(g, TokenAutomaton) for g in guides):
        raise ValueError("compile_guides: None, one TokenAutomaton, or %d entries that are TokenAutomata or None (got %d: %s)" % (
            n, len(guides), sorted({type(g).__name__ for g in guides})))
    distinct = []
    for g in guides:
        if g is not None and not any(g is d for d in distinct):
            distinct.append(g)
    if not distinct:
        return None
    V = distinct[0].vocab_size if vocab_size is None else int(vocab_size)
    if eos is not None and (int(eos) != eos or not 0 <= int(eos) < V):
        raise ValueError("compile_guides: eos is None or an id in 0 .. V - 1 = %d (got %r)" % (V - 1, eos))
    W = -(-V // 32)
    base, total = [], 0
    for k, a in enumerate(distinct):
        if a.vocab_size != V:
            raise ValueError("compile_guides: automaton %d has vocab_size = %d, not V = %d" % (k, a.vocab_size, V))
        base.append(total)
        total += len(a)
    allow, states, edges = np.zeros((total, W), np.uint32), np.full((total, STATE_WORDS), -1, np.int32), []
    for k, a in enumerate(distinct):
        reachable, frontier = {0}, [0]
        while frontier:
            s = frontier.pop()
            for t in list(a.edges[s].values()) + [a.default[s]]:
                if t >= 0 and t not in reachable:
                    reachable.add(t)
                    frontier.append(t)
        for s in range(len(a)):
            bits = np.zeros(W * 32, bool)
            if a.default[s] >= 0:
                bits[:V] = True
            own = sorted(a.edges[s].items())
            bits[[v for v, t in own if t < 0]] = False
            bits[[v for v, t in own if t >= 0]] = True
            if eos is not None:
                bits[int(eos)] = a.accepting[s]
            if s in reachable and not bits.any():
                raise ValueError("compile_guides: state %d of automaton %d is a dead end: it allows no id%s" % (
                    s, k, " and, without an eos, no end either" if eos is None else " and is not accepting"))
            allow[base[k] + s] = np.packbits(bits, bitorder="little").view("<u4")
            kept = [(v, base[k] + t) for v, t in own if t >= 0 and t != a.default[s]]
            allowed = np.flatnonzero(bits)
            states[base[k] + s] = (base[k] + a.default[s] if a.default[s] >= 0 else -1, len(edges), len(kept), int(allowed[0]) if allowed.size == 1 else -1)
            edges += kept
    edges = np.array(edges if edges else [(0, 0)], np.int32).reshape(-1, 2)
    start = np.array([-1 if g is None else base[[g is d for d in distinct].index(True)] for g in guides], np.int32)
    return GuideTables(allow.view(np.int32), states, edges, start, V)


def needs_eos(automaton) -> bool:
    """does the automaton have a state that allows nothing of its own, so that only an eos can follow it"""
    return any(automaton.default[s] < 0 and not any(t >= 0 for t in automaton.edges[s].values()) for s in range(len(automaton)))


def check_guide_rows_operands(logits, allow, states, edges, index, out, out_len, state):
    """the validated (rows, V, S, E, N, G) of a `guide_rows` call; the operands are tensors of either backend (shapes and dtypes
    only)"""
    shape, i32 = tuple(logits.shape), np.dtype(np.int32)
    if not np.issubdtype(np.dtype(logits.dtype), np.floating):
        raise ValueError("guide_rows: the logits must be floating point (got %s)" % np.dtype(logits.dtype))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[1] == 1)) or shape[-1] < 1:
        raise ValueError("guide_rows: the logits are (rows, V) or (rows, 1, V) with V >= 1 (got %s)" % (shape,))
    operands = (("allow", allow), ("states", states), ("edges", edges), ("index", index), ("out", out), ("out_len", out_len), ("state", state))
    for name, t in operands:
        if np.dtype(t.dtype) != i32:
            raise ValueError("guide_rows: %s must be int32 (got %s)" % (name, np.dtype(t.dtype)))
    V = shape[-1]
    W = -(-V // 32)
    shapes = [tuple(t.shape) for _, t in operands]
    S = shapes[0][0] if len(shapes[0]) == 2 else 0
    N = shapes[6][0] if len(shapes[6]) == 2 else 0
    if S < 1 or shapes[0] != (S, W) or shapes[1] != (S, STATE_WORDS) or len(shapes[2]) != 2 or shapes[2][0] < 1 or shapes[2][1] != 2:
        raise ValueError("guide_rows: allow (S, W) = (S, %d), states (S, %d), edges (E, 2) with S, E >= 1, as compile_guides lays them out for V = %d (got %s)" % (
            W, STATE_WORDS, V, shapes[:3]))
    if N < 1 or shapes[6] != (N, 2) or shapes[3] != (shape[0],) or len(shapes[4]) != 2 or shapes[4][0] != N or shapes[4][1] < 1 or shapes[5] != (N,):
        raise ValueError("guide_rows: index (rows,) = (%d,), out (N, G), out_len (N,), state (N, 2) with N, G >= 1 (got %s)" % (shape[0], shapes[3:]))
    return shape[0], V, S, shapes[2][0], N, shapes[4][1]


def guide_logits(logits, allow, states, edges, index, out, out_len, state):
    """The definition of `Tensor.guide_rows`: (y (rows, V), new_state (N, 2) int32, bad (rows,) bool).  logits (rows, V) float32 or
    float64; allow (S, W), states (S, 4), edges (E, 2) as `compile_guides` lays them out; index (rows,): row r names request
    i = index[r]; out (N, G), out_len (N,): the tokens every request has stored; state (N, 2): per request (q, k) - the state of its
    automaton behind its first k stored tokens.  Per row:
      1. i < 0 (a free row): untouched and unread;
      2. (q, k) = state[i]; q == -1: an unguided request - untouched, and not bad;
      3. the row is BAD when i >= N, g = out_len[i] is outside 0 .. G, q is outside [0, S) or k is outside 0 .. g;
      4. catch-up: for j = k .. g - 1 the state absorbs tok = out[i, j]: the row is BAD if tok is outside [0, V) or its bit is
         clear in q; q becomes the target of tok's exception among edges[first : first + count] (binary search) or else the
         state's default; the row is BAD if that range leaves [0, E] or the new q is outside [0, S) (a default of -1 taken);
      5. the row is BAD if the forced id f of the final q is outside -1 .. V - 1, or f >= 0 with its bit clear in q;
      6. a BAD row writes nothing - neither logits nor state - and is reported in bad[r]; the others are computed;
      7. every other row stores state[i] = (q, g), sets y[r, v] = -inf wherever the bit of v is clear in q, keeps every allowed
         value byte for byte (NaN payloads and -0.0 included) and stores +0.0 at f if f >= 0.
    Rows that name the same request compute the same pair.  Calling it again on its results changes nothing."""
    x = np.asarray(logits)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("guide_logits: float32 or float64 logits (got %s)" % x.dtype)
    allow, states, edges = (np.ascontiguousarray(a, np.int32) for a in (allow, states, edges))
    index, out_len = (np.asarray(a, np.int64).reshape(-1) for a in (index, out_len))
    out, state = np.asarray(out), np.asarray(state, np.int32)
    if x.ndim != 2 or x.shape[1] < 1 or allow.ndim != 2 or allow.shape[1] != -(-x.shape[1] // 32) or states.shape != (allow.shape[0], STATE_WORDS) or \
            edges.ndim != 2 or edges.shape[1] != 2 or index.shape != (x.shape[0],) or out.ndim != 2 or state.ndim != 2 or state.shape[1] != 2 or \
            not (out.shape[0] == out_len.size == state.shape[0]):
        raise ValueError("guide_logits: logits (rows, V), allow (S, ceil(V / 32)), states (S, 4), edges (E, 2), index (rows,), out (N, G), out_len (N,), "
                         "state (N, 2), got %s" % ([a.shape for a in (x, allow, states, edges, index, out, out_len, state)],))
    (rows, V), S, E, (N, G) = x.shape, allow.shape[0], edges.shape[0], out.shape
    words = allow.view(np.uint32)
    allowed = lambda q, v: bool((int(words[q, v >> 5]) >> (v & 31)) & 1)              # noqa: E731
    y, new_state, bad = x.copy(), state.copy(), np.zeros(rows, bool)
    for r in range(rows):
        i = int(index[r])
        if i < 0:
            continue
        if i >= N:
            bad[r] = True
            continue
        q, k = int(state[i, 0]), int(state[i, 1])
        if q == -1:
            continue
        g = int(out_len[i])
        if not (0 <= g <= G and 0 <= q < S and 0 <= k <= g):
            bad[r] = True
            continue
        for j in range(k, g):
            tok = int(out[i, j])
            if not 0 <= tok < V or not allowed(q, tok):
                bad[r] = True
                break
            default, first, count = (int(w) for w in states[q, :3])
            if first < 0 or count < 0 or first + count > E:
                bad[r] = True
                break
            at = first + int(np.searchsorted(edges[first:first + count, 0], tok))
            q = int(edges[at, 1]) if at < first + count and edges[at, 0] == tok else default
            if not 0 <= q < S:
                bad[r] = True
                break
        forced = int(states[q, 3]) if not bad[r] else -1
        if not bad[r] and (forced < -1 or forced >= V or (forced >= 0 and not allowed(q, forced))):
            bad[r] = True
        if bad[r]:
            continue
        new_state[i] = (q, g)
        clear = np.unpackbits(words[q].view(np.uint8), bitorder="little")[:V] == 0
        y[r, clear] = -np.inf
        if forced >= 0:
            y[r, forced] = 0.0
    return y, new_state, bad
