"""What test_serve_packed_cpu.py and test_hip_serve_packed.py share: `serve_commit_packed` and the token-packed schedule of
`serve(token_budget=)` written out by hand in plain python, the mixed commit states of serve_cases adapted to the packed words,
and the shapes of the packed attention launch.  The prompts, the float64 continuations and the margin rule are serve_cases'."""
import numpy as np
import serve_cases as sc

NAMES = ("prompts", "prompt_len", "budget", "out", "out_len", "queue", "req", "pos", "count", "cu", "ids", "position_ids", "last")
SLOTS = (1, 7, 64, 65, 200, 1024)               # the wave edges of the three scans: one lane, a part of a wave, 64, 64 + 1, 3 + waves, all 16
# (chunk, token budget as a function of the slots) of the runs
RUNS = ((1, lambda slots: slots), (4, lambda slots: slots + 3), (16, lambda slots: slots + 16), (16, lambda slots: slots * 16))


def budgets_of(slots, chunk):
    """the token budgets of the commit tests: every slot one row, a few rows to share, never binding"""
    return (slots, slots + 3, slots * chunk)


# ---- serve_commit_packed by hand ------------------------------------------------------------------------------------------------

def commit_packed_by_hand(state, nxt, capacity, chunk, eos):
    """the issue's words, slot by slot, on copies: ({name: array}, a slot raised the flag)"""
    st = {k: v.copy() for k, v in state.items()}
    b, T = st["req"].shape[0], st["ids"].shape[1]
    N, P = st["prompts"].shape
    G = st["out"].shape[1]
    nxt, flag = nxt.reshape(-1), False
    wants = []                                   # per slot: None (a bad slot) or [r, t, want, tokens, "decode" | "prefill" | "idle"]
    # steps 1 and 2: what every slot wants, in slot order
    for s in range(b):
        r, t, want, tokens, kind, bad = int(st["req"][s]), 0, 0, [], "idle", False
        if r >= 0:
            t = int(st["pos"][s]) + int(st["count"][s])
            if r >= N or t < 0 or t > capacity:
                bad = True
            elif t < st["prompt_len"][r]:
                want, kind = min(chunk, int(st["prompt_len"][r]) - t), "prefill"
                bad = t + want > P
                tokens = [] if bad else st["prompts"][r, t:t + want].tolist()
            else:
                g = int(st["out_len"][r])
                if not 0 <= g < G:
                    bad = True
                else:
                    st["out"][r, g] = nxt[s]
                    st["out_len"][r] = g + 1
                    if (eos is not None and eos >= 0 and nxt[s] == eos) or g + 1 == st["budget"][r]:
                        st["queue"][1] += 1
                        r = -1
                    else:
                        want, tokens, kind = 1, [int(nxt[s])], "decode"
        if not bad and r < 0:
            t = 0
            if 0 <= st["queue"][0] < N:
                r = int(st["queue"][0])
                st["queue"][0] += 1
                want, kind = min(chunk, int(st["prompt_len"][r])), "prefill"
                bad = not 0 <= want <= P
                tokens = [] if bad else st["prompts"][r, :want].tolist()
        if bad or t + want > capacity:
            wants.append(None)
            flag = True
        else:
            wants.append([r, t, want, tokens, kind])
    # step 3: the budget
    left = T - sum(1 for w in wants if w is not None and w[4] == "decode")
    grants = []
    for w in wants:
        if w is None:
            grants.append(0)
        elif w[4] == "decode":
            grants.append(1)
        else:
            n = min(w[2], left)
            left -= n
            grants.append(n)
    assert left >= 0
    # step 4: the words
    ids, position_ids, row = [0] * T, [0] * T, 0
    for s, (w, n) in enumerate(zip(wants, grants)):
        st["cu"][s] = row
        if w is None:
            st["count"][s] = 0
            continue
        r, t, want, tokens, kind = w
        st["req"][s], st["pos"][s], st["count"][s] = r, t, n
        for i in range(n):
            ids[row + i], position_ids[row + i] = tokens[i], t + i
        st["last"][s] = min(row + max(n - 1, 0), T - 1)
        row += n
    st["cu"][b] = row
    st["ids"][0], st["position_ids"][0] = ids, position_ids
    return st, flag


def packed_state(b, waiting, seed, T, chunk=4, capacity=12, eos=None, overflow=False):
    """serve_cases.commit_state (m = chunk) with the packed words in place of the (b, m) ones: ids / position_ids (1, T) and cu
    (b + 1,), all holding what a commit must overwrite"""
    st, nxt = sc.commit_state(b, waiting, seed, m=chunk, capacity=capacity, eos=eos, overflow=overflow)
    rng = np.random.RandomState(seed + 1)
    st["ids"], st["position_ids"] = rng.randint(1, 90, (1, T)).astype(np.int32), rng.randint(1, 9, (1, T)).astype(np.int32)
    st["cu"] = rng.randint(1, 9, b + 1).astype(np.int32)
    return {k: st[k] for k in NAMES}, nxt


def tight_state():
    """four slots, chunk 4, T = 6: slot 0 decodes, slots 1 and 2 are inside their prompts and want 4 rows each, slot 3 is free and
    nobody waits.  R = 5: slot 1 gets 4, the budget runs out in the middle of slot 2's want (1 of 4), the buffer is full and the
    idle slot 3 starts at row T - its `last` is clamped to T - 1.  Returns (state, nxt, T, chunk, capacity)"""
    st = dict(prompts=np.arange(1, 37, dtype=np.int32).reshape(3, 12), prompt_len=np.array([2, 12, 9], np.int32), budget=np.array([4, 4, 4], np.int32),
              out=np.full((3, 4), sc.PAD, np.int32), out_len=np.array([1, 0, 0], np.int32), queue=np.array([3, 0], np.int32),
              req=np.array([0, 1, 2, -1], np.int32), pos=np.array([2, 0, 4, 7], np.int32), count=np.array([1, 4, 0, 3], np.int32),
              cu=np.full(5, 77, np.int32), ids=np.full((1, 6), 77, np.int32), position_ids=np.full((1, 6), 77, np.int32), last=np.full(4, 77, np.int32))
    return st, np.array([50, 51, 52, 53], np.int32), 6, 4, 16


def upload(T, state, strided_out=False):
    return sc.upload(T, state, strided_out)


def commit_on(T, state, nxt, capacity, chunk, eos, strided_out=False):
    """`serve_commit_packed` on tensor class T: ({name: tensor}, the IndexError the numpy backend raised at once or None)"""
    tensors = upload(T, state, strided_out)
    t_nxt = T.from_numpy(nxt.copy(), requires_grad=False)
    error = None
    try:
        assert t_nxt.serve_commit_packed(*(tensors[k] for k in NAMES), capacity, chunk, eos=eos) is None
    except IndexError as e:
        error = e
    return tensors, error


# ---- the packed schedule --------------------------------------------------------------------------------------------------------

def simulate_packed(lengths, emitted, slots, chunk, T):
    """the steps `serve(token_budget=T)` takes with poll=1 when request r has lengths[r] prompt tokens and emits emitted[r] tokens:
    serve_cases.simulate with the budget - a decoding slot takes a row, the prefilling slots share T - (decoding slots) rows in
    slot order, a slot granted nothing stays where it is"""
    n_requests = len(lengths)
    state = dict(req=[-1] * slots, pos=[0] * slots, count=[0] * slots, drawn=[0] * n_requests, waiting=0, finished=0)

    def commit():
        wants = []
        for s in range(slots):
            r, t, want, decode = state["req"][s], 0, 0, False
            if r >= 0:
                t = state["pos"][s] + state["count"][s]
                if t < lengths[r]:
                    want = min(chunk, lengths[r] - t)
                else:
                    state["drawn"][r] += 1
                    if state["drawn"][r] == emitted[r]:
                        state["finished"] += 1
                        r = -1
                    else:
                        want, decode = 1, True
            if r < 0 and state["waiting"] < n_requests:
                r, t = state["waiting"], 0
                state["waiting"] += 1
                want = min(chunk, lengths[r])
            if r < 0:
                t = want = 0
            wants.append((r, t, want, decode))
        left = T - sum(1 for w in wants if w[3])
        for s, (r, t, want, decode) in enumerate(wants):
            n = 1 if decode else min(want, left)
            if not decode:
                left -= n
            state["req"][s], state["pos"][s], state["count"][s] = r, t, n

    commit()
    steps = 0
    while state["finished"] < n_requests:
        steps += 1
        commit()
        assert steps <= sum(length + e for length, e in zip(lengths, emitted))
    return steps


# ---- the packed attention launch ------------------------------------------------------------------------------------------------

PACKED_M_MAX = 33
# token rows of the launch per capacity.  48 for the first set of slots (10 rows in use, 38 belong to nobody, T exceeds the capacity
# of 17).  The second set owns 1 + 33 + 0 + 3 + 33 = 70 rows, which no buffer of 48 holds: it keeps every slot and takes 80 rows
PACKED_T = {17: 48, 160: 80}
# capacity -> the slots' (tokens already in the cache, tokens of this step), in slot order
LAUNCH_CASES = {17: ((6, 1), (0, 4), (14, 0), (12, 5)),
                # the seam at, before and behind the 128-key chunk edge; an element of two query blocks whose second holds one row;
                # slots that start at flat rows 1, 34, 37: no multiples of 32
                160: ((127, 1), (126, 33), (0, 0), (128, 3), (95, 33))}


def cu_of(slots):
    return np.concatenate([[0], np.cumsum([n for _, n in slots])]).astype(np.int32)
