"""What test_paged_cpu.py and test_hip_paged.py share: `serve_commit_paged` written out by hand in plain python from the words of
its definition (independent of the numpy backend's op), states that mix releases, admissions and a pool that runs dry, the
schedule of the paged `serve` in plain python, the seven prompts of serve_cases behind a common prefix of 9 tokens with the float64
greedy continuation of every prefixed prompt ALONE (computed once per process and never changed afterwards), one mixed model step
against a paged cache with shuffled tables, and the runs through `serve` on any tensor class."""
import functools
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc
import serve_cases as sc

bert, CFG = dc.bert, dc.CFG
BLOCK, MAX_BLOCKS = 4, 6                 # the serving runs: 24 positions a slot, reached through tables of 6 blocks of 4
PREFIX, PREFIX_SEED = 9, 1               # 9 common tokens in front of every prompt: F = 2 full blocks at B = 4
NAMES = sc.NAMES + ("block_table", "held", "free")


# ---- serve_commit_paged by hand -------------------------------------------------------------------------------------------------

def commit_by_hand(state, nxt, block_size, prefix_blocks, eos):
    """the issue's words on copies: ({name: array}, a slot raised the flag).  Step 1 of serve_commit for every slot, with the
    release of a finished slot's blocks; then the admission in slot and queue order with a reservation; then the slots' words"""
    st = {k: v.copy() for k, v in state.items()}
    b, m = st["ids"].shape
    N, P = st["prompts"].shape
    G, B, F = st["out"].shape[1], block_size, prefix_blocks
    max_blocks, num_blocks = st["block_table"].shape[1], len(st["free"]) - 1
    capacity = max_blocks * B
    nxt, free = nxt.reshape(-1), st["free"]
    stack_ok = 0 <= free[0] <= num_blocks
    slots = []
    for s in range(b):
        r, t, n, tokens, bad, ended = int(st["req"][s]), 0, 0, [], False, False
        if r >= 0:
            t = int(st["pos"][s]) + int(st["count"][s])
            if r >= N or t < 0 or t > capacity:
                bad = True
            elif t < st["prompt_len"][r]:
                n = min(m, int(st["prompt_len"][r]) - t)
                bad = t + n > P
                tokens = [] if bad else st["prompts"][r, t:t + n].tolist()
            else:
                g = int(st["out_len"][r])
                if not 0 <= g < G:
                    bad = True
                else:
                    st["out"][r, g] = nxt[s]
                    st["out_len"][r] = g + 1
                    if (eos is not None and eos >= 0 and nxt[s] == eos) or g + 1 == st["budget"][r]:
                        st["queue"][1] += 1
                        r, ended = -1, True
                    else:
                        n, tokens = 1, [int(nxt[s])]
        slots.append(dict(r=r, t=t, n=n, tokens=tokens, bad=bad, ended=ended))
    # release, slots in slot order and blocks in table order; a slot out of its bounds releases nothing
    releasing = []
    for s, slot in enumerate(slots):
        if slot["ended"]:
            held = int(st["held"][s])
            blocks = st["block_table"][s, F:max(held, F)].tolist() if 0 <= held <= max_blocks else None
            if not stack_ok or blocks is None or any(not 0 <= e < num_blocks for e in blocks):
                slot["bad"] = True
            else:
                releasing.append((s, blocks))
    if stack_ok and free[0] + sum(len(blocks) for _, blocks in releasing) > num_blocks:        # free[0] would leave 0 .. num_blocks
        for s, _ in releasing:
            slots[s]["bad"] = True
        releasing = []
    for s, blocks in releasing:
        for e in blocks:
            free[1 + free[0]] = e
            free[0] += 1
        st["block_table"][s] = -1
        st["held"][s] = 0
    # admission with a reservation: no overtaking
    stopped = False
    for s, slot in enumerate(slots):
        if slot["bad"] or slot["r"] >= 0:
            continue
        slot["t"] = 0
        if stopped or not 0 <= st["queue"][0] < N:
            continue
        r = int(st["queue"][0])
        need = -(-(int(st["prompt_len"][r]) + int(st["budget"][r]) - 1) // B) - F
        n = min(m, int(st["prompt_len"][r]) - F * B)
        if not stack_ok or need < 0 or F + need > max_blocks or n < 1 or F * B + n > P:
            st["queue"][0] += 1
            slot["bad"] = True
        elif need > free[0]:
            stopped = True
        else:
            st["queue"][0] += 1
            for i in range(need):
                st["block_table"][s, F + i] = free[free[0]]
                free[0] -= 1
            st["block_table"][s, :F] = np.arange(F)
            st["held"][s] = F + need
            slot.update(r=r, t=F * B, n=n, tokens=st["prompts"][r, F * B:F * B + n].tolist())
    flag = False
    for s, slot in enumerate(slots):
        r, t, n = slot["r"], slot["t"], slot["n"]
        if slot["bad"] or t + n > capacity:
            st["count"][s], flag = 0, True
            continue
        st["req"][s], st["pos"][s], st["count"][s] = r, t, n
        st["ids"][s] = slot["tokens"] + [0] * (m - n)
        st["position_ids"][s] = [t + i for i in range(n)] + [0] * (m - n)
        st["last"][s] = s * m + max(n - 1, 0)
    return st, flag


def needs(lengths, budgets, block_size, prefix_blocks):
    return [-(-(int(length) + int(budget) - 1) // block_size) - prefix_blocks for length, budget in zip(lengths, budgets)]


def commit_state(b, waiting, seed, prefix_blocks, spare, m=4, eos=None, block_size=4, max_blocks=6):
    """a state that mixes, over the b slots in turn: a slot in the middle of its prompt, one whose step held its last prompt
    tokens, decoding slots that go on, one whose budget ends and one that draws `eos` (both release their blocks), free slots -
    with `waiting` requests behind those the slots hold.  Every slot that holds a request holds the blocks of its whole life
    behind the `prefix_blocks` shared ones, drawn from a shuffled pool (tables are non-monotone and interleaved); `spare` blocks are
    on the stack, shuffled - with few of them the admissions of the commit need the blocks it has just released, and may stop.
    Returns ({name: array}, nxt (b, 1))"""
    rng = np.random.RandomState(seed)
    B, F = block_size, prefix_blocks
    N, P, G = b + waiting, F * B + 9, 5
    st = dict(prompts=rng.randint(1, 90, (N, P)).astype(np.int32), prompt_len=(F * B + rng.randint(1, 10, N)).astype(np.int32),
              budget=rng.randint(2, G + 1, N).astype(np.int32), out=np.full((N, G), sc.PAD, np.int32), out_len=np.zeros(N, np.int32),
              queue=np.array([b, 0], np.int32), req=np.full(b, -1, np.int32), pos=np.zeros(b, np.int32), count=np.zeros(b, np.int32),
              ids=rng.randint(0, 90, (b, m)).astype(np.int32), position_ids=rng.randint(0, 9, (b, m)).astype(np.int32),
              last=rng.randint(0, 9, b).astype(np.int32), block_table=np.full((b, max_blocks), -1, np.int32), held=np.zeros(b, np.int32))
    nxt = rng.randint(20, 90, (b, 1)).astype(np.int32)
    need = needs(st["prompt_len"], st["budget"], B, F)
    assert max(need) + F <= max_blocks
    kinds = [s % 7 for s in range(b)]
    running = [s for s in range(b) if kinds[s] != 5]
    num_blocks = F + sum(need[i] for i in range(len(running))) + spare
    pool = (F + rng.permutation(num_blocks - F)).tolist()
    for r, s in enumerate(running):
        kind, length = kinds[s], int(st["prompt_len"][r])
        own = length - F * B
        st["req"][s], st["held"][s] = r, F + need[r]
        st["block_table"][s, :F] = np.arange(F)
        st["block_table"][s, F:F + need[r]] = [pool.pop() for _ in range(need[r])]
        if kind == 0 and own > 1:                    # in the middle of its prompt
            st["pos"][s], st["count"][s] = F * B, min(m, own - 1)
        elif kind in (0, 1):                         # the step held its last prompt tokens
            st["pos"][s], st["count"][s] = max(length - m, F * B), min(m, own)
        else:                                        # decoding: g tokens out, the last of them fed in this step
            g = int(rng.randint(1, st["budget"][r]))
            if kind == 3:
                g = int(st["budget"][r]) - 1         # its budget ends with this token
            st["out"][r, :g], st["out_len"][r] = rng.randint(20, 90, g), g
            st["pos"][s], st["count"][s] = length + g - 1, 1
            if kind == 4 and eos is not None:
                nxt[s] = eos
    for s in range(b):
        if kinds[s] == 5:                            # free: what it holds of a position is overwritten
            st["pos"][s], st["count"][s] = rng.randint(0, 9), rng.randint(0, m + 1)
    st["queue"][0] = len(running)
    st["free"] = np.array([len(pool)] + pool + [0] * (num_blocks - len(pool)), np.int32)
    return st, nxt


def dry_pool_state():
    """three free slots, three waiting requests that need 1, 3 and 1 blocks (B = 4, F = 0), three blocks on the stack: the first is
    admitted, the second does not fit the two blocks left - and the third, which would, must NOT overtake it"""
    st = dict(prompts=np.arange(1, 31, dtype=np.int32).reshape(3, 10), prompt_len=np.array([3, 10, 2], np.int32), budget=np.array([2, 2, 3], np.int32),
              out=np.full((3, 3), sc.PAD, np.int32), out_len=np.zeros(3, np.int32), queue=np.zeros(2, np.int32), req=np.full(3, -1, np.int32),
              pos=np.zeros(3, np.int32), count=np.zeros(3, np.int32), ids=np.full((3, 4), 7, np.int32), position_ids=np.full((3, 4), 7, np.int32),
              last=np.zeros(3, np.int32), block_table=np.full((3, 3), -1, np.int32), held=np.zeros(3, np.int32),
              free=np.array([3, 4, 0, 2, 0, 0], np.int32))
    return st, np.zeros((3, 1), np.int32)


def commit_on(T, state, nxt, block_size, prefix_blocks, eos):
    """`serve_commit_paged` on tensor class T: ({name: tensor}, the IndexError of a flagged slot on the numpy backend or None)"""
    tensors = sc.upload(T, state)
    t_nxt = T.from_numpy(nxt.copy(), requires_grad=False)
    error = None
    try:
        assert t_nxt.serve_commit_paged(*(tensors[k] for k in NAMES), block_size, prefix_blocks, eos=eos) is None
    except IndexError as e:
        error = e
    return tensors, error


# ---- the schedule of the paged serve in plain python ----------------------------------------------------------------------------

def simulate(lengths, emitted, budgets, slots, chunk, block_size, num_blocks, prefix_blocks=0):
    """the steps the paged `serve` takes with poll=1: serve_cases.simulate with a count of free blocks - a request reserves
    ceil((length + budget - 1) / B) - F blocks when it is admitted (by its BUDGET, whatever it emits), a finished one returns them
    in the same commit, and the first waiting request that does not fit stops the admission of that commit"""
    n_requests, start = len(lengths), prefix_blocks * block_size
    need = needs(lengths, budgets, block_size, prefix_blocks)
    state = dict(req=[-1] * slots, pos=[0] * slots, count=[0] * slots, drawn=[0] * n_requests, waiting=0, finished=0, free=num_blocks - prefix_blocks)

    def commit():
        for s in range(slots):
            r, t, n = state["req"][s], 0, 0
            if r >= 0:
                t = state["pos"][s] + state["count"][s]
                if t < lengths[r]:
                    n = min(chunk, lengths[r] - t)
                else:
                    state["drawn"][r] += 1
                    if state["drawn"][r] == emitted[r]:
                        state["finished"] += 1
                        state["free"] += need[r]
                        r = -1
                    else:
                        n = 1
            if r < 0:
                t = n = 0
            state["req"][s], state["pos"][s], state["count"][s] = r, t, n
        for s in range(slots):
            if state["req"][s] < 0 and state["waiting"] < n_requests:
                r = state["waiting"]
                if need[r] > state["free"]:
                    break
                state["waiting"] += 1
                state["free"] -= need[r]
                state["req"][s], state["pos"][s], state["count"][s] = r, start, min(chunk, lengths[r] - start)

    commit()
    steps = 0
    while state["finished"] < n_requests:
        steps += 1
        commit()
        assert steps <= sum(-(-length // chunk) + e for length, e in zip(lengths, emitted))
    assert state["free"] == num_blocks - prefix_blocks
    return steps


# ---- prompts behind a common prefix ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def prefixed_prompts():
    prefix = np.random.RandomState(PREFIX_SEED).randint(0, CFG["vocab_size"], PREFIX).astype(np.int32)
    return [np.concatenate([prefix, p]) for p in sc.prompts()]


@functools.lru_cache(maxsize=None)
def prefixed_reference(new=sc.BUDGET):
    """serve_cases.greedy_reference for the prefixed prompts: greedy decoding of each ALONE by a full float64 recompute per token"""
    model64, model32 = dc.make_model(CpuTensor, np.float64, sc.SEED), dc.make_model(CpuTensor, np.float32, sc.SEED)
    tokens, margin, deviation = [], np.inf, 0.0
    for prompt in prefixed_prompts():
        seq = prompt[None, :].copy()
        for _ in range(new):
            l64, l32 = dc.full_logits(model64, seq)[:, -1], dc.full_logits(model32, seq)[:, -1]
            top = np.sort(l64, axis=-1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
            deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
            seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
        tokens.append(seq[0, len(prompt):])
    return tokens, margin, deviation


def assert_prefixed_margins_rule_out_ties():
    """decode_cases' rule, from the references alone: margin >= 100 x the float32 deviation"""
    tokens, margin, deviation = prefixed_reference()
    print("prefixed prompts: top-2 margin %.3g, float32 deviation %.3g" % (margin, deviation))
    assert margin >= 100 * deviation, "prefix seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick another seed" % (
        PREFIX_SEED, margin, deviation)
    return tokens


# ---- serve over a paged cache ---------------------------------------------------------------------------------------------------

def tight_blocks(rows, budgets, prefix_blocks=0):
    """the smallest pool the tests use: the shared blocks, the largest single need, and one more"""
    budgets = [budgets] * len(rows) if np.ndim(budgets) == 0 else budgets
    return prefix_blocks + max(needs([len(p) for p in rows], budgets, BLOCK, prefix_blocks)) + 1


def run_serve(T, slots, chunk, num_blocks, model=None, budgets=sc.BUDGET, eos=sc.EOS, rows=None, **options):
    """(out, out_len, stats, cache) of the paged `serve` over the seven prompts (or `rows`) on tensor class T: blocks of BLOCK positions,
    tables of MAX_BLOCKS, a pool of num_blocks"""
    model = dc.make_model(T, seed=sc.SEED) if model is None else model
    cache = nn.PagedKVCache(CFG["num_hidden_layers"], slots, num_blocks, BLOCK, CFG["hidden_size"], MAX_BLOCKS, like=model.cls.predictions.bias)
    (out, out_len), stats = bert.serve(model, sc.prompts() if rows is None else rows, budgets, slots=slots, chunk=chunk, eos_token_id=eos,
                                       pad_token_id=sc.PAD, cache=cache, **options)
    assert out.dtype == np.int32 and out_len.dtype == np.int32 and isinstance(out, T) and isinstance(out_len, T)
    assert stats["num_blocks"] == num_blocks and stats["block_size"] == BLOCK
    return out.numpy().copy(), out_len.numpy().copy(), stats, cache


def assert_no_block_leaked(cache, prefix_blocks=0):
    """after a run every block behind the shared ones is back on the stack, once, and no table names anything"""
    free = cache.free.numpy()
    n = cache.num_blocks - prefix_blocks
    assert free[0] == n and sorted(free[1:1 + n].tolist()) == list(range(prefix_blocks, cache.num_blocks)), free.tolist()
    assert (cache.block_table.numpy() == -1).all() and (cache.held.numpy() == 0).all()


# ---- one mixed model step against shuffled tables -------------------------------------------------------------------------------

MIXED_TABLES = ((9, 2, 11, 5, 0), (7, 1, -1, -1, -1), (3, 10, 6, 8, -1), (4, 12, 13, 14, 15))      # B = 4: non-monotone, interleaved; slot 3 fills its 5 blocks


def mixed_step(T, model=None, dtype=np.float32):
    """serve_cases.mixed_step against an nn.PagedKVCache of 5 blocks of 4 per table (20 >= CAPACITY positions): the logits of the real rows of ONE
    `model(ids, cache=, append=True, count=)` call per sequence; the tokens in front enter through the same call, one slot at a time"""
    seqs, b = sc.mixed_sequences(), len(sc.MIXED)
    model = dc.make_model(T, dtype, sc.SEED) if model is None else model
    cache = nn.PagedKVCache(CFG["num_hidden_layers"], b, 16, 4, CFG["hidden_size"], 5, like=model.cls.predictions.bias)
    tensor = lambda a: T.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    cache.block_table[:] = tensor(np.array(MIXED_TABLES, np.int32))
    for r, (t, n) in enumerate(sc.MIXED):
        if t:
            ids, count = np.zeros((b, t), np.int32), np.zeros(b, np.int32)
            ids[r], count[r] = seqs[r][:t], t
            model(tensor(ids), cache=cache, append=True, count=tensor(count))
            cache.advance(tensor(count))
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in sc.MIXED])
    ids, count = np.full((b, sc.MIXED_M), 7, np.int32), np.array([n for _, n in sc.MIXED], np.int32)
    for r, (t, n) in enumerate(sc.MIXED):
        ids[r, :n] = seqs[r][t:]
    logits = model(tensor(ids), cache=cache, append=True, count=tensor(count))
    assert tuple(logits.shape) == (b, sc.MIXED_M, CFG["vocab_size"]) and logits.ctx is None          # outside the tape
    logits = logits.numpy()
    return [logits[r, :n].copy() for r, (_, n) in enumerate(sc.MIXED)], cache
