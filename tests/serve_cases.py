"""What test_serve_cpu.py and test_hip_serve.py share: seven prompts of different lengths for the model of decode_cases, the
float64 greedy continuation of every prompt ALONE (computed once per process and never changed afterwards), `serve_commit` and
the schedule of `serve` written out by hand in plain python, and the runs through `serve` / one mixed model step on any tensor
class."""
import functools
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc

bert, CFG = dc.bert, dc.CFG
SEED = 3                                # model and ids (ragged_cases' seed): no greedy step of any prompt alone is a near-tie
BUDGET, EOS, CAPACITY, PAD = 6, 18, 17, 100
BUDGETS = (6, 3, 6, 6, 6, 1, 6)         # a budget per request, for the run without an end-of-sequence id
EMITTED = (6, 6, 6, 1, 2, 6, 5)         # tokens the float64 references emit under BUDGET with EOS: both stops and the budget occur
SLOTS, CHUNKS = (1, 3, 7), (1, 4, 16)


@functools.lru_cache(maxsize=None)
def prompts():
    ids = dc.parameters(SEED)[1]
    return [ids[0, :5].copy(), ids[1, :2].copy(), ids[0, 4:11].copy(), ids[1, 7:8].copy(), ids[1, 3:12].copy(), ids[0, 12:15].copy(),
            ids[1, 9:15].copy()]


@functools.lru_cache(maxsize=None)
def greedy_reference(new=BUDGET):
    """greedy decoding of each prompt alone at batch 1 by a full float64 recompute per token: ([tokens (new,)] per prompt, the
    smallest top-2 logit margin of any step, the largest deviation of the float32 full forward's last-row logits from float64)"""
    model64, model32 = dc.make_model(CpuTensor, np.float64, SEED), dc.make_model(CpuTensor, np.float32, SEED)
    tokens, margin, deviation = [], np.inf, 0.0
    for prompt in prompts():
        seq = prompt[None, :].copy()
        for _ in range(new):
            l64, l32 = dc.full_logits(model64, seq)[:, -1], dc.full_logits(model32, seq)[:, -1]
            top = np.sort(l64, axis=-1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
            deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
            seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
        tokens.append(seq[0, len(prompt):])
    return tokens, margin, deviation


def assert_margins_rule_out_ties():
    """decode_cases' rule, from the references alone: margin >= 100 x the float32 deviation"""
    tokens, margin, deviation = greedy_reference()
    print("top-2 margin %.3g, float32 deviation %.3g" % (margin, deviation))
    assert margin >= 100 * deviation, "seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick another seed" % (SEED, margin, deviation)
    return tokens


def expected(tokens, budgets, eos):
    """(out (N, G), out_len (N,)) that the reference tokens of each prompt alone imply: cut behind its EOS, or at its budget"""
    budgets = [budgets] * len(tokens) if np.ndim(budgets) == 0 else list(budgets)
    out, out_len = np.full((len(tokens), max(budgets)), PAD, np.int32), []
    for r, (toks, budget) in enumerate(zip(tokens, budgets)):
        toks = toks[:budget].tolist()
        n = toks.index(eos) + 1 if eos is not None and eos in toks else len(toks)
        out[r, :n] = toks[:n]
        out_len.append(n)
    return out, np.array(out_len, np.int32)


def run_serve(T, slots, chunk, model=None, budgets=BUDGET, eos=EOS, **options):
    """(out, out_len, stats) of `serve` over the seven prompts on tensor class T with a cache of CAPACITY positions"""
    model = dc.make_model(T, seed=SEED) if model is None else model
    cache = nn.KVCache(CFG["num_hidden_layers"], slots, CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    (out, out_len), stats = bert.serve(model, prompts(), budgets, slots=slots, chunk=chunk, eos_token_id=eos, pad_token_id=PAD, cache=cache, **options)
    assert out.dtype == np.int32 and out_len.dtype == np.int32 and isinstance(out, T) and isinstance(out_len, T)
    return out.numpy().copy(), out_len.numpy().copy(), stats


def simulate(lengths, emitted, slots, chunk):
    """the steps `serve` takes with poll=1 when request r has lengths[r] prompt tokens and emits emitted[r] tokens: the schedule of
    the definition in plain python - a slot works through its prompt in pieces of `chunk`, draws a token per step from the step
    that holds its last prompt token on, is freed by its last token and refilled by the same commit"""
    n_requests = len(lengths)
    state = dict(req=[-1] * slots, pos=[0] * slots, count=[0] * slots, drawn=[0] * n_requests, waiting=0, finished=0)

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
                        r = -1
                    else:
                        n = 1
            if r < 0 and state["waiting"] < n_requests:
                r, t = state["waiting"], 0
                state["waiting"] += 1
                n = min(chunk, lengths[r])
            if r < 0:
                t = n = 0
            state["req"][s], state["pos"][s], state["count"][s] = r, t, n

    commit()
    steps = 0
    while state["finished"] < n_requests:
        steps += 1
        commit()
        assert steps <= sum(-(-length // chunk) + e for length, e in zip(lengths, emitted))
    return steps


# ---- serve_commit by hand ---------------------------------------------------------------------------------------------------

NAMES = ("prompts", "prompt_len", "budget", "out", "out_len", "queue", "req", "pos", "count", "ids", "position_ids", "last")


def commit_by_hand(state, nxt, capacity, eos):
    """the issue's words, slot by slot, on copies: ({name: array}, a slot raised the flag)"""
    st = {k: v.copy() for k, v in state.items()}
    b, m = st["ids"].shape
    N, P = st["prompts"].shape
    G = st["out"].shape[1]
    nxt, flag = nxt.reshape(-1), False
    for s in range(b):
        r, t, n, tokens, bad = int(st["req"][s]), 0, 0, [], False
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
                    bad = True                       # a write to `out` would leave its columns
                else:
                    st["out"][r, g] = nxt[s]
                    st["out_len"][r] = g + 1
                    if (eos is not None and eos >= 0 and nxt[s] == eos) or g + 1 == st["budget"][r]:
                        st["queue"][1] += 1
                        r = -1
                    else:
                        n, tokens = 1, [int(nxt[s])]
        if not bad and r < 0:
            t = 0
            if 0 <= st["queue"][0] < N:
                r = int(st["queue"][0])
                st["queue"][0] += 1
                n = min(m, int(st["prompt_len"][r]))
                bad = not 0 <= n <= P
                tokens = [] if bad else st["prompts"][r, :n].tolist()
        if bad or t + n > capacity:
            st["count"][s], flag = 0, True
            continue
        st["req"][s], st["pos"][s], st["count"][s] = r, t, n
        st["ids"][s] = tokens + [0] * (m - n)
        st["position_ids"][s] = [t + i for i in range(n)] + [0] * (m - n)
        st["last"][s] = s * m + max(n - 1, 0)
    return st, flag


def commit_state(b, waiting, seed, m=4, capacity=12, eos=None, overflow=False):
    """a state that mixes, over the b slots in turn: a slot in the middle of its prompt, one whose step held its last prompt
    tokens (it stores its first token), decoding slots that go on, one that draws `eos` (if given), one whose budget ends, free
    slots - with `waiting` requests behind those the slots hold.  overflow: also a slot whose next token would land beyond the
    capacity and one whose row of `out` is full (both raise the flag).  Returns ({name: array}, nxt (b, 1))"""
    rng = np.random.RandomState(seed)
    N, P, G = b + waiting, 9, 5
    st = dict(prompts=rng.randint(1, 90, (N, P)).astype(np.int32), prompt_len=rng.randint(1, P + 1, N).astype(np.int32),
              budget=rng.randint(2, G + 1, N).astype(np.int32), out=np.full((N, G), PAD, np.int32), out_len=np.zeros(N, np.int32),
              queue=np.array([b, 0], np.int32), req=np.arange(b, dtype=np.int32), pos=np.zeros(b, np.int32), count=np.zeros(b, np.int32),
              ids=rng.randint(0, 90, (b, m)).astype(np.int32), position_ids=rng.randint(0, 9, (b, m)).astype(np.int32),
              last=rng.randint(0, 9, b).astype(np.int32))
    nxt = rng.randint(20, 90, (b, 1)).astype(np.int32)
    held = 0
    for s in range(b):
        kind = s % 7
        r = held
        length = int(st["prompt_len"][r])
        if kind == 0 and length > 1:                 # in the middle of its prompt
            st["pos"][s], st["count"][s] = 0, min(m, length - 1)
        elif kind == 1:                              # the step held its last prompt tokens
            st["pos"][s], st["count"][s] = max(length - m, 0), min(m, length)
        elif kind == 5 or (kind == 0 and length <= 1):   # free
            st["req"][s] = -1
            st["pos"][s], st["count"][s] = rng.randint(0, 9), rng.randint(0, m + 1)      # what a free slot holds is overwritten
            continue
        else:                                        # decoding: g tokens out, the last of them fed in this step
            g = int(rng.randint(1, st["budget"][r]))
            if kind == 3:
                g = int(st["budget"][r]) - 1         # its budget ends with this token
            st["out"][r, :g], st["out_len"][r] = rng.randint(20, 90, g), g
            st["pos"][s], st["count"][s] = min(length + g - 1, capacity - 1), 1
            if kind == 4 and eos is not None:
                nxt[s] = eos
            if kind == 6 and overflow:
                if (s // 7) % 2:
                    # its token is stored, and feeding it back would take position `capacity`: flagged in step 4
                    st["budget"][r], st["out_len"][r], st["pos"][s] = G, 1, capacity - 1
                else:
                    st["out_len"][r] = G             # the row of out is full: flagged before anything is written
        st["req"][s] = r
        held += 1
    st["queue"][0] = held
    # requests held .. N - 1 wait
    return st, nxt


def upload(T, state, strided_out=False):
    """{name: tensor} on tensor class T; strided_out: `out` is columns 2 .. 2 + G of a wider tensor (returned as "wide")"""
    tensors = {k: T.from_numpy(v.copy(), requires_grad=False) for k, v in state.items()}
    if strided_out:
        G = state["out"].shape[1]
        wide = np.full((state["out"].shape[0], G + 5), -7, np.int32)
        wide[:, 2:2 + G] = state["out"]
        tensors["wide"] = T.from_numpy(wide, requires_grad=False)
        if T is CpuTensor:
            tensors["out"] = CpuTensor.from_numpy(tensors["wide"].data[:, 2:2 + G], requires_grad=False)
        else:
            from lightgrad_amd.autograd.hip.ops import _idx_view
            tensors["out"] = _idx_view(tensors["wide"], (slice(None), slice(2, 2 + G)))
    return tensors


def commit_on(T, state, nxt, capacity, eos, strided_out=False):
    """`serve_commit` on tensor class T: ({name: array after}, tensors).  The caller deals with the IndexError of a flagged slot"""
    tensors = upload(T, state, strided_out)
    t_nxt = T.from_numpy(nxt.copy(), requires_grad=False)
    error = None
    try:
        assert t_nxt.serve_commit(*(tensors[k] for k in NAMES), capacity, eos=eos) is None
    except IndexError as e:              # the numpy backend raises at once, after every other slot has been committed
        error = e
    return tensors, error


# ---- one mixed model step ---------------------------------------------------------------------------------------------------

MIXED_M = 5
# (tokens already in the cache, tokens of this step): a row decoding, a 4-token prefill piece at t = 0, an idle row (with t + m
# beyond the capacity), a row whose tokens end at the capacity
MIXED = ((6, 1), (0, 4), (14, 0), (12, 5))


@functools.lru_cache(maxsize=None)
def mixed_sequences():
    rng = np.random.RandomState(21)
    return [rng.randint(0, CFG["vocab_size"], t + n).astype(np.int32) for t, n in MIXED]


@functools.lru_cache(maxsize=None)
def mixed_reference():
    """(ref64, cpu32): per sequence the logits (tokens of this step, vocab) of the full causal forward of that sequence ALONE"""
    out = []
    for dtype in (np.float64, np.float32):
        model = dc.make_model(CpuTensor, dtype, SEED)
        out.append([dc.full_logits(model, seq[None, :])[0][t:] if len(seq) else np.zeros((0, CFG["vocab_size"]), dtype)
                    for seq, (t, n) in zip(mixed_sequences(), MIXED)])
    return tuple(out)


def mixed_step(T, model=None, dtype=np.float32):
    """the logits of the real rows of ONE `model(ids, cache=, append=True, count=)` call on tensor class T, per sequence: the
    tokens in front of the step enter the cache one sequence at a time through the same call (every other row idle)"""
    seqs = mixed_sequences()
    b = len(MIXED)
    model = dc.make_model(T, dtype, SEED) if model is None else model
    cache = nn.KVCache(CFG["num_hidden_layers"], b, CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    tensor = lambda a: T.from_numpy(np.ascontiguousarray(a), requires_grad=False)          # noqa: E731
    for r, (t, n) in enumerate(MIXED):
        if t:
            ids, count = np.zeros((b, t), np.int32), np.zeros(b, np.int32)
            ids[r], count[r] = seqs[r][:t], t
            model(tensor(ids), cache=cache, append=True, count=tensor(count))
            cache.advance(tensor(count))
    np.testing.assert_array_equal(cache.pos.numpy(), [t for t, _ in MIXED])
    ids, count = np.full((b, MIXED_M), 7, np.int32), np.array([n for _, n in MIXED], np.int32)
    for r, (t, n) in enumerate(MIXED):
        ids[r, :n] = seqs[r][t:]
    logits = model(tensor(ids), cache=cache, append=True, count=tensor(count))
    assert tuple(logits.shape) == (b, MIXED_M, CFG["vocab_size"]) and logits.ctx is None          # outside the tape
    logits = logits.numpy()
    return [logits[r, :n].copy() for r, (_, n) in enumerate(MIXED)], cache


def named(rows):
    return {"sequence%d" % r: a for r, a in enumerate(rows) if len(a)}
