"""What test_ragged_cpu.py and test_hip_ragged.py share: three prompts of different lengths for the model of decode_cases, the
float64 yardsticks of every sequence ALONE (computed once per process and never changed afterwards) and the runs of the ragged
batch through an nn.KVCache(per_row=True) on any tensor class."""
import functools
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc

bert, CFG = dc.bert, dc.CFG
SEED = 3                                # model and ids: no greedy step of any sequence alone is a near-tie (greedy_reference)
LENGTHS = (5, 2, 7)
B, S0 = len(LENGTHS), max(LENGTHS)
CAPACITY, NEW = 17, 8
EOS = 18                                # the float64 reference of sequence 0 draws it as its 6th token, the others never
PAD = 100
FORCED = 6                              # teacher-forced tokens per row behind the prompt
SECOND = (3, 1, 2)                      # a ragged second piece appended through the extend path


@functools.lru_cache(maxsize=None)
def prompts():
    """[ids of sequence r] - the three prompts, as int32 arrays of their own lengths"""
    ids = dc.parameters(SEED)[1]
    out = [ids[0, :5].copy(), ids[1, :2].copy(), ids[0, 4:11].copy()]
    assert tuple(len(p) for p in out) == LENGTHS
    return out


def padded(rows, fill=PAD, width=None):
    """right-padded (b, width) int32 array of rows of different lengths"""
    width = max(len(r) for r in rows) if width is None else width
    out = np.full((len(rows), width), fill, np.int32)
    for r, row in enumerate(rows):
        out[r, :len(row)] = row
    return out


@functools.lru_cache(maxsize=None)
def greedy_reference(new=NEW):
    """greedy decoding of each sequence alone at batch 1 by a full float64 recompute per token: ([tokens (new,)] per sequence, the
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


def assert_margins_rule_out_ties(new=NEW):
    """decode_cases' rule, from the references alone: margin >= 100 x the float32 deviation"""
    tokens, margin, deviation = greedy_reference(new)
    assert margin >= 100 * deviation, "seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick another seed" % (SEED, margin, deviation)
    return tokens


def expected_ids(tokens, eos=EOS, new=NEW):
    """the (B, S0 + new) result of `generate(lengths=, eos_token_id=eos)` that the reference tokens of each sequence alone
    imply, and the position at which each row stops moving (its last token's column)"""
    out, stop = np.full((B, S0 + new), PAD, np.int32), []
    for r, (prompt, toks) in enumerate(zip(prompts(), tokens)):
        n = len(toks)
        if eos is not None and eos in toks.tolist():
            n = toks.tolist().index(eos) + 1
        out[r, :len(prompt)] = prompt
        out[r, len(prompt):len(prompt) + n] = toks[:n]
        stop.append(len(prompt) + min(n, new) - 1)
    return out, np.array(stop)


@functools.lru_cache(maxsize=None)
def forced_sequences():
    """[ids of sequence r]: prompt, FORCED given tokens, then the SECOND piece - arbitrary tokens of the vocabulary"""
    rng = np.random.RandomState(11)
    return [np.concatenate([p, rng.randint(0, CFG["vocab_size"], FORCED + SECOND[r]).astype(np.int32)]) for r, p in enumerate(prompts())]


@functools.lru_cache(maxsize=None)
def teacher_reference():
    """(ref64, cpu32): per sequence r the logits (len, vocab) of the full causal forward of that sequence ALONE, in float64 and on
    the float32 CPU backend"""
    out = []
    for dtype in (np.float64, np.float32):
        model = dc.make_model(CpuTensor, dtype, SEED)
        out.append([dc.full_logits(model, seq[None, :])[0] for seq in forced_sequences()])
    return tuple(out)


def teacher_forced(T, model=None, dtype=np.float32):
    """the same rows through ONE per-row cache on tensor class T: the right-padded prompts once, the last real row of each, then
    FORCED tokens one step at a time, then the ragged second pieces in one append.  Returns per sequence the logits (len, vocab)
    of every position the run computed a real row for"""
    seqs = forced_sequences()
    model = dc.make_model(T, dtype, SEED) if model is None else model
    cache = nn.KVCache(CFG["num_hidden_layers"], B, CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    assert tuple(cache.pos.shape) == (B,)
    tensor = lambda a: T.from_numpy(a, requires_grad=False)          # noqa: E731
    rows = [[] for _ in range(B)]
    logits = model(tensor(padded([s[:n] for s, n in zip(seqs, LENGTHS)])), cache=cache).numpy()
    cache.set_lengths(LENGTHS)
    for r, n in enumerate(LENGTHS):
        rows[r].extend(logits[r, :n])
    for i in range(FORCED):
        step = np.array([[s[n + i]] for s, n in zip(seqs, LENGTHS)], np.int32)
        logits = model(tensor(step), cache=cache)
        cache.advance()
        assert tuple(logits.shape) == (B, 1, CFG["vocab_size"]) and logits.ctx is None          # outside the tape
        for r in range(B):
            rows[r].append(logits.numpy()[r, 0])
    piece = padded([s[n + FORCED:] for s, n in zip(seqs, LENGTHS)])
    logits = model(tensor(piece), cache=cache, append=True).numpy()
    cache.advance(np.array(SECOND))
    for r, n in enumerate(SECOND):
        rows[r].extend(logits[r, :n])
    np.testing.assert_array_equal(cache.pos.numpy(), [len(s) for s in seqs])
    np.testing.assert_array_equal(cache.lengths, [len(s) for s in seqs])
    return [np.stack(r) for r in rows]


def generate(T, model=None, dtype=np.float32, new=NEW, lengths=LENGTHS, eos=EOS, **options):
    """(ids (B, S0 + new), the cache) of `generate(lengths=, eos_token_id=)` over the right-padded prompts on tensor class T"""
    model = dc.make_model(T, dtype, SEED) if model is None else model
    cache = nn.KVCache(CFG["num_hidden_layers"], B, CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    ids = T.from_numpy(padded(prompts(), fill=7), requires_grad=False)         # the caller's padding is not the result's
    out = bert.generate(model, ids, new, lengths=lengths, eos_token_id=eos, pad_token_id=PAD, cache=cache, **options)
    assert tuple(out.shape) == (B, S0 + new) and out.dtype == np.int32
    return out.numpy().copy(), cache


TURN_LENGTHS = (3, 1, 2)


def second_turn(T):
    """4 new tokens per row without an end-of-sequence id (the rows then stand at different positions), then - the cache kept - the
    last of them and 2 / 0 / 1 given tokens appended as a right-padded piece with append=True and lengths=, and 2 more new
    tokens: asserted against each sequence's own float64 continuation ALONE, after the margin rule from the references alone.
    Returns (model, cache, the appended piece) for what a caller checks next"""
    model = dc.make_model(T, seed=SEED)
    first, cache = generate(T, model=model, new=4, eos=None)
    assert cache.lengths.tolist() == [n + 3 for n in LENGTHS]              # `generate` feeds its last new token to nobody
    given = [np.array([first[0, 5 + 3], 40, 41], np.int32), np.array([first[1, 2 + 3]], np.int32), np.array([first[2, 7 + 3], 42], np.int32)]
    assert tuple(len(g) for g in given) == TURN_LENGTHS
    turn = T.from_numpy(padded(given, fill=9), requires_grad=False)
    out = bert.generate(model, turn, 2, lengths=TURN_LENGTHS, pad_token_id=PAD, cache=cache, append=True).numpy()
    assert out.shape == (B, max(TURN_LENGTHS) + 2)
    model64, model32 = dc.make_model(CpuTensor, np.float64, SEED), dc.make_model(CpuTensor, np.float32, SEED)
    for r, prompt in enumerate(prompts()):
        seq = np.concatenate([prompt, first[r, len(prompt):len(prompt) + 3], given[r]])
        for _ in range(2):
            l64, l32 = dc.full_logits(model64, seq[None, :])[0, -1], dc.full_logits(model32, seq[None, :])[0, -1]
            top = np.sort(l64)
            assert top[-1] - top[-2] >= 100 * np.abs(l32 - l64).max()          # no near-tie, from the references alone
            seq = np.append(seq, l64.argmax()).astype(np.int32)
        n = len(given[r])
        np.testing.assert_array_equal(out[r, :n + 2], seq[-(n + 2):], err_msg="row %d" % r)
        assert (out[r, n + 2:] == PAD).all()
    np.testing.assert_array_equal(cache.pos.numpy(), [n + 3 + g + 1 for n, g in zip(LENGTHS, TURN_LENGTHS)])
    return model, cache, turn


def named(rows):
    return {"sequence%d" % r: a for r, a in enumerate(rows)}


def commit_by_hand(nxt, token, out_ids, pos, done, eos):
    """the issue's words, row by row, on copies: (token, out_ids, pos, done, a row raised the flag)"""
    token, out_ids, pos, done, flag = token.copy(), out_ids.copy(), pos.copy(), done.copy(), False
    for r in range(len(pos)):
        if done[r] != 0:
            continue
        p = int(pos[r]) + 1
        if p < 0 or p >= out_ids.shape[1]:
            flag = True
            continue
        pos[r], token[r, 0], out_ids[r, p] = p, nxt.reshape(-1)[r], nxt.reshape(-1)[r]
        if eos is not None and eos >= 0 and nxt.reshape(-1)[r] == eos:
            done[r] = 1
    return token, out_ids, pos, done, flag
