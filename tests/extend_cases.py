"""What test_extend_cpu.py and test_hip_extend.py share: the append run (a prompt, then pieces of several given tokens into the
filled nn.KVCache) and the two-turn `generate` of decode_cases' small causal model on any tensor class, with their float64
yardsticks - full causal forwards over each prefix, computed once per process and never changed afterwards."""
import functools
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc

PIECES = (3, 1, 4)                      # behind the prompt of dc.S0 = 5: 13 of the 17 positions, the seam at 5, 8 and 9
TURN1, GIVEN, TURN2 = 4, 3, 3           # two turns: prompt 5 -> 4 new -> 3 given -> 3 new, 15 of the 17 positions
SEED2 = 2                               # model and ids of the two-turn run; picked on the CPU (two_turn_reference's margin rule)


def capacity_mask(dtype=np.float32):
    """decode_cases.PROMPT_MASK extended with ones to the capacity: what a step over the cache's rows reads"""
    return dc.prefix_mask(dc.CAPACITY).astype(dtype)


@functools.lru_cache(maxsize=None)
def append_reference(masked):
    """(ref64, cpu32): {"prefill": (B, S0, vocab), "piece<i>": (B, PIECES[i], vocab)} - the rows of the piece's tokens in a full
    causal forward over the prefix that ends with the piece, in float64 and on the float32 CPU backend"""
    _, ids = dc.parameters()
    out = []
    for dtype in (np.float64, np.float32):
        model = dc.make_model(CpuTensor, dtype)
        rows = {"prefill": dc.full_logits(model, ids[:, :dc.S0], dc.prefix_mask(dc.S0) if masked else None)}
        n = dc.S0
        for i, m in enumerate(PIECES):
            n += m
            rows["piece%d" % i] = dc.full_logits(model, ids[:, :n], dc.prefix_mask(n) if masked else None)[:, n - m:]
        out.append(rows)
    return tuple(out)


def append_run(T, masked, model=None, dtype=np.float32):
    """the same rows through an nn.KVCache on tensor class T: the prompt into the empty cache, then the PIECES of given tokens
    with `append=True`, the position moved on by the caller"""
    _, ids = dc.parameters()
    model = dc.make_model(T, dtype) if model is None else model
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    tensor = lambda a: T.from_numpy(a, requires_grad=False)          # noqa: E731
    prompt_mask = tensor(dc.PROMPT_MASK.astype(dtype)) if masked else None
    cache_mask = tensor(capacity_mask(dtype)) if masked else None
    rows = {"prefill": model(tensor(ids[:, :dc.S0]), attention_mask=prompt_mask, cache=cache).numpy().copy()}
    n = dc.S0
    for i, m in enumerate(PIECES):
        assert cache.length == n
        logits = model(tensor(ids[:, n:n + m]), attention_mask=cache_mask, cache=cache, append=True)
        cache.advance(m)
        assert tuple(logits.shape) == (dc.B, m, dc.CFG["vocab_size"]) and logits.ctx is None          # every row, outside the tape
        rows["piece%d" % i] = logits.numpy().copy()
        n += m
    assert cache.length == n and int(cache.pos.numpy()[0]) == n
    return rows


def given_tokens(seed=SEED2):
    """the GIVEN tokens of the second turn: the columns behind the prompt of decode_cases' ids"""
    _, ids = dc.parameters(seed)
    return ids[:, dc.S0:dc.S0 + GIVEN]


@functools.lru_cache(maxsize=None)
def two_turn_reference(seed=SEED2):
    """the two turns by a full float64 recompute per token: (turn-1 tokens (B, TURN1), turn-2 tokens (B, TURN2), the smallest
    top-2 logit margin of any greedy step, the largest deviation of the float32 full forward's last-row logits from the float64
    ones over the same prefixes)"""
    _, ids = dc.parameters(seed)
    model64, model32 = dc.make_model(CpuTensor, np.float64, seed), dc.make_model(CpuTensor, np.float32, seed)
    seq, margin, deviation = ids[:, :dc.S0].copy(), np.inf, 0.0

    def greedy_steps(seq, steps, margin, deviation):
        for _ in range(steps):
            l64, l32 = dc.full_logits(model64, seq)[:, -1], dc.full_logits(model32, seq)[:, -1]
            top = np.sort(l64, axis=-1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
            deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
            seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
        return seq, margin, deviation

    seq, margin, deviation = greedy_steps(seq, TURN1, margin, deviation)
    first = seq[:, dc.S0:]
    seq = np.concatenate([seq, given_tokens(seed)], axis=1)
    at = seq.shape[1]
    seq, margin, deviation = greedy_steps(seq, TURN2, margin, deviation)
    assert seq.shape[1] == dc.S0 + TURN1 + GIVEN + TURN2 <= dc.CAPACITY
    return first, seq[:, at:], margin, deviation


def assert_two_turn_margins_rule_out_ties(seed=SEED2):
    first, second, margin, deviation = two_turn_reference(seed)
    assert margin >= 100 * deviation, "seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick another seed" % (seed, margin, deviation)
    return first, second


def two_turns(T, seed=SEED2, model=None, **options):
    """(turn-1 tokens, turn-2 tokens) of `generate` on tensor class T: the prompt, TURN1 new tokens; then - the cache kept - the
    last of them (`generate` feeds its last token to nobody: a continuation starts with it) and the GIVEN tokens appended with
    append=True, TURN2 new tokens behind them"""
    _, ids = dc.parameters(seed)
    model = dc.make_model(T, seed=seed) if model is None else model
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    out1 = dc.bert.generate(model, T.from_numpy(ids[:, :dc.S0], requires_grad=False), TURN1, cache=cache, **options).numpy()
    assert out1.shape == (dc.B, dc.S0 + TURN1) and cache.length == dc.S0 + TURN1 - 1
    turn = np.concatenate([out1[:, -1:], given_tokens(seed)], axis=1).astype(np.int32)
    out2 = dc.bert.generate(model, T.from_numpy(turn, requires_grad=False), TURN2, cache=cache, append=True, **options)
    assert tuple(out2.shape) == (dc.B, 1 + GIVEN + TURN2)
    out2 = out2.numpy()
    np.testing.assert_array_equal(out2[:, :1 + GIVEN], turn)              # the appended ids come back in front of the new ones
    assert cache.length == dc.S0 + TURN1 + GIVEN + TURN2 - 1
    return out1[:, dc.S0:], out2[:, 1 + GIVEN:]
