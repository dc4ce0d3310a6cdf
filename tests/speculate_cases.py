"""What test_speculate_cpu.py and test_hip_speculate.py share: `speculate_commit` written out by hand in plain python, seeded
states that mix every kind of row, four prompts for the model of decode_cases with the float64 greedy continuation of each prompt
ALONE (computed once per process and never changed afterwards), the schedule of `generate(speculate=k)` simulated over those
reference tokens, and the runs through `generate` on any tensor class."""
import functools
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc

bert, CFG = dc.bert, dc.CFG
SEEDS, NEW, CAPACITY, PAD, EOS = (2, 3), 24, 35, 100, 18
KS, NGRAMS = (1, 3, 5), (3, 1)
NAMES = ("ids", "count", "position_ids", "out_ids", "pos", "end", "done", "stats")
JUNK = 900                               # ids >= JUNK lie where nothing may read them


# ---- speculate_commit by hand -----------------------------------------------------------------------------------------------

def lookup(seq, cap, max_ngram, min_ngram):
    """step 6's drafts for the python list `seq`: the continuation of the most recent earlier occurrence of its last n-gram"""
    L = len(seq)
    if cap <= 0:
        return []
    for n in range(max_ngram, min_ngram - 1, -1):
        if L < n + 1:
            continue
        for q in range(L - n - 1, -1, -1):
            if seq[q:q + n] == seq[L - n:L]:
                return seq[q + n:min(q + n + cap, L)]
    return []


def commit_by_hand(state, tgt, draft, max_ngram, min_ngram, eos):
    """the issue's steps 1 to 6, row by row, on copies: ({name: array}, a row raised the flag)"""
    st = {k: v.copy() for k, v in state.items()}
    b, m = st["ids"].shape
    columns, flag = st["out_ids"].shape[1], False
    for r in range(b):
        if st["done"][r] != 0:                                                   # 1
            st["count"][r] = 0
            continue
        c, p, last = int(st["count"][r]), int(st["pos"][r]), int(st["end"][r])
        if not (1 <= c <= m and p >= 0 and p + c <= last and last <= columns - 1):     # 2
            st["count"][r], flag = 0, True
            continue
        a = 0                                                                    # 3
        for j in range(c - 1):
            if st["ids"][r, j + 1] != tgt[r, j]:
                break
            a += 1
        emitted, stopped = [int(t) for t in tgt[r, :a + 1]], False
        if eos is not None and eos >= 0 and eos in emitted:
            emitted, stopped = emitted[:emitted.index(eos) + 1], True
        for j, t in enumerate(emitted):                                          # 4
            st["out_ids"][r, p + 1 + j] = t
        p += len(emitted)
        st["pos"][r] = p
        st["stats"][1] += c - 1
        st["stats"][2] += a
        if stopped or p == last:                                                 # 5
            st["done"][r], st["count"][r] = 1, 0
            st["stats"][0] += 1
            continue
        seq = [int(t) for t in st["out_ids"][r, :p + 1]]                         # 6
        drafts = lookup(seq, min(draft, last - p - 1), max_ngram, min_ngram)
        k = 1 + len(drafts)
        st["ids"][r] = [seq[p]] + drafts + [0] * (m - k)
        st["position_ids"][r] = [p + i for i in range(k)] + [0] * (m - k)
        st["count"][r] = k
    return st, flag


KINDS = ("full accept", "partial accept", "full reject", "count 1", "eos inside the accepted run", "reaches end", "done", "cap == 0",
         "only a shorter match", "two matches", "out of bounds")


def commit_state(b, m, columns, seed, draft, max_ngram=3, min_ngram=1, eos=None, overflow=False):
    """a state that mixes the KINDS over the b rows in turn, as far as m and the columns leave room for each (a kind without room
    becomes a plain random row): ({name: array}, tgt (b, m)).  The ids come from a vocabulary of 5, so n-grams recur by themselves;
    `only a shorter match` and `two matches` are built from ids that occur nowhere else.  overflow: every eleventh row breaks a
    clause of step 2 - count 0, count m + 1, a negative position, p + count beyond end, end beyond the columns - in turn"""
    rng = np.random.RandomState(seed)
    vocab = lambda *shape: rng.randint(1, 6, shape).astype(np.int32)             # noqa: E731
    st = dict(ids=rng.randint(JUNK, JUNK + 50, (b, m)).astype(np.int32), count=np.zeros(b, np.int32),
              position_ids=rng.randint(0, 9, (b, m)).astype(np.int32), out_ids=rng.randint(JUNK, JUNK + 50, (b, columns)).astype(np.int32),
              pos=np.zeros(b, np.int32), end=np.zeros(b, np.int32), done=np.zeros(b, np.int32), stats=rng.randint(0, 50, 3).astype(np.int32))
    tgt = vocab(b, m)
    for r in range(b):
        kind = KINDS[r % len(KINDS)]
        last = int(rng.randint(1, columns)) if columns > 1 else 1
        c = int(rng.randint(1, min(m, last) + 1))
        if kind == "count 1" or kind in ("only a shorter match", "two matches"):
            c = 1
        if kind == "cap == 0":
            c = min(c, 2)
        p = int(rng.randint(0, last - c + 1)) if last >= c else 0
        if kind == "reaches end":
            last = p + c
        if kind == "cap == 0" and p + 2 <= columns - 1:
            last = p + 2
        if kind in ("only a shorter match", "two matches"):
            last = min(columns - 1, max(last, p + 1 + draft + 1))
        seq = vocab(p + 1)
        drafts = vocab(c - 1)
        row_tgt = vocab(m)
        if kind in ("full accept", "reaches end", "eos inside the accepted run"):
            row_tgt[:c - 1] = drafts
            if kind[0] == "e" and eos is not None:
                row_tgt[(c - 1) // 2] = eos
                if (c - 1) // 2 < c - 1:
                    drafts[(c - 1) // 2] = eos
        elif kind == "partial accept" and c >= 3:
            a = int(rng.randint(1, c - 1))
            row_tgt[:a] = drafts[:a]
            row_tgt[a] = drafts[a] % 5 + 1                                       # another id of the vocabulary
        elif kind in ("full reject", "cap == 0") and c >= 2:
            row_tgt[0] = drafts[0] % 5 + 1
        elif kind == "only a shorter match" and p + 1 >= 4:
            # ids that occur once each; the new token's id stands once before, behind another id than the row's last: a 1-gram matches
            seq = (1000 + np.arange(p + 1)).astype(np.int32)
            row_tgt[0] = seq[(p + 1) // 2]
        elif kind == "two matches" and p + 1 >= 3 * max_ngram + 2:
            # the last max_ngram tokens (the new one included) stand twice before: the later occurrence's continuation is drafted
            n = max_ngram
            seq = (1000 + np.arange(p + 1)).astype(np.int32)
            gram = (2000 + np.arange(n)).astype(np.int32)
            first, second = 1, 1 + n + 1 + (p + 1 - 3 * n - 2) // 2
            seq[first:first + n], seq[second:second + n] = gram, gram
            seq[p + 1 - (n - 1):] = gram[:n - 1]
            row_tgt[0] = gram[n - 1]
        if kind == "done":
            st["done"][r] = 1
        if kind == "out of bounds":
            if not overflow:
                pass
            else:
                clause = (r // len(KINDS)) % 5
                if clause == 0:
                    c = 0
                elif clause == 1:
                    c = m + 1
                elif clause == 2:
                    p = -1 - int(rng.randint(0, 3))
                elif clause == 3:
                    last = p + c - 1
                else:
                    last = columns + int(rng.randint(0, 3))
        st["count"][r], st["pos"][r], st["end"][r] = c, p, last
        if p >= 0:
            st["out_ids"][r, :min(p + 1, columns)] = seq[:columns]
        if p >= 0 and p < columns:
            st["ids"][r, 0] = st["out_ids"][r, p]
        n_drafts = max(0, min(c, m) - 1)
        st["ids"][r, 1:1 + n_drafts] = drafts[:n_drafts] if len(drafts) >= n_drafts else vocab(n_drafts)
        tgt[r] = row_tgt
    return st, tgt


def upload(T, state, strided_out=False):
    """{name: tensor} on tensor class T; strided_out: `out_ids` is columns 3 .. 3 + columns of a wider tensor (returned as "wide")"""
    tensors = {k: T.from_numpy(v.copy(), requires_grad=False) for k, v in state.items()}
    if strided_out:
        columns = state["out_ids"].shape[1]
        wide = np.full((state["out_ids"].shape[0], columns + 5), -7, np.int32)
        wide[:, 3:3 + columns] = state["out_ids"]
        tensors["wide"] = T.from_numpy(wide, requires_grad=False)
        if T is CpuTensor:
            tensors["out_ids"] = CpuTensor.from_numpy(tensors["wide"].data[:, 3:3 + columns], requires_grad=False)
        else:
            from lightgrad_amd.autograd.hip.ops import _idx_view
            tensors["out_ids"] = _idx_view(tensors["wide"], (slice(None), slice(3, 3 + columns)))
    return tensors


def commit_on(T, state, tgt, draft, max_ngram, min_ngram, eos, strided_out=False):
    """`speculate_commit` on tensor class T: (tensors, the IndexError the numpy backend raised at once or None)"""
    tensors = upload(T, state, strided_out)
    t_tgt = T.from_numpy(tgt.copy(), requires_grad=False)
    error = None
    try:
        assert t_tgt.speculate_commit(*(tensors[k] for k in NAMES), draft, max_ngram=max_ngram, min_ngram=min_ngram, eos=eos) is None
    except IndexError as e:
        error = e
    tensors["tgt"] = t_tgt
    return tensors, error


# ---- generate(speculate=k) --------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def prompts(seed):
    """four prompts of 5, 2, 7 and 9 tokens; the third is ids[0, 4:8] twice over, cut to 7: a prompt that repeats itself"""
    ids = dc.parameters(seed)[1]
    return [ids[0, :5].copy(), ids[1, :2].copy(), np.array((ids[0, 4:8].tolist() * 2)[:7], np.int32), ids[1, 3:12].copy()]


@functools.lru_cache(maxsize=None)
def greedy_reference(seed, new=NEW):
    """greedy decoding of each prompt alone at batch 1 by a full float64 recompute per token: ([tokens (new,)] per prompt, the
    smallest top-2 logit margin of any step, the largest deviation of the float32 full forward's last-row logits from float64)"""
    model64, model32 = dc.make_model(CpuTensor, np.float64, seed), dc.make_model(CpuTensor, np.float32, seed)
    tokens, margin, deviation = [], np.inf, 0.0
    for prompt in prompts(seed):
        seq = prompt[None, :].copy()
        for _ in range(new):
            l64, l32 = dc.full_logits(model64, seq)[:, -1], dc.full_logits(model32, seq)[:, -1]
            top = np.sort(l64, axis=-1)
            margin = min(margin, float((top[:, -1] - top[:, -2]).min()))
            deviation = max(deviation, float(np.abs(l32.astype(np.float64) - l64).max()))
            seq = np.concatenate([seq, l64.argmax(-1).astype(np.int32)[:, None]], axis=1)
        tokens.append(seq[0, len(prompt):])
    return tokens, margin, deviation


def assert_margins_rule_out_ties(seed):
    """decode_cases' rule, from the references alone: margin >= 100 x the float32 deviation"""
    tokens, margin, deviation = greedy_reference(seed)
    print("seed %d: top-2 margin %.3g, float32 deviation %.3g" % (seed, margin, deviation))
    assert margin >= 100 * deviation, "seed %d: top-2 margin %.3g below 100 x the float32 deviation %.3g - pick other inputs" % (seed, margin, deviation)
    return tokens


def schedule(prompt, tokens, k, max_ngram=NGRAMS[0], min_ngram=NGRAMS[1], eos=None):
    """the steps `generate(speculate=k)` takes for one prompt whose continuation is `tokens`: [(drafts, accepted)] per step, and
    the tokens emitted - the definition's steps 3 to 6 with the reference tokens in place of the model"""
    prompt, tokens = [int(t) for t in prompt], [int(t) for t in tokens]
    budget = len(tokens)
    seq, g, steps = prompt + tokens[:1], 1, []                                   # the first commit: the prompt's own token
    stopped = eos is not None and tokens[0] == eos
    while not stopped and g < budget:
        drafts = lookup(seq, min(k, budget - g - 1), max_ngram, min_ngram)       # at most budget - g - 1: tokens[g + a] exists
        a = 0
        while a < len(drafts) and drafts[a] == tokens[g + a]:
            a += 1
        emitted = tokens[g:g + a + 1]                                            # the accepted drafts, then the model's own token
        if eos is not None and eos in emitted:
            emitted, stopped = emitted[:emitted.index(eos) + 1], True
        steps.append((len(drafts), a))
        seq, g = seq + emitted, g + len(emitted)
    return steps, tokens[:g]


def expected(seed, eos=None, new=NEW):
    """(rows (4, longest prompt + new) of prompt, reference tokens cut behind `eos`, PAD; steps with poll=1 per k; stats per k)"""
    refs, ps = greedy_reference(seed, new)[0], prompts(seed)
    rows = np.full((len(ps), max(len(p) for p in ps) + new), PAD, np.int32)
    per_k = {}
    for k in KS:
        plans = [schedule(p, t, k, eos=eos) for p, t in zip(ps, refs)]
        per_k[k] = dict(steps=max(len(s) for s, _ in plans), drafted=sum(d for s, _ in plans for d, _ in s),
                        accepted=sum(a for s, _ in plans for _, a in s), plans=[s for s, _ in plans])
    for r, (p, t) in enumerate(zip(ps, refs)):
        t = schedule(p, t, 1, eos=eos)[1]
        rows[r, :len(p)], rows[r, len(p):len(p) + len(t)] = p, t
    return rows, per_k


def run(T, seed, k=None, model=None, eos=None, new=NEW, tensors=None, **options):
    """(ids (4, longest prompt + new), stats, cache) of `generate` over the four prompts as one ragged batch on tensor class T;
    tensors: a list that receives the result as a tensor"""
    model = dc.make_model(T, seed=seed) if model is None else model
    ps = prompts(seed)
    lengths = [len(p) for p in ps]
    padded = np.zeros((len(ps), max(lengths)), np.int32)
    for r, p in enumerate(ps):
        padded[r, :len(p)] = p
    cache = nn.KVCache(CFG["num_hidden_layers"], len(ps), CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    stats = {}
    extra = {} if k is None else dict(speculate=k, max_ngram=NGRAMS[0], min_ngram=NGRAMS[1], stats=stats)
    out = bert.generate(model, T.from_numpy(padded, requires_grad=False), new, lengths=lengths, eos_token_id=eos, pad_token_id=PAD, cache=cache,
                        **extra, **options)
    assert out.dtype == np.int32 and isinstance(out, T) and tuple(out.shape) == (len(ps), max(lengths) + new)
    if tensors is not None:
        tensors.append(out)
    return out.numpy().copy(), stats, cache
