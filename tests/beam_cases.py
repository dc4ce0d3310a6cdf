"""What test_beam_cpu.py and test_hip_beam.py share: `beam_step` written out by hand in plain python, seeded states whose groups
mix every kind the definition names, the margin rule of decode_cases / speculate_cases for selections (from float64 and plain
float32 numpy evaluations alone), and a float64 reference beam search for the model of decode_cases - `decode_cases.full_logits`
per hypothesis - computed once per process and never changed afterwards."""
import functools
import math
import numpy as np
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor
import decode_cases as dc
import speculate_cases as sc

bert, CFG = dc.bert, dc.CFG
NAMES = ("scores", "parent", "token", "out_ids", "pos", "done", "stats")
KINDS = ("mixed", "initial", "done_top", "all_done", "ties_inside", "ties_across", "eos", "bad_negative", "bad_full", "bad_done_negative")
JUNK = 900                               # ids >= JUNK lie where nothing may read them
# the model and prompts of seed 6: chosen on the CPU so that every selection of 1, 2 and 4 beams keeps the margin rule
# (assert_reference_rules_out_ties).  With EOS some beams finish among live ones and the returned beam is not always the first; with
# EOS_ALL every beam of every prompt finishes within a few steps and the loop stops early
SEED, NEW, CAPACITY, PAD, EOS, EOS_ALL = 6, 10, 24, 100, 56, 99


# ---- beam_step by hand --------------------------------------------------------------------------------------------------------------

def step_by_hand(state, logits, w, eos=None):
    """the six points of the definition in plain python over copies of `state` ({name: ndarray}) and logits (rows, V) float32:
    ({name: ndarray}, was a group out of bounds?)"""
    st = {k: v.copy() for k, v in state.items()}
    rows, V = logits.shape
    columns, flagged = st["out_ids"].shape[1], False
    for lo in range(0, rows, w):
        pos, done = [int(p) for p in state["pos"][lo:lo + w]], [int(d) != 0 for d in state["done"][lo:lo + w]]
        st["parent"][lo:lo + w] = range(lo, lo + w)
        if any(p < 0 for p in pos) or any(not d and p + 1 >= columns for p, d in zip(pos, done)):        # 1. bounds
            flagged = True
            continue
        if all(done):                                                                                    # 6. finished groups
            continue
        cands = []                                                                                       # 2. (value, flat index, i, j)
        for i in range(w):
            s = float(state["scores"][lo + i])
            if done[i]:
                cands.append((s, i * V, i, None))
                continue
            x = [float(v) for v in logits[lo + i]]
            m = max(x)
            lse = math.log(math.fsum(math.exp(v - m) for v in x))
            cands.extend((s + (v - m - lse) if s != -math.inf else -math.inf, i * V + j, i, j) for j, v in enumerate(x))
        cands.sort(key=lambda c: (-c[0], c[1]))                                                          # 3. ties: the smaller flat index
        for n, (s, _, i, j) in enumerate(cands[:w]):                                                     # 4. commit
            st["parent"][lo + n] = lo + i
            keep = min(pos[i] + 1, columns)
            st["out_ids"][lo + n, :keep] = state["out_ids"][lo + i, :keep]
            if done[i]:
                st["scores"][lo + n], st["token"][lo + n, 0], st["pos"][lo + n], st["done"][lo + n] = state["scores"][lo + i], state["token"][lo + i, 0], pos[i], 1
            else:
                st["out_ids"][lo + n, pos[i] + 1] = j
                st["scores"][lo + n], st["token"][lo + n, 0], st["pos"][lo + n] = np.float32(s), j, pos[i] + 1
                st["done"][lo + n] = 1 if eos is not None and eos >= 0 and j == eos else 0
        st["stats"][0] += 1 if all(st["done"][lo:lo + w] != 0) else 0                                    # 5. statistics
        st["stats"][1] += sum(1 for n in range(w) if st["parent"][lo + n] != lo + n)
    return st, flagged


def candidates64(state, logits, w):
    """per group that selects: (float64 candidate values in flat-index order of the definition, the same from a plain float32 numpy
    evaluation) - for the margin rule"""
    rows, V = logits.shape
    out = []
    for lo in range(0, rows, w):
        pos, done = state["pos"][lo:lo + w].astype(np.int64), state["done"][lo:lo + w] != 0
        if (pos < 0).any() or (~done & (pos + 1 >= state["out_ids"].shape[1])).any() or done.all():
            continue
        v64, v32 = [], []
        with np.errstate(all="ignore"):
            for i in range(w):
                s = state["scores"][lo + i]
                if done[i]:
                    v64.append(np.array([np.float64(s)])), v32.append(np.array([s], np.float32))
                    continue
                x = logits[lo + i]
                x64 = x.astype(np.float64)
                v64.append(np.float64(s) + (x64 - x64.max() - np.log(np.exp(x64 - x64.max()).sum())))
                v32.append((s + (x - x.max() - np.log(np.exp(x - x.max()).sum(dtype=np.float32)))).astype(np.float32))
        out.append((np.concatenate(v64), np.concatenate(v32)))
    return out


def margins(state, logits, w):
    """(the smallest gap between two neighbouring candidates among the first w + 1 of any selection, planted exact ties apart; dev32,
    the largest deviation of the plain float32 evaluation from float64 over the finite candidates)"""
    gap, dev = np.inf, 0.0
    for v64, v32 in candidates64(state, logits, w):
        top = np.sort(v64[np.isfinite(v64)])[::-1][:w + 1]
        d = -np.diff(top)
        d = d[d > 0]                                                          # (an exact tie in float64 of float32 inputs is a planted one)
        gap = min(gap, float(d.min()) if d.size else np.inf)
        ok = np.isfinite(v64)
        dev = max(dev, float(np.abs(v32[ok].astype(np.float64) - v64[ok]).max()))
    return gap, dev


def assert_margins_rule_out_ties(state, logits, w, what=""):
    gap, dev = margins(state, logits, w)
    assert gap >= 100 * dev, "%s: candidate gap %.3g below 100 x the float32 deviation %.3g - pick other inputs" % (what, gap, dev)
    return dev


def step_by_hand_fast(state, logits, w, eos=None):
    """`step_by_hand` with numpy float64 rows in place of python lists (for wide vocabularies), plus "scores64": the unrounded
    float64 score of every row"""
    st = {k: v.copy() for k, v in state.items()}
    st["scores64"] = state["scores"].astype(np.float64)
    rows, V = logits.shape
    columns, flagged = st["out_ids"].shape[1], False
    for lo in range(0, rows, w):
        pos, done = state["pos"][lo:lo + w].astype(np.int64), state["done"][lo:lo + w] != 0
        st["parent"][lo:lo + w] = np.arange(lo, lo + w)
        if (pos < 0).any() or (~done & (pos + 1 >= columns)).any():
            flagged = True
            continue
        if done.all():
            continue
        value, flat = [], []
        with np.errstate(all="ignore"):
            for i in range(w):
                s = np.float64(state["scores"][lo + i])
                if done[i]:
                    value.append(np.array([s])), flat.append(np.array([i * V]))
                else:
                    x = logits[lo + i].astype(np.float64)
                    value.append(s + (x - x.max() - np.log(np.exp(x - x.max()).sum()))), flat.append(i * V + np.arange(V))
        value, flat = np.concatenate(value), np.concatenate(flat)
        order = np.lexsort((flat, -value))[:w]
        for n, c in enumerate(order):
            i, j = int(flat[c]) // V, int(flat[c]) % V
            st["parent"][lo + n] = lo + i
            keep = int(min(pos[i] + 1, columns))
            st["out_ids"][lo + n, :keep] = state["out_ids"][lo + i, :keep]
            if done[i]:
                st["scores"][lo + n], st["token"][lo + n, 0], st["pos"][lo + n], st["done"][lo + n] = state["scores"][lo + i], state["token"][lo + i, 0], pos[i], 1
                st["scores64"][lo + n] = np.float64(state["scores"][lo + i])
            else:
                st["out_ids"][lo + n, pos[i] + 1] = j
                st["scores"][lo + n], st["token"][lo + n, 0], st["pos"][lo + n] = np.float32(value[c]), j, pos[i] + 1
                st["scores64"][lo + n] = value[c]
                st["done"][lo + n] = 1 if eos is not None and eos >= 0 and j == eos else 0
        st["stats"][0] += 1 if (st["done"][lo:lo + w] != 0).all() else 0
        st["stats"][1] += int((st["parent"][lo:lo + w] != np.arange(lo, lo + w)).sum())
    return st, flagged


# ---- seeded states --------------------------------------------------------------------------------------------------------------------

def step_state(kinds, w, V, columns, seed, scale=4.0):
    """`draw_state` with the first of the seeds 1000 * seed, 1000 * seed + 1, ... whose candidates keep the margin rule with room to
    spare (gap >= 200 x dev32): the inputs are picked here, on the CPU, from the references alone"""
    for attempt in range(1000):
        state, logits, eos = draw_state(kinds, w, V, columns, 1000 * seed + attempt, scale)
        gap, dev = margins(state, logits, w)
        if gap >= 200 * dev:
            return state, logits, eos
    raise AssertionError("no seed behind %d gives candidates that keep the margin rule - pick other inputs" % (1000 * seed))


def draw_state(kinds, w, V, columns, seed, scale=4.0):
    """({name: ndarray}, logits (rows, V) float32, eos) with one group of w beams per entry of `kinds`:
      mixed         live beams with ragged positions and scores, a done beam among them where w > 1
      initial       scores [0, -inf, ...]: every winner is a continuation of the leader
      done_top      a done beam whose score outranks every live candidate: it stays first, as itself
      all_done      every beam done, scores descending: bytes unchanged
      ties_inside   the two largest logits of the best beam are equal: the smaller token wins
      ties_across   beams 0 and 1 hold identical logits and identical scores: beam 0's candidate comes first
      eos           the best continuation of the best beam is `eos`
      bad_negative / bad_full / bad_done_negative   a live row at pos < 0 / a live row at the last column / a done row at pos < 0"""
    rng = np.random.RandomState(seed)
    b = len(kinds)
    rows = b * w
    logits = (rng.standard_normal((rows, V)) * scale).astype(np.float32)
    hi = max(columns - 2, 0)
    pos = rng.randint(0, hi + 1, rows).astype(np.int32)
    st = dict(scores=(-rng.uniform(0.5, 12.0, rows)).astype(np.float32), parent=np.full(rows, -5, np.int32),
              token=rng.randint(0, V, (rows, 1)).astype(np.int32), out_ids=(JUNK + rng.randint(0, 50, (rows, columns))).astype(np.int32),
              pos=pos, done=np.zeros(rows, np.int32), stats=np.array([3, 40], np.int32))
    eos = int(V - 1)
    for g, kind in enumerate(kinds):
        lo = g * w
        grp = slice(lo, lo + w)
        st["scores"][grp] = np.sort(st["scores"][grp])[::-1]                 # best first, as a step leaves a group
        logits[grp, eos] = -3.0 * scale - rng.uniform(0, 1, w).astype(np.float32)       # `eos` is drawn only where planted
        if kind == "mixed" and w > 1:
            st["done"][lo + w // 2] = 1
        elif kind == "initial":
            st["scores"][grp] = -np.inf
            st["scores"][lo] = 0.0
            st["pos"][grp] = st["pos"][lo]
        elif kind == "done_top":
            st["done"][lo] = 1
            st["scores"][lo] = -0.25
            st["scores"][lo + 1:lo + w] -= 1.0
        elif kind == "all_done":
            st["done"][grp] = 1
        elif kind == "ties_inside":
            top = np.float32(logits[lo].max() + 1.5)
            j = sorted(rng.choice(V, 2, replace=False)) if V > 1 else [0, 0]
            logits[lo, j[0]] = logits[lo, j[1]] = top
            st["scores"][lo + 1:lo + w] -= 40.0
        elif kind == "ties_across" and w > 1:
            logits[lo + 1] = logits[lo]
            st["scores"][lo + 1] = st["scores"][lo]
            st["scores"][lo + 2:lo + w] -= 40.0
        elif kind == "eos":
            logits[lo, eos] = np.float32(logits[lo].max() + 2.0)
            st["scores"][lo + 1:lo + w] -= 40.0
        elif kind == "bad_negative":
            st["pos"][lo + w - 1] = -1
        elif kind == "bad_full":
            st["pos"][lo] = columns - 1
        elif kind == "bad_done_negative":
            st["done"][lo + w - 1] = 1
            st["pos"][lo + w - 1] = -2
    # what a row has written so far: real ids up to its position
    for r in range(rows):
        p = int(st["pos"][r])
        if p >= 0:
            st["out_ids"][r, :p + 1] = rng.randint(0, V, p + 1)
    return st, logits, eos


def upload(T, state, strided_out=False):
    """{name: tensor} on tensor class T; strided_out: `out_ids` is columns 3 .. 3 + columns of a wider tensor (returned as "wide")"""
    return sc.upload(T, state, strided_out)


def step_on(T, state, logits, w, eos, strided_out=False, three_d=False):
    """`beam_step` on tensor class T: (tensors, the IndexError the numpy backend raised at once or None)"""
    tensors = upload(T, state, strided_out)
    t_logits = T.from_numpy(logits.reshape(logits.shape[0], 1, -1).copy() if three_d else logits.copy(), requires_grad=False)
    error = None
    try:
        assert t_logits.beam_step(*(tensors[k] for k in NAMES), w, eos=eos) is None
    except IndexError as e:
        error = e
    tensors["logits"] = t_logits
    return tensors, error


# ---- KVCache.reorder ------------------------------------------------------------------------------------------------------------------

def parents(kind, b, w, seed=0):
    """absolute parents (b * w,) of one of the kinds: identity, swap ([1, 0, 2, ...]), cycle, leader, mixed (a draw with duplicates)"""
    rng = np.random.RandomState(seed)
    local = {"identity": np.arange(w), "swap": np.array(([1, 0] if w > 1 else [0]) + list(range(2, w))), "cycle": (np.arange(w) + 1) % w,
             "leader": np.zeros(w, np.int64)}.get(kind)
    out = np.zeros(b * w, np.int32)
    for g in range(b):
        out[g * w:(g + 1) * w] = g * w + (rng.randint(0, w, w) if local is None else local)
    return out


def reorder_by_take(arrays, parent, pos, w):
    """what KVCache.reorder must leave: per group one `take` along the rows for the positions below the group's largest one"""
    out = [a.copy() for a in arrays]
    for lo in range(0, len(parent), w):
        L = int(pos[lo:lo + w].max())
        for a, o in zip(arrays, out):
            o[lo:lo + w, :L] = np.take(a[:, :L], parent[lo:lo + w], axis=0)
    return out


# ---- generate(num_beams=w) ------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def beam_reference(seed, w, eos=None, new=NEW, length_penalty=1.0):
    """beam search of each of speculate_cases' four prompts ALONE by a full float64 recompute per hypothesis: per prompt the w
    hypotheses best first as (tokens, float64 score, done); the index of the returned beam; the smallest gap between neighbouring
    candidates among the first w + 1 of any selection; dev32, the largest deviation of the candidate scores of a plain float32
    evaluation (float32 model, float32 log-softmax, float32 running score) along the same hypotheses"""
    model64, model32 = dc.make_model(CpuTensor, np.float64, seed), dc.make_model(CpuTensor, np.float32, seed)
    V = CFG["vocab_size"]
    results, gap, dev = [], np.inf, 0.0
    for prompt in sc.prompts(seed):
        hyps = [([], 0.0, np.float32(0.0), False)] + [([], -np.inf, np.float32(-np.inf), False)] * (w - 1)      # tokens, score64, score32, done
        for _ in range(new):
            if all(h[3] for h in hyps):
                break
            live = [i for i, h in enumerate(hyps) if not h[3]]
            seqs = np.stack([np.concatenate([prompt, np.array(hyps[i][0], np.int32)]) for i in live]).astype(np.int32)
            l64, l32 = dc.full_logits(model64, seqs)[:, -1], dc.full_logits(model32, seqs)[:, -1]
            cands = []
            with np.errstate(all="ignore"):
                for i, h in enumerate(hyps):
                    if h[3]:
                        cands.append((h[1], i * V, i, None, h[2]))
                        continue
                    x64, x32 = l64[live.index(i)], l32[live.index(i)]
                    v64 = h[1] + (x64 - x64.max() - np.log(np.exp(x64 - x64.max()).sum()))
                    v32 = (h[2] + (x32 - x32.max() - np.log(np.exp(x32 - x32.max()).sum(dtype=np.float32)))).astype(np.float32)
                    cands.extend((float(v64[j]), i * V + j, i, j, v32[j]) for j in range(V))
            cands.sort(key=lambda c: (-c[0], c[1]))
            top = [c for c in cands[:w + 1] if np.isfinite(c[0])]
            gap = min([gap] + [a[0] - b[0] for a, b in zip(top, top[1:])])
            dev = max([dev] + [abs(float(c[4]) - c[0]) for c in cands if np.isfinite(c[0])])
            hyps = [hyps[i] if j is None else (hyps[i][0] + [j], s, s32, eos is not None and j == eos) for s, _, i, j, s32 in cands[:w]]
        ranked = [h[1] / len(h[0]) ** length_penalty for h in hyps]
        results.append(([(np.array(h[0], np.int32), h[1], h[3]) for h in hyps], int(np.argmax(ranked))))
    return results, gap, dev


def assert_reference_rules_out_ties(seed, w, eos=None):
    """decode_cases' rule, from the references alone: gap >= 100 x the float32 deviation"""
    results, gap, dev = beam_reference(seed, w, eos)
    print("seed %d, %d beams, eos %s: candidate gap %.3g, float32 deviation %.3g" % (seed, w, eos, gap, dev))
    assert gap >= 100 * dev, "seed %d, %d beams: candidate gap %.3g below 100 x the float32 deviation %.3g - pick other inputs" % (seed, w, gap, dev)
    return results, dev


def expected(seed, w, eos=None, new=NEW):
    """(rows (4, longest prompt + new) of prompt, returned beam, PAD; sequences (4, w, columns); scores (4, w) float64)"""
    results, _, _ = beam_reference(seed, w, eos, new)
    ps = sc.prompts(seed)
    columns = max(len(p) for p in ps) + new
    rows, seqs, scores = np.full((len(ps), columns), PAD, np.int32), np.full((len(ps), w, columns), PAD, np.int32), np.zeros((len(ps), w))
    for r, (p, (hyps, best)) in enumerate(zip(ps, results)):
        for n, (tokens, score, _) in enumerate(hyps):
            seqs[r, n, :len(p)], seqs[r, n, len(p):len(p) + len(tokens)], scores[r, n] = p, tokens, score
        rows[r] = seqs[r, best]
    return rows, seqs, scores


def run(T, seed, w, model=None, eos=None, new=NEW, **options):
    """(ids (4, longest prompt + new), beams {sequences, scores, steps} as arrays, cache) of `generate(num_beams=w)` over
    speculate_cases' four prompts as one ragged batch on tensor class T"""
    model = dc.make_model(T, seed=seed) if model is None else model
    ps = sc.prompts(seed)
    lengths = [len(p) for p in ps]
    padded = np.zeros((len(ps), max(lengths)), np.int32)
    for r, p in enumerate(ps):
        padded[r, :len(p)] = p
    cache = nn.KVCache(CFG["num_hidden_layers"], len(ps) * w, CAPACITY, CFG["hidden_size"], like=model.cls.predictions.bias, per_row=True)
    beams = {}
    out = bert.generate(model, T.from_numpy(padded, requires_grad=False), new, lengths=lengths, eos_token_id=eos, pad_token_id=PAD, cache=cache,
                        num_beams=w, beams=beams, **options)
    assert out.dtype == np.int32 and isinstance(out, T) and tuple(out.shape) == (len(ps), max(lengths) + new)
    assert isinstance(beams["sequences"], T) and isinstance(beams["scores"], T)
    ids = out.numpy().copy()                                                  # the first read of anything but the poll word
    return ids, dict(sequences=beams["sequences"].numpy().copy(), scores=beams["scores"].numpy().copy(), steps=beams["steps"]), cache


def compare_with_reference(ids, beams, seed, w, eos, dev):
    """tokens exactly - every column up to a beam's position, PAD behind -, scores within the tolerance of the issue"""
    rows, seqs, scores = expected(seed, w, eos)
    np.testing.assert_array_equal(ids, rows)
    ps = sc.prompts(seed)
    results, _, _ = beam_reference(seed, w, eos)
    for r, (p, (hyps, _)) in enumerate(zip(ps, results)):
        for n, (tokens, score, _) in enumerate(hyps):
            used = len(p) + len(tokens)
            np.testing.assert_array_equal(beams["sequences"][r, n, :used], seqs[r, n, :used], err_msg="prompt %d beam %d" % (r, n))
            tol = 8 * dev + 2.0 ** -22 * max(1.0, abs(score))
            assert abs(float(beams["scores"][r, n]) - score) <= tol, (r, n, float(beams["scores"][r, n]), score, tol)
