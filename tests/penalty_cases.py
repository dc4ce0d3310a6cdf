"""What test_penalize_cpu.py and test_hip_penalize.py share: the cases of `penalize_rows` - nine rows of every kind, the
history-length edges - and the run of `serve` with per-request penalties over the seven prompts of serve_cases with its reference:
each request ALONE by a full float64 recompute per token, the float64 logits passed through the definition
(`random.penalize_logits`) with the request's own history, in the manner of sample_rows_cases.forwards.  Computed once per process
and never changed afterwards.  No tests of its own.

Near-ties are ruled out from the references alone, over all 42 steps of a run.  d is the largest deviation of the float32 full
forward's last-row logits from float64 over those steps.  The penalty map is piecewise linear with a slope of at most
lam = max(rho, 1 / rho), so a logit that moves by d moves by at most lam d behind it, and the rules are the project's own with
that factor:
  * a greedy step needs a top-2 margin of the penalised float64 logits >= 100 lam d;
  * a sampled step needs a one-token band under sample_cases.acceptable with eps = max(1e-5, 400 lam d inv_T);
  * with top-k on, the gap between the k-th and the (k + 1)-th largest penalised logit must be >= 100 lam d.
`reference(mode)` asserts this; no step is left out.  Two modes: "greedy", and "sampled" - sample_rows_cases.PARAMETERS under the
seed base 1 (base 0 leaves near-ties)."""
import functools
import numpy as np
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import paged_cases as pg
import sample_cases as smp
import sample_rows_cases as rc
import serve_cases as sc

# (rho, alpha, beta, min_new) per request
PARAMETERS = ((1.0, 0.0, 0.0, 0), (1.3, 0.0, 0.0, 0), (1.0, 0.6, 0.0, 0), (1.0, 0.0, 0.4, 2), (1.5, 0.5, 0.25, 0), (0.8, 0.0, 0.0, 0), (1.2, 0.0, 0.3, 5))
BUDGET, EOS = sc.BUDGET, sc.EOS
BASE = 1
MODES = ("greedy", "sampled")


def keywords():
    rho, alpha, beta, min_new = (list(c) for c in zip(*PARAMETERS))
    return dict(repetition_penalty=rho, presence_penalty=alpha, frequency_penalty=beta, min_new_tokens=min_new)


def table():
    return lg_random.penalty_table(*(list(c) for c in zip(*PARAMETERS)))


def options(mode, **more):
    """the keywords of `serve` for a mode"""
    return dict(keywords(), **(rc.options(BASE) if mode == "sampled" else {}), **more)


def sampling(mode, r):
    return rc.PARAMETERS[r] if mode == "sampled" else (0, 0, 1)


@functools.lru_cache(maxsize=None)
def models():
    return dc.make_model(CpuTensor, np.float64, sc.SEED), dc.make_model(CpuTensor, np.float32, sc.SEED)


def penalised(l64, r, prompt, tokens):
    """the float64 logits of request r behind `prompt` and `tokens`, through the definition with that history"""
    out = np.zeros((1, BUDGET), np.int32)
    out[0, :len(tokens)] = tokens
    y, bad = lg_random.penalize_logits(l64[None, :], table()[r:r + 1], [0], prompt[None, :], [len(prompt)], out, [len(tokens)], eos=EOS)
    assert not bad.any()
    return y[0]


@functools.lru_cache(maxsize=None)
def forwards(mode, prefixed=False):
    """per request the steps (penalised float64 last-row logits, |float32 - float64| of the logits in front of the penalties, token)
    of its run alone"""
    model64, model32 = models()
    runs = []
    for r, prompt in enumerate(pg.prefixed_prompts() if prefixed else sc.prompts()):
        t, k, p = sampling(mode, r)
        seq, steps, tokens = prompt[None, :].copy(), [], []
        for g in range(BUDGET):
            l64, l32 = dc.full_logits(model64, seq)[0, -1], dc.full_logits(model32, seq)[0, -1]
            y = penalised(l64, r, prompt, tokens)
            if t == 0:
                token = int(np.argmax(y))
            else:
                token = int(lg_random.sample_tokens(BASE + r, 0, np.repeat(y[None, :], g + 1, axis=0), t, k, p)[g])
            steps.append((y, float(np.abs(l32.astype(np.float64) - l64).max()), token))
            tokens.append(token)
            seq = np.concatenate([seq, np.array([[token]], np.int32)], axis=1)
        runs.append(steps)
    return runs


def near_ties(mode, prefixed=False):
    """(d, the steps (request, g, why) that the rules of the module text do not rule out)"""
    runs = forwards(mode, prefixed)
    d = max(dev for steps in runs for _, dev, _ in steps)
    failed = []
    for r, steps in enumerate(runs):
        t, k, p = sampling(mode, r)
        lam = max(float(np.float32(PARAMETERS[r][0])), 1.0 / float(np.float32(PARAMETERS[r][0])))
        for g, (y, _, token) in enumerate(steps):
            top = np.sort(y)
            if t == 0:
                if not top[-1] - top[-2] >= 100 * lam * d:
                    failed.append((r, g, "top-2 margin %.3g" % (top[-1] - top[-2])))
                continue
            inv_t = float(np.float32(1.0 / np.float64(t)))
            band = smp.acceptable(y, rc.uniform(BASE + r, g), t, k, p, eps=max(1e-5, 400 * lam * d * inv_t))
            if band.tolist() != [token]:
                failed.append((r, g, "band %s around token %d" % (band[:6].tolist(), token)))
            if 1 <= k < y.size and not top[-k] - top[-k - 1] >= 100 * lam * d:
                failed.append((r, g, "top-k gap %.3g" % (top[-k] - top[-k - 1])))
    return d, failed


@functools.lru_cache(maxsize=None)
def reference(mode, prefixed=False):
    """[tokens (BUDGET,)] per request, with the condition of the module text asserted over all 42 steps"""
    d, failed = near_ties(mode, prefixed)
    print("penalty reference (%s%s): float32 deviation d = %.3g" % (mode, ", prefixed prompts" if prefixed else "", d))
    assert not failed, "%s%s: near-ties (request, step, why): %s" % (mode, " prefixed" if prefixed else "", failed)
    tokens = [np.array([token for _, _, token in steps], np.int32) for steps in forwards(mode, prefixed)]
    for t in tokens:
        t.setflags(write=False)
    return tokens


def expected(mode, prefixed=False):
    """(out, out_len) that the references imply under BUDGET and EOS"""
    return sc.expected(reference(mode, prefixed), BUDGET, EOS)


# ---- the op: nine rows of every kind ----------------------------------------------------------------------------------------------

V, NINE_EOS = 101, 18
SPECIALS = np.array([-2.5, 3.25, 0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
PAD_IDS = (1000, -5, V, 2 ** 31 - 1)        # what lies behind len and behind g: never read


@functools.lru_cache(maxsize=None)
def nine_rows(V=V):
    """{name: array} of one launch over rc.INDEX = (-1, 0, 3, 3, 1, 2, "n", 0, 4) with n = 5 requests:
      row 0        free, its logits all NaN
      rows 1, 7    request 0: `eos` inside its history and g = 2 < min_new = 4
      rows 2, 3    request 3, shared: row 2 has negative, positive, +0.0, -0.0, +inf, -inf and NaN logits at ids of the prompt alone
                   (10 .. 16) and at ids of the tokens (20 .. 26, counts 1 and 2)
      row 4        request 1: g = 0
      row 5        request 2: its whole history is one id repeated
      row 6        beyond the table
      row 8        request 4: neutral penalties, `eos` outside its history and g = 1 < min_new = 3"""
    n, P, G = 5, 9, 11
    rng = np.random.RandomState(5)
    x = (3 * rng.standard_normal((9, V))).astype(np.float32)
    x[0] = np.nan
    x[2, 10:17], x[2, 20:27] = SPECIALS, SPECIALS
    prompts, out = np.resize(np.array(PAD_IDS, np.int32), (n, P)), np.resize(np.array(PAD_IDS[::-1], np.int32), (n, G))
    history = {0: ([4, NINE_EOS, 9, 4], [30, NINE_EOS]), 1: ([1, 2, 3, 2, 1], []), 2: ([7, 7, 7], [7, 7, 7, 7]),
               3: ([10, 11, 12, 13, 14, 15, 16, 20, 21], [20, 21, 22, 23, 24, 25, 26, 22, 23, 24, 25]), 4: ([40, 41], [42])}
    prompt_len, out_len = np.zeros(n, np.int32), np.zeros(n, np.int32)
    for i, (a, b) in history.items():
        prompts[i, :len(a)], out[i, :len(b)], prompt_len[i], out_len[i] = a, b, len(a), len(b)
    table = lg_random.penalty_table([1.3, 0.8, 1.5, 1.2, 1.0], [0.5, 0.6, 0.2, 0.7, 0.0], [0.25, 0.4, 0.3, 0.35, 0.0], [4, 0, 0, 0, 3])
    index = np.array([n if i == "n" else i for i in rc.INDEX], np.int32)
    case = dict(logits=x, table=table, index=index, prompts=prompts, prompt_len=prompt_len, out=out, out_len=out_len)
    for a in case.values():
        a.setflags(write=False)
    return case


NINE_BAD = [False] * 6 + [True] + [False] * 2


def bad_causes():
    """{what: a change of nine_rows() that makes row 4 (request 1) - and nothing else - bad}: {name: (position, value)}"""
    bits = lambda f: int(np.float32(f).view(np.int32))           # noqa: E731
    return {"len < 0": dict(prompt_len=(1, -1)), "len > P": dict(prompt_len=(1, 10)), "g < 0": dict(out_len=(1, -1)), "g > G": dict(out_len=(1, 12)),
            "rho = 0": dict(table=((1, 0), 0)), "rho = -0.0": dict(table=((1, 0), bits(-0.0))), "rho < 0": dict(table=((1, 0), bits(-1.5))),
            "rho inf": dict(table=((1, 0), bits(np.inf))), "rho NaN": dict(table=((1, 0), bits(np.nan))),
            "alpha inf": dict(table=((1, 1), bits(-np.inf))), "alpha NaN": dict(table=((1, 1), bits(np.nan))),
            "beta inf": dict(table=((1, 2), bits(np.inf))), "beta NaN": dict(table=((1, 2), bits(np.nan))),
            "min_new < 0": dict(table=((1, 3), -1)),
            "prompt id = V": dict(prompts=((1, 4), V)), "prompt id < 0": dict(prompts=((1, 0), -1)),
            "token id = V": dict(out=((1, 0), V), out_len=(1, 1)), "token id < 0": dict(out=((1, 1), -3), out_len=(1, 2))}


def changed(case, change):
    case = {k: v.copy() for k, v in case.items()}
    for name, (at, value) in change.items():
        case[name][at] = value
    return case


# ---- the op: the edges of the history length ------------------------------------------------------------------------------------

EDGES = (1, 63, 64, 65, 255, 256, 257, 512, 4096)       # the wave, the workgroup, the project's positions, the LDS bound


@functools.lru_cache(maxsize=None)
def edge(L):
    """{name: array}: two requests with a history of L ids each, P + G = L (L = 1: P = G = 1 with g = 0 - both arrays have a
    column), one row per request: request 0 has L DISTINCT ids (V = max(101, L + 3)), request 1 draws its ids from 7 values, so
    that counts reach the hundreds"""
    G = max(L // 2, 1)
    P = max(L - G, 1)
    g = L - P
    width = max(V, L + 3)
    rng = np.random.RandomState(L)
    ids = np.stack([rng.permutation(width)[:P + G], rng.choice(rng.permutation(width)[:7], P + G)]).astype(np.int32)
    case = dict(logits=(3 * rng.standard_normal((2, width))).astype(np.float32), table=lg_random.penalty_table([1.3, 0.8], 0.5, [0.25, 0.015625], 0),
                index=np.array([0, 1], np.int32), prompts=ids[:, :P].copy(), prompt_len=np.full(2, P, np.int32), out=ids[:, P:].copy(),
                out_len=np.full(2, g, np.int32))
    for a in case.values():
        a.setflags(write=False)
    return case


def by_hand(case, eos=None):
    """the definition as a plain loop over the elements, in the logits' own precision: (y, bad)"""
    x, table = case["logits"], case["table"]
    real = x.dtype.type
    n, P, G, width = table.shape[0], case["prompts"].shape[1], case["out"].shape[1], x.shape[1]
    y, bad = x.copy(), np.zeros(x.shape[0], bool)
    with np.errstate(all="ignore"):
        for r, i in enumerate(case["index"].tolist()):
            if i < 0:
                continue
            if i >= n:
                bad[r] = True
                continue
            rho, alpha, beta = (real(v) for v in table[i, :3].view(np.float32))
            length, g, min_new = int(case["prompt_len"][i]), int(case["out_len"][i]), int(table[i, 3])
            if not (0 <= length <= P and 0 <= g <= G and np.isfinite(rho) and rho > 0 and np.isfinite(alpha) and np.isfinite(beta) and min_new >= 0):
                bad[r] = True
                continue
            history = case["prompts"][i, :length].tolist() + case["out"][i, :g].tolist()
            if any(not 0 <= v < width for v in history):
                bad[r] = True
                continue
            count = {}
            for v in case["out"][i, :g].tolist():
                count[v] = count.get(v, 0) + 1
            for v in sorted(set(history)):
                value = y[r, v]
                value = value * rho if value < 0 else value / rho
                if v in count:
                    value = (value - beta * real(count[v])) - alpha
                y[r, v] = value
            if eos is not None and g < min_new:
                y[r, eos] = -np.inf
    return y, bad


def same_bits(got, want):
    """equal bit for bit where the value is no NaN, a NaN for a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    nan = np.isnan(want)
    word = np.uint32 if want.dtype == np.float32 else np.uint64
    return got.dtype == want.dtype and got.shape == want.shape and bool((np.isnan(got) == nan).all()) and \
        bool((got.view(word)[~nan] == want.view(word)[~nan]).all())
