"""What test_logprob_cpu.py and test_hip_logprob.py share: the cases of `logprob_rows` - nine rows of every kind at any width, the
definition once more as a plain loop - and the float64 references of `serve(logprobs=)` over the seven prompts of serve_cases:
each request ALONE by a full float64 recompute per token, as serve_cases.greedy_reference builds its tokens, its last-row logits
passed through the definition (`random.token_logprobs_rows`) into float64 arrays.  Computed once per process and never changed
afterwards.  No tests of its own.

Bounds, from the references alone.  d is the deviation serve_cases.greedy_reference measures: the float32 full forward's last-row
logits against float64.  The project's rule allows a backend 100 d on a logit; log-softmax moves at most twice as far as its
logits (x_t - L with |dL| <= max |dx|), so a log-probability may differ by 200 d.  An id of `top_ids` is held exactly wherever the
reference's gaps to both neighbouring ranks are >= 100 d; `reference()` asserts that for the plain model this is EVERY gap between
consecutive ranks 1 .. 9 at every step ("pick another seed" otherwise), so no id is left out there.  With K and V rounded to
bfloat16 (kv_dtype="bf16") the reference is paged_bf16_cases' rounded model and the factor its 20 in place of 100: 40 d' on a
value, ids exact where the gaps are >= 20 d'."""
import functools
import numpy as np
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import serve_cases as sc

N_MAX = lg_random.LOGPROB_MAX_TOP
MIXED = (3, 0, 8, -1, 3, 8, None)       # per request: the mix of none, the token's only, 3 and 8
BUDGET, EOS = sc.BUDGET, sc.EOS


# ---- the op: nine rows of every kind ------------------------------------------------------------------------------------------

INDEX = (-1, 0, 3, 6, 1, 2, 7, 5, 4)    # row -> request: a free row, then eight distinct requests
WANT = (0, 3, 8, -1, 1, 8, 5, 2)        # per request
COUNTER = (0, 3, 1, 2, 0, 3, 2, 1)      # per request: its column of G = 4
G = 4


@functools.lru_cache(maxsize=None)
def nine_rows(V=101, seed=0):
    """{name: array} of one launch over INDEX:
      row 0   free, its logits all NaN                      row 1   request 0: the token's log-probability only
      row 2   request 3, which wants nothing: all NaN       row 3   request 6 (5 ids): a NaN in it - degenerate
      row 4   request 1 (3 ids): negative values, -inf at every third id, -0.0 and +0.0 side by side as its largest; the token is
              one of the -inf ids where there is one
      row 5   request 2 (8 ids): every value equal          row 6   request 7 (2 ids): a +inf in it - degenerate
      row 7   request 5 (8 ids): nothing but -inf - degenerate
      row 8   request 4 (1 id): random"""
    rng = np.random.RandomState(1000 * seed + V % 997)
    x = (3 * rng.standard_normal((9, V))).astype(np.float32)
    token = rng.randint(0, V, 9).astype(np.int32)
    x[0], x[2] = np.nan, np.nan
    x[3, V // 2] = np.nan
    x[4] = -np.abs(x[4]) - 0.5
    if V >= 4:
        x[4, ::3] = -np.inf
        token[4] = 3 * (V // 6)
    if V >= 2:
        x[4, V - 2], x[4, V - 1] = -0.0, 0.0
    x[5] = np.float32(1.25)
    x[6, V - 1] = np.inf
    x[7] = -np.inf
    case = dict(logits=x, token=token, want=np.array(WANT, np.int32), index=np.array(INDEX, np.int32), counter=np.array(COUNTER, np.int32))
    for a in case.values():
        a.setflags(write=False)
    return case


def fills(n, g=G, n_max=N_MAX, real=np.float32):
    """the three outputs as a pool starts them: (logprob (n, g), top_ids (n, g, n_max), top_logprob (n, g, n_max))"""
    return np.zeros((n, g), real), np.full((n, g, n_max), -1, np.int32), np.zeros((n, g, n_max), real)


def defined(case, real=np.float64, n_max=N_MAX, g=G):
    """(logprob, top_ids, top_logprob, bad) of the definition from the fills, in `real`"""
    out = fills(len(case["want"]), g, n_max, real)
    bad = lg_random.token_logprobs_rows(case["logits"], case["token"], case["want"], case["index"], case["counter"], *out)
    return out + (bad,)


def by_hand(case, n_max=N_MAX, g_columns=G):
    """the definition once more, element by element in python floats: (logprob, top_ids, top_logprob, bad) in float64"""
    import math
    x, want = case["logits"], case["want"]
    V, N = x.shape[1], len(want)
    logprob, top_ids, top = fills(N, g_columns, n_max, np.float64)
    bad = np.zeros(x.shape[0], bool)
    for r, i in enumerate(case["index"].tolist()):
        if i < 0 or (i < N and want[i] == -1):
            continue
        if i >= N or not (0 <= want[i] <= n_max and 0 <= case["counter"][i] < g_columns and 0 <= case["token"][r] < V):
            bad[r] = True
            continue
        k, g, row = int(want[i]), int(case["counter"][i]), [float(v) for v in x[r]]
        m = max(row) if not any(math.isnan(v) for v in row) else math.nan
        if math.isnan(m) or math.isinf(m):
            logprob[i, g], top_ids[i, g, :k], top[i, g, :k] = math.nan, -1, math.nan
            continue
        L = m + math.log(math.fsum(math.exp(v - m) for v in row))
        logprob[i, g] = row[int(case["token"][r])] - L
        order = sorted(range(V), key=lambda j: (-row[j], j))[:k]         # (-0.0 == 0.0 for python's comparison, too)
        for rank, j in enumerate(order):
            top_ids[i, g, rank], top[i, g, rank] = j, row[j] - L
    return logprob, top_ids, top, bad


def bad_causes(V=101):
    """{what: a change of nine_rows(V) that makes row 8 (request 4) - and nothing else - bad}: {name: (position, value)}"""
    return {"i = N": dict(index=(8, 8)), "i beyond N": dict(index=(8, 2 ** 31 - 1)), "g < 0": dict(counter=(4, -1)), "g = G": dict(counter=(4, G)),
            "want < -1": dict(want=(4, -2)), "want > n_max": dict(want=(4, N_MAX + 1)), "token < 0": dict(token=(8, -1)), "token = V": dict(token=(8, V))}


def changed(case, change):
    case = {k: v.copy() for k, v in case.items()}
    for name, (at, value) in change.items():
        case[name][at] = value
    return case


def same_bits(got, want):
    """equal bit for bit where the value is no NaN, a NaN for a NaN"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return bool((got == want).all())
    nan = np.isnan(want)
    word = np.uint32 if want.dtype == np.float32 else np.uint64
    return bool((np.isnan(got) == nan).all()) and bool((got.view(word)[~nan] == want.view(word)[~nan]).all())


def assert_close_to_definition(got, case, n_max=N_MAX, g=G):
    """the op's contract against the float64 definition: ids equal, values within 1e-5 max(1, |want|), -inf and NaN exact, and
    whatever the definition leaves at its fill keeps the fill's bytes"""
    logprob, top_ids, top, _ = defined(case, np.float64, n_max, g)
    np.testing.assert_array_equal(got[1], top_ids)
    for name, have, want in (("logprob", got[0], logprob), ("top_logprob", got[2], top)):
        assert have.dtype == np.float32 and have.shape == want.shape, name
        finite = np.isfinite(want)
        assert (np.isnan(have) == np.isnan(want)).all() and (have[~finite & ~np.isnan(want)] == want[~finite & ~np.isnan(want)]).all(), name
        error = np.abs(have[finite].astype(np.float64) - want[finite]) / np.maximum(1.0, np.abs(want[finite]))
        assert error.size == 0 or error.max() <= 1e-5, "%s: %.3g" % (name, error.max())
    untouched = np.ones(logprob.shape, bool)
    for r, i in enumerate(case["index"].tolist()):
        if 0 <= i < len(case["want"]) and case["want"][i] >= 0 and 0 <= case["counter"][i] < g and 0 <= case["token"][r] < case["logits"].shape[1]:
            untouched[i, case["counter"][i]] = False
    assert same_bits(got[0][untouched], np.zeros(int(untouched.sum()), np.float32)), "a cell nobody owns changed"
    behind = (top_ids < 0) & ~np.isnan(top)
    assert same_bits(got[2][behind], np.zeros(int(behind.sum()), np.float32)), "an entry behind k changed"


# ---- serve: the float64 references ------------------------------------------------------------------------------------------------

def want_of(logprobs):
    return lg_random.logprob_want(logprobs, len(sc.prompts()))


@functools.lru_cache(maxsize=None)
def forwards(rounded=False):
    """per request the float64 last-row logits of every step of its greedy run alone, and (tokens, d): the run's tokens and the
    float32 deviation, both as serve_cases.greedy_reference (rounded: paged_bf16_cases.rounded_reference) gives them"""
    if rounded:
        import paged_bf16_cases as pb
        model64, (tokens, _, d) = pb.rounded_model(np.float64), pb.rounded_reference(False)
    else:
        model64, (tokens, _, d) = dc.make_model(CpuTensor, np.float64, sc.SEED), sc.greedy_reference()
    runs = []
    for prompt, toks in zip(sc.prompts(), tokens):
        steps = []
        for g in range(BUDGET):
            l64 = dc.full_logits(model64, np.concatenate([prompt, toks[:g]])[None, :].astype(np.int32))[0, -1]
            assert int(l64.argmax()) == int(toks[g])
            l64.setflags(write=False)
            steps.append(l64)
        runs.append(steps)
    return runs, tokens, d


def smallest_gap(steps_of_runs):
    """the smallest gap between consecutive ranks 1 .. 9 over the steps given"""
    return min(float((-np.diff(np.sort(l)[::-1][:N_MAX + 1])).min()) for steps in steps_of_runs for l in steps)


def from_logits(rows, tokens, out_len, want, factor, d):
    """the references of a run from per-request float64 logits `rows[r][g]` and tokens: (logprob (N, G) float64, top_ids (N, G, n),
    top (N, G, n) float64, exact (N, G, n) bool: the ids whose gaps to both neighbouring ranks are >= factor * d)"""
    n = len(rows)
    width = max(int(want.max()), 1)
    logprob, top_ids, top = fills(n, BUDGET, width, np.float64)
    exact = np.ones(top_ids.shape, bool)
    for r in range(n):
        for g in range(int(out_len[r])):
            one = fills(1, 1, width, np.float64)
            bad = lg_random.token_logprobs_rows(rows[r][g][None, :], [int(tokens[r][g])], [int(want[r])], [0], [0], *one)
            assert not bad.any()
            logprob[r, g], top_ids[r, g], top[r, g] = one[0][0, 0], one[1][0, 0], one[2][0, 0]
            gaps = -np.diff(np.sort(rows[r][g])[::-1][:width + 1])                     # gaps[j]: between ranks j + 1 and j + 2
            safe = gaps >= factor * d
            exact[r, g, :len(safe)] = safe & np.r_[True, safe[:-1]]
    return logprob, top_ids, top, exact


@functools.lru_cache(maxsize=None)
def reference(logprobs, rounded=False):
    """(logprob, top_ids, top, exact, bound) for `serve(logprobs=)` under BUDGET and EOS: the float64 arrays with their fills, which
    ids are held exactly, and the bound on a value.  For the plain model every gap is asserted, so `exact` is all True"""
    runs, tokens, d = forwards(rounded)
    factor = 20 if rounded else 100
    if not rounded:
        gap = smallest_gap(runs)
        print("log-probability reference: smallest gap between ranks 1 .. %d %.3g, float32 deviation %.3g" % (N_MAX + 1, gap, d))
        assert gap >= factor * d, "seed %d: a gap of %.3g between consecutive ranks below 100 x the float32 deviation %.3g - pick another seed" % (sc.SEED, gap, d)
    _, out_len = sc.expected(tokens, BUDGET, EOS)
    out = from_logits(runs, tokens, out_len, want_of(logprobs), factor, d) + (2 * factor * d,)
    assert rounded or out[3].all()
    for a in out[:4]:
        a.setflags(write=False)
    return out


def assert_matches(got, ref):
    """got: the three arrays of a run (`stats["logprobs"]` read back); ref: (logprob, top_ids, top, exact, bound)"""
    logprob, top_ids, top, exact, bound = ref
    assert got["token"].dtype == np.float32 and got["top"].dtype == np.float32 and got["top_ids"].dtype == np.int32
    assert got["token"].shape == logprob.shape and got["top_ids"].shape == top_ids.shape and got["top"].shape == top.shape
    np.testing.assert_array_equal(got["top_ids"][exact], top_ids[exact])
    np.testing.assert_array_equal(got["top_ids"] < 0, top_ids < 0)                       # the fills, whatever is exact
    for name, have, want, filled in (("token", got["token"], logprob, logprob == 0), ("top", got["top"], top, top_ids < 0)):
        assert same_bits(have[filled], np.zeros(int(filled.sum()), np.float32)), "%s: a fill changed" % name
        error = np.abs(have[~filled].astype(np.float64) - want[~filled])
        print("%s: largest error %.3g against the bound %.3g" % (name, error.max() if error.size else 0.0, bound))
        assert error.size == 0 or error.max() <= bound, "%s: %.3g above %.3g" % (name, error.max(), bound)


def read_back(stats):
    return {k: t.numpy().copy() for k, t in stats["logprobs"].items()}


def alone(model32, out, out_len, want, d, penalties=None, factor=100):
    """the references of a run whose tokens `out` are given (penalised or sampled: not the greedy ones), from the float32 CpuTensor
    model's full forward of every request ALONE along those tokens, its logits through `random.penalize_logits` (penalties: the
    table) and the definition.  lam = max(rho, 1 / rho) is the penalty map's largest slope: the bound is 2 * factor * lam * d"""
    rows, lam = [], 1.0
    for r, prompt in enumerate(sc.prompts()):
        steps = []
        for g in range(int(out_len[r])):
            l = dc.full_logits(model32, np.concatenate([prompt, out[r, :g]])[None, :].astype(np.int32))[0, -1].astype(np.float64)
            if penalties is not None:
                stored = np.zeros((1, BUDGET), np.int32)
                stored[0, :g] = out[r, :g]
                y, bad = lg_random.penalize_logits(l[None, :], penalties[r:r + 1], [0], prompt[None, :], [len(prompt)], stored, [g], eos=EOS)
                assert not bad.any()
                l = y[0]
                rho = float(penalties[r:r + 1, 0].view(np.float32)[0])
                lam = max(lam, rho, 1.0 / rho)
            steps.append(l)
        rows.append(steps)
    return from_logits(rows, out, out_len, want, factor * lam, d) + (2 * factor * lam * d,)
