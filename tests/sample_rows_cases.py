"""What test_sample_rows_cpu.py and test_hip_sample_rows.py share: the per-request sampling run of `serve` over the seven prompts
of serve_cases - a parameter set and a seed per request -, and its reference: each request ALONE by a full float64 recompute per
token, its g-th token drawn by the definition (`random.sample_tokens(seed, 0, L, T, k, p)[g]`, row g of L the logits behind the
prompt and the first g tokens).  Computed once per process and never changed afterwards.  No tests of its own.

Near-ties are ruled out from the references alone, over all 42 steps.  d is the largest deviation of the float32 full forward's
last-row logits from float64 over those steps.
  * a greedy step needs a top-2 margin >= 100 d (serve_cases' rule);
  * a sampled step needs a one-token band under sample_cases.acceptable(x, u, T, k, p, eps) with eps = max(1e-5, 400 d inv_T):
    logits that each move by at most d move (x_j - m) by at most 2 d, every weight by a factor within e^(+-2 d inv_T), a
    normalised cumulative sum by at most 4 d inv_T - and 100 times that bound is the margin the project uses for greedy ties;
  * with top-k on, additionally the gap between the k-th and the (k + 1)-th largest logit must be >= 100 d (`acceptable` does
    not band the top-k set).
BASE is the first seed base, counting up from 0, that satisfies this (request r has the seed BASE + r); it was found on the
float64 references alone - no backend was run - and `reference()` asserts the condition for it."""
import functools
import numpy as np
from lightgrad_amd import CpuTensor
from lightgrad_amd import random as lg_random
import decode_cases as dc
import sample_cases as smp
import serve_cases as sc

# (temperature, top_k, top_p) per request: two greedy ones, two that share a set, every filter alone and together
PARAMETERS = ((0, 0, 1), (1.0, 0, 1.0), (0.9, 20, 0.95), (0.7, 5, 1.0), (1.3, 0, 0.8), (0, 0, 1), (0.9, 20, 0.95))
BASE = 1
INDEX = (-1, 0, 3, 3, 1, 2, "n", 0, 4)      # the 9-row launch: a free row, two rows that share a table row, a row beyond the table


def columns():
    """temperature, top_k, top_p as three lists"""
    return [list(c) for c in zip(*PARAMETERS)]


def seeds(base=BASE):
    return [base + r for r in range(len(PARAMETERS))]


def table(base=BASE):
    return lg_random.sampling_table(*columns(), seeds(base))


def uniform(seed, g):
    return lg_random.sample_uniforms(seed, 0, g + 1)[g]


@functools.lru_cache(maxsize=None)
def forwards(base):
    """per request the steps (float64 last-row logits, float32 ones, token) of its run alone under seed base + r"""
    model64, model32 = dc.make_model(CpuTensor, np.float64, sc.SEED), dc.make_model(CpuTensor, np.float32, sc.SEED)
    runs = []
    for r, prompt in enumerate(sc.prompts()):
        t, k, p = PARAMETERS[r]
        seq, steps = prompt[None, :].copy(), []
        for g in range(sc.BUDGET):
            l64, l32 = dc.full_logits(model64, seq)[0, -1], dc.full_logits(model32, seq)[0, -1]
            if t == 0:
                token = int(np.argmax(l64))
            else:
                token = int(lg_random.sample_tokens(base + r, 0, np.repeat(l64[None, :], g + 1, axis=0), t, k, p)[g])
            steps.append((l64, l32, token))
            seq = np.concatenate([seq, np.array([[token]], np.int32)], axis=1)
        runs.append(steps)
    return runs


def near_ties(base):
    """(d, the steps (request, g, why) that the rules of the module text do not rule out)"""
    runs = forwards(base)
    d = max(float(np.abs(l32.astype(np.float64) - l64).max()) for steps in runs for l64, l32, _ in steps)
    failed = []
    for r, steps in enumerate(runs):
        t, k, p = PARAMETERS[r]
        for g, (l64, _, token) in enumerate(steps):
            top = np.sort(l64)
            if t == 0:
                if top[-1] - top[-2] < 100 * d:
                    failed.append((r, g, "top-2 margin %.3g" % (top[-1] - top[-2])))
                continue
            inv_t = float(np.float32(1.0 / np.float64(t)))
            band = smp.acceptable(l64, uniform(base + r, g), t, k, p, eps=max(1e-5, 400 * d * inv_t))
            if band.tolist() != [token]:
                failed.append((r, g, "band %s around token %d" % (band[:6].tolist(), token)))
            if 1 <= k < l64.size and top[-k] - top[-k - 1] < 100 * d:
                failed.append((r, g, "top-k gap %.3g" % (top[-k] - top[-k - 1])))
    return d, failed


@functools.lru_cache(maxsize=None)
def reference():
    """[tokens (BUDGET,)] per request under BASE, with the condition of the module text asserted over all 42 steps"""
    d, failed = near_ties(BASE)
    print("per-request reference: float32 deviation d = %.3g, seed base %d" % (d, BASE))
    assert not failed, "seed base %d leaves near-ties (request, step, why): %s - pick the next base" % (BASE, failed)
    tokens = [np.array([token for _, _, token in steps], np.int32) for steps in forwards(BASE)]
    for t in tokens:
        t.setflags(write=False)
    return tokens


def expected():
    """(out, out_len) that the references imply under serve_cases' BUDGET and EOS"""
    return sc.expected(reference(), sc.BUDGET, sc.EOS)


def options(base=BASE, **more):
    """the keywords of the per-request route"""
    t, k, p = columns()
    return dict(temperature=t, top_k=k, top_p=p, seeds=base, **more)
