"""What test_sample_cpu.py and test_hip_sample.py share: the cases of `Tensor.sample`, their logits (computed once per process and
never changed afterwards) and the ACCEPTANCE BAND of a row - the tokens a correct sampler may answer once its weights carry the
rounding of float32.  No tests of its own.

The band is evaluated in float64 from the definition in lightgrad_amd/random.py, with eps = 1e-5, the project's parity bar ("1e-5
relative otherwise", README), applied to CUMULATIVE PROBABILITY:
  * a nucleus level v (a value occurring in K) is admissible when mass{x_j >= v} >= (top_p - eps) * W and
    mass{x_j > v} < (top_p + eps) * W; with top-p off the only admissible level is K itself;
  * for an admissible level with set N, a token i with w_i > 0 is acceptable when C_{i-1} / W' - eps <= u <= C_i / W' + eps;
  * the band is the union over the admissible levels.
A degenerate row (a NaN, a maximum of +inf or -inf) has the one-token band {argmax}.

The logits are rows of standard_normal * 4 rounded to multiples of 1/8: peaked mass, and ties at both the top-k and the nucleus
boundary.  A case is (V, rows, parameters); its logits are the first `rows` rows of the 64 drawn for V, so the band of a row is
computed once.  The seed of each width's logits was chosen on the float64 definition alone (no backend was run): the first one,
counting up from 0, at which rows 0 .. 4 have a one-token band under every parameter set with stream seed STREAM_SEED and call
number STREAM_CALL - the condition test_sample_cpu.py asserts for the 1- and 5-row cases."""
import functools
import numpy as np
from lightgrad_amd import random as lg_random

EPS = 1e-5
STREAM_SEED, STREAM_CALL = 7, 3
WIDTHS = (1, 2, 33, 257, 4097, 30522)
CPU_WIDE = 40961                          # on the CPU side, in place of L and L + 1 (the widest row the LDS kernel takes, and one more)
ROWS = (1, 5, 64)
PARAMETERS = ((1.0, 0, 1.0), (0.7, 40, 1.0), (1.3, 0, 0.9), (0.8, 50, 0.95), (1.0, 1, 1.0), (0.25, 0, 0.5))
LOGIT_SEEDS = {40961: 1}                  # see the module text; every other width: seed 0
FREQUENCY_ROW = np.array([0, 1, -1, 2, 0.5, -np.inf, 2, -3], np.float32)
FREQUENCY_ROWS = 65536


@functools.lru_cache(maxsize=None)
def logits64(V):
    """(64, V) float32 logits of width V, read-only"""
    rng = np.random.RandomState(LOGIT_SEEDS.get(V, 0))
    x = (np.round(rng.standard_normal((64, V)) * 4.0 * 8.0) / 8.0).astype(np.float32)
    x.setflags(write=False)
    return x


def logits(V, rows):
    return logits64(V)[:rows]


def case_id(case):
    V, rows, (t, k, p) = case
    return "V%d-r%d-T%g-k%d-p%g" % (V, rows, t, k, p)


def cases(widths):
    return [(V, rows, prm) for V in widths for rows in ROWS for prm in PARAMETERS]


def acceptable(x, u, temperature, top_k, top_p, eps=EPS):
    """the band of ONE row x (1-D) for the uniform number u: a sorted int64 array of token indices"""
    x = np.asarray(x, np.float64)
    V = x.size
    m = np.max(x) if not np.isnan(x).any() else np.nan
    if np.isnan(m) or np.isinf(m):
        return np.array([np.argmax(x)], np.int64)
    keep = x >= np.partition(x, V - top_k)[V - top_k] if 1 <= top_k < V else np.ones(V, bool)
    inv_t = np.float64(np.float32(1.0 / np.float64(temperature)))
    w = np.where(keep, np.exp((x - m) * inv_t), 0.0)
    W = w.sum()
    if 0.0 < top_p < 1.0:
        values, inverse = np.unique(x[keep], return_inverse=True)                   # ascending
        per_value = np.bincount(inverse, weights=w[keep], minlength=values.size)
        at_or_above = np.cumsum(per_value[::-1])[::-1]
        above = at_or_above - per_value
        levels = values[(at_or_above >= (top_p - eps) * W) & (above < (top_p + eps) * W)]
    else:
        levels = np.array([x[keep].min()])
    band = np.zeros(V, bool)
    for v in levels:
        wn = np.where(keep & (x >= v), w, 0.0)
        c = np.cumsum(wn) / wn.sum()
        before = np.concatenate([[0.0], c[:-1]])
        band |= (wn > 0.0) & (before - eps <= u) & (u <= c + eps)
    return np.flatnonzero(band).astype(np.int64)


@functools.lru_cache(maxsize=None)
def bands(V, parameters, seed=STREAM_SEED, call=STREAM_CALL):
    """the bands of the 64 rows of width V under `parameters` for call number `call` of the stream seeded `seed`: a tuple of arrays"""
    u = lg_random.sample_uniforms(seed, call, 64)
    x = logits64(V)
    return tuple(acceptable(x[r], u[r], *parameters) for r in range(64))


def singleton_share(V, rows, parameters):
    return np.mean([b.size == 1 for b in bands(V, parameters)[:rows]])


def assert_in_band(tokens, V, rows, parameters, what):
    """every token of `tokens` (rows,) lies in its row's band; returns the boolean mask of the rows whose band is one token"""
    tokens = np.asarray(tokens).reshape(-1)
    assert tokens.shape == (rows,)
    band = bands(V, parameters)[:rows]
    outside = [(r, int(tokens[r]), band[r][:8].tolist()) for r in range(rows) if tokens[r] not in band[r]]
    assert not outside, "%s: (row, token, band) outside the acceptance band: %s" % (what, outside[:5])
    return np.array([b.size == 1 for b in band])


def frequency_z(tokens, temperature):
    """(counts, z scores) of the frequency case: tokens of FREQUENCY_ROWS rows of FREQUENCY_ROW against the multinomial expectation"""
    p = np.exp(FREQUENCY_ROW.astype(np.float64) / temperature)
    p /= p.sum()
    counts = np.bincount(np.asarray(tokens).reshape(-1), minlength=FREQUENCY_ROW.size)
    n = FREQUENCY_ROWS
    with np.errstate(divide="ignore", invalid="ignore"):
        z = np.where(p > 0, (counts - n * p) / np.sqrt(n * p * (1 - p)), 0.0)
    return counts, z
