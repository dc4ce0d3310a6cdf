"""The random stream behind `Tensor.dropout` and `Tensor.mlm_mask`: one definition, arithmetic only, shared by both backends.

The generator is Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds).  Its
state is a 64-bit `seed` and the 64-bit number of dropout calls so far, `draws`.  For the call with draws == b, element i of
the flattened dense tensor takes word i % 4 of

    philox4x32_10(counter = (lo32(i // 4), hi32(i // 4), lo32(b), hi32(b)), key = (lo32(seed), hi32(seed)))

and is kept iff that word >= T, T = min(floor(p * 2**32), 2**32 - 1); kept elements are scaled by s = float32(1 / (1 - p)).
A call advances `draws` by exactly one, whatever the tensor's size.  The numpy backend evaluates this here; the HIP backend
evaluates the same arithmetic in csrc/dropout.hip from a state that lives in device memory, so the two produce the same mask
bit for bit, and a captured hipGraph draws a fresh mask on every replay.

`Tensor.mlm_mask` (BERT's token masking) is one call of the same stream, `draws` advancing by one: for the call with
draws == b, element i of the flattened ids takes the WHOLE block

    w = philox4x32_10(counter = (lo32(i), hi32(i), lo32(b), hi32(b)), key)        = words(seed, b, 4 * n).reshape(n, 4)[i]

and is selected iff ids[i] is none of the special ids and w[0] < T (the T above).  An element that is not selected keeps its id
and gets the label `ignore_index`; a selected one gets its id as label and becomes the mask token if w[1] < floor(0.8 * 2**32),
the uniform token (uint64(w[2]) * vocab_size) >> 32 if w[1] < floor(0.9 * 2**32), and stays as it is otherwise.
`mlm_mask_words` below is the definition; csrc/mlm.hip evaluates it on the device.

`Tensor.sample` (sampled decoding: temperature, top-k, top-p) is one call of the same stream too: for the call with draws == b,
ROW r of the logits takes word 0 of the block of counter r and u = ((word >> 8) + 0.5) * 2**-24.  `sample_tokens` below is the
definition, in float64, and is the numpy backend; csrc/sample.hip evaluates it on the device with float32 weights held as
integers - its token is the definition's wherever u is further than that rounding from a boundary of the cumulative weights.

    manual_seed(seed)        seed every backend's generator, draws back to 0
    get_state(backend)       (seed, draws) of "cpu" or "hip"
"""
import ctypes
import numpy as np

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LOW, _SHIFT = np.uint64(0xFFFFFFFF), np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, key: two 32-bit ints -> uint32 array [..., 4]"""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & _LOW for c in counter])
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> _SHIFT) ^ c1 ^ np.uint64(k0), p1 & _LOW, (p0 >> _SHIFT) ^ c3 ^ np.uint64(k1), p0 & _LOW
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return np.stack([c0, c1, c2, c3], axis=-1).astype(np.uint32)


def words(seed: int, draw: int, n: int, first_group: int = 0) -> np.ndarray:
    """the stream's words for elements 4 * first_group ... 4 * first_group + n - 1 of call number `draw`"""
    groups = np.arange(first_group, first_group + (n + 3) // 4, dtype=np.uint64)
    w = philox4x32_10((groups & _LOW, groups >> _SHIFT, draw & 0xFFFFFFFF, (draw >> 32) & 0xFFFFFFFF),
                      (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return w.reshape(-1)[:n]


def threshold(p: float) -> int:
    """T: an element is kept iff its word >= T"""
    return min(int(np.floor(np.float64(p) * 4294967296.0)), 4294967295)


def scale(p: float) -> np.float32:
    """s: the division in double, rounded to float32 once"""
    return np.float32(1.0 / (1.0 - np.float64(p)))


def keep_mask(seed: int, draw: int, n: int, p: float) -> np.ndarray:
    return words(seed, draw, n) >= np.uint32(threshold(p))


MLM_MASK_BELOW, MLM_RANDOM_BELOW = 3435973836, 3865470566        # floor(0.8 * 2**32), floor(0.9 * 2**32)
MLM_MAX_SPECIAL = 8


def check_mlm_arguments(dtype, p, mask_token_id, vocab_size, special_ids, ignore_index):
    """the validated (p, mask_token_id, vocab_size, special_ids, ignore_index) of an `mlm_mask` call on ids of `dtype`"""
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise TypeError("mlm_mask: ids must be int32 or int64 (got %s)" % dtype)
    p = check_probability(p)
    mask_token_id, vocab_size, ignore_index = int(mask_token_id), int(vocab_size), int(ignore_index)
    special_ids = tuple(int(t) for t in special_ids)
    if len(special_ids) > MLM_MAX_SPECIAL:
        raise ValueError("mlm_mask: at most %d special ids (got %d)" % (MLM_MAX_SPECIAL, len(special_ids)))
    if not 1 <= vocab_size <= 1 << 31:
        raise ValueError("mlm_mask: vocab_size must lie in [1, 2**31] (got %r)" % vocab_size)
    info = np.iinfo(dtype)
    for name, v in (("mask_token_id", mask_token_id), ("ignore_index", ignore_index)):
        if not info.min <= v <= info.max:
            raise ValueError("mlm_mask: %s = %d does not fit %s" % (name, v, dtype))
    return p, mask_token_id, vocab_size, special_ids, ignore_index


def mlm_mask_words(seed: int, draw: int, ids, p: float, mask_token_id: int, vocab_size: int, special_ids=(), ignore_index: int = -100):
    """(masked ids, labels) of call number `draw` for the integer array `ids`: same dtype and shape"""
    ids = np.asarray(ids)
    flat = ids.reshape(-1)
    w = words(seed, draw, 4 * flat.size).reshape(flat.size, 4)          # element i: the block of counter i
    selected = (w[:, 0] < np.uint32(threshold(p))) & ~np.isin(flat, np.asarray(special_ids, dtype=np.int64))
    uniform = ((w[:, 2].astype(np.uint64) * np.uint64(vocab_size)) >> _SHIFT).astype(ids.dtype)
    replaced = np.where(w[:, 1] < np.uint32(MLM_MASK_BELOW), ids.dtype.type(mask_token_id),
                        np.where(w[:, 1] < np.uint32(MLM_RANDOM_BELOW), uniform, flat))
    masked = np.where(selected, replaced, flat).astype(ids.dtype)
    labels = np.where(selected, flat, ids.dtype.type(ignore_index)).astype(ids.dtype)
    return masked.reshape(ids.shape), labels.reshape(ids.shape)


def check_sample_arguments(logits_dtype, vocab, temperature, top_k, top_p, dtype):
    """the validated (temperature, top_k, top_p, dtype) of a `sample` call on logits of `logits_dtype` whose last axis is `vocab` wide"""
    if not np.issubdtype(np.dtype(logits_dtype), np.floating):
        raise ValueError("sample: the logits must be floating point (got %s)" % np.dtype(logits_dtype))
    if vocab is None or vocab < 1:
        raise ValueError("sample: the logits need a last axis of at least one element")
    temperature, top_k, top_p = float(temperature), int(top_k), float(top_p)
    if not (temperature > 0.0 and np.isfinite(temperature) and np.isfinite(np.float32(1.0 / temperature))):
        raise ValueError("sample: temperature must be positive and finite, with 1 / temperature finite in float32 (got %r)" % temperature)
    if top_k < 0:
        raise ValueError("sample: top_k must be >= 0, 0 = off (got %r)" % top_k)
    if not 0.0 < top_p <= 1.0:
        raise ValueError("sample: top_p must satisfy 0 < top_p <= 1, 1 = off (got %r)" % top_p)
    dtype = np.dtype(dtype)
    if dtype not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError("sample: the tokens are int32 or int64 (got %s)" % dtype)
    return temperature, top_k, top_p, dtype


def sample_uniforms(seed: int, draw: int, rows: int) -> np.ndarray:
    """u of rows 0 .. rows - 1 of call number `draw`: ((word 0 of the row's own block >> 8) + 0.5) * 2**-24, strictly inside (0, 1)"""
    w0 = words(seed, draw, 4 * rows).reshape(rows, 4)[:, 0]                 # row r: the block of counter r
    return ((w0 >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def sample_tokens(seed: int, draw: int, logits, temperature: float = 1.0, top_k: int = 0, top_p: float = 1.0) -> np.ndarray:
    """The definition of `Tensor.sample`, in float64: one token (int64) per row of `logits` (the last axis is the vocabulary,
    the leading axes are the rows) for call number `draw` of the stream - ONE call, whatever the shape.  Row r draws
    u = sample_uniforms(seed, draw, rows)[r].  For a row x with maximum m:
      * a degenerate row (a NaN, m == +inf or m == -inf) answers numpy's argmax (the first NaN, the lowest index);
      * top-k (1 <= top_k < V): K = {j : x_j >= the k-th largest value}, ties at the boundary kept; otherwise K is everything;
      * w_j = exp((x_j - m) * float32(1 / temperature)) on K, 0 elsewhere; W = sum w;
      * top-p (0 < top_p < 1): t = the largest value v occurring in K with sum{w_j : x_j >= v} >= top_p * W, N = {j in K : x_j >= t};
        otherwise N = K;
      * the token is the lowest i in N with sum{w_j : j in N, j <= i} >= u * W', W' = sum over N (if rounding leaves none: the
        highest index of N with w > 0).  A -inf logit has weight 0 and is never returned."""
    x = np.asarray(logits)
    temperature, top_k, top_p, _ = check_sample_arguments(x.dtype, x.shape[-1] if x.ndim else None, temperature, top_k, top_p, np.int64)
    lead, V = x.shape[:-1], x.shape[-1]
    x = x.reshape(-1, V).astype(np.float64)
    rows = x.shape[0]
    tokens = np.zeros(rows, np.int64)
    if rows == 0:
        return tokens.reshape(lead)
    u = sample_uniforms(seed, draw, rows)
    inv_t = np.float64(np.float32(1.0 / np.float64(temperature)))
    block = max(1, (1 << 21) // V)                                          # rows at a time: a bound on the temporaries
    for r0 in range(0, rows, block):
        xb, ub = x[r0:r0 + block], u[r0:r0 + block]
        nan = np.isnan(xb).any(axis=1)
        m = np.where(nan, np.nan, np.max(np.where(np.isnan(xb), 0.0, xb), axis=1))
        degenerate = nan | np.isinf(m)
        tok = np.argmax(xb, axis=1).astype(np.int64)                        # numpy's rules: what a degenerate row answers
        live = np.flatnonzero(~degenerate)
        if live.size:
            xl, ml = xb[live], m[live][:, None]
            if 1 <= top_k < V:
                keep = xl >= np.partition(xl, V - top_k, axis=1)[:, V - top_k][:, None]
            else:
                keep = np.ones(xl.shape, bool)
            w = np.where(keep, np.exp((xl - ml) * inv_t), 0.0)
            if 0.0 < top_p < 1.0:
                order = np.argsort(-xl, axis=1, kind="stable")
                xs, cs = np.take_along_axis(xl, order, axis=1), np.cumsum(np.take_along_axis(w, order, axis=1), axis=1)
                # the mass at or above a value: the running sum at the END of its run of equal values
                last = np.concatenate([xs[:, 1:] != xs[:, :-1], np.ones((xs.shape[0], 1), bool)], axis=1)
                ends = np.where(last, np.arange(V)[None, :], V)
                ends = np.minimum.accumulate(ends[:, ::-1], axis=1)[:, ::-1]
                mass = np.take_along_axis(cs, ends, axis=1)
                reached = (mass >= top_p * w.sum(axis=1)[:, None]) & np.take_along_axis(keep, order, axis=1)
                first = np.argmax(reached, axis=1)
                t = np.where(reached.any(axis=1), xs[np.arange(xs.shape[0]), first], -np.inf)
                keep &= xl >= t[:, None]
                w = np.where(keep, w, 0.0)
            c = np.cumsum(w, axis=1)
            hit = c >= (ub[live] * w.sum(axis=1))[:, None]
            hit &= w > 0.0
            highest = V - 1 - np.argmax((w > 0.0)[:, ::-1], axis=1)
            tok[live] = np.where(hit.any(axis=1), np.argmax(hit, axis=1), highest)
        tokens[r0:r0 + block] = tok
    return tokens.reshape(lead)


def check_probability(p) -> float:
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must satisfy 0 <= p < 1 (got %r)" % p)
    return p


class _CpuGenerator(object):
    seed, draws = 0, 0

    @classmethod
    def next_draw(cls) -> int:
        cls.draws += 1
        return cls.draws - 1


# the HIP generator lives in device memory (lg_init: seed 0, draws 0).  A seed set before the library is loaded - or on a machine
# without a GPU - waits here until the backend is first used.
_pending_hip_seed = None


def _apply_pending_hip_seed() -> None:
    """called by the HIP backend before it draws or reports its state"""
    global _pending_hip_seed
    if _pending_hip_seed is not None:
        from .autograd.hip import lib as _l
        seed, _pending_hip_seed = _pending_hip_seed, None
        _l.check(_l.lib().lg_rng_seed(seed))


def manual_seed(seed: int) -> None:
    """seed the generator of every backend and set its `draws` back to 0 (not inside a hipGraph capture: seed between replays)"""
    global _pending_hip_seed
    seed = int(seed)
    if not 0 <= seed < 1 << 64:
        raise ValueError("seed must fit 64 bits (got %r)" % seed)
    _CpuGenerator.seed, _CpuGenerator.draws = seed, 0
    from .autograd.hip import lib as _l
    _pending_hip_seed = seed
    if _l._lib is not None:                 # the library is initialised: a stream-ordered write, now
        _apply_pending_hip_seed()


def get_state(backend: str = "cpu") -> tuple:
    """(seed, draws) of a backend's generator; "hip" synchronises with the device"""
    if backend == "cpu":
        return _CpuGenerator.seed, _CpuGenerator.draws
    if backend == "hip":
        from .autograd.hip import lib as _l
        L = _l.lib()
        _apply_pending_hip_seed()
        seed, draws = ctypes.c_uint64(0), ctypes.c_uint64(0)
        _l.check(L.lg_rng_state(ctypes.byref(seed), ctypes.byref(draws)))
        return seed.value, draws.value
    raise ValueError("unknown backend %r (cpu, hip)" % (backend,))
