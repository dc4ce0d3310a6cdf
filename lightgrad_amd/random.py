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

`Tensor.sample_rows` (per-request sampling) takes NOTHING from the generator's state: every row names a row of a parameter table
(`sampling_table`: temperature, top-k, top-p and a 64-bit seed of its own) and a counter g, and draws
u = sample_uniforms(seed, 0, g + 1)[g] - the g-th number of a stream that belongs to the request alone.  `sample_tokens_rows` is
the definition and the numpy backend; csrc/sample_rows.hip evaluates it with the row body of csrc/sample.hip.

`Tensor.penalize_rows` (per-request repetition, presence and frequency penalties, a minimum of new tokens) draws nothing: it
rewrites the logits at the ids of a request's own history in front of the draw.  `penalty_table` lays the parameters out,
`penalize_logits` is the definition and the numpy backend; csrc/penalize.hip evaluates it in float32 bit for bit.

`Tensor.logprob_rows` (per-token log-probabilities and the top-n alternatives) draws nothing either: behind the draw it scores
the token against the logits the draw read.  `token_logprobs_rows` is the definition, in float64, and the numpy backend;
csrc/logprob.hip evaluates it in float32 with the sum of exponentials held as integers.

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


def _sample_block(xb, ub, inv_t, top_k: int, top_p: float) -> np.ndarray:
    """the tokens (int64) of the float64 rows `xb` (rows, V) for the uniform numbers `ub` (rows,): the steps of `sample_tokens`"""
    V = xb.shape[1]
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
    return tok


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
        tokens[r0:r0 + block] = _sample_block(x[r0:r0 + block], u[r0:r0 + block], inv_t, top_k, top_p)
    return tokens.reshape(lead)


SAMPLING_WORDS = 8


def sampling_table(temperature=1.0, top_k=0, top_p=1.0, seeds=0) -> np.ndarray:
    """The parameter table of `Tensor.sample_rows`: int32 (n, 8), one row per request.  Each argument is a scalar or a sequence
    of n; scalars broadcast (all scalars: n = 1).  Row i holds
        word 0      the bits of inv_T = float32(1 / float64(temperature_i)); +0.0 - temperature 0 - means GREEDY
        word 1      top_k
        words 2, 3  the low and high half of the bits of top_p as a float64
        words 4, 5  the low and high half of the 64-bit seed
        words 6, 7  0
    Every entry passes `check_sample_arguments`, except that a temperature of 0 is allowed; a seed must fit 64 bits and top_k 31."""
    columns = [np.atleast_1d(np.asarray(c, dtype=object)) for c in (temperature, top_k, top_p, seeds)]
    if any(c.ndim != 1 for c in columns):
        raise ValueError("sampling_table: temperature, top_k, top_p and seeds are scalars or sequences")
    n = max(c.size for c in columns)
    if n < 1 or any(c.size not in (1, n) for c in columns):
        raise ValueError("sampling_table: sequences of one length >= 1 (got %s)" % [c.size for c in columns])
    table = np.zeros((n, SAMPLING_WORDS), np.uint32)
    for i in range(n):
        t, k, p, s = (c[i if c.size == n else 0] for c in columns)
        t = float(t)
        if t == 0.0 and not np.signbit(t):
            _, k, p, _ = check_sample_arguments(np.float32, 1, 1.0, k, p, np.int32)
            inv_t = np.float32(0.0)
        else:
            t, k, p, _ = check_sample_arguments(np.float32, 1, t, k, p, np.int32)
            inv_t = np.float32(1.0 / np.float64(t))
        s = int(s)
        if not 0 <= s < 1 << 64:
            raise ValueError("sampling_table: a seed must fit 64 bits (got %r)" % s)
        if k >= 1 << 31:
            raise ValueError("sampling_table: top_k must fit an int32 (got %r)" % k)
        p_bits = int(np.float64(p).view(np.uint64))
        table[i] = (int(inv_t.view(np.uint32)), k, p_bits & 0xFFFFFFFF, p_bits >> 32, s & 0xFFFFFFFF, s >> 32, 0, 0)
    return table.view(np.int32)


def check_sample_rows_operands(logits, table, index, counter, dtype):
    """the validated token dtype of a `sample_rows` call; the operands are tensors of either backend (shapes and dtypes only)"""
    shape, i32 = tuple(logits.shape), np.dtype(np.int32)
    if not np.issubdtype(np.dtype(logits.dtype), np.floating):
        raise ValueError("sample_rows: the logits must be floating point (got %s)" % np.dtype(logits.dtype))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[1] == 1)) or shape[-1] < 1:
        raise ValueError("sample_rows: the logits are (rows, V) or (rows, 1, V) with V >= 1 (got %s)" % (shape,))
    for name, t in (("table", table), ("index", index), ("counter", counter)):
        if np.dtype(t.dtype) != i32:
            raise ValueError("sample_rows: %s must be int32 (got %s)" % (name, np.dtype(t.dtype)))
    if len(table.shape) != 2 or table.shape[1] != SAMPLING_WORDS or table.shape[0] < 1:
        raise ValueError("sample_rows: the table is (n, %d) with n >= 1, as sampling_table lays it out (got %s)" % (SAMPLING_WORDS, tuple(table.shape)))
    if tuple(index.shape) != (shape[0],) or tuple(counter.shape) != (table.shape[0],):
        raise ValueError("sample_rows: index is (rows,) = (%d,) and counter (n,) = (%d,) (got %s and %s)" % (
            shape[0], table.shape[0], tuple(index.shape), tuple(counter.shape)))
    dtype = np.dtype(dtype)
    if dtype not in (i32, np.dtype(np.int64)):
        raise ValueError("sample_rows: the tokens are int32 or int64 (got %s)" % dtype)
    return dtype


def sample_tokens_rows(logits, table, index, counter):
    """The definition of `Tensor.sample_rows`, in float64: (tokens (rows,) int64, bad (rows,) bool).  logits (rows, V); table
    int32 (n, 8) as `sampling_table` lays it out; index (rows,): row r uses table row i = index[r]; counter (n,): g = counter[i].
    Per row, in this order:
      1. i < 0 (a free slot): the token is 0 and the row's logits are not read (they may hold NaN);
      2. the row is BAD if i >= n, g < 0, top_k < 0, top_p is not in (0, 1], or inv_T has its sign set, is NaN or infinite: the
         token is 0 and bad[r] is set; the other rows are computed;
      3. inv_T == +0.0 is GREEDY: numpy's argmax of the row (the first NaN, the lowest index);
      4. otherwise the token is that of `sample_tokens` for the row under (inv_T, top_k, top_p) with
         u = sample_uniforms(seed, 0, g + 1)[g]: the g-th number of a stream of the request's own."""
    x = np.asarray(logits)
    table = np.ascontiguousarray(table, np.int32)
    index, counter = np.asarray(index, np.int64).reshape(-1), np.asarray(counter, np.int64).reshape(-1)
    if x.ndim != 2 or table.ndim != 2 or table.shape[1] != SAMPLING_WORDS or index.shape != (x.shape[0],) or counter.shape != (table.shape[0],):
        raise ValueError("sample_tokens_rows: logits (rows, V), table (n, 8), index (rows,), counter (n,), got %s %s %s %s" % (
            x.shape, table.shape, index.shape, counter.shape))
    rows, n = x.shape[0], table.shape[0]
    words = table.view(np.uint32)
    tokens, bad = np.zeros(rows, np.int64), np.zeros(rows, bool)
    for r in range(rows):
        i = int(index[r])
        if i < 0:
            continue
        if i >= n:
            bad[r] = True
            continue
        g, top_k = int(counter[i]), int(table[i, 1])
        inv_t = words[i, 0:1].view(np.float32)[0]
        top_p = float(np.array([int(words[i, 2]) | (int(words[i, 3]) << 32)], np.uint64).view(np.float64)[0])
        seed = int(words[i, 4]) | (int(words[i, 5]) << 32)
        if g < 0 or top_k < 0 or not 0.0 < top_p <= 1.0 or np.signbit(inv_t) or not np.isfinite(inv_t):
            bad[r] = True
            continue
        if inv_t == 0.0:
            tokens[r] = int(np.argmax(x[r]))
            continue
        tokens[r] = _sample_block(x[r:r + 1].astype(np.float64), np.array([_row_uniform(seed, g)]), np.float64(inv_t), top_k, top_p)[0]
    return tokens, bad


def _row_uniform(seed: int, g: int) -> float:
    """sample_uniforms(seed, 0, g + 1)[g] without the g numbers in front of it"""
    w0 = philox4x32_10((g & 0xFFFFFFFF, (g >> 32) & 0xFFFFFFFF, 0, 0), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))[..., 0]
    return float(((np.uint32(w0) >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24)


PENALTY_WORDS = 4
PENALTY_MAX_HISTORY = 4096                                # P + G: what csrc/penalize.hip keeps in LDS (speculate.hip's bound for a sequence)


def penalty_table(repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, min_new_tokens=0) -> np.ndarray:
    """The parameter table of `Tensor.penalize_rows`: int32 (n, 4), one row per request.  Each argument is a scalar or a sequence
    of n; scalars broadcast (all scalars: n = 1).  Row i holds
        word 0  the bits of rho = float32(repetition_penalty_i)       word 1  the bits of alpha = float32(presence_penalty_i)
        word 2  the bits of beta = float32(frequency_penalty_i)       word 3  min_new_tokens_i
    The float32 value IS the parameter: rho must be finite and > 0, alpha and beta finite, 0 <= min_new_tokens < 2**31."""
    columns = [np.atleast_1d(np.asarray(c, dtype=object)) for c in (repetition_penalty, presence_penalty, frequency_penalty, min_new_tokens)]
    if any(c.ndim != 1 for c in columns):
        raise ValueError("penalty_table: the penalties and min_new_tokens are scalars or sequences")
    n = max(c.size for c in columns)
    if n < 1 or any(c.size not in (1, n) for c in columns):
        raise ValueError("penalty_table: sequences of one length >= 1 (got %s)" % [c.size for c in columns])
    table = np.zeros((n, PENALTY_WORDS), np.uint32)
    for i in range(n):
        rho, alpha, beta, m = (c[i if c.size == n else 0] for c in columns)
        with np.errstate(over="ignore"):
            rho, alpha, beta = np.float32(float(rho)), np.float32(float(alpha)), np.float32(float(beta))
        if not (np.isfinite(rho) and rho > 0):
            raise ValueError("penalty_table: repetition_penalty must be finite and > 0 as a float32 (got %r)" % (rho,))
        if not (np.isfinite(alpha) and np.isfinite(beta)):
            raise ValueError("penalty_table: presence_penalty and frequency_penalty must be finite as float32 (got %r, %r)" % (alpha, beta))
        if int(m) != m or not 0 <= int(m) < 1 << 31:
            raise ValueError("penalty_table: min_new_tokens must be an int in [0, 2**31) (got %r)" % (m,))
        table[i] = (int(rho.view(np.uint32)), int(alpha.view(np.uint32)), int(beta.view(np.uint32)), int(m))
    return table.view(np.int32)


def check_penalize_operands(logits, table, index, prompts, prompt_len, out, out_len, eos):
    """the validated (rows, V, eos or -1) of a `penalize_rows` call; the operands are tensors of either backend (shapes and dtypes
    only)"""
    shape, i32 = tuple(logits.shape), np.dtype(np.int32)
    if not np.issubdtype(np.dtype(logits.dtype), np.floating):
        raise ValueError("penalize_rows: the logits must be floating point (got %s)" % np.dtype(logits.dtype))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[1] == 1)) or shape[-1] < 1:
        raise ValueError("penalize_rows: the logits are (rows, V) or (rows, 1, V) with V >= 1 (got %s)" % (shape,))
    operands = (("table", table), ("index", index), ("prompts", prompts), ("prompt_len", prompt_len), ("out", out), ("out_len", out_len))
    for name, t in operands:
        if np.dtype(t.dtype) != i32:
            raise ValueError("penalize_rows: %s must be int32 (got %s)" % (name, np.dtype(t.dtype)))
    n = table.shape[0] if len(table.shape) == 2 else 0
    if n < 1 or table.shape[1] != PENALTY_WORDS:
        raise ValueError("penalize_rows: the table is (n, %d) with n >= 1, as penalty_table lays it out (got %s)" % (PENALTY_WORDS, tuple(table.shape)))
    if tuple(index.shape) != (shape[0],) or tuple(prompt_len.shape) != (n,) or tuple(out_len.shape) != (n,) or len(prompts.shape) != 2 or \
            len(out.shape) != 2 or prompts.shape[0] != n or out.shape[0] != n or prompts.shape[1] < 1 or out.shape[1] < 1:
        raise ValueError("penalize_rows: index (rows,) = (%d,), prompts (n, P), out (n, G), prompt_len and out_len (n,) with n = %d, P, G >= 1 (got %s)" % (
            shape[0], n, [tuple(t.shape) for _, t in operands[1:]]))
    assert prompts.shape[1] + out.shape[1] <= PENALTY_MAX_HISTORY, \
        "penalize_rows: a history of P + G = %d + %d ids exceeds the %d the launch keeps in LDS" % (prompts.shape[1], out.shape[1], PENALTY_MAX_HISTORY)
    if eos is not None and (int(eos) != eos or not 0 <= int(eos) < shape[-1]):
        raise ValueError("penalize_rows: eos is None or an id in 0 .. V - 1 = %d (got %r)" % (shape[-1] - 1, eos))
    return shape[0], shape[-1], -1 if eos is None else int(eos)


def penalize_logits(logits, table, index, prompts, prompt_len, out, out_len, eos=None):
    """The definition of `Tensor.penalize_rows`: (y (rows, V), bad (rows,) bool).  logits (rows, V) float32 or float64; table int32
    (n, 4) as `penalty_table` lays it out (rho, alpha, beta, min_new); index (rows,): row r uses request i = index[r]; prompts
    (n, P), prompt_len (n,), out (n, G), out_len (n,): the request's history; eos: None or an id in 0 .. V - 1.  Float32 logits are
    computed in float32, every operation rounded once and in this order; float64 logits by the same expressions in float64 with
    the float32 parameters widened.  Per row:
      1. i < 0 (a free slot): the row comes back as it is; its logits are not read (they may hold NaN);
      2. with len = prompt_len[i], g = out_len[i], the row is BAD if i >= n, len is outside 0 .. P, g is outside 0 .. G, rho is
         not finite, <= 0 or has its sign set, alpha or beta is not finite, min_new < 0, or any of prompts[i, :len], out[i, :g]
         lies outside 0 .. V - 1: it comes back bit for bit and bad[r] is set; the other rows are computed.  Words behind len and
         g are never read;
      3. for every id v that occurs in prompts[i, :len] or out[i, :g], once however often: x = x * rho if x < 0 else x / rho (a NaN
         stays one, -0.0 takes the division, an infinity stays itself);
      4. for every v that occurs c_v > 0 times in out[i, :g]: x = (x - beta * c_v) - alpha (one product, two subtractions);
      5. if eos is given and g < min_new: y[eos] = -inf, whatever steps 3 and 4 left there."""
    x = np.asarray(logits)
    if x.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise ValueError("penalize_logits: float32 or float64 logits (got %s)" % x.dtype)
    table = np.ascontiguousarray(table, np.int32)
    index, prompt_len, out_len = (np.asarray(a, np.int64).reshape(-1) for a in (index, prompt_len, out_len))
    prompts, out = np.asarray(prompts), np.asarray(out)
    if x.ndim != 2 or x.shape[1] < 1 or table.ndim != 2 or table.shape[1] != PENALTY_WORDS or prompts.ndim != 2 or out.ndim != 2 or \
            index.shape != (x.shape[0],) or not (prompts.shape[0] == out.shape[0] == prompt_len.size == out_len.size == table.shape[0]):
        raise ValueError("penalize_logits: logits (rows, V), table (n, 4), index (rows,), prompts (n, P), prompt_len (n,), out (n, G), out_len (n,), got %s" % (
            [a.shape for a in (x, table, index, prompts, prompt_len, out, out_len)],))
    (rows, V), n, P, G = x.shape, table.shape[0], prompts.shape[1], out.shape[1]
    if eos is not None and (int(eos) != eos or not 0 <= int(eos) < V):
        raise ValueError("penalize_logits: eos is None or an id in 0 .. V - 1 = %d (got %r)" % (V - 1, eos))
    real = x.dtype.type
    parameters = table.view(np.float32)
    y, bad = x.copy(), np.zeros(rows, bool)
    for r in range(rows):
        i = int(index[r])
        if i < 0:
            continue
        if i >= n:
            bad[r] = True
            continue
        length, g = int(prompt_len[i]), int(out_len[i])
        rho, alpha, beta, min_new = parameters[i, 0], parameters[i, 1], parameters[i, 2], int(table[i, 3])
        if not (0 <= length <= P and 0 <= g <= G and np.isfinite(rho) and rho > 0 and np.isfinite(alpha) and np.isfinite(beta) and min_new >= 0):
            bad[r] = True
            continue
        drawn = np.asarray(out[i, :g], np.int64)
        history = np.concatenate([np.asarray(prompts[i, :length], np.int64), drawn])
        if history.size and (history.min() < 0 or history.max() >= V):
            bad[r] = True
            continue
        with np.errstate(all="ignore"):
            seen = np.unique(history)
            v = y[r, seen]
            y[r, seen] = np.where(v < 0, v * real(rho), v / real(rho))
            counted, counts = np.unique(drawn, return_counts=True)
            y[r, counted] = (y[r, counted] - real(beta) * counts.astype(x.dtype)) - real(alpha)
        if eos is not None and g < min_new:
            y[r, int(eos)] = -np.inf
    return y, bad


LOGPROB_MAX_TOP = 8                                      # n_max: the alternatives a thread of csrc/logprob.hip keeps in registers
LOGPROB_LDS_COLS = 36864                                 # rows of up to this many floats are staged in LDS by csrc/logprob.hip


def logprob_want(logprobs, n: int) -> np.ndarray:
    """`want` (n,) int32 of `Tensor.logprob_rows` from what `serve(logprobs=)` takes: an int 0 .. 8 for every request, or one entry
    per request - None or -1: no log-probabilities for it, 0: the chosen token's only, k in 1 .. 8: also the k most likely ids."""
    entries = [logprobs] * n if logprobs is None or np.ndim(logprobs) == 0 else list(logprobs)
    if len(entries) != n:
        raise ValueError("logprobs: an int or one entry per request (%d), got %d" % (n, len(entries)))
    want = np.zeros(n, np.int32)
    for i, k in enumerate(entries):
        k = -1 if k is None else k
        if int(k) != k or not -1 <= int(k) <= LOGPROB_MAX_TOP:
            raise ValueError("logprobs: every entry is None, -1 or an int in 0 .. %d (got %r)" % (LOGPROB_MAX_TOP, k))
        want[i] = int(k)
    return want


def check_logprob_operands(logits, token, want, index, counter, logprob, top_ids, top_logprob):
    """the validated (rows, V, N, G, n_max) of a `logprob_rows` call; the operands are tensors of either backend (shapes and dtypes
    only)"""
    shape, i32, f32 = tuple(logits.shape), np.dtype(np.int32), np.dtype(np.float32)
    if not np.issubdtype(np.dtype(logits.dtype), np.floating):
        raise ValueError("logprob_rows: the logits must be floating point (got %s)" % np.dtype(logits.dtype))
    if not (len(shape) == 2 or (len(shape) == 3 and shape[1] == 1)) or shape[-1] < 1:
        raise ValueError("logprob_rows: the logits are (rows, V) or (rows, 1, V) with V >= 1 (got %s)" % (shape,))
    for name, t in (("token", token), ("want", want), ("index", index), ("counter", counter), ("top_ids", top_ids)):
        if np.dtype(t.dtype) != i32:
            raise ValueError("logprob_rows: %s must be int32 (got %s)" % (name, np.dtype(t.dtype)))
    for name, t in (("logprob", logprob), ("top_logprob", top_logprob)):
        if np.dtype(t.dtype) != f32:
            raise ValueError("logprob_rows: %s must be float32 (got %s)" % (name, np.dtype(t.dtype)))
    rows = shape[0]
    if tuple(token.shape) not in ((rows,), (rows, 1)) or tuple(index.shape) != (rows,):
        raise ValueError("logprob_rows: token is (rows,) or (rows, 1) and index (rows,) with rows = %d (got %s and %s)" % (
            rows, tuple(token.shape), tuple(index.shape)))
    if len(want.shape) != 1 or want.shape[0] < 1 or tuple(counter.shape) != tuple(want.shape):
        raise ValueError("logprob_rows: want and counter are (N,) with N >= 1 (got %s and %s)" % (tuple(want.shape), tuple(counter.shape)))
    N = want.shape[0]
    if len(logprob.shape) != 2 or logprob.shape[0] != N or logprob.shape[1] < 1 or len(top_ids.shape) != 3 or tuple(top_ids.shape[:2]) != tuple(logprob.shape) or \
            not 1 <= top_ids.shape[2] <= LOGPROB_MAX_TOP or tuple(top_logprob.shape) != tuple(top_ids.shape):
        raise ValueError("logprob_rows: logprob (N, G), top_ids and top_logprob (N, G, n) with N = %d, G >= 1 and n in 1 .. %d (got %s, %s and %s)" % (
            N, LOGPROB_MAX_TOP, tuple(logprob.shape), tuple(top_ids.shape), tuple(top_logprob.shape)))
    return rows, shape[-1], N, logprob.shape[1], top_ids.shape[2]


def token_logprobs_rows(logits, token, want, index, counter, logprob, top_ids, top_logprob):
    """The definition of `Tensor.logprob_rows`, in float64: writes `logprob` (N, G), `top_ids` (N, G, n_max) and `top_logprob`
    (N, G, n_max) IN PLACE (numpy arrays; float32 in a pool, any float type here) and returns bad (rows,) bool.  logits (rows, V)
    float32 or float64 - the logits the draw reads: behind `penalize_rows`, in front of temperature, top-k and top-p; token (rows,)
    the id just drawn; want (N,) per request: -1 = nothing, 0 = the chosen token's log-probability only, k in 1 .. n_max <= 8 =
    also the k most likely ids; index (rows,): row r belongs to request i = index[r], -1 = a free row; counter (N,): the column
    g = counter[i].  Per row, in this order:
      1. i < 0 or (i < N and want[i] == -1): nothing is written and the row's logits are not read (they may hold NaN);
      2. the row is BAD if i >= N, g < 0 or g >= G, want[i] is outside -1 .. n_max, or the token is outside 0 .. V - 1: nothing
         is written and bad[r] is set; the other rows are computed;
      3. with m = max x and L = m + log(sum_j exp(x_j - m)): logprob[i, g] = x_token - L, and for k = want[i], k' = min(k, V):
         top_ids[i, g, :k'] = np.argsort(-x, kind="stable")[:k'] - descending value, equal values (-0.0 == +0.0) to the lower
         index - and top_logprob[i, g, :k'] their x_j - L; the entries k' .. n_max - 1 keep what they hold.  A -inf logit has the
         log-probability -inf;
      4. a DEGENERATE row - a NaN in it, or m infinite - writes NaN to logprob[i, g], -1 to top_ids[i, g, :k] and NaN to
         top_logprob[i, g, :k].
    The fills a pool starts from: +0.0 in logprob and top_logprob, -1 in top_ids."""
    x = np.asarray(logits)
    token, index, want, counter = (np.asarray(a, np.int64).reshape(-1) for a in (token, index, want, counter))
    if x.ndim != 2 or x.shape[1] < 1 or token.shape != (x.shape[0],) or index.shape != (x.shape[0],) or want.size < 1 or counter.shape != want.shape or \
            logprob.ndim != 2 or logprob.shape[0] != want.size or top_ids.ndim != 3 or top_ids.shape[:2] != logprob.shape or top_logprob.shape != top_ids.shape or \
            not 1 <= top_ids.shape[2] <= LOGPROB_MAX_TOP:
        raise ValueError("token_logprobs_rows: logits (rows, V), token (rows,), want (N,), index (rows,), counter (N,), logprob (N, G), top_ids and "
                         "top_logprob (N, G, n <= %d), got %s" % (LOGPROB_MAX_TOP, [np.shape(a) for a in (x, token, want, index, counter, logprob, top_ids, top_logprob)]))
    (rows, V), N, G, n_max = x.shape, want.size, logprob.shape[1], top_ids.shape[2]
    bad = np.zeros(rows, bool)
    for r in range(rows):
        i = int(index[r])
        if i < 0:
            continue
        if i >= N:
            bad[r] = True
            continue
        k, g, t = int(want[i]), int(counter[i]), int(token[r])
        if k == -1:
            continue
        if not (0 <= k <= n_max and 0 <= g < G and 0 <= t < V):
            bad[r] = True
            continue
        row = x[r].astype(np.float64)
        m = row.max()                                    # (a NaN in the row makes it NaN)
        if not np.isfinite(m):
            logprob[i, g], top_ids[i, g, :k], top_logprob[i, g, :k] = np.nan, -1, np.nan
            continue
        with np.errstate(divide="ignore"):
            L = m + np.log(np.exp(row - m).sum())
        logprob[i, g] = row[t] - L
        best = np.argsort(-row, kind="stable")[:min(k, V)]
        top_ids[i, g, :best.size], top_logprob[i, g, :best.size] = best, row[best] - L
    return bad


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
