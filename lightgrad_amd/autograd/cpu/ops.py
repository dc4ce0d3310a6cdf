"""First-class ops of the numpy backend.

Restates the arithmetic of the reference's `lightgrad/autograd/cpu/ops.py`
(op by op; line numbers in each docstring) so that `CpuTensor` here produces
the same numbers as the reference's CPU backend on the same inputs - it is
pinned against fixtures generated from the reference (tests/golden/).

Two gaps of the reference's CPU backend are closed here, following its OpenCL
backend as SURVEY.md §8c prescribes:
  * `sum.backward` (reference cpu/ops.py:293 is a TODO) = broadcast of the
    gradient to the input shape                       (opencl/ops.py:353-368)
  * `dot.backward` for batched operands swaps the last two axes instead of
    reversing all axes                                (opencl/ops.py:127-132)
`conv` (cpu/ops.py:298-356) is restated at the end of this file for the CNN example (SURVEY.md §8f row 4 tail).
"""
import numpy as np
from ..func import Function
from ..dropout import DropoutFunction
from ... import random as _random
from ... import guide as _guide
from .tensor import CpuTensor


def _raw(x):
    return x.data if isinstance(x, CpuTensor) else x


def _numpy_op(fn_cls):
    """Let an op be written on ndarrays: unwrap tensor arguments, wrap results
    (reference helper `_use_tensor_data`, cpu/ops.py:8-21)."""

    class Op(fn_cls):
        def forward(ctx, *args, **kwargs):
            out = fn_cls.forward(ctx, *[_raw(a) for a in args], **{k: _raw(v) for k, v in kwargs.items()})
            return CpuTensor(data=out, dtype=out.dtype)

        def backward(ctx, out_grad):
            grads = fn_cls.backward(ctx, out_grad.data)
            grads = grads if isinstance(grads, tuple) else (grads,)
            return tuple(CpuTensor(data=g, dtype=g.dtype) for g in grads)

    Op.__name__ = fn_cls.__name__
    Op.__qualname__ = fn_cls.__qualname__
    Op.__doc__ = fn_cls.__doc__
    return Op


def _op(*names, overwrite=False):
    def deco(fn_cls):
        op = _numpy_op(fn_cls)
        for n in (names or (fn_cls.__name__,)):
            CpuTensor.register_op(n, op, overwrite=overwrite)
        return op
    return deco


""" Transformations """


@_op("astype")
class astype(Function):
    """ t.astype(dtype) - not an op of the reference (its tensors change dtype through numpy on the host, cpu/tensor.py:12);
    here so that code written for HipTensor.astype runs on the CPU backend too.  Differentiable between float dtypes. """
    def forward(ctx, a, dtype=np.float32):
        ctx.save_for_backward(a.dtype, np.dtype(dtype))
        return a.astype(dtype)

    def backward(ctx, out_grad):
        src, dst = ctx.get_saved_tensors()
        if src.kind != "f" or dst.kind != "f":
            raise RuntimeError("Cannot Backward through astype(%s -> %s)!" % (src, dst))
        return out_grad.astype(src)


@_op("T", "transpose")
class transpose(Function):
    """ axis permutation view; backward = inverse permutation (cpu/ops.py:25-36) """
    def forward(ctx, a, *axes):
        ctx.save_for_backward(axes)
        return np.transpose(a, axes=(axes if len(axes) > 0 else None))

    def backward(ctx, out_grad):
        axes, = ctx.get_saved_tensors()
        if len(axes) == 0:
            return out_grad.transpose()
        inverse = [0] * len(axes)
        for i, j in enumerate(axes):
            inverse[j] = i
        return out_grad.transpose(*inverse)


@_op()
class reshape(Function):
    """ cpu/ops.py:38-47 """
    def forward(ctx, a, *shape):
        ctx.save_for_backward(a.shape)
        return a.reshape(shape)

    def backward(ctx, out_grad):
        shape, = ctx.get_saved_tensors()
        return out_grad.reshape(shape)


""" Element-wise arithmetic, matrix product, non-linearities

One table instead of one class per op: each row gives the value and the gradients as plain numpy expressions - the
reference's own (cpu/ops.py:52-116, :158-229; operand order kept, so results are its bits) - and says what the backward needs
kept.  `_formula_op` turns a row into a tape node. """

_KEEP_NOTHING, _KEEP_INPUTS, _KEEP_OUTPUT, _KEEP_BOTH = range(4)


def _formula_op(name, value, gradients, keep, aliases=(), overwrite=False, cite=""):
    def forward(ctx, *inputs):
        y = value(*inputs)
        if keep == _KEEP_INPUTS:
            ctx.save_for_backward(*inputs)
        elif keep == _KEEP_OUTPUT:
            ctx.save_for_backward(y)
        elif keep == _KEEP_BOTH:
            ctx.save_for_backward(*(inputs + (y,)))
        return y

    def backward(ctx, out_grad):
        return gradients(out_grad, *ctx.get_saved_tensors())

    node = type(name, (Function,), {"forward": forward, "backward": backward, "__doc__": cite})
    return _op(*((name,) + tuple(aliases)), overwrite=overwrite)(node)


def _last_two_swapped(m):
    return np.swapaxes(m, -1, -2)


def _pow_gradients(g, a, b, y):
    # the exponent's gradient is always formed (NaN for a < 0, as in the reference, cpu/ops.py:101-105)
    with np.errstate(invalid='ignore', divide='ignore'):
        return b * (a ** (b - 1)) * g, g * y * np.log(a)


_FORMULAS = [
    # name        value                                  gradients(g, *kept)                                   kept            extra
    ("neg",       lambda a: -a,                          lambda g: -g,                                          _KEEP_NOTHING,  {}),
    ("add",       lambda a, b: a + b,                    lambda g: (g, g),                                      _KEEP_NOTHING,  {}),
    ("sub",       lambda a, b: a - b,                    lambda g: (g, -g),                                     _KEEP_NOTHING,  {"overwrite": True}),
    ("mul",       lambda a, b: a * b,                    lambda g, a, b: (g * b, a * g),                        _KEEP_INPUTS,   {}),
    ("div",       lambda a, b: a / b,                    lambda g, a, b: (g / b, -a / b**2 * g),                _KEEP_INPUTS,   {"overwrite": True}),
    ("pow",       lambda a, b: a ** b,                   _pow_gradients,                                        _KEEP_BOTH,     {}),
    # a @ b; the backward swaps the last two axes so that it is also right for batched operands (opencl/ops.py:127-132)
    ("dot",       lambda a, b: a @ b,                    lambda g, a, b: (g @ _last_two_swapped(b), _last_two_swapped(a) @ g),
                                                                                                                _KEEP_INPUTS,   {"aliases": ("__matmul__",)}),
    ("sin",       np.sin,                                lambda g, t: np.cos(t) * g,                            _KEEP_INPUTS,   {}),
    ("cos",       np.cos,                                lambda g, t: -np.sin(t) * g,                           _KEEP_INPUTS,   {}),
    ("exp",       np.exp,                                lambda g, y: y * g,                                    _KEEP_OUTPUT,   {}),
    ("log",       np.log,                                lambda g, x: (1 / x) * g,                              _KEEP_INPUTS,   {}),
    ("sigmoid",   lambda t: 1 / (1 + np.exp(-t)),        lambda g, y: y * (1 - y) * g,                          _KEEP_OUTPUT,   {"overwrite": True}),
    ("tanh",      np.tanh,                               lambda g, y: (1 - y**2) * g,                           _KEEP_OUTPUT,   {"overwrite": True}),
    # the gradient passes at exactly 0 (cpu/ops.py:221-229)
    ("relu",      lambda t: np.maximum(t, 0.0),          lambda g, t: g * (t >= 0),                             _KEEP_INPUTS,   {}),
]
for _name, _value, _gradients, _keep, _extra in _FORMULAS:
    globals()[_name] = _formula_op(_name, _value, _gradients, _keep, cite="reference cpu/ops.py, op `%s`" % _name, **_extra)


""" Products with bfloat16 operands (not ops of the reference): fp32 tensors, both operands of a product rounded to bfloat16
on their way into it, the sum formed in fp32 - what `lg_gemm_bf16_f32` computes on the bf16 matrix cores (DESIGN.md) """


def bf16_round_array(x):
    """r(x): every value rounded to bfloat16 (8-bit significand; nearest, ties to even) and kept in x's own float dtype.  NaN
    stays NaN, +-Inf and the sign of zero are kept, a finite value beyond the largest bfloat16 becomes +-Inf.  THE definition
    of the rounding for both backends; subnormal fp32 inputs are unspecified (the matrix cores may flush them).  A float64
    array (the float64 run of a float32 tape) is rounded to float32 first and comes back as float64."""
    x = np.asarray(x)
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) & np.uint32(0xFFFF0000)).view(np.float32)
    return np.where(np.isnan(f), f, r).astype(x.dtype if x.dtype.kind == "f" else np.float32)


def bf16_bits(x):
    """bits(x): the upper 16 bits of r(x) = `bf16_round_array`(x) as int16 - the word a bfloat16 key / value cache stores.  A NaN
    stores (u >> 16) | 0x0040: a NaN whatever its low half held.  A float64 array goes through float32, as in r."""
    f = np.ascontiguousarray(np.asarray(x), dtype=np.float32)
    u = f.view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    return np.where(np.isnan(f), (u >> np.uint32(16)) | np.uint32(0x0040), r).astype(np.uint16).view(np.int16)


def bf16_widen(w):
    """widen(w): the float32 whose upper 16 bits are the int16 word w and whose lower 16 are 0 - what a word of a bfloat16 cache
    stands for.  widen(bits(x)) == r(x) bit for bit for every x that is no NaN."""
    w = np.ascontiguousarray(np.asarray(w))
    assert w.dtype == np.int16, "bf16_widen takes int16 words, got %s" % w.dtype
    return (w.view(np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def _require_bf16_operands(name, *operands):
    for t in operands:
        if t is not None and t.dtype != np.float32 and not (t.dtype == np.float64 and CpuTensor.default_dtype == np.float64):
            raise TypeError("%s is float32-only (got %s)" % (name, t.dtype))


def _require_matrix_ranks(name, a, b):
    if a.ndim < 2 or b.ndim != 2:
        raise ValueError("%s: (M, K) @ (K, N) or (..., M, K) @ (K, N) only (got %s and %s)" % (name, a.shape, b.shape))


@_op()
class dot_bf16(Function):
    """ a.dot_bf16(b) = r(a) @ r(b), r = `bf16_round_array`: (M, K) @ (K, N), or (..., M, K) @ (K, N) as one tall product.
    backward: dA = r(g) @ r(b)^T, dB = r(a)^T @ r(g) - every operand, the gradient included, is rounded again. """
    def forward(ctx, a, b):
        _require_bf16_operands("dot_bf16", a, b)
        _require_matrix_ranks("dot_bf16", a, b)
        ra, rb = bf16_round_array(a), bf16_round_array(b)
        ctx.save_for_backward(ra, rb)
        return ra @ rb

    def backward(ctx, out_grad):
        ra, rb = ctx.get_saved_tensors()
        rg = bf16_round_array(out_grad)
        return rg @ rb.T, ra.reshape(-1, ra.shape[-1]).T @ rg.reshape(-1, rg.shape[-1])


@_op()
class linear_bf16(Function):
    """ x.linear_bf16(weight, bias=None) = r(x) @ r(weight)^T + bias, weight as nn.Linear holds it ((out, in)); the sum is
    rounded to fp32 before the bias is added.  backward: dx = r(g) @ r(W), dW = r(g)^T @ r(x), db = column sums of the
    (unrounded) g. """
    def forward(ctx, x, weight, bias=None):
        _require_bf16_operands("linear_bf16", x, weight, bias)
        _require_matrix_ranks("linear_bf16", x, weight)
        rx, rw = bf16_round_array(x), bf16_round_array(weight)
        ctx.save_for_backward(rx, rw, bias is not None)
        y = rx @ rw.T
        return y if bias is None else y + bias

    def backward(ctx, out_grad):
        rx, rw, has_bias = ctx.get_saved_tensors()
        g2 = out_grad.reshape(-1, rw.shape[0])
        rg = bf16_round_array(g2)
        dx, dw = (rg @ rw).reshape(rx.shape), rg.T @ rx.reshape(-1, rx.shape[-1])
        return (dx, dw, g2.sum(axis=0)) if has_bias else (dx, dw)


def _bf16_round(t):
    """ t.bf16_round() (also `lightgrad_amd.bf16_round(t)`): r(t) as a new tensor, a constant of the tape (no gradient) """
    return CpuTensor.from_numpy(bf16_round_array(t.data), requires_grad=False)


CpuTensor.bf16_round = _bf16_round


""" In-place operators and fill: no backward, the result IS the input's storage (cpu/ops.py:120-153) """


def _in_place_op(name, apply, registered_as=None):
    def forward(ctx, t, other):
        apply(t, other)
        return t
    node = type(name, (Function,), {"forward": forward})          # the class name shows in "Cannot Backward through <name>!"
    return _op(registered_as or name, overwrite=True)(node)


iadd = _in_place_op("iadd", lambda t, other: t.__iadd__(other), "__iadd__")
isub = _in_place_op("isub", lambda t, other: t.__isub__(other), "__isub__")
imul = _in_place_op("imul", lambda t, other: t.__imul__(other), "__imul__")
itruediv = _in_place_op("itruediv", lambda t, other: t.__itruediv__(other), "__itruediv__")
fill = _in_place_op("fill", lambda t, value: t.fill(value))


""" Selectors """


def _raw_index(idx):
    if isinstance(idx, tuple):
        return tuple(_raw(i) for i in idx)
    return _raw(idx)


@_op("__getitem__")
class getitem(Function):
    """ cpu/ops.py:234-246 """
    def forward(ctx, a, idx):
        idx = _raw_index(idx)
        ctx.save_for_backward(a.shape, idx)
        return a[idx]

    def backward(ctx, out_grad):
        shape, idx = ctx.get_saved_tensors()
        grad = np.zeros(shape, dtype=CpuTensor.default_dtype)
        parts = idx if isinstance(idx, tuple) else (idx,)
        if any(isinstance(i, (list, range)) or (isinstance(i, np.ndarray) and i.dtype.kind in "iu") for i in parts):
            # integer-array (embedding) index: repeated ids must ACCUMULATE.  The reference's `grad[idx] = out_grad`
            # (cpu/ops.py:245) keeps only the last occurrence; identical whenever ids are unique.
            np.add.at(grad, idx, out_grad)
        else:
            grad[idx] = out_grad
        return grad


@_op("__setitem__")
class setitem(Function):
    """ cpu/ops.py:248-255 """
    def forward(ctx, a, idx, val):
        a[_raw_index(idx)] = val
        return a


""" Reductions """


def _all_axes(x, axis):
    return tuple(range(x.ndim)) if axis is None else axis


@_op()
class max(Function):
    """ every tied maximum receives the full gradient (cpu/ops.py:260-272) """
    def forward(ctx, x, axis=None, keepdims=False):
        axis = _all_axes(x, axis)
        val = np.max(x, axis=axis, keepdims=True)
        ctx.save_for_backward(x, val, axis, keepdims)
        return val if keepdims else np.squeeze(val, axis=axis)

    def backward(ctx, out_grad):
        x, val, axis, keepdims = ctx.get_saved_tensors()
        if not keepdims:
            out_grad = np.expand_dims(out_grad, axis=axis)
        return out_grad * (x == val)


@_op()
class min(Function):
    """ cpu/ops.py:274-286 """
    def forward(ctx, x, axis=None, keepdims=False):
        axis = _all_axes(x, axis)
        val = np.min(x, axis=axis, keepdims=True)
        ctx.save_for_backward(x, val, axis, keepdims)
        return val if keepdims else np.squeeze(val, axis=axis)

    def backward(ctx, out_grad):
        x, val, axis, keepdims = ctx.get_saved_tensors()
        if not keepdims:
            out_grad = np.expand_dims(out_grad, axis=axis)
        return out_grad * (x == val)


@_op()
class sum(Function):
    """ forward = ndarray.sum (cpu/ops.py:288-293); backward = gradient broadcast back to
    the input shape, the semantics of the reference's only sum.backward (opencl/ops.py:353-368) """
    def forward(ctx, t, axis=None, keepdims=False):
        ctx.save_for_backward(t.shape, axis, keepdims)
        return np.asarray(t.sum(axis=axis, keepdims=keepdims))

    def backward(ctx, out_grad):
        shape, axis, keepdims = ctx.get_saved_tensors()
        if not keepdims:
            axes = tuple(range(len(shape))) if axis is None else (axis if isinstance(axis, tuple) else (axis,))
            axes = tuple(sorted(a % len(shape) for a in axes))
            out_grad = np.expand_dims(out_grad, axis=axes) if len(shape) > 0 else out_grad
        return np.broadcast_to(out_grad, shape)


""" Dropout (not an op of the reference, whose BERT example replaces it by the identity: examples/bert.py:37) """


@_op()
class dropout(DropoutFunction):
    """ x.dropout(p, residual=None): the mask of `lightgrad_amd.random` for this call's number, kept elements times float32(1 / (1 - p)),
    dropped ones +0.0 (a dropped NaN too), then `+ residual`.  Nothing is kept but (seed, call number, p): the backward makes the
    mask again.  float32 only - and float64 while CpuTensor.default_dtype is float64 (the yardstick run of a float32 tape: the
    same mask, the same float32 value of the scale) """
    @staticmethod
    def check_operands(x, residual):
        DropoutFunction.check_residual(x, residual)
        for t in (x, residual):
            if t is not None and t.dtype != np.float32 and not (t.dtype == np.float64 and CpuTensor.default_dtype == np.float64):
                raise TypeError("dropout is float32-only (got %s)" % t.dtype)

    def forward(ctx, x, residual, p):
        seed, draw = _random._CpuGenerator.seed, _random._CpuGenerator.next_draw()
        ctx.save_for_backward(seed, draw, p, residual is not None)
        keep = _random.keep_mask(seed, draw, x.size, p).reshape(x.shape)      # element index = index in the dense (row-major) result
        y = np.where(keep, x * x.dtype.type(_random.scale(p)), x.dtype.type(0))
        return y if residual is None else y + residual

    def backward(ctx, out_grad):
        seed, draw, p, has_residual = ctx.get_saved_tensors()
        keep = _random.keep_mask(seed, draw, out_grad.size, p).reshape(out_grad.shape)
        dx = np.where(keep, out_grad * out_grad.dtype.type(_random.scale(p)), out_grad.dtype.type(0))
        return (dx, out_grad) if has_residual else dx


def _mlm_mask(ids, p, mask_token_id, vocab_size, special_ids=(), ignore_index=-100):
    """ ids.mlm_mask(p, mask_token_id, vocab_size, special_ids=(), ignore_index=-100) -> (masked_ids, labels): BERT's token
    masking as `lightgrad_amd.random.mlm_mask_words` defines it for this call's number - one call of the stream.  int32 / int64
    ids of any shape; both results have the ids' dtype and shape and are constants of the tape. """
    args = _random.check_mlm_arguments(ids.dtype, p, mask_token_id, vocab_size, special_ids, ignore_index)
    seed, draw = _random._CpuGenerator.seed, _random._CpuGenerator.next_draw()
    masked, labels = _random.mlm_mask_words(seed, draw, ids.data, *args)
    return CpuTensor.from_numpy(masked, requires_grad=False), CpuTensor.from_numpy(labels, requires_grad=False)


CpuTensor.mlm_mask = _mlm_mask


def _sample(logits, temperature=1.0, top_k=0, top_p=1.0, dtype=np.int64):
    """ logits.sample(temperature=1.0, top_k=0, top_p=1.0, dtype=np.int64) -> one token per row of the last axis, drawn from
    softmax(logits / temperature) restricted by top-k and top-p: `lightgrad_amd.random.sample_tokens` for this call's number - one
    call of the stream, whatever the shape.  The result has the leading shape and is a constant of the tape. """
    shape = logits.shape
    temperature, top_k, top_p, dtype = _random.check_sample_arguments(logits.dtype, shape[-1] if len(shape) else None, temperature, top_k,
                                                                      top_p, dtype)
    seed, draw = _random._CpuGenerator.seed, _random._CpuGenerator.next_draw()
    tokens = _random.sample_tokens(seed, draw, logits.data, temperature, top_k, top_p)
    return CpuTensor.from_numpy(np.asarray(tokens, dtype=dtype), requires_grad=False)


CpuTensor.sample = _sample


def _sample_rows(logits, table, index, counter, dtype=np.int32):
    """ logits.sample_rows(table, index, counter, dtype=np.int32) -> one token per row, every row under the parameters and the
    random stream of a table row of its own: `lightgrad_amd.random.sample_tokens_rows`.  logits (rows, V) or (rows, 1, V); table
    int32 (n, 8) (`random.sampling_table`); index int32 (rows,), -1 = a free row (token 0, its logits are not read); counter int32
    (n,).  The generator's state is neither read nor advanced.  A bad row (see the definition) answers 0 and the call raises
    IndexError after every other row has been answered - `err.tokens` is the result.  A constant of the tape. """
    shape, dtype = logits.shape, _random.check_sample_rows_operands(logits, table, index, counter, dtype)
    tokens, bad = _random.sample_tokens_rows(logits.data.reshape(shape[0], shape[-1]), table.data, index.data, counter.data)
    out = CpuTensor.from_numpy(np.asarray(tokens, dtype=dtype).reshape(shape[:-1]), requires_grad=False)
    if bad.any():
        err = IndexError("sample_rows: rows %s name no table row, or one whose counter or parameters are out of range" % np.flatnonzero(bad).tolist())
        err.tokens = out
        raise err
    return out


CpuTensor.sample_rows = _sample_rows


def _penalize_rows(logits, table, index, prompts, prompt_len, out, out_len, eos=None):
    """ logits.penalize_rows(table, index, prompts, prompt_len, out, out_len, eos=None): the repetition, presence and frequency
    penalties and the minimum of new tokens of `lightgrad_amd.random.penalize_logits`, IN PLACE and outside the tape; returns
    `logits`, so that `logits.penalize_rows(...).sample_rows(...)` reads well.  logits (rows, V) or (rows, 1, V), which must not
    require a gradient; table int32 (n, 4) (`random.penalty_table`); index int32 (rows,), -1 = a free row (untouched, unread);
    prompts (n, P), prompt_len (n,), out (n, G), out_len (n,) int32: the history of every request.  A bad row (see the definition)
    keeps its bits and the call raises IndexError after every other row has been computed. """
    rows, V, _ = _random.check_penalize_operands(logits, table, index, prompts, prompt_len, out, out_len, eos)
    from ..grads import Gradients
    assert logits.ctx is None and not (Gradients._is_enabled() and logits.requires_grad), \
        "penalize_rows writes the logits in place: they must not require a gradient (run it under Gradients.no_grad(), or pass requires_grad=False)"
    y, bad = _random.penalize_logits(logits.data.reshape(rows, V), table.data, index.data, prompts.data, prompt_len.data, out.data, out_len.data, eos)
    good = np.flatnonzero((index.data >= 0) & ~bad)
    logits.data[good] = y[good].reshape((len(good),) + tuple(logits.shape[1:]))      # a view keeps the bytes between its rows
    if bad.any():
        raise IndexError("penalize_rows: rows %s name no request, or one whose lengths, parameters or history are out of range" % np.flatnonzero(bad).tolist())
    return logits


CpuTensor.penalize_rows = _penalize_rows


def _logprob_rows(logits, token, want, index, counter, logprob, top_ids, top_logprob):
    """ logits.logprob_rows(token, want, index, counter, logprob, top_ids, top_logprob): the log-probability of the token just
    drawn and the top-n alternatives of `lightgrad_amd.random.token_logprobs_rows`, written IN PLACE into the three outputs and
    outside the tape - the definition of the op; returns None.  logits (rows, V) or (rows, 1, V): what the draw read; token int32
    (rows,) or (rows, 1); want int32 (N,): -1 nothing, 0 the token's only, k also the k most likely ids; index int32 (rows,), -1 =
    a free row (unread); counter int32 (N,): the column; logprob float32 (N, G), top_ids int32 and top_logprob float32 (N, G, n),
    n <= 8.  A bad row (see the definition) writes nothing and the call raises IndexError after every other row has been written. """
    rows, V, _, _, _ = _random.check_logprob_operands(logits, token, want, index, counter, logprob, top_ids, top_logprob)
    bad = _random.token_logprobs_rows(logits.data.reshape(rows, V), token.data, want.data, index.data, counter.data, logprob.data, top_ids.data,
                                      top_logprob.data)
    if bad.any():
        raise IndexError("logprob_rows: rows %s name no request, or one whose column, count of alternatives or token is out of range" % np.flatnonzero(bad).tolist())


CpuTensor.logprob_rows = _logprob_rows


def _guide_rows(logits, allow, states, edges, index, out, out_len, state):
    """ logits.guide_rows(allow, states, edges, index, out, out_len, state): the token automata of `lightgrad_amd.guide.guide_logits`,
    IN PLACE and outside the tape; returns `logits`.  logits (rows, V) or (rows, 1, V), which must not require a gradient; allow
    (S, W), states (S, 4), edges (E, 2) int32 (`guide.compile_guides`); index int32 (rows,), -1 = a free row (untouched, unread);
    out (N, G), out_len (N,) int32: the tokens every request has stored; state int32 (N, 2): (q, k) per request, moved to
    (the state behind the out_len[i] stored tokens, out_len[i]) in place.  The ids the state does not allow go to -inf, a forced
    id to +0.0, everything else keeps its bytes.  A bad row (see the definition) keeps its bits and its state, and the call raises
    IndexError after every other row has been computed. """
    rows, V = _guide.check_guide_rows_operands(logits, allow, states, edges, index, out, out_len, state)[:2]
    from ..grads import Gradients
    assert logits.ctx is None and not (Gradients._is_enabled() and logits.requires_grad), \
        "guide_rows writes the logits in place: they must not require a gradient (run it under Gradients.no_grad(), or pass requires_grad=False)"
    y, new_state, bad = _guide.guide_logits(logits.data.reshape(rows, V), allow.data, states.data, edges.data, index.data, out.data, out_len.data, state.data)
    good = np.flatnonzero((index.data >= 0) & ~bad)
    logits.data[good] = y[good].reshape((len(good),) + tuple(logits.shape[1:]))      # a view keeps the bytes between its rows
    state.data[...] = new_state
    if bad.any():
        raise IndexError("guide_rows: rows %s name no request, or one whose lengths, state or stored tokens its automaton does not allow" % np.flatnonzero(bad).tolist())
    return logits


CpuTensor.guide_rows = _guide_rows


def _decode_commit(nxt, token, out_ids, pos, done, eos=None):
    """ nxt.decode_commit(token, out_ids, pos, done, eos=None): the per-row bookkeeping of one decode step, in place and outside
    the tape - the definition of the op.  nxt (b,) or (b, 1), token (b, 1), out_ids (b, columns), pos (b,), done (b,), all int32.
    For each row r with done[r] == 0: p = pos[r] + 1; pos[r] = p, token[r] = nxt[r], out_ids[r, p] = nxt[r], and done[r] = 1 if
    `eos` is an id >= 0 and nxt[r] equals it.  A row with done[r] != 0 is not touched at all.  A live row whose p is no column
    of out_ids is left untouched as well and the call raises IndexError - after the other rows have been committed, as the
    device flag of the HipTensor op does at its next synchronisation. """
    b = _check_decode_commit(nxt, token, out_ids, pos, done, eos)
    arrays = [t.data for t in (nxt, token, out_ids, pos, done)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "decode_commit: two operands overlap"
    new, columns = nxt.data.reshape(b), out_ids.shape[1]
    p = pos.data.astype(np.int64) + 1
    live = done.data == 0
    bad = live & ((p < 0) | (p >= columns))
    rows = np.nonzero(live & ~bad)[0]
    pos.data[rows] = p[rows]
    token.data[rows, 0] = new[rows]
    out_ids.data[rows, p[rows]] = new[rows]
    if eos is not None and int(eos) >= 0:
        done.data[rows[new[rows] == int(eos)]] = 1
    if bad.any():
        raise IndexError("decode_commit: position %d + 1 of row %d is no column of out_ids (%d columns)" % (
            int(pos.data[np.nonzero(bad)[0][0]]), int(np.nonzero(bad)[0][0]), columns))


def _check_decode_commit(nxt, token, out_ids, pos, done, eos):
    """the operand shapes and dtypes of `decode_commit`, on any backend; returns the batch"""
    b = pos.shape[0] if len(pos.shape) == 1 else -1
    i32 = np.dtype(np.int32)
    assert b >= 1 and tuple(nxt.shape) in ((b,), (b, 1)) and tuple(token.shape) == (b, 1) and len(out_ids.shape) == 2 and out_ids.shape[0] == b \
        and out_ids.shape[1] >= 1 and tuple(done.shape) == (b,), \
        "decode_commit: nxt (b,) or (b, 1), token (b, 1), out_ids (b, columns), pos (b,), done (b,) - got %s, %s, %s, %s, %s" % (
            tuple(nxt.shape), tuple(token.shape), tuple(out_ids.shape), tuple(pos.shape), tuple(done.shape))
    assert all(np.dtype(t.dtype) == i32 for t in (nxt, token, out_ids, pos, done)), "decode_commit: every operand is int32"
    assert eos is None or int(eos) == eos, "decode_commit: eos is an int or None"
    return b


CpuTensor.decode_commit = _decode_commit


def _serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity, eos=None):
    """ nxt.serve_commit(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity,
    eos=None): the slot bookkeeping of one step of continuous batching, in place and outside the tape - the definition of the op,
    written as the loop it is.  All int32: prompts (N, P) right-padded ids, prompt_len (N,), budget (N,) new tokens per request
    (>= 1), out (N, G) generated tokens, out_len (N,), queue (2,) = {next request to admit, requests finished}, req (b,) the
    request each slot holds (-1: free), pos (b,) the cache's positions, count (b,) the real new tokens of the step, ids and
    position_ids (b, m) the step's inputs, last (b,) the row of the flattened (b * m) hidden rows that goes to the head; nxt (b,) or
    (b, 1) the tokens just drawn.  For slot s = 0 .. b - 1, in this order:
      1. r = req[s].  If r >= 0: t = pos[s] + count[s] (the step's tokens are in the cache now).  t < prompt_len[r]: the slot goes
         on prefilling, n = min(m, prompt_len[r] - t) tokens prompts[r, t:t + n], and nxt[s] is ignored.  Otherwise nxt[s] is the
         request's next token: out[r, out_len[r]] = nxt[s], out_len[r] += 1; if it is `eos` (an id >= 0) or the budget is used
         up, queue[1] += 1 and the slot is free (r = -1: the last token is fed to nobody), else n = 1 and the token is nxt[s].
      2. A free slot while queue[0] < N: r = queue[0], queue[0] += 1, t = 0, n = min(m, prompt_len[r]) tokens prompts[r, :n].
      3. Still free: n = 0, t = 0.
      4. req[s] = r, pos[s] = t, count[s] = n, ids[s] = the n tokens then 0, position_ids[s] = t .. t + n - 1 then 0,
         last[s] = s * m + max(n - 1, 0).
    A slot that would leave its bounds - t + n > capacity, a token beyond the columns of out, a request id >= N, t < 0, prompt
    tokens beyond the columns of prompts - gets count[s] = 0 and nothing else of the slot (req, pos, ids, position_ids, last) is
    written; the call raises IndexError after every other slot has been committed, as the device flag of the HipTensor op does at
    its next synchronisation.  (What step 1 wrote to out, out_len and queue for that slot before step 4 found t + n > capacity
    stays written.) """
    b, m, N = _check_serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity, eos)
    arrays = [t.data for t in (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "serve_commit: two operands overlap"
    eos, capacity = (-1 if eos is None else int(eos)), int(capacity)
    bad = []
    for s in range(b):
        r, t, n, row, tok, fault, _ = _serve_slot_request(s, m, capacity, eos, nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count)
        r, t, n, row, fault = _serve_slot_admit(m, r, t, n, row, fault, prompts, prompt_len, queue)
        if not _serve_slot_write(s, m, capacity, r, t, n, row, tok, fault, prompts, req, pos, count, ids, position_ids, last):
            bad.append(s)
    if bad:
        raise IndexError("serve_commit: slot %d (of %d that did) would leave the cache, its prompt or its row of out" % (bad[0], len(bad)))


def _serve_slot_request(s, m, capacity, eos, nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count):
    """step 1 of `serve_commit` for slot s, once for the three commits (`m`: the most tokens a slot takes in a step).  Returns
    (r, t, n, row, tok, fault, finished): the slot's request (-1: none), the position of its first token, how many tokens, where
    they come from - the prompt of request `row`, or (row = -1) the one token `tok` just drawn -, whether the slot would leave its
    bounds, whether its request has just finished"""
    (N, P), G = prompts.shape, out.shape[1]
    r, t, n, row, tok, fault, finished = int(req.data[s]), 0, 0, -1, 0, False, False
    if r >= 0:
        t = int(pos.data[s]) + int(count.data[s])
        if r >= N or t < 0 or t > capacity:
            fault = True
        elif t < int(prompt_len.data[r]):
            n, row = np.minimum(m, int(prompt_len.data[r]) - t).item(), r
            fault = t + n > P
        else:
            g = int(out_len.data[r])
            if g < 0 or g >= G:
                fault = True
            else:
                tok = nxt.data.reshape(-1)[s]
                out.data[r, g], out_len.data[r] = tok, g + 1
                if (eos >= 0 and int(tok) == eos) or g + 1 == int(budget.data[r]):
                    queue.data[1] += 1
                    r, finished = -1, True
                else:
                    n = 1
    return r, t, n, row, tok, fault, finished


def _serve_slot_admit(m, r, t, n, row, fault, prompts, prompt_len, queue):
    """steps 2 and 3 of `serve_commit`: a free slot takes the next waiting request, if there is one; returns (r, t, n, row, fault)"""
    if not fault and r < 0:
        t = 0
        if 0 <= int(queue.data[0]) < prompts.shape[0]:
            r = row = int(queue.data[0])
            queue.data[0] += 1
            n = np.minimum(m, int(prompt_len.data[r])).item()
            fault = n < 0 or n > prompts.shape[1]
    return r, t, n, row, fault


def _serve_slot_write(s, m, capacity, r, t, n, row, tok, fault, prompts, req, pos, count, ids, position_ids, last):
    """step 4 of `serve_commit` for slot s of a step of (b, m) rows; False, and count[s] = 0 alone, for a slot that would leave its
    bounds"""
    if fault or t + n > capacity:
        count.data[s] = 0
        return False
    req.data[s], pos.data[s], count.data[s] = r, t, n
    ids.data[s, :n], ids.data[s, n:] = (prompts.data[row, t:t + n] if row >= 0 else tok), 0
    position_ids.data[s, :n], position_ids.data[s, n:] = t + np.arange(n), 0
    last.data[s] = s * m + (n - 1 if n > 0 else 0)
    return True


def _check_serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity, eos,
                        name="serve_commit", cu=None):
    """the operand shapes and dtypes of `serve_commit`, on any backend; returns (slots b, tokens per slot m, requests N).  With `cu`
    those of `serve_commit_packed`: ids / position_ids are (1, T) with T >= b, cu is (b + 1,), and T is returned for m"""
    packed = cu is not None
    b = req.shape[0] if len(req.shape) == 1 else -1
    m = ids.shape[1] if len(ids.shape) == 2 and (ids.shape[0] == 1 or not packed) else -1
    N = prompts.shape[0] if len(prompts.shape) == 2 else -1
    i32 = np.dtype(np.int32)
    operands = (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last) + ((cu,) if packed else ())
    shapes = [tuple(t.shape) for t in operands]
    assert 1 <= b <= 1024 and m >= (b if packed else 1) and N >= 1 and prompts.shape[1] >= 1 and shapes[0] in ((b,), (b, 1)) \
        and shapes[2] == shapes[3] == shapes[5] == (N,) and len(out.shape) == 2 and out.shape[0] == N and out.shape[1] >= 1 and shapes[6] == (2,) \
        and shapes[8] == shapes[9] == shapes[12] == (b,) and shapes[10] == shapes[11] == ((1, m) if packed else (b, m)) and shapes[13:] in ([], [(b + 1,)]), \
        "%s: nxt (b,) or (b, 1), prompts (N, P), prompt_len / budget / out_len (N,), out (N, G), queue (2,), req / pos / count / last (b,) " \
        "with 1 <= b <= 1024, ids / position_ids %s - got %s" % (name, "(1, T) with T >= b, cu (b + 1,)" if packed else "(b, m)", shapes)
    assert all(np.dtype(t.dtype) == i32 for t in operands), "%s: every operand is int32" % name
    assert eos is None or int(eos) == eos, "%s: eos is an int or None" % name
    assert int(capacity) == capacity and 1 <= capacity < 2 ** 31, "%s: capacity is an int >= 1" % name
    return b, m, N


CpuTensor.serve_commit = _serve_commit


def _serve_commit_packed(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last, capacity, chunk, eos=None):
    """ nxt.serve_commit_packed(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last,
    capacity, chunk, eos=None): `serve_commit` for a TOKEN-PACKED step, in place and outside the tape - the definition of the op,
    written as the loops it is.  The step has T token rows for all slots together, the token budget: ids and position_ids are
    (1, T) with T >= b, cu is (b + 1,) and slot s owns rows cu[s] .. cu[s + 1] - 1; every other operand is `serve_commit`'s.
      1., 2. For slot s = 0 .. b - 1 in this order, steps 1 and 2 of `serve_commit` with m = chunk: the slot's request r, its
         position t and the tokens it WANTS - min(chunk, prompt_len[r] - t) of its prompt (a prefilling slot, one just admitted
         included), the one token just drawn (a decoding slot), none (a free slot nobody waits for: r = -1, t = 0).
      3. The budget.  Every decoding slot gets its token: n = 1.  With R = T - the number of decoding slots, the prefilling slots
         take n = min(want, what is left of R) in slot order.  A prefilling slot granted 0 keeps its request and its position: it
         gets count 0 and asks again in the next step (if any slot prefills, R >= 1: some slot moves on).
      4. cu = the exclusive sum of the n in slot order, cu[b] = their total; req[s] = r, pos[s] = t, count[s] = n; rows cu[s] + i
         of ids / position_ids = token i of the slot / t + i; the rows >= cu[b] get id 0 and position 0;
         last[s] = min(cu[s] + max(n - 1, 0), T - 1) (an idle slot behind a full buffer must not name row T).
    A slot that would leave its bounds - those of `serve_commit`, with t + want > capacity - gets count[s] = 0, takes no rows (it
    counts neither as decoding nor as prefilling) and nothing else of it (req, pos, last) is written; the call raises IndexError
    after every other slot has been committed. """
    b, T, N = _check_serve_commit_packed(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last, capacity,
                                         chunk, eos)
    arrays = [t.data for t in (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "serve_commit_packed: two operands overlap"
    eos, capacity, chunk = (-1 if eos is None else int(eos)), int(capacity), int(chunk)
    slots, bad = [], []
    for s in range(b):
        r, t, n, row, tok, fault, _ = _serve_slot_request(s, chunk, capacity, eos, nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count)
        r, t, n, row, fault = _serve_slot_admit(chunk, r, t, n, row, fault, prompts, prompt_len, queue)
        if fault or t + n > capacity:
            bad.append(s)
            slots.append(None)
        else:
            slots.append((r, t, n, row, tok))
    left = T - len([x for x in slots if x is not None and x[3] < 0 and x[2] == 1])
    ids.data[...], position_ids.data[...] = 0, 0
    start = 0
    for s, x in enumerate(slots):
        cu.data[s] = start
        if x is None:
            count.data[s] = 0
            continue
        r, t, n, row, tok = x
        if row >= 0:                # (a decoding slot: row < 0 and n = 1; an idle one: n = 0)
            n = np.minimum(n, left).item()
            left -= n
        req.data[s], pos.data[s], count.data[s] = r, t, n
        ids.data[0, start:start + n] = prompts.data[row, t:t + n] if row >= 0 else tok
        position_ids.data[0, start:start + n] = t + np.arange(n)
        last.data[s] = np.minimum(start + (n - 1 if n > 0 else 0), T - 1)
        start += n
    cu.data[b] = start
    if bad:
        raise IndexError("serve_commit_packed: slot %d (of %d that did) would leave the cache, its prompt or its row of out" % (bad[0], len(bad)))


def _check_serve_commit_packed(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last, capacity, chunk, eos):
    """the operand shapes and dtypes of `serve_commit_packed`, on any backend; returns (slots b, token rows T, requests N)"""
    b, T, N = _check_serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity, eos,
                                  name="serve_commit_packed", cu=cu)
    assert int(chunk) == chunk and 1 <= chunk and b * chunk < 2 ** 31, "serve_commit_packed: chunk is an int >= 1"
    return b, T, N


CpuTensor.serve_commit_packed = _serve_commit_packed


def _serve_commit_paged(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free,
                        block_size, prefix_blocks=0, eos=None):
    """ nxt.serve_commit_paged(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last,
    block_table, held, free, block_size, prefix_blocks=0, eos=None): `serve_commit` over a PAGED cache (nn.PagedKVCache), in place
    and outside the tape - the definition of the op.  block_table (b, max_blocks): word n of row s is the pool block that holds
    positions n * B .. n * B + B - 1 of slot s, -1 = none; held (b,): the blocks a slot's table names; free (num_blocks + 1,): word
    0 the number n of free blocks, words 1 .. n their indices, a stack whose top is word n.  B = block_size, F = prefix_blocks
    (host ints): blocks 0 .. F - 1 hold a prefix every request shares.  capacity = max_blocks * B.  Every other operand is
    `serve_commit`'s.  Two passes over the slots, each in slot order:
      1. Step 1 of `serve_commit`.  A slot whose request has just finished then RELEASES its blocks: block_table[s, F ..
         held[s] - 1] are pushed in table order (free[1 + free[0]] = block, free[0] += 1), its whole table row becomes -1 and
         held[s] = 0.
      2. ADMISSION: a free slot (one just released included) while queue[0] < N is offered r = queue[0], which needs
         need = ceil((prompt_len[r] + budget[r] - 1) / B) - F blocks.  need > free[0]: admission stops for this commit - this
         slot and every later free slot stay free, whatever the requests behind r need.  Otherwise queue[0] += 1, the slot pops
         block_table[s, F + i] = free[free[0]], free[0] -= 1 for i = 0 .. need - 1, takes block_table[s, :F] = 0 .. F - 1,
         held[s] = F + need, t = F * B and n = min(m, prompt_len[r] - t) tokens prompts[r, t:t + n].
      Steps 3 and 4 of `serve_commit` follow for every slot.
    Bounds, on top of `serve_commit`'s: a releasing slot whose held is outside 0 .. max_blocks or that names a block outside
    0 .. num_blocks - 1 in the words it releases; free[0] outside 0 .. num_blocks before the commit (every releasing slot and every
    offered request) or behind the pushes of all releasing slots together (every releasing slot); an offered request with
    need < 0, F + need > max_blocks, or no prompt token at or behind F * B (it leaves the queue all the same).  Such a slot gets
    count[s] = 0 and nothing else of it is written - no block is pushed or popped for it; the call raises IndexError after every
    other slot has been committed. """
    b, m, N = _check_serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, 1, eos)
    MB, NB, B, F = _check_paged_state("serve_commit_paged", b, block_table, held, free, block_size, prefix_blocks)
    arrays = [t.data for t in (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "serve_commit_paged: two operands overlap"
    P = prompts.shape[1]
    eos, capacity = (-1 if eos is None else int(eos)), MB * B
    table, stack = block_table.data, free.data
    stack_ok = 0 <= int(stack[0]) <= NB
    # per slot: [r, t, n, row, tok, fault, finished]
    state = [list(_serve_slot_request(s, m, capacity, eos, nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count)) for s in range(b)]
    # the release: which slots may push is settled first (the bounds of each, then the room for all of them together)
    pushes = {}
    for s in range(b):
        if state[s][6]:
            h = int(held.data[s])
            if stack_ok and 0 <= h <= MB and all(0 <= int(e) < NB for e in table[s, F:h]):
                pushes[s] = [int(e) for e in table[s, F:h]]
            else:
                state[s][5] = True
    if stack_ok and int(stack[0]) + len([e for p in pushes.values() for e in p]) > NB:
        for s in pushes:
            state[s][5] = True
        pushes = {}
    for s in sorted(pushes):
        for e in pushes[s]:
            stack[1 + stack[0]] = e
            stack[0] += 1
        table[s, :], held.data[s] = -1, 0
    # the admission
    stopped = False
    for s in range(b):
        r, t, n, row, _, fault, _ = state[s]
        if fault or r >= 0:
            continue
        t = 0
        if not stopped and 0 <= int(queue.data[0]) < N:
            k = int(queue.data[0])
            need = -(-(int(prompt_len.data[k]) + int(budget.data[k]) - 1) // B) - F
            n0 = np.minimum(m, int(prompt_len.data[k]) - F * B).item()
            if not stack_ok or need < 0 or F + need > MB or n0 < 1 or F * B + n0 > P:
                queue.data[0] += 1
                fault = True
            elif need > int(stack[0]):
                stopped = True
            else:
                queue.data[0] += 1
                for i in range(need):
                    table[s, F + i] = stack[stack[0]]
                    stack[0] -= 1
                table[s, :F], held.data[s] = np.arange(F), F + need
                r, t, n, row = k, F * B, n0, k
        state[s][:4], state[s][5] = (r, t, n, row), fault
    bad = [s for s, (r, t, n, row, tok, fault, _) in enumerate(state)
           if not _serve_slot_write(s, m, capacity, r, t, n, row, tok, fault, prompts, req, pos, count, ids, position_ids, last)]
    if bad:
        raise IndexError("serve_commit_paged: slot %d (of %d that did) would leave the cache, its prompt, its row of out or the block pool" % (bad[0], len(bad)))


def _check_paged_state(name, b, block_table, held, free, block_size, prefix_blocks):
    """the paging operands of `serve_commit_paged`, on any backend; returns (max_blocks, num_blocks, B, F)"""
    i32 = np.dtype(np.int32)
    assert len(block_table.shape) == 2 and block_table.shape[0] == b and tuple(held.shape) == (b,) and len(free.shape) == 1 and free.shape[0] >= 2 \
        and all(np.dtype(t.dtype) == i32 for t in (block_table, held, free)), \
        "%s: block_table (b, max_blocks), held (b,) and free (num_blocks + 1,) are int32 - got %s" % (
            name, [(str(t.dtype), tuple(t.shape)) for t in (block_table, held, free)])
    MB, NB = block_table.shape[1], free.shape[0] - 1
    assert int(block_size) == block_size and 4 <= block_size <= 128 and block_size & (block_size - 1) == 0 and 1 <= MB and MB * block_size <= 512, \
        "%s: block_size is a power of two within 4 .. 128 and max_blocks * block_size <= 512, got %s and %d blocks per table" % (name, block_size, MB)
    assert int(prefix_blocks) == prefix_blocks and 0 <= prefix_blocks <= MB and prefix_blocks <= NB, \
        "%s: prefix_blocks is an int within 0 .. max_blocks = %d and 0 .. num_blocks = %d, got %s" % (name, MB, NB, prefix_blocks)
    return MB, NB, int(block_size), int(prefix_blocks)


CpuTensor.serve_commit_paged = _serve_commit_paged


def _speculate_commit(tgt, ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram=3, min_ngram=1, eos=None):
    """ tgt.speculate_commit(ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram=3, min_ngram=1, eos=None):
    the bookkeeping of one step of speculative decoding by prompt lookup, in place and outside the tape - the definition of the
    op, written as the loop it is.  All int32: tgt (b, m) the tokens drawn from the logits of the step's m rows; ids and
    position_ids (b, m) and count (b,) the step's inputs on entry and the next step's on exit; out_ids (b, columns) a column per
    position of each row's sequence; pos (b,) the position of each row's input token (the cache's positions, as in
    `decode_commit`); end (b,) the last column a row may write; done (b,); stats (3,) = {rows finished, tokens drafted, drafts
    accepted}.  0 <= draft <= m - 1 drafts per step at most, n-grams of min_ngram .. max_ngram tokens.  For each row r on its own:
      1. done[r] != 0: count[r] = 0 and nothing else of the row is written.
      2. c = count[r], p = pos[r].  Unless 1 <= c <= m, p >= 0 and p + c <= end[r] <= columns - 1: count[r] = 0, nothing else of
         the row is written and the call raises IndexError after every other row has been committed, as the device flag of the
         HipTensor op does at its next synchronisation.
      3. a = the number of leading j in 0 .. c - 2 with ids[r, j + 1] == tgt[r, j]: the drafts the model agrees with.  The row
         emits e = a + 1 tokens tgt[r, :e]; if `eos` (an id >= 0) is among them, e ends at the first one and the row stops.
      4. out_ids[r, p + 1 .. p + e] = tgt[r, :e]; p += e, pos[r] = p; stats[1] += c - 1, stats[2] += a (before the cut at eos).
      5. The row stopped, or p == end[r]: done[r] = 1, stats[0] += 1, count[r] = 0.  Otherwise:
      6. L = p + 1, seq = out_ids[r, :L], cap = min(draft, end[r] - p - 1).  For n = max_ngram down to min_ngram with L >= n + 1:
         the largest q in 0 .. L - n - 1 with seq[q:q + n] == seq[L - n:L]; the first n that has one wins and the drafts are
         seq[q + n:min(q + n + cap, L)]; no such n, or cap == 0: no drafts.  ids[r] = [seq[p]] + drafts then 0,
         count[r] = 1 + len(drafts), position_ids[r, i] = p + i for i < count[r], else 0.
    Rejected drafts have left keys and values in the cache beyond the new position: nothing reads them (nn.KVCache). """
    b, m = _check_speculate_commit(tgt, ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram, min_ngram, eos)
    arrays = [t.data for t in (tgt, ids, count, position_ids, out_ids, pos, end, done, stats)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "speculate_commit: two operands overlap"
    columns = out_ids.shape[1]
    eos, draft, max_ngram, min_ngram = (-1 if eos is None else int(eos)), int(draft), int(max_ngram), int(min_ngram)
    bad = []
    for r in range(b):
        if done.data[r] != 0:
            count.data[r] = 0
            continue
        c, p, last = int(count.data[r]), int(pos.data[r]), int(end.data[r])
        if not (1 <= c <= m and p >= 0 and p + c <= last <= columns - 1):
            count.data[r] = 0
            bad.append(r)
            continue
        a = 0
        while a < c - 1 and ids.data[r, a + 1] == tgt.data[r, a]:
            a += 1
        e, stopped = a + 1, False
        if eos >= 0 and (tgt.data[r, :e] == eos).any():
            e, stopped = int(np.argmax(tgt.data[r, :e] == eos)) + 1, True
        out_ids.data[r, p + 1:p + 1 + e] = tgt.data[r, :e]
        p += e
        pos.data[r] = p
        stats.data[1] += c - 1
        stats.data[2] += a
        if stopped or p == last:
            done.data[r] = 1
            stats.data[0] += 1
            count.data[r] = 0
            continue
        # (this module's `min` is the tensor op)
        L, cap, drafts = p + 1, (draft if draft < last - p - 1 else last - p - 1), ()
        seq = out_ids.data[r, :L]
        if cap > 0:
            for n in range(max_ngram if max_ngram < L - 1 else L - 1, min_ngram - 1, -1):
                q = next((q for q in range(L - n - 1, -1, -1) if (seq[q:q + n] == seq[L - n:]).all()), -1)
                if q >= 0:
                    drafts = seq[q + n:q + n + cap].copy()       # (the slice ends at L by itself)
                    break
        k = 1 + len(drafts)
        ids.data[r, 0], ids.data[r, 1:k], ids.data[r, k:] = seq[p], drafts, 0
        position_ids.data[r, :k], position_ids.data[r, k:] = p + np.arange(k), 0
        count.data[r] = k
    if bad:
        raise IndexError("speculate_commit: row %d (of %d that did) holds a count, a position or an end outside its bounds" % (bad[0], len(bad)))


def _check_speculate_commit(tgt, ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram, min_ngram, eos):
    """the operand shapes and dtypes of `speculate_commit`, on any backend; returns (rows b, tokens per row m)"""
    b = pos.shape[0] if len(pos.shape) == 1 else -1
    m = ids.shape[1] if len(ids.shape) == 2 else -1
    i32 = np.dtype(np.int32)
    operands = (tgt, ids, count, position_ids, out_ids, pos, end, done, stats)
    shapes = [tuple(t.shape) for t in operands]
    assert b >= 1 and m >= 1 and shapes[0] == shapes[1] == shapes[3] == (b, m) and shapes[2] == shapes[6] == shapes[7] == (b,) \
        and len(out_ids.shape) == 2 and out_ids.shape[0] == b and out_ids.shape[1] >= 1 and shapes[8] == (3,), \
        "speculate_commit: tgt / ids / position_ids (b, m), count / pos / end / done (b,), out_ids (b, columns), stats (3,) - got %s" % (shapes,)
    assert all(np.dtype(t.dtype) == i32 for t in operands), "speculate_commit: every operand is int32"
    assert eos is None or int(eos) == eos, "speculate_commit: eos is an int or None"
    assert int(draft) == draft and 0 <= draft <= m - 1, "speculate_commit: draft is an int within 0 .. m - 1 = %d (got %s)" % (m - 1, draft)
    assert int(min_ngram) == min_ngram and int(max_ngram) == max_ngram and 1 <= min_ngram <= max_ngram < 2 ** 31, \
        "speculate_commit: 1 <= min_ngram <= max_ngram are ints (got %s, %s)" % (min_ngram, max_ngram)
    return b, m


CpuTensor.speculate_commit = _speculate_commit


def _beam_step(logits, scores, parent, token, out_ids, pos, done, stats, num_beams, eos=None):
    """ logits.beam_step(scores, parent, token, out_ids, pos, done, stats, num_beams, eos=None): one step of beam search, in place
    and outside the tape - the definition of the op, written as the loop it is.  Beams are rows: `rows = b * w` with w =
    num_beams (1 .. 8), group g is rows g * w .. g * w + w - 1, best first.  logits (rows, V) or (rows, 1, V) float32 with V >= w;
    scores (rows,) float32, the cumulative log-probability; token (rows, 1), out_ids (rows, columns), pos (rows,), done (rows,),
    parent (rows,), stats (2,) = {groups finished, slots that changed their beam}: int32.  The floating-point part is evaluated in
    float64 from the float32 inputs.  For each group on its own:
      1. Any row with pos < 0, or a live row (done == 0) with pos + 1 >= columns: the group keeps every byte, parent is the
         identity and the call raises IndexError after every other group has been committed, as the device flag of the HipTensor
         op does at its next synchronisation.
      2. A group whose rows are all done keeps every byte; parent is the identity.
      3. Candidates: a live beam i with logits x offers (scores[i] + x[j] - m - log sum_k exp(x[k] - m), i, j) for every j, with
         m = max x; a done beam offers exactly one, (scores[i], i, -), itself, at flat index i * V.
      4. The w largest candidates, ties to the smaller flat index i * V + j, best first.
      5. Output slot n takes candidate (s, i, j): parent[n] = g * w + i.  Beam i done: slot n becomes a copy of row i - score, token,
         pos, done = 1, out_ids columns 0 .. pos[i].  Otherwise p = pos[i] + 1: out_ids columns 0 .. pos[i] of row i, column p = j,
         pos = p, token = j, scores = float32(s), done = (eos is an id >= 0 and j == eos).  Columns beyond the slot's new pos keep
         what they held.
      6. stats[0] += 1 when the step takes the group from "some beam live" to "all done"; stats[1] += the slots with
         parent[n] != g * w + n. """
    rows, V, w = _check_beam_step(logits, scores, parent, token, out_ids, pos, done, stats, num_beams, eos)
    arrays = [t.data for t in (logits, scores, parent, token, out_ids, pos, done, stats)]
    assert not any(np.shares_memory(x, y) for i, x in enumerate(arrays) for y in arrays[i + 1:]), "beam_step: two operands overlap"
    x_all, columns, eos = logits.data.reshape(rows, V), out_ids.shape[1], (-1 if eos is None else int(eos))
    bad = []
    for lo in range(0, rows, w):
        group = slice(lo, lo + w)
        parent.data[group] = np.arange(lo, lo + w)
        p_old, d_old = pos.data[group].astype(np.int64), done.data[group] != 0
        if (p_old < 0).any() or (~d_old & (p_old + 1 >= columns)).any():
            bad.append(lo // w)
            continue
        if d_old.all():
            continue
        value, beam, tok = [], [], []
        with np.errstate(all="ignore"):
            for i in range(w):
                s = np.float64(scores.data[lo + i])
                if d_old[i]:
                    value.append(np.array([s])), beam.append(np.array([i])), tok.append(np.array([-1]))
                    continue
                x = x_all[lo + i].astype(np.float64)
                m = x.max()
                value.append(s + (x - m - np.log(np.exp(x - m).sum())))
                beam.append(np.full(V, i)), tok.append(np.arange(V))
        value, beam, tok = np.concatenate(value), np.concatenate(beam), np.concatenate(tok)
        # candidates lie in flat-index order: a stable sort by descending value leaves ties to the smaller index (NaN: last)
        best = np.argsort(-value, kind="stable")[:w]
        s_old, t_old, ids_old = scores.data[group].copy(), token.data[group, 0].copy(), out_ids.data[group].copy()
        for n, c in enumerate(best):
            i, j = int(beam[c]), int(tok[c])
            parent.data[lo + n] = lo + i
            out_ids.data[lo + n, :p_old[i] + 1] = ids_old[i, :p_old[i] + 1]
            if d_old[i]:
                scores.data[lo + n], token.data[lo + n, 0], pos.data[lo + n], done.data[lo + n] = s_old[i], t_old[i], p_old[i], 1
            else:
                out_ids.data[lo + n, p_old[i] + 1] = j
                scores.data[lo + n], token.data[lo + n, 0], pos.data[lo + n] = np.float32(value[c]), j, p_old[i] + 1
                done.data[lo + n] = 1 if eos >= 0 and j == eos else 0
        stats.data[0] += 1 if (done.data[group] != 0).all() else 0
        stats.data[1] += int((parent.data[group] != np.arange(lo, lo + w)).sum())
    if bad:
        raise IndexError("beam_step: group %d (of %d that did) holds a position outside the columns of out_ids (%d)" % (bad[0], len(bad), columns))


def _check_beam_step(logits, scores, parent, token, out_ids, pos, done, stats, num_beams, eos):
    """the operand shapes and dtypes of `beam_step`, on any backend; returns (rows b * w, vocabulary V, beams w)"""
    rows = pos.shape[0] if len(pos.shape) == 1 else -1
    V = logits.shape[-1] if len(logits.shape) in (2, 3) else -1
    assert int(num_beams) == num_beams and 1 <= num_beams <= 8, "beam_step: num_beams is an int within 1 .. 8 (got %s)" % (num_beams,)
    w = int(num_beams)
    shapes = [tuple(t.shape) for t in (logits, scores, parent, token, out_ids, pos, done, stats)]
    assert rows >= 1 and rows % w == 0 and V >= w and shapes[0] in ((rows, V), (rows, 1, V)) and shapes[1] == shapes[2] == shapes[6] == (rows,) \
        and shapes[3] == (rows, 1) and len(out_ids.shape) == 2 and out_ids.shape[0] == rows and out_ids.shape[1] >= 1 and shapes[7] == (2,), \
        "beam_step: logits (rows, V) or (rows, 1, V) with V >= num_beams = %d and rows a multiple of it, scores / parent / pos / done (rows,), " \
        "token (rows, 1), out_ids (rows, columns), stats (2,) - got %s" % (w, shapes)
    assert np.dtype(logits.dtype) == np.float32 and np.dtype(scores.dtype) == np.float32, "beam_step: logits and scores are float32"
    assert all(np.dtype(t.dtype) == np.int32 for t in (parent, token, out_ids, pos, done, stats)), \
        "beam_step: parent, token, out_ids, pos, done and stats are int32"
    assert eos is None or int(eos) == eos, "beam_step: eos is an int or None"
    return rows, V, w


CpuTensor.beam_step = _beam_step


def _kv_reorder(tensors, parent, pos, num_beams):
    """ CpuTensor.kv_reorder(tensors, parent, pos, num_beams): what nn.KVCache.reorder does - the definition.  tensors: (rows,
    capacity, width) arrays with rows = b * w; parent, pos (rows,) int32.  For each group g of w rows, L = max pos over the group
    (within 0 .. capacity): row n of the group becomes the old row parent[n] at cache positions j < L, in every tensor; positions
    >= L are not touched.  A parent outside its group leaves the group as it is and raises IndexError after the other groups have
    been moved.  One `take` per tensor and group. """
    rows, w = _check_kv_reorder(tensors, parent, pos, num_beams)
    capacity = tensors[0].shape[1]
    bad = []
    for lo in range(0, rows, w):
        src = parent.data[lo:lo + w].astype(np.int64)
        if ((src < lo) | (src >= lo + w)).any():
            bad.append(lo // w)
            continue
        L = int(np.clip(pos.data[lo:lo + w].max(), 0, capacity))
        if L == 0 or (src == np.arange(lo, lo + w)).all():
            continue
        for t in tensors:
            t.data[lo:lo + w, :L] = np.take(t.data[:, :L], src, axis=0)
    if bad:
        raise IndexError("kv_reorder: group %d (of %d that did) names a parent outside its own rows" % (bad[0], len(bad)))


def _check_kv_reorder(tensors, parent, pos, num_beams):
    """the operands of `kv_reorder`, on any backend; returns (rows, beams w)"""
    assert int(num_beams) == num_beams and 1 <= num_beams <= 8, "kv_reorder: num_beams is an int within 1 .. 8 (got %s)" % (num_beams,)
    w = int(num_beams)
    assert 1 <= len(tensors) <= 64, "kv_reorder: 1 .. 64 cache tensors in one call (got %d)" % len(tensors)
    shape = tuple(tensors[0].shape)
    rows = shape[0] if len(shape) == 3 else -1
    assert rows >= 1 and rows % w == 0 and all(tuple(t.shape) == shape and np.dtype(t.dtype) == np.float32 for t in tensors) \
        and tuple(parent.shape) == tuple(pos.shape) == (rows,) and np.dtype(parent.dtype) == np.dtype(pos.dtype) == np.int32, \
        "kv_reorder: float32 tensors of one shape (rows, capacity, width) with rows a multiple of num_beams = %d, parent and pos int32 (rows,) - got " \
        "%s, %s, %s" % (w, [tuple(t.shape) for t in tensors], tuple(parent.shape), tuple(pos.shape))
    return rows, w


CpuTensor.kv_reorder = staticmethod(_kv_reorder)


def _next_token_labels(ids, ignore_index=-100):
    """ ids.next_token_labels(ignore_index=-100): the labels of the next-token objective - `ids` shifted left by one along the last
    axis, `ignore_index` in the last column; same dtype and shape, a constant of the tape. """
    assert ids.dtype in (np.dtype(np.int32), np.dtype(np.int64)) and len(ids.shape) >= 1, \
        "next_token_labels: ids must be int32 or int64 with at least one axis (got %s %s)" % (ids.dtype, ids.shape)
    ignore_index = int(ignore_index)
    assert np.iinfo(ids.dtype).min <= ignore_index <= np.iinfo(ids.dtype).max, "next_token_labels: ignore_index does not fit %s" % ids.dtype
    labels = np.full(ids.shape, ignore_index, dtype=ids.dtype)
    labels[..., :-1] = ids.data[..., 1:]
    return CpuTensor.from_numpy(labels, requires_grad=False)


CpuTensor.next_token_labels = _next_token_labels


def _arg_extremum(name):
    np_fn = getattr(np, name)

    def method(t, axis=None, keepdims=False):
        return CpuTensor.from_numpy(np.asarray(np_fn(t.data, axis=axis, keepdims=keepdims), dtype=np.int64), requires_grad=False)
    method.__name__ = method.__qualname__ = name
    method.__doc__ = (""" t.%s(axis=None, keepdims=False) -> int64 indices, numpy's: the lowest index among equal extrema, the first NaN
    when the reduced run holds one, the row-major flattening of the view for axis=None.  A constant of the tape. """ % name)
    return method


CpuTensor.argmax, CpuTensor.argmin = _arg_extremum("argmax"), _arg_extremum("argmin")


""" Convolution (CNN example; reference cpu/ops.py:298-356) """


def _conv_strides(strides, n):
    """per-window-axis strides; the first window axis is the channel axis and always moves by 1"""
    if isinstance(strides, int):
        return (1,) + (strides,) * (n - 1) if n > 1 else (strides,)
    strides = tuple(strides)
    return (1,) + strides if len(strides) == n - 1 else strides


def _windows(x, kshape, strides):
    """read-only view of all `kshape` windows over the trailing len(kshape) axes: (..., out positions..., window...)"""
    n = len(kshape)
    out = tuple((d - k) // s + 1 for d, k, s in zip(x.shape[-n:], kshape, strides))
    st = x.strides[:-n] + tuple(a * s for a, s in zip(x.strides[-n:], strides)) + x.strides[-n:]
    return np.lib.stride_tricks.as_strided(x, shape=x.shape[:-n] + out + tuple(kshape), strides=st, writeable=False)


@_op()
class conv(Function):
    """ valid N-d cross-correlation: t (..., C, d1..dm), kernel (out_c, C, k1..km) -> (..., out_c, o1..om), computed as
    one matrix product of the window matrix with the flattened kernel; strides apply to the spatial axes """
    def forward(ctx, t, kernel, strides=1):
        n = kernel.ndim - 1
        st = _conv_strides(strides, n)
        assert t.ndim >= n and len(st) == n
        win = _windows(t, kernel.shape[1:], st)
        cols = win.reshape(-1, int(np.prod(kernel.shape[1:])))
        w2 = kernel.reshape(kernel.shape[0], -1)
        y = cols @ w2.T
        ctx.save_for_backward(cols, w2, t.shape, kernel.shape, st, win.shape)
        y = y.reshape(*win.shape[:-n], -1)                     # (..., o0, o1..om, out_c) with o0 the channel position (1)
        return np.ascontiguousarray(np.squeeze(np.swapaxes(y, -n - 1, -1), -1))

    def backward(ctx, out_grad):
        cols, w2, in_shape, k_shape, st, win_shape = ctx.get_saved_tensors()
        n = len(k_shape) - 1
        g2 = np.moveaxis(out_grad, -n, -1).reshape(-1, k_shape[0])
        dw = (g2.T @ cols).reshape(k_shape)
        dwin = (g2 @ w2).reshape(win_shape)
        dx = np.zeros(in_shape, dtype=CpuTensor.default_dtype)
        lead = len(in_shape) - n
        out_pos = win_shape[lead:lead + n]
        # every window offset contributes one strided slab of the input gradient (slabs of one offset never overlap)
        for off in np.ndindex(*k_shape[1:]):
            dst = (Ellipsis,) + tuple(slice(o, o + s * p, s) for o, s, p in zip(off, st, out_pos))
            dx[dst] += dwin[(Ellipsis,) + off]
        return dx, dw
