"""Fused attention of the HipTensor backend: `attention`, `masked_attention`, `long_attention`, `self_attention` and their
`*_supported` predicates over the lg_attention_* launches (csrc/attention.hip, csrc/attention_long.hip).

The library has four entry families - plain, masked, long, and the dropout pair that covers every length - and every op here
goes through the same two helpers, `_launch_attention_fwd` / `_launch_attention_bwd`: the op names its form, `dropout > 0`
takes the dropout entries instead.  That rule, and each symbol's name, stand here once.  `causal=True` on any op swaps the
forward launch for the causal entry (one for every form, with or without dropout); the backward launch stays the form's own.

`decode_attention` / `self_attention_decode` are the inference ops of incremental decoding: one new token against a key / value
cache, over lg_attention_decode_f32 (csrc/decode.hip).  They share nothing with the forms above and stay outside the tape.
"""
import ctypes
import numpy as np
from ..func import Function
from ..grads import Gradients
from ... import random as _random
from ... import guide as _guide
from .tensor import HipTensor, GradGroup, flush_lazy_readers
from . import lib as _l
from .ops import _F32, _require_f32, _dropout_base, linear

# form -> (length predicate, forward entry, backward entry) of the C ABI; "dropout" is no form of its own: see the helpers
_ENTRIES = {
    "plain": ("lg_attention_supported", "lg_attention_fwd_f32", "lg_attention_bwd_f32"),
    "masked": ("lg_attention_masked_supported", "lg_attention_masked_fwd_f32", "lg_attention_masked_bwd_f32"),
    "long": ("lg_attention_long_supported", "lg_attention_long_fwd_f32", "lg_attention_long_bwd_f32"),
    "dropout": ("lg_attention_dropout_supported", "lg_attention_dropout_fwd_f32", "lg_attention_dropout_bwd_f32"),
    # `causal=True`: one forward entry for every form, with or without dropout; the backward is the form's own (it reads P)
    "causal": ("lg_attention_causal_supported", "lg_attention_causal_fwd_f32", None),
}


def _fits(form, s, d):
    return bool(getattr(_l.lib(), _ENTRIES[form][0])(s, d))


def _token_rows(t):
    """(tensor, row pitch, batch pitch) of a (batch, positions, width) tensor whose rows the attention kernels can address as
    they lie: width contiguous, pitches multiples of 4, 16-byte aligned; anything else is copied once"""
    st, sh = t._strides, t._shape
    if st[2] != 1 or st[1] % 4 or st[0] % 4 or st[1] < sh[2] or t._byte_offset % 16:
        t = t.contiguous()
        st = t._strides
    return t, st[1], st[0]


def _attention_dropout(dropout):
    """the validated probability of an attention form's `dropout=`; 0.0 means the launches without it"""
    return _random.check_probability(dropout)


def _key_mask(mask, b, s, what):
    """(tensor kept alive, address, batch pitch) of a key-padding mask as the forward launches read it: float32, (b, s) or
    (1, s) - one row for the whole batch, pitch 0 -, rows contiguous (anything else is copied once), no gradient"""
    if mask is None:
        return None, None, 0
    assert isinstance(mask, HipTensor) and mask._dtype == _F32, "%s: the mask must be a float32 HipTensor, got %s" % (
        what, mask._dtype if isinstance(mask, HipTensor) else type(mask).__name__)
    assert not mask.requires_grad, "%s: the mask takes no gradient (requires_grad must be False)" % what
    assert mask._shape in ((b, s), (1, s)), "%s: mask of shape %s, expected (%d, %d) or (1, %d)" % (what, mask._shape, b, s, s)
    if (s > 1 and mask._strides[1] != 1) or (mask._shape[0] > 1 and mask._strides[0] < s):
        mask = mask.contiguous()
    return mask, mask.ptr, (0 if mask._shape[0] == 1 else mask._strides[0])


def _launch_attention_fwd(form, q3, k3, v3, out, probs, dims, scale, mask3, dropout, causal=False):
    """the forward launch of `form` ("plain", "masked" or "long"), or the dropout entry where dropout > 0; causal=True: the causal
    entry, which takes both.  q3, k3, v3: (address, row pitch, batch pitch); out (b, s, heads * d) and probs dense; dims =
    (b, heads, s, d); mask3 as `_key_mask` returns it.
    Returns the word the dropout launch wrote the call's number to, None without dropout."""
    b, heads, s, d = dims
    args = (*q3, *k3, *v3, out.ptr, heads * d, s * heads * d, probs.ptr, b, heads, s, d, scale)
    if causal:
        base = _dropout_base() if dropout > 0.0 else None
        _l.check(getattr(_l.lib(), _ENTRIES["causal"][1])(*args, mask3[1], mask3[2], dropout, None if base is None else base.ptr))
        return base
    if dropout > 0.0:
        base = _dropout_base()
        _l.check(getattr(_l.lib(), _ENTRIES["dropout"][1])(*args, mask3[1], mask3[2], dropout, base.ptr))
        return base
    if form != "plain":
        args += (mask3[1], mask3[2])
    _l.check(getattr(_l.lib(), _ENTRIES[form][1])(*args))
    return None


def _launch_attention_bwd(form, q3, k3, v3, g3, probs, dq3, dk3, dv3, dims, scale, dropout, base):
    """the backward launch that belongs to `_launch_attention_fwd(form, ...)`, whose result `base` is - causal or not: the
    probabilities carry the zeros; every operand as (address, row pitch, batch pitch)"""
    b, heads, s, d = dims
    args = (*q3, *k3, *v3, *g3, probs.ptr, *dq3, *dk3, *dv3, b, heads, s, d, scale)
    if base is not None:
        _l.check(getattr(_l.lib(), _ENTRIES["dropout"][2])(*args, dropout, base.ptr))
    else:
        _l.check(getattr(_l.lib(), _ENTRIES[form][2])(*args))


def _attention_supported(form, positive_batch, doc):
    def supported(q, heads, causal=False):
        return len(q._shape) == 3 and q._dtype == _F32 and q._shape[2] % heads == 0 and (not positive_batch or q._shape[0] > 0) and \
            _fits(form, q._shape[1], q._shape[2] // heads) and (not causal or _fits("causal", q._shape[1], q._shape[2] // heads))
    supported.__doc__ = doc
    return supported


def _attention_op(name, supported, form, takes_mask, doc):
    def forward(ctx, q, k, v, heads=1, scale=1.0, mask=None, dropout=0.0, causal=False):
        dropout = _attention_dropout(dropout)           # > 0: `probs.dropout(p)` inside the two launches
        _require_f32(q, k, v)
        assert q._shape == k._shape == v._shape and supported(q, heads, causal), \
            "%s: unsupported shapes %s / %s / %s with %d heads" % (name, q._shape, k._shape, v._shape, heads)
        b, s, width = q._shape
        dims = (b, heads, s, width // heads)
        mask3 = _key_mask(mask, b, s, name)
        (q, ldq, sbq), (k, ldk, sbk), (v, ldv, sbv) = _token_rows(q), _token_rows(k), _token_rows(v)
        out = HipTensor.empty((b, s, width))
        probs = HipTensor.empty((b, heads, s, s), requires_grad=False)
        base = _launch_attention_fwd(form, (q.ptr, ldq, sbq), (k.ptr, ldk, sbk), (v.ptr, ldv, sbv), out, probs, dims, float(scale), mask3, dropout,
                                     bool(causal))
        ctx.save_for_backward(q, k, v, probs, dims, float(scale), dropout, base)
        out.attention_probs = probs
        return out

    if not takes_mask:
        with_mask = forward

        def forward(ctx, q, k, v, heads=1, scale=1.0, dropout=0.0, causal=False):
            return with_mask(ctx, q, k, v, heads, scale, None, dropout, causal)

    def backward(ctx, out_grad):
        q, k, v, probs, dims, scale, dropout, base = ctx.get_saved_tensors()
        b, s, width = q._shape
        (q, ldq, sbq), (k, ldk, sbk), (v, ldv, sbv), (g, ldg, sbg) = _token_rows(q), _token_rows(k), _token_rows(v), _token_rows(out_grad)
        dq, dk, dv = HipTensor.empty((b, s, width)), HipTensor.empty((b, s, width)), HipTensor.empty((b, s, width))
        _launch_attention_bwd(form, (q.ptr, ldq, sbq), (k.ptr, ldk, sbk), (v.ptr, ldv, sbv), (g.ptr, ldg, sbg), probs,
                              (dq.ptr, width, s * width), (dk.ptr, width, s * width), (dv.ptr, width, s * width), dims, scale, dropout, base)
        return dq, dk, dv
    return HipTensor.register_op(name, type(name, (Function,), {"forward": forward, "backward": backward, "__doc__": doc}))


attention_supported = HipTensor.attention_supported = _attention_supported(
    "plain", False,
    """does `q.attention(k, v, heads, scale)` exist for this shape? (b, s, heads * d) with d = 32 or 64 and s = 32 .. 128 in 32s""")
masked_attention_supported = HipTensor.masked_attention_supported = _attention_supported(
    "masked", True,
    """does `q.masked_attention(k, v, heads, scale, mask)` exist for this shape? (b, s, heads * d) with d = 32 or 64 and ANY s in 1 .. 128""")
long_attention_supported = HipTensor.long_attention_supported = _attention_supported(
    "long", True,
    """does `q.long_attention(k, v, heads, scale, mask)` exist for this shape? (b, s, heads * d) with d = 32 or 64 and any s in 129 .. 512""")

attention = _attention_op(
    "attention", attention_supported, "plain", False,
    """ softmax((q k^T) * scale) v per head, forward and backward in one launch each (csrc/attention.hip); q, k, v are the
    (batch, positions, heads * d) outputs of the three projections as they stand - the head split of examples/bert.py:78-80
    happens in the kernels' addressing.  The probabilities (batch, heads, s, s) the reference model returns next to the context
    (bert.py:88) are on the result as `.attention_probs`, outside the tape (the composite form differentiates through them).
    dropout=p > 0: `probs.dropout(p)` between the softmax and the context inside the same two launches - the mask the composite
    draws (one call of the stream, lightgrad_amd/random.py); `.attention_probs` stays undropped.
    causal=True: query i sees keys j <= i only (the composite's `scores + (1 - tril) * -10000`); the forward is the causal launch
    (lg_attention_causal_fwd_f32), `.attention_probs` holds exact zeros above the diagonal and the backward is the same launch
    as without - here and in `masked_attention`, `long_attention` and `self_attention` """)
masked_attention = _attention_op(
    "masked_attention", masked_attention_supported, "masked", True,
    """ `attention` for what a tokenizer produces: any s in 1 .. 128 and a key-padding mask (reference examples/bert.py:80-83:
    `scores + (1.0 - mask) * -10000.0` before the softmax), forward and backward in one launch each (the TAIL kernels of
    csrc/attention.hip).  mask: float32 (b, s) or (1, s), no gradient, None for none.  A mask of ones gives the bits of `attention`.
    `.attention_probs` (b, heads, s, s) as there, outside the tape. """)
long_attention = _attention_op(
    "long_attention", long_attention_supported, "long", True,
    """ `masked_attention` for the lengths one CU's LDS does not hold a (batch, head) pair of: any s in 129 .. 512, with or without
    a key-padding mask, forward and backward still in one launch each (csrc/attention_long.hip: K, V, Q and dO stream through LDS
    in chunks).  mask: float32 (b, s) or (1, s), no gradient, None for none (the bits of a mask of ones).
    `.attention_probs` (b, heads, s, s) as there, outside the tape. """)


def self_attention_supported(x, wq, heads, masked=False, long=False, causal=False):
    """does `x.self_attention(wq, bq, wk, bk, wv, bv, heads, scale)` exist for these shapes?  (b, s, hidden) input, three
    (width, hidden) weights with width = heads * d, d = 32 or 64, width a multiple of 64, s = 32 .. 128 in 32s; masked=True:
    the same question for the form with `mask=` or a length that is no multiple of 32 - any s in 1 .. 128; long=True: the
    same question for the lengths beyond - any s in 129 .. 512, with or without a mask; causal=True: and with `causal=True`"""
    form = "long" if long else "masked" if masked else "plain"
    return (len(x._shape) == 3 and x._dtype == _F32 and len(wq._shape) == 2 and wq._shape[1] == x._shape[2] and wq._shape[0] % heads == 0
            and wq._shape[0] % 64 == 0 and x._shape[2] % 4 == 0 and x.numel() > 0
            and _fits(form, x._shape[1], wq._shape[0] // heads) and (not causal or _fits("causal", x._shape[1], wq._shape[0] // heads)))


def _ptr3(a, b, c):
    return (ctypes.c_void_p * 3)(a, b, c)


@HipTensor.register_op()
class self_attention(Function):
    """ the query / key / value projections and the attention over them as ONE tape node (reference examples/bert.py:78-88:
    three nn.Linear, scores, scaling, softmax, context): the three projections are one launch (lg_gemm_multi3_f32 - the weights
    stay the separately allocated parameters they are) into one (b, s, 3 * width) buffer that the attention kernel reads in
    place; backward: the attention kernel writes dq | dk | dv into one buffer of that shape, the input gradient is ONE product
    whose K runs through the three weights (lg_gemm_kseg3_f32, added to a gradient the input already holds in its epilogue),
    the weight / bias gradients take the routes of `linear`.  `.attention_probs` as for `attention`.  With a key-padding
    `mask` (as for `masked_attention`) or a length that is no multiple of 32 the attention launches are the masked / tail ones,
    beyond 128 positions (up to 512, mask or none) the long ones of csrc/attention_long.hip; everything else about the node is
    the same - also with causal=True, which only picks the causal forward launch of the attention. """
    def forward(ctx, x, wq, bq, wk, bk, wv, bv, heads=1, scale=1.0, mask=None, dropout=0.0, causal=False):
        dropout = _attention_dropout(dropout)           # > 0: `probs.dropout(p)` inside the attention launches, as for `attention`
        _require_f32(x, wq, bq, wk, bk, wv, bv)
        long = len(x._shape) == 3 and x._shape[1] > 128
        tail = mask is not None or (len(x._shape) == 3 and x._shape[1] % 32 != 0)
        assert self_attention_supported(x, wq, heads, masked=tail, long=long, causal=causal) and wq._shape == wk._shape == wv._shape and bq._shape == bk._shape == bv._shape == (wq._shape[0],), \
            "self_attention: unsupported shapes %s with weights %s / %s / %s and %d heads" % (x._shape, wq._shape, wk._shape, wv._shape, heads)
        form = "long" if long else "masked" if tail else "plain"
        b, s, hidden = x._shape
        width = wq._shape[0]
        x = x.contiguous()
        ws, bs = [w.contiguous() for w in (wq, wk, wv)], [t.contiguous() for t in (bq, bk, bv)]
        qkv = HipTensor.empty((b, s, 3 * width), requires_grad=False)
        base = qkv.ptr
        _l.check(_l.lib().lg_gemm_multi3_f32(0, 1, b * s, width, hidden, x.ptr, hidden, _ptr3(*(w.ptr for w in ws)), hidden,
                                             _ptr3(base, base + 4 * width, base + 8 * width), 3 * width, _ptr3(*(t.ptr for t in bs))))
        out = HipTensor.empty((b, s, width))
        probs = HipTensor.empty((b, heads, s, s), requires_grad=False)
        ld, sb = 3 * width, s * 3 * width
        mask3 = _key_mask(mask, b, s, "self_attention")
        drop_base = _launch_attention_fwd(form, (base, ld, sb), (base + 4 * width, ld, sb), (base + 8 * width, ld, sb), out, probs,
                                          (b, heads, s, width // heads), float(scale), mask3, dropout, bool(causal))
        ctx.save_for_backward(x, qkv, probs, heads, float(scale), form, dropout, drop_base)
        out.attention_probs = probs
        out.attention_qkv = qkv             # q | k | v as the projection launch wrote them (a key / value cache copies its rows from here)
        return out

    def backward(ctx, out_grad):
        x, qkv, probs, heads, scale, form, dropout, drop_base = ctx.get_saved_tensors()
        x_in = ctx._parents[0]
        params = ctx._parents[1:7]
        b, s, hidden = x._shape
        width = qkv._shape[2] // 3
        g, ldg, sbg = _token_rows(out_grad)
        dqkv = HipTensor.empty((b, s, 3 * width), requires_grad=False)
        base, dbase = qkv.ptr, dqkv.ptr
        ld, sb = 3 * width, s * 3 * width
        _launch_attention_bwd(form, (base, ld, sb), (base + 4 * width, ld, sb), (base + 8 * width, ld, sb), (g.ptr, ldg, sbg), probs,
                              (dbase, ld, sb), (dbase + 4 * width, ld, sb), (dbase + 8 * width, ld, sb),
                              (b, heads, s, width // heads), scale, dropout, drop_base)
        x2 = x.reshape(-1, hidden)
        grads = []
        for i in range(3):
            weight, bias = params[2 * i], params[2 * i + 1]
            gi = HipTensor(dqkv.data, (b * s, width), (3 * width, 1), dqkv._offset + i * width, _F32, requires_grad=False)
            want_db = bias.requires_grad
            acc_w = weight._grad_accumulator() if weight.requires_grad else None
            acc_w = acc_w if (acc_w is not None and acc_w.is_contiguous()) else None
            acc_b = bias._grad_accumulator() if want_db else None
            acc_b = acc_b if (acc_b is not None and acc_b.is_contiguous()) else None
            if acc_w is not None and (not want_db or acc_b is not None) and GradGroup.usable_for(weight, bias):
                with GradGroup.issue(reads=(gi, x2), writes=(acc_w, acc_b)):
                    grads += list(linear._weight_products(x2, weight, bias, want_db, gi, acc_w, acc_b))
            else:
                grads += list(linear._weight_products(x2, weight, bias, want_db, gi, acc_w, acc_b))
        dx = None
        if x_in.requires_grad:
            ws = [params[0].contiguous(), params[2].contiguous(), params[4].contiguous()]
            wptrs = _ptr3(*(w.ptr for w in ws))
            have = x_in._grad if (x_in._ctx is not None and x_in._view_of_leaf is None) else None
            if (have is not None and have.__class__ is HipTensor and have._shape == x_in._shape and have._dtype == _F32 and have.is_contiguous()):
                # the input already holds a contribution (the residual branch): added in this product's epilogue
                if x_in._grad_shared:
                    new = HipTensor.empty(x_in._shape, requires_grad=False)
                    _l.check(_l.lib().lg_gemm_kseg3_f32(0, 0, b * s, hidden, width, dbase, 3 * width, wptrs, hidden, new.ptr, hidden, 0,
                                                        have.ptr, hidden))
                    x_in._grad, x_in._grad_shared = new, False
                else:
                    flush_lazy_readers(have)
                    _l.check(_l.lib().lg_gemm_kseg3_f32(0, 0, b * s, hidden, width, dbase, 3 * width, wptrs, hidden, have.ptr, hidden, 1, None, 0))
            else:
                dx = HipTensor.empty(x_in._shape, requires_grad=False)
                _l.check(_l.lib().lg_gemm_kseg3_f32(0, 0, b * s, hidden, width, dbase, 3 * width, wptrs, hidden, dx.ptr, hidden, 0, None, 0))
        return (dx,) + tuple(grads)


HipTensor.self_attention_supported = self_attention_supported


""" Incremental decoding: one new token against a key / value cache (csrc/decode.hip) """

_I32 = np.dtype(np.int32)


def _inference_only(name, *operands):
    """the decode ops have no backward: outside `no_grad` they refuse operands that ask for a gradient"""
    if Gradients._is_enabled():
        for t in operands:
            assert t is None or not t.requires_grad, \
                "%s is an inference op (no backward): run it under Gradients.no_grad(), or pass operands with requires_grad=False" % name


def _token_row(t, name):
    """(tensor, batch pitch) of the new token's (b, 1, width) or (b, width) rows as the decode kernel addresses them: width
    contiguous, a batch pitch that is a multiple of 4, 16-byte aligned - a slice of a projection buffer is taken in place,
    anything else is copied once"""
    assert len(t._shape) in (2, 3) and (len(t._shape) == 2 or t._shape[1] == 1), "%s: expected (b, 1, width) or (b, width), got %s" % (name, t._shape)
    st = t._strides
    if (t._shape[-1] > 1 and st[-1] != 1) or (t._shape[0] > 1 and st[0] % 4) or t._byte_offset % 16:
        t = t.contiguous()
        st = t._strides
    return t, (st[0] if t._shape[0] > 1 else 0)


def _check_cache(name, k_cache, v_cache, pos, b, width):
    for c in (k_cache, v_cache):
        assert isinstance(c, HipTensor) and c._dtype == _F32 and len(c._shape) == 3 and c._shape[0] == b and c._shape[2] == width, \
            "%s: the caches are float32 (batch, capacity, width) = (%d, *, %d) tensors, got %s" % (name, b, width, getattr(c, "_shape", c))
        assert not c.requires_grad, "%s: a cache is state, not a parameter (requires_grad must be False)" % name
    assert k_cache._shape == v_cache._shape and k_cache._strides == v_cache._strides, "%s: the two caches must have one shape and one layout" % name
    # the kernel writes row t in place: a cache it cannot address as it lies is an error, never a copy
    st = k_cache._strides
    assert st[2] == 1 and st[1] % 4 == 0 and st[0] % 4 == 0 and st[1] >= width and k_cache._byte_offset % 16 == 0 and v_cache._byte_offset % 16 == 0, \
        "%s: cache rows must be contiguous and 16-byte aligned with pitches that are multiples of 4 (strides %s)" % (name, st)
    assert isinstance(pos, HipTensor) and pos._dtype == _I32 and (pos.numel() == 1 or pos._shape == (b,)), \
        "%s: pos is an int32 HipTensor of one element (one position for the batch) or of shape (batch,) = (%d,) (a position per sequence), got %s %s" % (
            name, b, getattr(pos, "_dtype", type(pos).__name__), getattr(pos, "_shape", ""))
    for c in (k_cache, v_cache):
        assert not _shares_bytes(pos, c), "%s: pos overlaps a cache (the launch writes the caches while it reads the positions)" % name


def _shares_bytes(x, y):
    """do two HipTensors of one allocation span common bytes?  (extents of the views, whatever their strides)"""
    if x._data is None or x._data is not y._data:
        return False
    def span(t):
        lo = hi = 0
        for n, st in zip(t._shape, t._strides):
            if n == 0:
                return t._byte_offset, t._byte_offset
            lo, hi = lo + min(0, (n - 1) * st), hi + max(0, (n - 1) * st)
        return t._byte_offset + lo * t._dtype.itemsize, t._byte_offset + (hi + 1) * t._dtype.itemsize
    (a0, a1), (b0, b1) = span(x), span(y)
    return a0 < b1 and b0 < a1


def _positions(pos, b):
    """(contiguous tensor, per-row?) of the position operand: one word keeps the one-word entry - at batch 1 the two mean the same -,
    (batch,) words take the `_rows` entry"""
    if pos.numel() == 1 or b == 1:
        return pos, False
    return (pos if pos._strides[0] == 1 else pos.contiguous()), True


def _launch_decode(name, q2, k2, v2, k_cache, v_cache, pos, out, heads, scale, mask, probs):
    """q2, k2, v2: (address, batch pitch); out: (b, ..., width) dense.  Returns the probabilities (b, heads, 1, capacity) or None"""
    b, capacity, width = k_cache._shape
    mask3 = _key_mask(mask, b, capacity, name)
    p = HipTensor.empty((b, heads, 1, capacity), requires_grad=False) if probs else None
    flush_lazy_readers(k_cache)
    flush_lazy_readers(v_cache)
    pos, per_row = _positions(pos, b)
    entry = _l.lib().lg_attention_decode_rows_f32 if per_row else _l.lib().lg_attention_decode_f32
    _l.check(entry(*q2, *k2, *v2, k_cache.ptr, v_cache.ptr, k_cache._strides[1], k_cache._strides[0], pos.ptr,
                   out.ptr, width, p.ptr if probs else None, b, heads, capacity, width // heads, float(scale), mask3[1], mask3[2]))
    return p


def decode_attention_supported(q, heads, capacity):
    """does `q.decode_attention(k_new, v_new, k_cache, v_cache, pos, heads, scale)` exist for this shape?  (b, 1, heads * d) or
    (b, heads * d) float32 with d = 32 or 64, b >= 1 and a cache of 1 .. 512 rows"""
    sh = q._shape
    return (len(sh) in (2, 3) and (len(sh) == 2 or sh[1] == 1) and q._dtype == _F32 and sh[0] > 0 and sh[-1] % heads == 0
            and bool(_l.lib().lg_attention_decode_supported(capacity, sh[-1] // heads)))


def decode_attention(q, k_new, v_new, k_cache, v_cache, pos, heads=1, scale=1.0, mask=None, probs=False):
    """ attention of ONE new token per sequence against a key / value cache, one launch (lg_attention_decode_f32): with t = the
    int32 word `pos` holds ON THE DEVICE (`pos` of shape (b,): a position per sequence, t = pos[r] for sequence r, everything
    below per sequence - lg_attention_decode_rows_f32; a sequence whose position is outside the cache writes nothing, the others
    are computed), k_new / v_new become row t of the caches (b, capacity, heads * d) and the result is
    softmax(scale * q K[0..t]^T + (1 - mask[0..t]) * -10000) V[0..t] per head - the row the causal forward computes for query t.
    q, k_new, v_new: (b, 1, width) or (b, width); slices of one (b, 1, 3 * width) projection buffer are read in place.  mask:
    float32 (b, capacity) or (1, capacity) over the cache's rows, None for none.  probs=True: `.attention_probs` (b, heads, 1,
    capacity), exact zeros beyond t.  A position outside the cache writes nothing and raises IndexError at the next
    synchronisation.  An inference op: the result is outside the tape. """
    name = "decode_attention"
    _inference_only(name, q, k_new, v_new)
    _require_f32(q, k_new, v_new)
    assert q._shape == k_new._shape == v_new._shape and decode_attention_supported(q, heads, k_cache._shape[1] if len(k_cache._shape) == 3 else 0), \
        "%s: unsupported shapes %s / %s / %s with %d heads and caches %s" % (name, q._shape, k_new._shape, v_new._shape, heads, k_cache._shape)
    _check_cache(name, k_cache, v_cache, pos, q._shape[0], q._shape[-1])
    (q, sbq), (k_new, sbk), (v_new, sbv) = _token_row(q, name), _token_row(k_new, name), _token_row(v_new, name)
    out = HipTensor.empty(q._shape, requires_grad=False)
    p = _launch_decode(name, (q.ptr, sbq), (k_new.ptr, sbk), (v_new.ptr, sbv), k_cache, v_cache, pos, out, heads, scale, mask, probs)
    if probs:
        out.attention_probs = p
    return out


def self_attention_decode(x, wq, bq, wk, bk, wv, bv, k_cache, v_cache, pos, heads=1, scale=1.0, mask=None, probs=False):
    """ the one-node form of a decode step's attention: the three projections of the new token in ONE launch (lg_gemm_multi3_f32,
    as in `self_attention`) into a (b, 1, 3 * width) buffer that the decode launch reads in place - two launches per layer.
    x: (b, 1, hidden); everything else as for `decode_attention`. """
    name = "self_attention_decode"
    _inference_only(name, x, wq, bq, wk, bk, wv, bv)
    _require_f32(x, wq, bq, wk, bk, wv, bv)
    assert self_attention_decode_supported(x, wq, heads, k_cache._shape[1] if len(k_cache._shape) == 3 else 0) and \
        wq._shape == wk._shape == wv._shape and bq._shape == bk._shape == bv._shape == (wq._shape[0],), \
        "%s: unsupported shapes %s with weights %s / %s / %s, %d heads and caches %s" % (name, x._shape, wq._shape, wk._shape, wv._shape, heads, k_cache._shape)
    b, _, hidden = x._shape
    width = wq._shape[0]
    _check_cache(name, k_cache, v_cache, pos, b, width)
    x = x.contiguous()
    ws, bs = [w.contiguous() for w in (wq, wk, wv)], [t.contiguous() for t in (bq, bk, bv)]
    qkv = HipTensor.empty((b, 1, 3 * width), requires_grad=False)
    base = qkv.ptr
    _l.check(_l.lib().lg_gemm_multi3_f32(0, 1, b, width, hidden, x.ptr, hidden, _ptr3(*(w.ptr for w in ws)), hidden,
                                         _ptr3(base, base + 4 * width, base + 8 * width), 3 * width, _ptr3(*(t.ptr for t in bs))))
    out = HipTensor.empty((b, 1, width), requires_grad=False)
    sb = 3 * width
    p = _launch_decode(name, (base, sb), (base + 4 * width, sb), (base + 8 * width, sb), k_cache, v_cache, pos, out, heads, scale, mask, probs)
    if probs:
        out.attention_probs = p
    return out


def self_attention_decode_supported(x, wq, heads, capacity):
    """does `x.self_attention_decode(...)` exist for these shapes?  (b, 1, hidden) input, (width, hidden) weights with width =
    heads * d, d = 32 or 64, width a multiple of 64, a cache of 1 .. 512 rows"""
    return (len(x._shape) == 3 and x._shape[1] == 1 and x._dtype == _F32 and len(wq._shape) == 2 and wq._shape[1] == x._shape[2]
            and wq._shape[0] % heads == 0 and wq._shape[0] % 64 == 0 and x._shape[2] % 4 == 0 and x._shape[0] > 0
            and bool(_l.lib().lg_attention_decode_supported(capacity, wq._shape[0] // heads)))


HipTensor.decode_attention, HipTensor.decode_attention_supported = decode_attention, decode_attention_supported
HipTensor.self_attention_decode, HipTensor.self_attention_decode_supported = self_attention_decode, self_attention_decode_supported


""" Appending several tokens to a filled key / value cache in one attention launch (csrc/extend.hip) """


def _token_rows_in_place(t, name):
    """(tensor, row pitch, batch pitch) of (b, m, width) rows as the extend kernel addresses them: width contiguous, pitches that
    are multiples of 4, 16-byte aligned - a slice of a projection buffer is taken in place, anything else is copied once"""
    assert len(t._shape) == 3, "%s: expected (b, m, width), got %s" % (name, t._shape)
    st = t._strides
    if (t._shape[2] > 1 and st[2] != 1) or (t._shape[1] > 1 and (st[1] % 4 or st[1] < 0)) or (t._shape[0] > 1 and (st[0] % 4 or st[0] < 0)) \
            or t._byte_offset % 16:
        t = t.contiguous()
        st = t._strides
    return t, (st[1] if t._shape[1] > 1 else 0), (st[0] if t._shape[0] > 1 else 0)


def _token_counts(name, count, pos, b, k_cache, v_cache):
    """the `count=` operand of the extend ops as the launch reads it: int32 (b,) next to a `pos` of shape (b,), dense, apart
    from the caches and from pos"""
    assert isinstance(count, HipTensor) and count._dtype == _I32 and count._shape == (b,) and pos._shape == (b,), \
        "%s: count is an int32 HipTensor of shape (batch,) = (%d,) and goes with a pos of that shape, got count %s %s and pos %s" % (
            name, b, getattr(count, "_dtype", type(count).__name__), getattr(count, "_shape", ""), pos._shape)
    for other in (k_cache, v_cache, pos):
        assert not _shares_bytes(count, other), "%s: count overlaps a cache or pos" % name
    return count if b == 1 or count._strides[0] == 1 else count.contiguous()


def _launch_extend(name, q3, k3, v3, m, k_cache, v_cache, pos, out, heads, scale, mask, probs, count=None):
    """q3, k3, v3: (address, row pitch, batch pitch); out: (b, m, width) dense.  Returns the probabilities (b, heads, m, capacity) or None"""
    b, capacity, width = k_cache._shape
    if count is not None:
        count = _token_counts(name, count, pos, b, k_cache, v_cache)
    mask3 = _key_mask(mask, b, capacity, name)
    p = HipTensor.empty((b, heads, m, capacity), requires_grad=False) if probs else None
    flush_lazy_readers(k_cache)
    flush_lazy_readers(v_cache)
    if count is not None:
        # a token count per sequence next to its position: the counts entry, at any batch
        pos = pos if b == 1 or pos._strides[0] == 1 else pos.contiguous()
        entry, words = _l.lib().lg_attention_extend_counts_f32, (pos.ptr, count.ptr)
    else:
        pos, per_row = _positions(pos, b)
        entry, words = (_l.lib().lg_attention_extend_rows_f32 if per_row else _l.lib().lg_attention_extend_f32), (pos.ptr,)
    _l.check(entry(*q3, *k3, *v3, k_cache.ptr, v_cache.ptr, k_cache._strides[1], k_cache._strides[0], *words,
                   out.ptr, width, m * width, p.ptr if probs else None, b, heads, m, capacity, width // heads, float(scale), mask3[1], mask3[2]))
    return p


def _packed_rows(name, cu, count, pos, rows, k_cache, v_cache, m_max):
    """the `cu=` operand of the extend ops as the packed launch reads it, and the largest piece: (cu, slots, m_max).  int32
    (slots + 1,) next to flat (1, T, .) token rows, caches of `slots` rows and a `pos` of shape (slots,); dense, apart from the
    caches and from pos"""
    assert count is None, "%s: cu= (token-packed rows) and count= (a count per batch row) exclude each other" % name
    slots, capacity = k_cache._shape[0], k_cache._shape[1]
    assert isinstance(cu, HipTensor) and cu._dtype == _I32 and cu._shape == (slots + 1,) and pos._shape == (slots,) and rows[0] == 1, \
        "%s: cu is an int32 HipTensor of shape (slots + 1,) = (%d,) and goes with token rows (1, T, .) and a pos of shape (slots,), got cu %s %s, rows %s and pos %s" % (
            name, slots + 1, getattr(cu, "_dtype", type(cu).__name__), getattr(cu, "_shape", ""), rows, pos._shape)
    for other in (k_cache, v_cache, pos):
        assert not _shares_bytes(cu, other), "%s: cu overlaps a cache or pos" % name
    m_max = min(rows[1], capacity) if m_max is None else int(m_max)
    assert 1 <= m_max <= capacity, "%s: m_max = %d outside 1 .. capacity = %d" % (name, m_max, capacity)
    return (cu if cu._strides[0] == 1 else cu.contiguous()), slots, m_max


def _launch_extend_packed(name, q2, k2, v2, T, k_cache, v_cache, pos, cu, m_max, out, heads, scale, mask, probs):
    """q2, k2, v2: (address, row pitch) of flat (T, width) rows; out: (1, T, width) dense.  Returns the probabilities
    (heads, T, capacity) or None"""
    slots, capacity, width = k_cache._shape
    mask3 = _key_mask(mask, slots, capacity, name)
    p = HipTensor.empty((heads, T, capacity), requires_grad=False) if probs else None
    flush_lazy_readers(k_cache)
    flush_lazy_readers(v_cache)
    pos = pos if slots == 1 or pos._strides[0] == 1 else pos.contiguous()
    _l.check(_l.lib().lg_attention_extend_packed_f32(*q2, *k2, *v2, k_cache.ptr, v_cache.ptr, k_cache._strides[1], k_cache._strides[0], pos.ptr, cu.ptr,
                                                     out.ptr, width, p.ptr if probs else None, slots, heads, T, m_max, capacity, width // heads,
                                                     float(scale), mask3[1], mask3[2]))
    return p


_I16 = np.dtype(np.int16)


def _block_table(name, block_table, block_size, count, pos, rows, k_pool, v_pool, kv_dtype=None):
    """the `block_table=` / `block_size=` operands of the extend ops as the paged launch reads them: (table, B).  int32 (b, max_blocks)
    next to (b, m, width) token rows, pools (num_blocks, B, width), a count and a pos of shape (b,); dense, apart from the pools, pos
    and count.  kv_dtype: None - float32 pools -, or "bf16" - int16 pools of bfloat16 words; each form refuses the other's pools"""
    assert kv_dtype in (None, "bf16"), "%s: kv_dtype is None (float32 pools) or \"bf16\" (int16 pools of bfloat16 words), got %r" % (name, kv_dtype)
    for c in (k_pool, v_pool):
        if isinstance(c, HipTensor) and c._dtype == _I16 and kv_dtype is None:
            raise TypeError("%s: int16 pools hold bfloat16 words and go with kv_dtype=\"bf16\" (lg_attention_extend_paged_bf16_f32); "
                            "without the keyword the pools are float32" % name)
        if isinstance(c, HipTensor) and c._dtype == _F32 and kv_dtype == "bf16":
            raise TypeError("%s: kv_dtype=\"bf16\" takes int16 pools of bfloat16 words (nn.PagedKVCache(..., kv_dtype=\"bf16\")); float32 pools "
                            "go without the keyword (lg_attention_extend_paged_f32)" % name)
    pool_dtype, align = (_I16, 8) if kv_dtype == "bf16" else (_F32, 16)
    assert block_table is not None and block_size is not None and count is not None, \
        "%s: a paged cache takes block_table=, block_size= and count= together" % name
    B = int(block_size)
    assert B == block_size and 4 <= B <= 128 and B & (B - 1) == 0, "%s: block_size is a power of two within 4 .. 128, got %s" % (name, block_size)
    b, width = rows[0], rows[2]
    assert isinstance(block_table, HipTensor) and block_table._dtype == _I32 and len(block_table._shape) == 2 and block_table._shape[0] == b \
        and 1 <= block_table._shape[1] and block_table._shape[1] * B <= 512, \
        "%s: block_table is an int32 HipTensor (batch, max_blocks) = (%d, *) with max_blocks * block_size <= 512, got %s %s" % (
            name, b, getattr(block_table, "_dtype", type(block_table).__name__), getattr(block_table, "_shape", ""))
    for c in (k_pool, v_pool):
        assert isinstance(c, HipTensor) and c._dtype == pool_dtype and len(c._shape) == 3 and c._shape[0] >= 1 and c._shape[1] == B and c._shape[2] == width, \
            "%s: the pools are %s (num_blocks, block_size, width) = (*, %d, %d) tensors, got %s" % (name, pool_dtype, B, width, getattr(c, "_shape", c))
        assert not c.requires_grad, "%s: a cache is state, not a parameter (requires_grad must be False)" % name
    assert k_pool._shape == v_pool._shape and k_pool._strides == v_pool._strides, "%s: the two pools must have one shape and one layout" % name
    st = k_pool._strides
    # the kernel writes rows in place and addresses the pool as (num_blocks * B) rows of one pitch
    assert st[2] == 1 and st[1] % 4 == 0 and st[1] >= width and (k_pool._shape[0] == 1 or st[0] == B * st[1]) and k_pool._byte_offset % align == 0 \
        and v_pool._byte_offset % align == 0, "%s: pool rows must be contiguous, %d-byte aligned and of one pitch across the blocks (strides %s)" % (name, align, st)
    assert isinstance(pos, HipTensor) and pos._dtype == _I32 and pos._shape == (b,), "%s: a paged cache takes an int32 pos of shape (batch,) = (%d,)" % (name, b)
    count = _token_counts(name, count, pos, b, k_pool, v_pool)
    assert not _shares_bytes(k_pool, v_pool), "%s: the two pools overlap" % name
    for other in (k_pool, v_pool, pos, count):
        assert not _shares_bytes(block_table, other), "%s: block_table overlaps a pool, pos or count" % name
        assert other is count or other is pos or not _shares_bytes(pos, other), "%s: pos overlaps a pool" % name
    return (block_table if block_table.is_contiguous() else block_table.contiguous()), B


def _launch_extend_paged(name, q3, k3, v3, m, k_pool, v_pool, pos, count, block_table, B, out, heads, scale, mask, probs):
    """q3, k3, v3: (address, row pitch, batch pitch); out: (b, m, width) dense.  Returns the probabilities (b, heads, m, capacity) or None.
    int16 pools (bfloat16 words; `_block_table` has matched them with kv_dtype=) take the bf16 entry, the same argument list"""
    b, max_blocks = block_table._shape
    num_blocks, _, width = k_pool._shape
    capacity = max_blocks * B
    count = count if b == 1 or count._strides[0] == 1 else count.contiguous()
    pos = pos if b == 1 or pos._strides[0] == 1 else pos.contiguous()
    mask3 = _key_mask(mask, b, capacity, name)
    p = HipTensor.empty((b, heads, m, capacity), requires_grad=False) if probs else None
    flush_lazy_readers(k_pool)
    flush_lazy_readers(v_pool)
    entry = _l.lib().lg_attention_extend_paged_bf16_f32 if k_pool._dtype == _I16 else _l.lib().lg_attention_extend_paged_f32
    _l.check(entry(*q3, *k3, *v3, k_pool.ptr, v_pool.ptr, k_pool._strides[1], pos.ptr, count.ptr, block_table.ptr,
                   out.ptr, width, m * width, p.ptr if probs else None, b, heads, m, max_blocks, num_blocks,
                   B.bit_length() - 1, width // heads, float(scale), mask3[1], mask3[2]))
    return p


def extend_attention_supported(q, heads, capacity, m_max=None):
    """(m_max: the call is token-packed - `cu=` -: (1, T, heads * d) rows with any T >= 1 and pieces of at most m_max, default
    min(T, capacity))
    does `q.extend_attention(k_new, v_new, k_cache, v_cache, pos, heads, scale)` exist for this shape?  (b, m, heads * d) float32
    with d = 32 or 64, b >= 1 and 1 <= m <= capacity <= 512"""
    sh = q._shape
    return (len(sh) == 3 and q._dtype == _F32 and sh[0] > 0 and sh[2] % heads == 0
            and bool(_l.lib().lg_attention_extend_supported(sh[1] if m_max is None else m_max, capacity, sh[2] // heads)))


def extend_attention(q, k_new, v_new, k_cache, v_cache, pos, heads=1, scale=1.0, mask=None, probs=False, count=None, cu=None, m_max=None,
                     block_table=None, block_size=None, kv_dtype=None):
    """ attention of m NEW tokens per sequence against a filled key / value cache, one launch (lg_attention_extend_f32): with t =
    the int32 word `pos` holds ON THE DEVICE (`pos` of shape (b,): a position per sequence, t = pos[r] for sequence r, everything
    below per sequence - lg_attention_extend_rows_f32; a sequence with t + m beyond the cache writes nothing, the others are computed), rows i of k_new / v_new become rows t + i of the caches (b, capacity, heads * d) and
    row i of the result is softmax(scale * q_i K[0..t+i]^T + (1 - mask[0..t+i]) * -10000) V[0..t+i] per head - the rows the causal
    forward computes for queries t .. t + m - 1.  q, k_new, v_new: (b, m, width); slices of one (b, m, 3 * width) projection
    buffer are read in place.  mask: float32 (b, capacity) or (1, capacity) over the cache's rows, None for none.  probs=True:
    `.attention_probs` (b, heads, m, capacity), exact zeros beyond column t + i of row i.  t < 0 or t + m > capacity writes
    nothing and raises IndexError at the next synchronisation.  An inference op: the result is outside the tape.
    count= (an int32 HipTensor (b,), with a per-sequence `pos`): sequence r has n = count[r] real tokens among its m rows - one
    launch of lg_attention_extend_counts_f32.  Its rows < n are those of the call on it alone with m = n, only cache rows
    t .. t + n - 1 are written, only t + n has to fit the cache (n = 0: an idle sequence), and rows >= n of the result and of
    `.attention_probs` are +0.0.  Without count= the call is the one it was.
    cu= (an int32 HipTensor (slots + 1,), with a `pos` of shape (slots,) and caches of `slots` rows): the call is TOKEN-PACKED - one
    launch of lg_attention_extend_packed_f32.  q, k_new, v_new are (1, T, width), the step's tokens of all slots; slot s owns rows
    cu[s] .. cu[s + 1] - 1 (at most m_max= of them, default min(T, capacity); T may exceed the capacity) and is computed as by the
    call on those rows alone against its own cache rows at t = pos[s]; rows >= cu[slots] of the result are +0.0.
    `.attention_probs` is (heads, T, capacity); mask is (slots, capacity) or (1, capacity).  cu= and count= exclude each other.
    Without cu= the call is the one it was.
    block_table= (an int32 HipTensor (b, max_blocks)) with block_size= B (a power of two, 4 .. 128) and count=: the cache is PAGED -
    one launch of lg_attention_extend_paged_f32.  k_cache / v_cache are pools (num_blocks, B, width) and position j of sequence r
    is row j % B of block block_table[r, j // B]; capacity = max_blocks * B.  Sequence r is computed bit for bit as the count=
    call computes it on a contiguous cache that holds the same rows.  A word outside 0 .. num_blocks - 1 among the first
    ceil((t + n) / B) of a row makes that sequence write nothing and raises IndexError at the next synchronisation; the words
    behind are not used.  Without block_table= the call is the one it was.
    kv_dtype="bf16" (with block_table=): the pools are int16 tensors of BFLOAT16 words - one launch of
    lg_attention_extend_paged_bf16_f32.  With r = `bf16_round_array`, the result (and `.attention_probs`) is bit for bit that of
    the paged call on r(k_new), r(v_new) and `bf16_widen` of the pools, and the new rows are stored as `bf16_bits`: a key counts as
    r of it whichever call brought it in; q is not rounded.  int16 pools without the keyword, or the keyword with float32 pools,
    are a TypeError. """
    name = "extend_attention"
    _inference_only(name, q, k_new, v_new)
    _require_f32(q, k_new, v_new)
    assert kv_dtype is None or block_table is not None, "%s: kv_dtype= goes with a paged cache (block_table=, block_size=, count=): the contiguous " \
        "caches are float32" % name
    if block_table is not None or block_size is not None:
        assert cu is None and m_max is None, "%s: block_table= (a paged cache) goes with count=, not with cu= (token-packed rows)" % name
        block_table, B = _block_table(name, block_table, block_size, count, pos, q._shape, k_cache, v_cache, kv_dtype)
        capacity = block_table._shape[1] * B
        assert q._shape == k_new._shape == v_new._shape and extend_attention_supported(q, heads, capacity), \
            "%s: unsupported shapes %s / %s / %s with %d heads and a paged cache of %d positions" % (name, q._shape, k_new._shape, v_new._shape, heads, capacity)
        m = q._shape[1]
        (q, ldq, sbq), (k_new, ldk, sbk), (v_new, ldv, sbv) = (_token_rows_in_place(t, name) for t in (q, k_new, v_new))
        out = HipTensor.empty(q._shape, requires_grad=False)
        p = _launch_extend_paged(name, (q.ptr, ldq, sbq), (k_new.ptr, ldk, sbk), (v_new.ptr, ldv, sbv), m, k_cache, v_cache, pos, count, block_table, B, out,
                                 heads, scale, mask, probs)
        if probs:
            out.attention_probs = p
        return out
    if cu is not None:
        assert len(k_cache._shape) == 3 and len(q._shape) == 3, "%s: expected (1, T, width) rows and (slots, capacity, width) caches" % name
        cu, slots, m_max = _packed_rows(name, cu, count, pos, q._shape, k_cache, v_cache, m_max)
        assert q._shape == k_new._shape == v_new._shape and extend_attention_supported(q, heads, k_cache._shape[1], m_max), \
            "%s: unsupported shapes %s / %s / %s with %d heads and caches %s" % (name, q._shape, k_new._shape, v_new._shape, heads, k_cache._shape)
        _check_cache(name, k_cache, v_cache, pos, slots, q._shape[2])
        T = q._shape[1]
        (q, ldq, _), (k_new, ldk, _), (v_new, ldv, _) = (_token_rows_in_place(t, name) for t in (q, k_new, v_new))
        width = q._shape[2]
        out = HipTensor.empty(q._shape, requires_grad=False)
        p = _launch_extend_packed(name, (q.ptr, ldq if T > 1 else width), (k_new.ptr, ldk if T > 1 else width), (v_new.ptr, ldv if T > 1 else width), T,
                                  k_cache, v_cache, pos, cu, m_max, out, heads, scale, mask, probs)
        if probs:
            out.attention_probs = p
        return out
    assert m_max is None, "%s: m_max= goes with cu=" % name
    assert q._shape == k_new._shape == v_new._shape and extend_attention_supported(q, heads, k_cache._shape[1] if len(k_cache._shape) == 3 else 0), \
        "%s: unsupported shapes %s / %s / %s with %d heads and caches %s" % (name, q._shape, k_new._shape, v_new._shape, heads, k_cache._shape)
    _check_cache(name, k_cache, v_cache, pos, q._shape[0], q._shape[2])
    m = q._shape[1]
    (q, ldq, sbq), (k_new, ldk, sbk), (v_new, ldv, sbv) = (_token_rows_in_place(t, name) for t in (q, k_new, v_new))
    out = HipTensor.empty(q._shape, requires_grad=False)
    p = _launch_extend(name, (q.ptr, ldq, sbq), (k_new.ptr, ldk, sbk), (v_new.ptr, ldv, sbv), m, k_cache, v_cache, pos, out, heads, scale, mask, probs,
                       **({} if count is None else {"count": count}))
    if probs:
        out.attention_probs = p
    return out


def self_attention_extend(x, wq, bq, wk, bk, wv, bv, k_cache, v_cache, pos, heads=1, scale=1.0, mask=None, probs=False, count=None, cu=None,
                          m_max=None, block_table=None, block_size=None, kv_dtype=None):
    """ the one-node form of an append's attention: the three projections of the m new tokens in ONE launch (lg_gemm_multi3_f32,
    as in `self_attention`) into a (b, m, 3 * width) buffer that the extend launch reads in place - two launches per layer.
    x: (b, m, hidden); everything else as for `extend_attention`, `count=` included (the projections take all b * m rows) and
    `cu=` / `m_max=` too: x is (1, T, hidden) then, the projection launch runs on the T rows, the packed launch reads them in place.
    block_table= / block_size= with count=: the caches are pools and the second launch is the paged one - still two per layer;
    kv_dtype="bf16": int16 pools of bfloat16 words, the second launch is lg_attention_extend_paged_bf16_f32 (see `extend_attention`). """
    name = "self_attention_extend"
    _inference_only(name, x, wq, bq, wk, bk, wv, bv)
    _require_f32(x, wq, bq, wk, bk, wv, bv)
    assert cu is not None or m_max is None, "%s: m_max= goes with cu=" % name
    assert kv_dtype is None or block_table is not None, "%s: kv_dtype= goes with a paged cache (block_table=, block_size=, count=): the contiguous " \
        "caches are float32" % name
    paged = block_table is not None or block_size is not None
    if paged:
        assert cu is None, "%s: block_table= (a paged cache) goes with count=, not with cu= (token-packed rows)" % name
        assert len(x._shape) == 3 and len(wq._shape) == 2, "%s: expected (b, m, hidden) rows and (width, hidden) weights" % name
        block_table, B = _block_table(name, block_table, block_size, count, pos, (x._shape[0], x._shape[1], wq._shape[0]), k_cache, v_cache, kv_dtype)
        assert self_attention_extend_supported(x, wq, heads, block_table._shape[1] * B) and \
            wq._shape == wk._shape == wv._shape and bq._shape == bk._shape == bv._shape == (wq._shape[0],), \
            "%s: unsupported shapes %s with weights %s / %s / %s, %d heads and a paged cache of %d positions" % (
                name, x._shape, wq._shape, wk._shape, wv._shape, heads, block_table._shape[1] * B)
        b, m, hidden = x._shape
        width = wq._shape[0]
        x = x.contiguous()
        ws, bs = [w.contiguous() for w in (wq, wk, wv)], [t.contiguous() for t in (bq, bk, bv)]
        qkv = HipTensor.empty((b, m, 3 * width), requires_grad=False)
        base = qkv.ptr
        _l.check(_l.lib().lg_gemm_multi3_f32(0, 1, b * m, width, hidden, x.ptr, hidden, _ptr3(*(w.ptr for w in ws)), hidden,
                                             _ptr3(base, base + 4 * width, base + 8 * width), 3 * width, _ptr3(*(t.ptr for t in bs))))
        out = HipTensor.empty((b, m, width), requires_grad=False)
        ld, sb = 3 * width, m * 3 * width
        p = _launch_extend_paged(name, (base, ld, sb), (base + 4 * width, ld, sb), (base + 8 * width, ld, sb), m, k_cache, v_cache, pos, count, block_table,
                                 B, out, heads, scale, mask, probs)
        if probs:
            out.attention_probs = p
        return out
    if cu is not None:
        assert len(k_cache._shape) == 3 and len(x._shape) == 3, "%s: expected (1, T, hidden) rows and (slots, capacity, width) caches" % name
        cu, slots, m_max = _packed_rows(name, cu, count, pos, x._shape, k_cache, v_cache, m_max)
    assert self_attention_extend_supported(x, wq, heads, k_cache._shape[1] if len(k_cache._shape) == 3 else 0, m_max) and \
        wq._shape == wk._shape == wv._shape and bq._shape == bk._shape == bv._shape == (wq._shape[0],), \
        "%s: unsupported shapes %s with weights %s / %s / %s, %d heads and caches %s" % (name, x._shape, wq._shape, wk._shape, wv._shape, heads, k_cache._shape)
    b, m, hidden = x._shape
    width = wq._shape[0]
    _check_cache(name, k_cache, v_cache, pos, b if cu is None else slots, width)
    x = x.contiguous()
    ws, bs = [w.contiguous() for w in (wq, wk, wv)], [t.contiguous() for t in (bq, bk, bv)]
    qkv = HipTensor.empty((b, m, 3 * width), requires_grad=False)
    base = qkv.ptr
    _l.check(_l.lib().lg_gemm_multi3_f32(0, 1, b * m, width, hidden, x.ptr, hidden, _ptr3(*(w.ptr for w in ws)), hidden,
                                         _ptr3(base, base + 4 * width, base + 8 * width), 3 * width, _ptr3(*(t.ptr for t in bs))))
    out = HipTensor.empty((b, m, width), requires_grad=False)
    ld, sb = 3 * width, m * 3 * width
    if cu is not None:
        p = _launch_extend_packed(name, (base, ld), (base + 4 * width, ld), (base + 8 * width, ld), m, k_cache, v_cache, pos, cu, m_max, out, heads,
                                  scale, mask, probs)
        if probs:
            out.attention_probs = p
        return out
    p = _launch_extend(name, (base, ld, sb), (base + 4 * width, ld, sb), (base + 8 * width, ld, sb), m, k_cache, v_cache, pos, out, heads, scale,
                       mask, probs, **({} if count is None else {"count": count}))
    if probs:
        out.attention_probs = p
    return out


def self_attention_extend_supported(x, wq, heads, capacity, m_max=None):
    """(m_max: the call is token-packed - `cu=` -: x is (1, T, hidden) with any T >= 1 and pieces of at most m_max)
    does `x.self_attention_extend(...)` exist for these shapes?  (b, m, hidden) input, (width, hidden) weights with width =
    heads * d, d = 32 or 64, width a multiple of 64, 1 <= m <= capacity <= 512"""
    return (len(x._shape) == 3 and x._dtype == _F32 and len(wq._shape) == 2 and wq._shape[1] == x._shape[2]
            and wq._shape[0] % heads == 0 and wq._shape[0] % 64 == 0 and x._shape[2] % 4 == 0 and x._shape[0] > 0
            and (m_max is None or x._shape[0] == 1)
            and bool(_l.lib().lg_attention_extend_supported(x._shape[1] if m_max is None else m_max, capacity, wq._shape[0] // heads)))


HipTensor.extend_attention, HipTensor.extend_attention_supported = extend_attention, extend_attention_supported
HipTensor.self_attention_extend, HipTensor.self_attention_extend_supported = self_attention_extend, self_attention_extend_supported


""" The per-row bookkeeping of a decode step in one launch (csrc/commit.hip) """


def decode_commit(nxt, token, out_ids, pos, done, eos=None):
    """ nxt.decode_commit(token, out_ids, pos, done, eos=None): what `CpuTensor.decode_commit` defines, in ONE launch
    (lg_decode_commit_i32), in place and outside the tape.  For each row r with done[r] == 0: p = pos[r] + 1; pos[r] = p,
    token[r] = nxt[r], out_ids[r, p] = nxt[r], and done[r] = 1 if `eos` is an id >= 0 that nxt[r] equals; a row with done[r] != 0
    is not touched.  nxt (b,) or (b, 1), token (b, 1), out_ids (b, columns) with any row pitch, pos (b,), done (b,): int32
    HipTensors that do not overlap.  A live row whose p is no column of out_ids keeps its bytes and raises IndexError at the next
    synchronisation.  No host read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_decode_commit
    name = "decode_commit"
    assert all(isinstance(t, HipTensor) for t in (nxt, token, out_ids, pos, done)), "%s: every operand is a HipTensor" % name
    b = _check_decode_commit(nxt, token, out_ids, pos, done, eos)
    columns = out_ids._shape[1]
    if b > 1 and nxt._strides[0] < 1:
        nxt = nxt.contiguous()
    # the launch writes these where they lie: a layout it cannot address is an error, never a copy
    assert (b == 1 or (token._strides[0] == 1 and pos._strides[0] == 1 and done._strides[0] == 1)) and (columns == 1 or out_ids._strides[1] == 1) \
        and (b == 1 or out_ids._strides[0] >= columns), "%s: token, pos and done must be dense and the rows of out_ids contiguous" % name
    written = (token, out_ids, pos, done)
    for i, x in enumerate(written):
        assert not _shares_bytes(nxt, x), "%s: nxt overlaps an operand that is written" % name
        for y in written[i + 1:]:
            assert not _shares_bytes(x, y), "%s: two of token, out_ids, pos and done overlap" % name
        flush_lazy_readers(x)
    _l.check(_l.lib().lg_decode_commit_i32(nxt.ptr, nxt._strides[0] if b > 1 else 1, token.ptr, out_ids.ptr, out_ids._strides[0] if b > 1 else columns,
                                           columns, pos.ptr, done.ptr, b, -1 if eos is None else int(eos)))


HipTensor.decode_commit = decode_commit


""" The slot bookkeeping of a serving step in one launch (csrc/serve.hip) """


def _serve_commit_operands(name, b, N, reads, written, dense):
    """the operands of a commit launch as it addresses them.  reads = (nxt, prompts, prompt_len, budget): what is only read may be
    copied once into a layout the launch takes; written = (out, out_len, queue, req, pos, count, ...): the launch writes these
    where they lie, so a layout it cannot address is an error, never a copy - the rows of out contiguous at any pitch, every other
    one dense (`dense` names them for the message).  No two operands share bytes.  Returns the leading arguments all three
    lg_serve_commit*_i32 entries take, nxt .. count."""
    nxt, prompts, prompt_len, budget = reads
    out, out_len, queue, req, pos, count = written[:6]
    P, G = prompts._shape[1], out._shape[1]
    if b > 1 and nxt._strides[0] < 1:
        nxt = nxt.contiguous()
    if (P > 1 and prompts._strides[1] != 1) or (N > 1 and prompts._strides[0] < P):
        prompts = prompts.contiguous()
    prompt_len, budget = (t if N == 1 or t._strides[0] == 1 else t.contiguous() for t in (prompt_len, budget))
    assert all(t.is_contiguous() for t in written[1:]) and (G == 1 or out._strides[1] == 1) and (N == 1 or out._strides[0] >= G), \
        "%s: %s must be dense and the rows of out contiguous" % (name, dense)
    operands = (nxt, prompts, prompt_len, budget) + written
    for i, x in enumerate(operands):
        for y in operands[i + 1:]:
            assert not _shares_bytes(x, y), "%s: two operands overlap" % name
    for x in written:
        flush_lazy_readers(x)
    return (nxt.ptr, nxt._strides[0] if b > 1 else 1, prompts.ptr, prompts._strides[0] if N > 1 else P, P, prompt_len.ptr, budget.ptr,
            out.ptr, out._strides[0] if N > 1 else G, G, out_len.ptr, queue.ptr, N, req.ptr, pos.ptr, count.ptr)


def serve_commit(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity, eos=None):
    """ nxt.serve_commit(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, capacity,
    eos=None): what `CpuTensor.serve_commit` defines - a finished slot freed, the next waiting request admitted to it, the next
    piece of a prompt or the token just drawn made the step's input - in ONE launch (lg_serve_commit_i32), in place and outside the
    tape.  Int32 HipTensors that do not overlap; prompts and out may have any row pitch, everything that is written per slot is
    dense.  A slot that would leave its bounds gets count 0, keeps its other bytes and raises IndexError at the next
    synchronisation.  No host read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_serve_commit
    name = "serve_commit"
    operands = (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last)
    assert all(isinstance(t, HipTensor) for t in operands), "%s: every operand is a HipTensor" % name
    b, m, N = _check_serve_commit(*operands, capacity, eos)
    leading = _serve_commit_operands(name, b, N, operands[:4], operands[4:], "out_len, queue, req, pos, count, last, ids and position_ids")
    _l.check(_l.lib().lg_serve_commit_i32(*leading, ids.ptr, position_ids.ptr, last.ptr, b, m, int(capacity), -1 if eos is None else int(eos)))


HipTensor.serve_commit = serve_commit


""" Per-request penalties on the logits of a serving step in one launch (csrc/penalize.hip) """


def penalize_rows(logits, table, index, prompts, prompt_len, out, out_len, eos=None):
    """ logits.penalize_rows(table, index, prompts, prompt_len, out, out_len, eos=None): what `CpuTensor.penalize_rows` defines
    (`lightgrad_amd.random.penalize_logits`) - repetition, presence and frequency penalties and the minimum of new tokens, every
    row under the parameters and the history of the request index[r] - in ONE launch (lg_penalize_rows_f32), IN PLACE and outside
    the tape; returns `logits`.  logits float32 (rows, V) or (rows, 1, V) that require no gradient, the last stride 1 and the row
    pitch at least V (rows of a wider tensor are fine; a lazy producer is computed first); the others int32 HipTensors that share
    no byte with the logits.  Only the logits at ids of the history are touched.  Everything the launch needs is device state, no
    host value enters: a captured step replays as it stands.  A bad row keeps its bytes and raises the device's status flag
    (IndexError at the next synchronisation). """
    name = "penalize_rows"
    operands = (table, index, prompts, prompt_len, out, out_len)
    assert all(isinstance(t, HipTensor) for t in (logits,) + operands), "%s: every operand is a HipTensor" % name
    if logits._dtype != _F32:
        raise TypeError("penalize_rows is float32-only on HipTensor (got %s)" % logits._dtype)
    rows, cols, eos = _random.check_penalize_operands(logits, table, index, prompts, prompt_len, out, out_len, eos)
    assert logits.ctx is None and not (Gradients._is_enabled() and logits.requires_grad), \
        "penalize_rows writes the logits in place: they must not require a gradient (run it under Gradients.no_grad(), or pass requires_grad=False)"
    assert rows <= 65535, "%s: at most 65535 rows in a launch (got %d)" % (name, rows)
    if rows == 0:
        return logits
    n, P, G = table._shape[0], prompts._shape[1], out._shape[1]
    logits.data                                          # a lazy producer is computed now: the launch writes into its result
    pitch = logits._strides[0] if rows > 1 else cols
    # the launch writes the logits where they lie: a layout it cannot address is an error, never a copy
    assert (cols == 1 or logits._strides[-1] == 1) and pitch >= cols, \
        "%s: the vocabulary must be contiguous and the row pitch at least V = %d (strides %s)" % (name, cols, logits._strides)
    # what is only read may be copied once into a layout the launch addresses
    table, index, prompt_len, out_len = (t.contiguous() for t in (table, index, prompt_len, out_len))
    prompts, out = ((t if (t._shape[1] == 1 or t._strides[1] == 1) and (n == 1 or t._strides[0] >= t._shape[1]) else t.contiguous()) for t in (prompts, out))
    for t in (table, index, prompts, prompt_len, out, out_len):
        assert not _shares_bytes(logits, t), "%s: the logits overlap an integer operand" % name
    flush_lazy_readers(logits)
    _l.check(_l.lib().lg_penalize_rows_f32(logits.ptr, rows, cols, pitch, table.ptr, n, index.ptr, prompts.ptr, prompts._strides[0] if n > 1 else P, P,
                                           prompt_len.ptr, out.ptr, out._strides[0] if n > 1 else G, G, out_len.ptr, eos))
    return logits


HipTensor.penalize_rows = penalize_rows


""" Per-token log-probabilities and top-n alternatives of a serving step in one launch (csrc/logprob.hip) """


def logprob_rows(logits, token, want, index, counter, logprob, top_ids, top_logprob):
    """ logits.logprob_rows(token, want, index, counter, logprob, top_ids, top_logprob): what `CpuTensor.logprob_rows` defines
    (`lightgrad_amd.random.token_logprobs_rows`) - the log-probability of the token just drawn from each row and the want[i] most
    likely ids with theirs, into column counter[i] of request i = index[r] - in ONE launch (lg_logprob_rows_f32), IN PLACE on the
    three outputs and outside the tape; returns None.  logits float32 (rows, V) or (rows, 1, V), the last stride 1 and the row
    pitch at least V (rows of a wider tensor are fine; another layout is copied once: the logits are only read); token, want,
    index, counter int32; logprob float32 (N, G), top_ids int32 and top_logprob float32 (N, G, n), dense, sharing no byte with
    each other or with anything the launch reads.  Everything the launch needs is device state, no host value enters: a captured
    step replays as it stands.  A bad row writes nothing and raises the device's status flag (IndexError at the next
    synchronisation). """
    name = "logprob_rows"
    reads, writes = (token, want, index, counter), (logprob, top_ids, top_logprob)
    assert all(isinstance(t, HipTensor) for t in (logits,) + reads + writes), "%s: every operand is a HipTensor" % name
    if logits._dtype != _F32:
        raise TypeError("logprob_rows is float32-only on HipTensor (got %s)" % logits._dtype)
    rows, cols, n, G, n_max = _random.check_logprob_operands(logits, token, want, index, counter, logprob, top_ids, top_logprob)
    assert rows <= 65535, "%s: at most 65535 rows in a launch (got %d)" % (name, rows)
    if rows == 0:
        return None
    src, pitch = logits, logits._strides[0] if rows > 1 else cols
    if (cols > 1 and src._strides[-1] != 1) or pitch < cols:
        src, pitch = logits.contiguous(), cols           # the vocabulary contiguous, one pitch from row to row
    token, want, index, counter = (t.contiguous() for t in reads)
    for t in writes:
        # the launch writes the outputs where they lie: a layout it cannot address is an error, never a copy
        assert t.is_contiguous(), "%s: logprob, top_ids and top_logprob must be dense (shape %s, strides %s)" % (name, t._shape, t._strides)
    for k, t in enumerate(writes):
        for other in (src, token, want, index, counter) + writes[:k]:
            assert not _shares_bytes(t, other), "%s: an output overlaps another operand" % name
        t.data                                           # a lazy producer is computed now: the launch writes into its result
        flush_lazy_readers(t)
    _l.check(_l.lib().lg_logprob_rows_f32(src.ptr, rows, cols, pitch, token.ptr, want.ptr, n, index.ptr, counter.ptr, logprob.ptr, G, top_ids.ptr,
                                          top_logprob.ptr, n_max))
    return None


HipTensor.logprob_rows = logprob_rows


""" Guided decoding: per-request token automata on the logits of a serving step in one launch (csrc/guide.hip) """


def guide_rows(logits, allow, states, edges, index, out, out_len, state):
    """ logits.guide_rows(allow, states, edges, index, out, out_len, state): what `CpuTensor.guide_rows` defines
    (`lightgrad_amd.guide.guide_logits`) - the automaton of request index[r] absorbs the tokens that request has stored since its
    pair in `state`, the ids its state does not allow go to -inf and a forced id to +0.0 - in ONE launch (lg_guide_rows_f32), IN
    PLACE on the logits and on `state` and outside the tape; returns `logits`.  logits float32 (rows, V) or (rows, 1, V) that
    require no gradient, the last stride 1 and the row pitch at least V (rows of a wider tensor are fine, whatever their alignment;
    a lazy producer is computed first); the others int32 HipTensors; `state` (N, 2) dense.  The logits and `state` share no byte
    with any other operand.  No logit is read: an allowed value keeps its bytes.  Everything the launch needs is device state, no
    host value enters: a captured step replays as it stands.  A bad row keeps its bytes and its state and raises the device's
    status flag (IndexError at the next synchronisation). """
    name = "guide_rows"
    reads = (allow, states, edges, index, out, out_len)
    assert all(isinstance(t, HipTensor) for t in (logits, state) + reads), "%s: every operand is a HipTensor" % name
    if logits._dtype != _F32:
        raise TypeError("guide_rows is float32-only on HipTensor (got %s)" % logits._dtype)
    rows, cols, S, E, N, G = _guide.check_guide_rows_operands(logits, allow, states, edges, index, out, out_len, state)
    assert logits.ctx is None and not (Gradients._is_enabled() and logits.requires_grad), \
        "guide_rows writes the logits in place: they must not require a gradient (run it under Gradients.no_grad(), or pass requires_grad=False)"
    assert rows <= 65535, "%s: at most 65535 rows in a launch (got %d)" % (name, rows)
    if rows == 0:
        return logits
    logits.data                                          # a lazy producer is computed now: the launch writes into its result
    state.data
    pitch = logits._strides[0] if rows > 1 else cols
    # the launch writes the logits and the state where they lie: a layout it cannot address is an error, never a copy
    assert (cols == 1 or logits._strides[-1] == 1) and pitch >= cols, \
        "%s: the vocabulary must be contiguous and the row pitch at least V = %d (strides %s)" % (name, cols, logits._strides)
    assert state.is_contiguous(), "%s: state must be dense (shape %s, strides %s)" % (name, state._shape, state._strides)
    # what is only read may be copied once into a layout the launch addresses
    allow, states, edges, index, out_len = (t.contiguous() for t in (allow, states, edges, index, out_len))
    out = out if (G == 1 or out._strides[1] == 1) and (N == 1 or out._strides[0] >= G) else out.contiguous()
    for t in (allow, states, edges, index, out, out_len):
        assert not _shares_bytes(logits, t), "%s: the logits overlap an integer operand" % name
        assert not _shares_bytes(state, t), "%s: state overlaps another integer operand" % name
    assert not _shares_bytes(logits, state), "%s: the logits overlap state" % name
    flush_lazy_readers(logits)
    flush_lazy_readers(state)
    _l.check(_l.lib().lg_guide_rows_f32(logits.ptr, rows, cols, pitch, allow.ptr, states.ptr, S, edges.ptr, E, index.ptr, out.ptr,
                                        out._strides[0] if N > 1 else G, G, out_len.ptr, state.ptr, N))
    return logits


HipTensor.guide_rows = guide_rows


def serve_commit_packed(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last, capacity, chunk, eos=None):
    """ nxt.serve_commit_packed(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last,
    capacity, chunk, eos=None): what `CpuTensor.serve_commit_packed` defines - `serve_commit` for a token-packed step: ids and
    position_ids (1, T) hold the step's tokens of all slots, T >= slots is the token budget, cu (slots + 1,) says which rows are
    whose; decoding slots get their token, prefilling slots share what is left in slot order - in ONE launch
    (lg_serve_commit_packed_i32, csrc/serve_packed.hip), in place and outside the tape.  Operands as for `serve_commit`.  A slot
    that would leave its bounds gets count 0, takes no rows, keeps its other bytes and raises IndexError at the next
    synchronisation.  No host read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_serve_commit_packed
    name = "serve_commit_packed"
    operands = (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, cu, ids, position_ids, last)
    assert all(isinstance(t, HipTensor) for t in operands), "%s: every operand is a HipTensor" % name
    b, T, N = _check_serve_commit_packed(*operands, capacity, chunk, eos)
    leading = _serve_commit_operands(name, b, N, operands[:4], operands[4:], "out_len, queue, req, pos, count, cu, last, ids and position_ids")
    _l.check(_l.lib().lg_serve_commit_packed_i32(*leading, cu.ptr, ids.ptr, position_ids.ptr, last.ptr, b, T, int(chunk), int(capacity),
                                                 -1 if eos is None else int(eos)))


HipTensor.serve_commit_packed = serve_commit_packed


def serve_commit_paged(nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free,
                       block_size, prefix_blocks=0, eos=None):
    """ nxt.serve_commit_paged(prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last,
    block_table, held, free, block_size, prefix_blocks=0, eos=None): what `CpuTensor.serve_commit_paged` defines - `serve_commit`
    over a paged cache: a finished slot pushes its blocks back on the `free` stack, a free slot is admitted only if the blocks its
    request needs for its whole life are there and pops them into its row of `block_table` behind the `prefix_blocks` shared
    ones - in ONE launch (lg_serve_commit_paged_i32, csrc/serve_paged.hip), in place and outside the tape.  Operands as for
    `serve_commit`; block_table (slots, max_blocks), held (slots,) and free (num_blocks + 1,) are dense int32 HipTensors.  A slot
    that would leave its bounds gets count 0, keeps its other bytes and raises IndexError at the next synchronisation.  No host
    read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_serve_commit, _check_paged_state
    name = "serve_commit_paged"
    operands = (nxt, prompts, prompt_len, budget, out, out_len, queue, req, pos, count, ids, position_ids, last, block_table, held, free)
    assert all(isinstance(t, HipTensor) for t in operands), "%s: every operand is a HipTensor" % name
    b, m, N = _check_serve_commit(*operands[:13], 1, eos)
    MB, NB, B, F = _check_paged_state(name, b, block_table, held, free, block_size, prefix_blocks)
    leading = _serve_commit_operands(name, b, N, operands[:4], operands[4:],
                                     "out_len, queue, req, pos, count, last, ids, position_ids, block_table, held and free")
    _l.check(_l.lib().lg_serve_commit_paged_i32(*leading, ids.ptr, position_ids.ptr, last.ptr, block_table.ptr, held.ptr, free.ptr, b, m, MB, NB,
                                                B.bit_length() - 1, F, -1 if eos is None else int(eos)))


HipTensor.serve_commit_paged = serve_commit_paged


""" The bookkeeping of a speculative decoding step in one launch (csrc/speculate.hip) """


def speculate_commit(tgt, ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram=3, min_ngram=1, eos=None):
    """ tgt.speculate_commit(ids, count, position_ids, out_ids, pos, end, done, stats, draft, max_ngram=3, min_ngram=1, eos=None):
    what `CpuTensor.speculate_commit` defines - per row the longest prefix of its drafts that the model agrees with is kept with
    one token of the model's own, a row that draws `eos` or reaches `end` is finished, and the next step's drafts are looked up in
    the row's own ids - in ONE launch (lg_speculate_commit_i32), in place and outside the tape.  Int32 HipTensors that do not
    overlap; out_ids may have any row pitch, every other operand is dense.  A row whose count, position or end is out of bounds
    gets count 0, keeps its other bytes and raises IndexError at the next synchronisation.  No host read: a captured step replays
    it as it stands. """
    from ..cpu.ops import _check_speculate_commit
    name = "speculate_commit"
    operands = (tgt, ids, count, position_ids, out_ids, pos, end, done, stats)
    assert all(isinstance(t, HipTensor) for t in operands), "%s: every operand is a HipTensor" % name
    b, m = _check_speculate_commit(*operands, draft, max_ngram, min_ngram, eos)
    columns = out_ids._shape[1]
    # what is only read may be copied once into a layout the launch addresses
    tgt, end = (t if t.is_contiguous() else t.contiguous() for t in (tgt, end))
    # the launch writes these where they lie: a layout it cannot address is an error, never a copy
    assert all(t.is_contiguous() for t in (ids, count, position_ids, pos, done, stats)) and (columns == 1 or out_ids._strides[1] == 1) \
        and (b == 1 or out_ids._strides[0] >= columns), \
        "%s: ids, count, position_ids, pos, done and stats must be dense and the rows of out_ids contiguous" % name
    operands = (tgt, ids, count, position_ids, out_ids, pos, end, done, stats)
    for i, x in enumerate(operands):
        for y in operands[i + 1:]:
            assert not _shares_bytes(x, y), "%s: two operands overlap" % name
    for x in (ids, count, position_ids, out_ids, pos, done, stats):
        flush_lazy_readers(x)
    _l.check(_l.lib().lg_speculate_commit_i32(tgt.ptr, ids.ptr, count.ptr, position_ids.ptr, out_ids.ptr, out_ids._strides[0] if b > 1 else columns,
                                              columns, pos.ptr, end.ptr, done.ptr, stats.ptr, b, m, int(draft), int(max_ngram), int(min_ngram),
                                              -1 if eos is None else int(eos)))


HipTensor.speculate_commit = speculate_commit


""" Beam search between two decode forwards in two launches (csrc/beam.hip) """


def beam_step(logits, scores, parent, token, out_ids, pos, done, stats, num_beams, eos=None):
    """ logits.beam_step(scores, parent, token, out_ids, pos, done, stats, num_beams, eos=None): what `CpuTensor.beam_step` defines
    - per group of num_beams rows the best num_beams of its continuations (a live beam offers score + log_softmax(logits), a done
    beam itself), ties to the smaller flat index, committed to scores, token, pos, done, parent and the rows of out_ids - in ONE
    launch (lg_beam_step_f32), in place and outside the tape.  logits and out_ids may have any row pitch, every other operand is
    dense; no two operands overlap.  A group with a position out of bounds keeps its bytes and raises IndexError at the next
    synchronisation.  No host read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_beam_step
    name = "beam_step"
    operands = (logits, scores, parent, token, out_ids, pos, done, stats)
    assert all(isinstance(t, HipTensor) for t in operands), "%s: every operand is a HipTensor" % name
    rows, V, w = _check_beam_step(*operands, num_beams, eos)
    columns = out_ids._shape[1]
    # what is only read may be copied once into a layout the launch addresses
    if (V > 1 and logits._strides[-1] != 1) or (rows > 1 and logits._strides[0] < V):
        logits = logits.contiguous()
    # the launch writes these where they lie: a layout it cannot address is an error, never a copy
    assert all(t.is_contiguous() for t in (scores, parent, token, pos, done, stats)) and (columns == 1 or out_ids._strides[1] == 1) \
        and (rows == 1 or out_ids._strides[0] >= columns), \
        "%s: scores, parent, token, pos, done and stats must be dense and the rows of out_ids contiguous" % name
    operands = (logits, scores, parent, token, out_ids, pos, done, stats)
    for i, x in enumerate(operands):
        for y in operands[i + 1:]:
            assert not _shares_bytes(x, y), "%s: two operands overlap" % name
    for x in operands[1:]:
        flush_lazy_readers(x)
    _l.check(_l.lib().lg_beam_step_f32(logits.ptr, logits._strides[0] if rows > 1 else V, scores.ptr, parent.ptr, token.ptr, out_ids.ptr,
                                       out_ids._strides[0] if rows > 1 else columns, columns, pos.ptr, done.ptr, stats.ptr, rows, V, w,
                                       -1 if eos is None else int(eos)))


HipTensor.beam_step = beam_step


def kv_reorder(tensors, parent, pos, num_beams):
    """ HipTensor.kv_reorder(tensors, parent, pos, num_beams): what `CpuTensor.kv_reorder` defines - in every (rows, capacity,
    width) tensor row n of each group of num_beams rows becomes the old row parent[n] at the cache positions below the group's
    largest `pos` - in ONE launch for all tensors (lg_beam_reorder_f32), in place.  Dense float32 HipTensors of one shape (at most
    64, width a multiple of 4) that overlap neither each other nor parent / pos.  A parent outside its group leaves the group as it
    is and raises IndexError at the next synchronisation.  No host read: a captured step replays it as it stands. """
    from ..cpu.ops import _check_kv_reorder
    name = "kv_reorder"
    tensors = list(tensors)
    assert all(isinstance(t, HipTensor) for t in tensors + [parent, pos]), "%s: every operand is a HipTensor" % name
    rows, w = _check_kv_reorder(tensors, parent, pos, num_beams)
    _, capacity, width = tensors[0]._shape
    assert width % 4 == 0, "%s: the cache's width %d is no multiple of 4" % (name, width)
    # the launch moves rows where they lie: a layout it cannot address is an error, never a copy
    assert all(t.is_contiguous() for t in tensors) and parent.is_contiguous() and pos.is_contiguous(), "%s: every operand must be dense" % name
    for i, x in enumerate(tensors):
        assert not _shares_bytes(x, parent) and not _shares_bytes(x, pos), "%s: parent / pos overlap a cache tensor" % name
        for y in tensors[i + 1:]:
            assert not _shares_bytes(x, y), "%s: two cache tensors overlap" % name
        flush_lazy_readers(x)
    assert not _shares_bytes(parent, pos), "%s: parent and pos overlap" % name
    table = (ctypes.c_void_p * len(tensors))(*[t.ptr for t in tensors])
    _l.check(_l.lib().lg_beam_reorder_f32(table, len(tensors), width, capacity * width, capacity, width, parent.ptr, pos.ptr, rows, w))


HipTensor.kv_reorder = staticmethod(kv_reorder)
