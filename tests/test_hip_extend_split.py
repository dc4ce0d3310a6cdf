"""lg_attention_extend_split_f32 / _rows_f32 / _counts_f32 (csrc/extend_split.hip): m new tokens against a cache of up to 16384
rows, the keys split over workgroups of L = lg_attention_extend_split_slice() keys and merged inside the launch;
`extend_attention(split=True)` and the append path of examples/bert.py beyond 512 positions.  Context and log-sum-exp within 1e-5
(relative Frobenius, as test_hip_attention_stream.py) of a float64 numpy reference; caches, rows and counts bit for bit."""
import math
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from lightgrad_amd import CpuTensor
from common import rel_frobenius, float64_tape
from test_hip_attention_dispatch import recorder  # noqa: F401  (fixture)
from test_hip_decode_split import long_model, tensor, bits
from test_hip_extend import operands
import decode_cases as dc

pytestmark = pytest.mark.gpu

LG_EINVAL, SENTINEL = -1, 3.0


def slice_length():
    return int(hiplib.lib().lg_attention_extend_split_slice())


def reference64(q, kn, vn, k, v, t, heads, mask):
    """one batch element in float64: (context (n, width), lse (heads, n)) of its n new rows behind t cached ones"""
    n, d = q.shape[0], q.shape[1] // heads
    K, V = (np.concatenate([c[:t], new]).astype(np.float64).reshape(t + n, heads, d) for c, new in ((k, kn), (v, vn)))
    s = np.einsum("ihd,jhd->hij", q.astype(np.float64).reshape(n, heads, d), K) / math.sqrt(d)
    if mask is not None:
        s = s + (1.0 - mask[:t + n].astype(np.float64)) * -10000.0
    s = np.where(np.arange(t + n)[None, :] <= t + np.arange(n)[:, None], s, -np.inf)
    top = s.max(-1, keepdims=True)
    e = np.exp(s - top)
    return np.einsum("hij,jhd->ihd", e / e.sum(-1, keepdims=True), V).reshape(n, heads * d), top[..., 0] + np.log(e.sum(-1))


def extend(hip, arrays, pos, heads, mask=None, count=None):
    """one split launch on fresh device copies; pos: an int or a position per row.  (context, lse, caches after) as numpy"""
    k, v, q, kn, vn = arrays
    tk, tv, tq = tensor(hip, k), tensor(hip, v), tensor(hip, q)
    extra = {} if count is None else {"count": tensor(hip, np.asarray(count, np.int32))}
    assert tq.extend_attention_supported(heads, k.shape[1], split=True)
    out = tq.extend_attention(tensor(hip, kn), tensor(hip, vn), tk, tv, tensor(hip, np.atleast_1d(np.asarray(pos, np.int32))), heads=heads,
                              scale=math.sqrt(q.shape[2] // heads) ** -1, mask=None if mask is None else tensor(hip, mask), split=True, lse=True, **extra)
    assert out.attention_lse.shape == (q.shape[0], heads, q.shape[1]) and not hasattr(out, "attention_probs")
    return out.numpy(), out.attention_lse.numpy(), tk.numpy(), tv.numpy()


def poisoned(arrays, t):
    """the operands with NaN in every cache row >= t (a position per element or one for all)"""
    k, v = arrays[0].copy(), arrays[1].copy()
    for r, tr in enumerate(np.broadcast_to(t, (k.shape[0],))):
        k[r, tr:], v[r, tr:] = np.nan, np.nan
    return (k, v) + tuple(arrays[2:])


def check_element(got, arrays, r, t, n, heads, mask, what, bound=1e-5):
    ctx, lse, ka, va = got
    k, v, q, kn, vn = (a[r] for a in arrays)
    want, want_lse = reference64(q[:n], kn[:n], vn[:n], k, v, t, heads, None if mask is None else mask[r % mask.shape[0]])
    errors = rel_frobenius(ctx[r, :n], want), rel_frobenius(lse[r, :, :n], want_lse)
    print("%s element %d t %d n %d: context %.3e, lse %.3e" % (what, r, t, n, *errors))
    assert np.isfinite(ctx[r]).all() and np.isfinite(lse[r]).all() and errors[0] <= bound and errors[1] <= 1e-5, (what, r, errors)
    for after, before, new in ((ka[r], k, kn), (va[r], v, vn)):              # the new rows bit for bit, every other word unchanged
        np.testing.assert_array_equal(bits(after[t:t + n]), bits(new[:n]), err_msg=what)
        np.testing.assert_array_equal(bits(after[:t]), bits(before[:t]), err_msg=what)
        np.testing.assert_array_equal(bits(after[t + n:]), bits(before[t + n:]), err_msg=what)


def hole_mask(b, capacity):
    mask = np.ones((b, capacity), np.float32)
    mask[:, 1::7] = 0
    return mask


# (capacity, t, m) in units of L: one slice; rows across a slice edge; two blocks with different `live`; four blocks
SHAPES = [lambda L: (8, 0, 3), lambda L: (L + 40, L - 2, 5), lambda L: (2 * L + 70, 2 * L + 1, 33), lambda L: (3 * L, L, 128)]
CASES = [(i, d, masked) for i in range(4) for d in (32, 64) for masked in (False, True)] + [(4, 64, False), (4, 64, True)]


@pytest.mark.parametrize("case,d,masked", CASES, ids=["case%d-d%d-%s" % (c[0], c[1], "mask" if c[2] else "nomask") for c in CASES])
def test_against_the_float64_reference(hip, case, d, masked):
    b, heads = (1, 1) if case == 4 else (2, 2)                               # case 4: the largest slice count
    capacity, t, m = (16384, 16384 - 128, 128) if case == 4 else SHAPES[case](slice_length())
    arrays = poisoned(operands(b, capacity, m, heads, d, seed=5 + case), t)
    mask = hole_mask(b, capacity) if masked else None
    got = extend(hip, arrays, t, heads, mask)
    for r in range(b):
        check_element(got, arrays, r, t, m, heads, mask, "case %d" % case)


def test_rows_and_counts_are_the_one_word_entry_per_element(hip):
    L, m, heads = slice_length(), 37, 2
    pos, counts, capacity = [3, L - 1, 2 * L + 5], [0, 1, 37], 2 * L + 5 + 37
    arrays = poisoned(operands(3, capacity, m, heads, 32, seed=9), pos)
    mask = hole_mask(3, capacity)
    alone = lambda r, n: extend(hip, tuple(a[r:r + 1, :n] if i > 1 else a[r:r + 1] for i, a in enumerate(arrays)), pos[r], heads, mask[r:r + 1])  # noqa: E731
    rows, counted = extend(hip, arrays, pos, heads, mask), extend(hip, arrays, pos, heads, mask, count=counts)
    for r in range(3):
        for got, n in ((rows, m), (counted, counts[r])):
            mine = (got[0][r:r + 1, :n], got[1][r:r + 1, :, :n], got[2][r:r + 1], got[3][r:r + 1])
            for x, y in zip(mine, alone(r, n) if n else ()):
                np.testing.assert_array_equal(bits(x), bits(y))
            assert (bits(got[0][r, n:]) == 0).all() and (bits(got[1][r, :, n:]) == 0).all()          # rows >= n: +0.0
            if n == 0:                                                        # an idle element: its cache rows untouched
                np.testing.assert_array_equal(bits(got[2][r]), bits(arrays[0][r]))
                np.testing.assert_array_equal(bits(got[3][r]), bits(arrays[1][r]))
    check_element(rows, arrays, 2, pos[2], m, heads, mask, "rows")


def test_degenerate_partials(hip):
    """element 0: the mask hides the whole first slice (the late maximum, weights of +0); element 1: every key masked - each score
    is x - 10000 rounded to fp32, whose spacing there is 2^-10, so a probability is off by up to that factor: the context within
    2^-10, the log-sum-exp (near -10000) still within 1e-5"""
    L, heads, m = slice_length(), 2, 5
    capacity, t = 2 * L + 8, L + 3
    arrays = poisoned(operands(2, capacity, m, heads, 64, seed=17), t)
    mask = np.ones((2, capacity), np.float32)
    mask[0, :L], mask[1] = 0, 0
    got = extend(hip, arrays, t, heads, mask)
    check_element(got, arrays, 0, t, m, heads, mask, "first slice hidden")
    check_element(got, arrays, 1, t, m, heads, mask, "fully masked", bound=2.0 ** -10)


def test_tickets_are_zero_again_and_the_bits_repeat(hip):
    L, heads, m = slice_length(), 2, 5
    arrays = operands(2, 2 * L + 40, m, heads, 64, seed=21)
    for x, y in zip(extend(hip, arrays, 2 * L + 1, heads), extend(hip, arrays, 2 * L + 1, heads)):
        np.testing.assert_array_equal(bits(x), bits(y))
    tk, tv, tq, tkn, tvn = (tensor(hip, a) for a in arrays)
    for t in (2 * L + 1, L - 3):                                             # the same tensors: a ticket left non-zero would break the second call
        out = tq.extend_attention(tkn, tvn, tk, tv, tensor(hip, np.array([t], np.int32)), heads=heads, scale=0.125, split=True)
    for r in range(2):
        want = reference64(arrays[2][r], arrays[3][r], arrays[4][r], arrays[0][r], arrays[1][r], L - 3, heads, None)[0]
        assert rel_frobenius(out.numpy()[r], want) <= 1e-5


class Call(object):
    """one entry through the C ABI on sentinel outputs"""
    def __init__(self, hip, pos, count=None, entry="lg_attention_extend_split_f32", b=3, heads=2, d=32, capacity=8, m=2):
        self.lib, self.entry, width = hiplib.lib(), entry, heads * d
        k, v, q, kn, vn = operands(b, capacity, m, heads, d)
        self.k, self.v, self.q, self.kn, self.vn = (tensor(hip, a) for a in (k, v, q, kn, vn))
        self.o, self.lse = tensor(hip, np.full((b, m, width), SENTINEL, np.float32)), tensor(hip, np.full((b, heads, m), SENTINEL, np.float32))
        self.mask, self.pos, self.host = tensor(hip, np.ones((b, capacity), np.float32)), tensor(hip, np.asarray(pos, np.int32)), dict(k=k, v=v)
        self.count = None if count is None else tensor(hip, np.asarray(count, np.int32))
        self.args = dict(q=self.q.ptr, ldq=width, sbq=m * width, k_new=self.kn.ptr, ldk=width, sbk=m * width, v_new=self.vn.ptr, ldv=width, sbv=m * width,
                         k_cache=self.k.ptr, v_cache=self.v.ptr, ldc=width, sbc=capacity * width, pos=self.pos.ptr,
                         **({} if count is None else {"count": self.count.ptr}), o=self.o.ptr, ldo=width, sbo=m * width, lse=self.lse.ptr, batch=b,
                         heads=heads, m=m, capacity=capacity, D=d, scale=0.2, mask=None, sbm=0)

    def __call__(self, **override):
        return getattr(self.lib, self.entry)(*dict(self.args, **override).values())

    def untouched(self, rows=slice(None)):
        return ((self.o.numpy()[rows] == SENTINEL).all() and (self.lse.numpy()[rows] == SENTINEL).all()
                and (bits(self.k.numpy()[rows]) == bits(self.host["k"][rows])).all() and (bits(self.v.numpy()[rows]) == bits(self.host["v"][rows])).all())


def test_an_element_out_of_range_is_reported_and_the_others_are_computed(hip):
    capacity = 2 * slice_length() + 8
    call = Call(hip, [3, capacity - 1, capacity - 2], count=[2, 2, 2], entry="lg_attention_extend_split_counts_f32", capacity=capacity)
    assert call() == 0                                                        # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                                   # reported once
    assert call.untouched(slice(1, 2))
    for r, t in ((0, 3), (2, capacity - 2)):
        assert np.isfinite(call.o.numpy()[r]).all() and not (call.o.numpy()[r] == SENTINEL).any() and not (call.lse.numpy()[r] == SENTINEL).any()
        np.testing.assert_array_equal(bits(call.k.numpy()[r, t:t + 2]), bits(call.kn.numpy()[r]))


REFUSALS = [("m129", dict(m=129, capacity=512), b"unsupported"), ("m-beyond-capacity", dict(m=9), b"unsupported"), ("capacity16385", dict(capacity=16385), b"unsupported"),
            ("D48", dict(D=48), b"unsupported"), ("heads0", dict(heads=0), b"bad batch"), ("grid", dict(heads=20000, m=128, capacity=512), b"grid dimension"),
            ("base-q", dict(q=4), b"16-byte aligned"), ("pitch-k", dict(ldk=66), b"multiples of 4"), ("pitch-negative", dict(sbo=-64), b"non-negative"),
            ("row-pitch", dict(ldc=32), b"row pitch"), ("mask-pitch", dict(mask=True, sbm=7), b"mask batch pitch"), ("k_new-in-cache", dict(k_new="k_cache"), b"overlap a cache"),
            ("pos-in-cache", dict(pos="k_cache"), b"pos overlaps a cache"), ("count-null", dict(count=None), b"count must be"),
            ("count-in-cache", dict(count="v_cache"), b"count overlaps a cache"), ("count-is-pos", dict(count="pos"), b"count overlaps pos"),
            ("lse-misaligned", dict(lse=2), b"lse must be"), ("lse-in-o", dict(lse="o"), b"lse overlaps"), ("lse-in-cache", dict(lse="v_cache"), b"lse overlaps"),
            ("tickets", dict(batch=40000, sbq=0, sbk=0, sbv=0, sbo=0, sbc=0, lse=None), b"ticket pool")]


@pytest.mark.parametrize("name,change,message", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_launch_nothing(hip, name, change, message):
    # (the ticket pool through the one-word entry: at batch 40000 the `batch` position words of the others would cover the caches)
    call = Call(hip, [3], entry="lg_attention_extend_split_f32") if name == "tickets" else \
        Call(hip, [3, 3, 3], count=[2, 2, 2], entry="lg_attention_extend_split_counts_f32")
    change = dict(change, mask=call.mask.ptr) if change.get("mask") is True else dict(change)
    for key, value in list(change.items()):
        if isinstance(value, str):                                            # one operand inside another
            change[key] = call.args[value]
        elif key in ("q", "lse") and isinstance(value, int):                  # a base off its alignment
            change[key] = call.args[key] + value
    assert call(**change) == LG_EINVAL, name
    error = call.lib.lg_last_error()
    assert call.entry.encode() + b":" in error and message in error, error
    HipDevice.synchronize()
    assert call.untouched(), name


def test_the_predicate_and_the_keyword(hip):
    supported = hiplib.lib().lg_attention_extend_split_supported
    assert supported(128, 16384, 64) and not supported(129, 16384, 64) and not supported(1, 16385, 64) and not supported(1, 8, 48)
    k, v, q, kn, vn = (tensor(hip, a) for a in operands(2, 8, 2, 2, 32))
    pos = tensor(hip, np.array([3], np.int32))
    assert not q.extend_attention_supported(2, 513) and q.extend_attention_supported(2, 513, split=True)
    with pytest.raises(AssertionError, match="extend_attention: probs=True with split=True"):
        q.extend_attention(kn, vn, k, v, pos, heads=2, probs=True, split=True)
    for keyword in ("cu", "m_max", "block_table", "kv_dtype"):
        with pytest.raises(AssertionError, match="extend_attention: %s= with split=True" % keyword):
            q.extend_attention(kn, vn, k, v, pos, heads=2, split=True, **{keyword: 1})


def test_the_model_appends_beyond_512_positions(hip, recorder):  # noqa: F811
    L, m = slice_length(), 5
    prompt, capacity = 2 * L + 10, 2 * L + 100
    cfg = dict(dc.CFG, num_hidden_layers=1, max_position_embeddings=capacity, attention_probs=False, causal=True)
    np.random.seed(dc.SEED)
    params = {n: p.numpy().astype(np.float32) * (dc.GAIN if p.numpy().ndim == 2 else 1.0) for n, p in dc.bert.BertForMaskedLM(**cfg).named_parameters()}
    ids = np.random.randint(0, cfg["vocab_size"], (dc.B, prompt + m)).astype(np.int32)

    def run(T, model):
        cache = nn.KVCache(1, dc.B, capacity, cfg["hidden_size"], like=model.cls.predictions.bias)
        first = model(T.from_numpy(ids[:, :prompt], requires_grad=False), cache=cache).numpy().copy()
        tokens = T.from_numpy(ids[:, prompt:], requires_grad=False)
        del recorder.calls[:]
        return first, model(tokens, cache=cache, append=True).numpy().copy(), list(recorder.calls), tokens, cache

    with float64_tape():
        want = run(CpuTensor, long_model(CpuTensor, cfg, params, np.float64))
    model = long_model(hip, cfg, params)
    first, eager, calls, tokens, cache = run(hip, model)
    assert calls == ["lg_attention_extend_split_f32"]
    assert rel_frobenius(first, want[0]) <= 1e-5 and rel_frobenius(eager, want[1]) <= 1e-5
    graph = HipGraph()                                                        # the position has not moved: the same step again, captured
    with graph.capture():
        captured = model(tokens, cache=cache, append=True)
    for _ in range(3):
        graph.replay()
        np.testing.assert_array_equal(bits(captured.numpy()), bits(eager))
    graph.destroy()
