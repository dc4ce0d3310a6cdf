"""lg_attention_decode_split_f32 / _rows_f32 (csrc/decode_split.hip): one new token against a cache of up to 16384 rows, the keys
split over workgroups of L = lg_attention_decode_split_slice() keys and merged inside the launch; `decode_attention(split=True)`,
and the cached forward of examples/bert.py beyond 512 positions.  The error rule is test_hip_decode.py's: within 1e-5 (relative
Frobenius) of the float64 composite and no further from it than twice the fp32 composite on the same backend plus 2e-7 - for the
log-sum-exp that composite is the log of the sum of the exponentials of the composite's scores.  The positions stand one below, at
and one above the edges of a pass (16 / 32 keys) and of a slice (L)."""
import math
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from lightgrad_amd.autograd.hip import lib as hiplib
from lightgrad_amd import CpuTensor
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius, float64_tape
from test_hip_attention_masked import padding_mask
from test_hip_attention_dispatch import recorder  # noqa: F401  (fixture)
from test_hip_decode import operands, prefix, reference64, composite32, bits
import decode_cases as dc

pytestmark = pytest.mark.gpu

LG_EINVAL, SENTINEL = -1, 3.0


def slice_length():
    return int(hiplib.lib().lg_attention_decode_split_slice())


def tensor(hip, a):
    return hip.from_numpy(np.ascontiguousarray(a), requires_grad=False)


def decode(hip, q, kn, vn, k_cache, v_cache, t, heads, mask=None):
    """one split launch on fresh device copies; t: an int or a position per row.  (context, lse, caches after) as numpy"""
    d = q.shape[-1] // heads
    tk, tv = tensor(hip, k_cache), tensor(hip, v_cache)
    tm = None if mask is None else tensor(hip, mask)
    assert tensor(hip, q).decode_attention_supported(heads, k_cache.shape[1], split=True)
    out = tensor(hip, q).decode_attention(tensor(hip, kn), tensor(hip, vn), tk, tv, tensor(hip, np.atleast_1d(np.asarray(t, np.int32))),
                                          heads=heads, scale=math.sqrt(d) ** -1, mask=tm, split=True, lse=True)
    assert out.shape == q.shape and out.attention_lse.shape == (q.shape[0], heads) and not hasattr(out, "attention_probs")
    return out.numpy(), out.attention_lse.numpy(), tk.numpy(), tv.numpy()


def scores(xp, q, k, heads, mask, dtype):
    """(b, heads, t + 1) scores of the composite: float64 numpy, or float32 over the tensor API of the HIP backend (xp)"""
    b, n, width = k.shape
    d = width // heads
    if dtype == np.float64:
        s = np.einsum("bhd,bjhd->bhj", q.astype(dtype).reshape(b, heads, d), k.astype(dtype).reshape(b, n, heads, d)) / math.sqrt(d)
        return s if mask is None else s + ((1.0 - mask[:, :n].astype(dtype)) * -10000.0)[:, None, :]
    s = (tensor(xp, q).reshape(b, 1, heads, d).transpose(0, 2, 1, 3) @ tensor(xp, k).reshape(b, n, heads, d).transpose(0, 2, 3, 1)) / math.sqrt(d)
    if mask is not None:
        s = s + (1.0 - tensor(xp, mask[:, :n]).reshape(b, 1, 1, n)) * -10000.0
    return s.numpy().reshape(b, heads, n)


def check(hip, shape, capacity, t, mask):
    b, heads, d = shape
    k, v, q, kn, vn = operands(b, capacity, heads, d)
    ctx, lse, _, _ = decode(hip, q, kn, vn, k, v, t, heads, mask)
    kp, vp = prefix(k, kn, t), prefix(v, vn, t)
    s64, s32 = scores(None, q, kp, heads, mask, np.float64), scores(hip, q, kp, heads, mask, np.float32)
    want = {"context": reference64(q, kp, vp, heads, mask)[0], "lse": np.log(np.exp(s64 - s64.max(-1, keepdims=True)).sum(-1)) + s64.max(-1)}
    comp = {"context": composite32(hip, q, kp, vp, heads, mask)[0], "lse": np.log(np.exp(s32).sum(-1, dtype=np.float32))}
    what = "%s cap %d t %d %s" % (shape, capacity, t, "nomask" if mask is None else "mask")
    for name, g in (("context", ctx), ("lse", lse)):
        e_fused, e_comp = rel_frobenius(g, want[name]), rel_frobenius(comp[name], want[name])
        print("%s %s: split %.3e, fp32 composite %.3e" % (what, name, e_fused, e_comp))
        assert np.isfinite(g).all(), (what, name)
        assert e_fused <= 1e-5 and e_fused <= 2 * e_comp + 2e-7, (what, name, e_fused, e_comp)
    if t == 0 and mask is None:
        np.testing.assert_array_equal(bits(ctx), bits(vn), err_msg=what)


@pytest.mark.parametrize("shape", [(2, 2, 32), (3, 1, 64)], ids=["2x2x32", "3x1x64"])
def test_sweep_against_the_float64_composite(hip, shape):
    L = slice_length()
    capacity = 3 * L + 5
    for t in sorted({0, 1, 15, 16, 17, 31, 32, 33, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, capacity - 1}):
        for mask in (None, padding_mask(shape[0], capacity)):
            check(hip, shape, capacity, t, mask)


def test_the_longest_cache_and_a_fully_masked_slice(hip):
    L = slice_length()
    check(hip, (1, 1, 64), 16384, 16383, None)
    mask = np.ones((3, 3 * L + 5), np.float32)
    mask[:, L:2 * L] = 0                                                                 # the whole second slice: w_s = +0, exact zeros
    check(hip, (3, 1, 64), 3 * L + 5, 2 * L + 3, mask)


@pytest.mark.parametrize("where", ["L-1", "L", "2L+1"])
def test_cache_discipline_bit_for_bit(hip, where):
    """rows >= t are not read (NaN), rows other than t keep their bits, row t becomes k_new / v_new; mask entries beyond t do not matter"""
    L = slice_length()
    t = {"L-1": L - 1, "L": L, "2L+1": 2 * L + 1}[where]
    b, heads, d, capacity = 2, 2, 32, 3 * L + 5
    k, v, q, kn, vn = operands(b, capacity, heads, d, seed=11)
    mask = padding_mask(b, capacity)
    k0, v0, k1, v1 = k.copy(), v.copy(), k.copy(), v.copy()
    k0[:, t:], v0[:, t:], k1[:, t:], v1[:, t:] = 0, 0, np.nan, np.nan
    ctx0, lse0, ka0, va0 = decode(hip, q, kn, vn, k0, v0, t, heads, mask)
    ctx1, lse1, ka1, va1 = decode(hip, q, kn, vn, k1, v1, t, heads, mask)
    hole = mask.copy()
    hole[:, t + 1:] = np.nan
    ctx2, lse2, _, _ = decode(hip, q, kn, vn, k0, v0, t, heads, hole)
    assert np.isfinite(ctx1).all() and np.isfinite(lse1).all()
    for got, want in ((ctx1, ctx0), (lse1, lse0), (ctx2, ctx0), (lse2, lse0)):
        np.testing.assert_array_equal(bits(got), bits(want))
    for before, after, new in ((k0, ka0, kn), (v0, va0, vn), (k1, ka1, kn), (v1, va1, vn)):
        np.testing.assert_array_equal(bits(after[:, :t]), bits(before[:, :t]))
        np.testing.assert_array_equal(bits(after[:, t:t + 1]), bits(new))
        np.testing.assert_array_equal(bits(after[:, t + 1:]), bits(before[:, t + 1:]))


def test_determinism_independence_tickets_and_rows(hip):
    L = slice_length()
    b, heads, d, capacity = 3, 2, 64, 3 * L + 8
    k, v, q, kn, vn = operands(b, capacity, heads, d, seed=13)
    mask = padding_mask(b, capacity)
    first = decode(hip, q, kn, vn, k, v, 2 * L + 1, heads, mask)
    again = decode(hip, q, kn, vn, k, v, 2 * L + 1, heads, mask)
    for x, y in zip(first, again):                                                       # two identical calls: identical bits
        np.testing.assert_array_equal(bits(x), bits(y))
    alone = lambda i, t: decode(hip, q[i:i + 1], kn[i:i + 1], vn[i:i + 1], k[i:i + 1], v[i:i + 1], t, heads, mask[i:i + 1])      # noqa: E731
    for i in range(b):                                                                   # an element of the batch alone
        for x, y in zip(alone(i, 2 * L + 1)[:2], first[:2]):
            np.testing.assert_array_equal(bits(x), bits(y[i:i + 1]))
    tk, tv, tm, tq, tkn, tvn = (tensor(hip, a) for a in (k, v, mask, q, kn, vn))
    for t in (2 * L + 1, L):                                  # the same tensors again: a ticket left non-zero would break the second call
        out = tq.decode_attention(tkn, tvn, tk, tv, tensor(hip, np.array([t], np.int32)), heads=heads, scale=math.sqrt(d) ** -1, mask=tm, split=True)
    want = reference64(q, prefix(k, kn, L), prefix(v, vn, L), heads, mask)[0]
    assert rel_frobenius(out.numpy(), want) <= 1e-5
    pos = [3, L + 2, 2 * L + 7]                               # a position per row: each row is the one-word entry on that row alone
    rows = decode(hip, q, kn, vn, k, v, pos, heads, mask)
    for i, t in enumerate(pos):
        one = alone(i, t)
        for x, y in zip(rows, one):
            np.testing.assert_array_equal(bits(x[i:i + 1]), bits(y))


class Call(object):
    def __init__(self, hip, pos, entry="lg_attention_decode_split_f32", b=3, heads=2, d=32, capacity=8):
        self.lib, self.entry, width = hiplib.lib(), entry, heads * d
        k, v, q, kn, vn = operands(b, capacity, heads, d)
        self.k, self.v, self.q, self.kn, self.vn = (tensor(hip, a) for a in (k, v, q, kn, vn))
        self.o, self.lse = tensor(hip, np.full((b, width), SENTINEL, np.float32)), tensor(hip, np.full((b, heads), SENTINEL, np.float32))
        self.mask, self.pos, self.host = tensor(hip, np.ones((b, capacity), np.float32)), tensor(hip, np.asarray(pos, np.int32)), dict(k=k, v=v)
        self.args = dict(q=self.q.ptr, sbq=width, k_new=self.kn.ptr, sbk=width, v_new=self.vn.ptr, sbv=width, k_cache=self.k.ptr,
                         v_cache=self.v.ptr, ldc=width, sbc=capacity * width, pos=self.pos.ptr, o=self.o.ptr, sbo=width, lse=self.lse.ptr,
                         batch=b, heads=heads, capacity=capacity, D=d, scale=0.2, mask=None, sbm=0)

    def __call__(self, **override):
        return getattr(self.lib, self.entry)(*dict(self.args, **override).values())

    def untouched(self, rows=slice(None)):
        return ((self.o.numpy()[rows] == SENTINEL).all() and (self.lse.numpy()[rows] == SENTINEL).all()
                and (bits(self.k.numpy()[rows]) == bits(self.host["k"][rows])).all() and (bits(self.v.numpy()[rows]) == bits(self.host["v"][rows])).all())


def test_a_row_out_of_range_is_reported_once_and_the_others_are_computed(hip):
    capacity = 2 * slice_length() + 8
    call = Call(hip, [3, capacity, capacity - 1], entry="lg_attention_decode_split_rows_f32", capacity=capacity)
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the words
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert call.untouched(slice(1, 2))
    got, lse = call.o.numpy(), call.lse.numpy()
    for r, t in ((0, 3), (2, capacity - 1)):
        assert np.isfinite(got[r]).all() and not (got[r] == SENTINEL).any() and not (lse[r] == SENTINEL).any()
        np.testing.assert_array_equal(bits(call.k.numpy()[r, t]), bits(call.kn.numpy()[r, 0]))


REFUSALS = [("capacity0", dict(capacity=0)), ("capacity16385", dict(capacity=16385)), ("D48", dict(D=48)), ("base-q", "q"),
            ("row-pitch-below-width", dict(ldc=32)), ("mask-pitch-1", dict(mask=True, sbm=1)),
            # the rows of test_hip_decode.py's table: the entries run the same host checks
            ("heads0", dict(heads=0)), ("pitch-q", dict(sbq=66)), ("pitch-cache-row", dict(ldc=66)), ("pitch-cache-batch", dict(sbc=8 * 64 + 2)),
            ("pitch-o", dict(sbo=65)), ("base-k_new", "k_new"), ("base-v_new", "v_new"), ("base-k_cache", "k_cache"), ("base-v_cache", "v_cache"),
            ("base-o", "o"), ("pos-null", dict(pos=None)), ("mask-pitch", dict(mask=True, sbm=7)), ("pos-in-k_cache", dict(pos="k_cache")),
            ("pos-in-v_cache", dict(pos="v_cache+"))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_launch_nothing(hip, name, change):
    call = Call(hip, [3])
    if isinstance(change, str):
        change = {change: call.args[change] + 4}                          # a base that is not 16-byte aligned
    change = dict(change, mask=call.mask.ptr) if change.get("mask") is True else change
    for key, value in list(change.items()):
        if isinstance(value, str):                                        # the position word inside a cache: at its base, or 64 bytes in
            change[key] = call.args[value.rstrip("+")] + (64 if value.endswith("+") else 0)
    assert call(**change) == LG_EINVAL, name
    assert b"lg_attention_decode_split_f32" in call.lib.lg_last_error()
    if name.startswith("pos-in"):
        assert b"pos overlaps a cache" in call.lib.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched(), name


@pytest.mark.parametrize("entry", ["lg_attention_decode_split_f32", "lg_attention_decode_split_rows_f32"])
def test_an_empty_batch_is_fine_and_launches_nothing(hip, entry):
    """batch == 0 returns before the operands are looked at, after the shape and the heads; `_rows` refuses under its own name"""
    call = Call(hip, [3, 3, 3], entry=entry)
    assert call(batch=0) == 0 and call(batch=0, q=call.args["q"] + 4, pos=None) == 0
    assert call(batch=0, D=48) == LG_EINVAL and call(batch=0, heads=0) == LG_EINVAL
    assert call(pos=call.args["k_cache"]) == LG_EINVAL and entry.encode() + b": pos overlaps a cache" in call.lib.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched()


def test_a_negative_batch_pitch_is_taken(hip):
    """batch 2 with q at its second row and sbq = -width: the launch of the two query rows swapped, bit for bit"""
    call, width = Call(hip, [3], b=2), 64
    swapped = tensor(hip, call.q.numpy()[::-1])
    assert call(q=swapped.ptr) == 0
    HipDevice.synchronize()
    want, want_lse = call.o.numpy().copy(), call.lse.numpy().copy()
    assert not (want == SENTINEL).any()
    call.o.upload_(np.full_like(want, SENTINEL))
    assert call(q=call.args["q"] + 4 * width, sbq=-width) == 0
    HipDevice.synchronize()
    np.testing.assert_array_equal(bits(call.o.numpy()), bits(want))
    np.testing.assert_array_equal(bits(call.lse.numpy()), bits(want_lse))


def test_probabilities_are_refused_by_name(hip):
    k, v, q, kn, vn = (tensor(hip, a) for a in operands(2, 8, 2, 32))
    with pytest.raises(AssertionError, match="decode_attention: probs=True with split=True"):
        q.decode_attention(kn, vn, k, v, tensor(hip, np.array([3], np.int32)), heads=2, scale=1.0, probs=True, split=True)
    assert not q.decode_attention_supported(2, 513) and q.decode_attention_supported(2, 513, split=True)


def long_model(T, cfg, params, dtype=np.float32):
    """decode_cases.make_model for another config (float64: inside float64_tape())"""
    model = dc.bert.BertForMaskedLM(**cfg)
    model.load_parameters({n: a.astype(dtype) for n, a in params.items()})
    return model.eval() if T is CpuTensor else model.eval().map_parameters(lambda p: T.from_numpy(p.numpy()))


def cached_rows(T, model, ids, prompt, capacity, cfg):
    """the prompt through the causal forward into an nn.KVCache, then three given tokens one at a time; the rows and the cache"""
    cache = nn.KVCache(cfg["num_hidden_layers"], ids.shape[0], capacity, cfg["hidden_size"], like=model.cls.predictions.bias)
    rows = {"prefill": model(T.from_numpy(ids[:, :prompt], requires_grad=False), cache=cache).numpy().copy()}
    for i in range(3):
        rows["step%d" % i] = model(T.from_numpy(ids[:, prompt + i:prompt + i + 1], requires_grad=False), cache=cache).numpy().copy()
        cache.advance()
    return rows, cache


def test_the_model_decodes_beyond_512_positions(hip, recorder):  # noqa: F811
    prompt, capacity = 2 * slice_length() + 3, 2 * slice_length() + 8
    cfg = dict(dc.CFG, max_position_embeddings=capacity + 8, attention_probs=False, causal=True)
    np.random.seed(dc.SEED)
    params = {n: p.numpy().astype(np.float32) * (dc.GAIN if p.numpy().ndim == 2 else 1.0) for n, p in dc.bert.BertForMaskedLM(**cfg).named_parameters()}
    ids = np.random.randint(0, cfg["vocab_size"], (dc.B, prompt + 4)).astype(np.int32)
    with float64_tape():
        ref64, _ = cached_rows(CpuTensor, long_model(CpuTensor, cfg, params, np.float64), ids, prompt, capacity, cfg)
    cpu32, _ = cached_rows(CpuTensor, long_model(CpuTensor, cfg, params), ids, prompt, capacity, cfg)
    model = long_model(hip, cfg, params)
    got, cache = cached_rows(hip, model, ids, prompt, capacity, cfg)
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="cached forward beyond 512 positions on HipTensor")
    token = tensor(hip, ids[:, prompt + 3:prompt + 4])        # one more step: two split launches; captured and replayed, the eager bits
    del recorder.calls[:]
    eager = model(token, cache=cache).numpy().copy()
    assert recorder.calls == ["lg_attention_decode_split_f32"] * 2
    graph = HipGraph()
    with graph.capture():
        captured = model(token, cache=cache)
    for _ in range(3):
        graph.replay()
        np.testing.assert_array_equal(bits(captured.numpy()), bits(eager))
    graph.destroy()
