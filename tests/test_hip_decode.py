"""lg_attention_decode_f32 (csrc/decode.hip) and what stands on it: `decode_attention`, `self_attention_decode`, the cached
forward of examples/bert.py on HipTensor, `generate`, and a captured decode step.

The error rule is the project's own (test_hip_attention_masked.py): a result must be within 1e-5 (relative Frobenius) of the
float64 composite and no further from it than twice the fp32 composite on the same backend plus 2e-7.

The kernel's partition of the keys 0 .. t (csrc/decode.hip): a key row is read by G = D / 4 lanes, so a wave covers KW = 64 / G
keys per load (D = 64: 4, D = 32: 8), the workgroup KP = 4 KW keys per pass (16 / 32), and 16 passes are loaded together
(256 / 512 keys, the first group of V ahead of the softmax); the softmax gives thread i the scores i and i + 256.  The sweep
takes t one below, at and one above the first boundary of each kind for both D - keys per wave {3, 4, 5, 7, 8, 9}, per pass
{15, 16, 17, 31, 32, 33}, per group of passes and the softmax's second score {255, 256, 257} (D = 32: one group holds all 512
keys; its last, 511, is capacity - 1) - next to the issue's {0, 1, 31, 32, 63, 64, 127, 128, 255, 256, capacity - 1} and their
neighbours 65, 129 (one key per lane group:
every t is such a boundary)."""
import math
import numpy as np
import pytest
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from test_hip_attention_masked import padding_mask
from test_hip_attention_dispatch import recorder  # noqa: F401  (fixture)
import decode_cases as dc

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
T_VALUES = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SHAPES = [(1, 1, 32), (2, 2, 32), (3, 1, 64), (2, 2, 64)]
CAPACITIES = [1, 5, 64, 129, 512]


def operands(b, capacity, heads, d, seed=7):
    """uniform(-1.5, 1.5) draws as test_hip_attention_masked.operands: the cache's rows (b, capacity, width) twice, and the new
    token's q, k_new, v_new (b, 1, width)"""
    rng = np.random.RandomState(seed)
    width = heads * d
    k, v = (rng.uniform(-1.5, 1.5, (b, capacity, width)).astype(np.float32) for _ in range(2))
    q, kn, vn = (rng.uniform(-1.5, 1.5, (b, 1, width)).astype(np.float32) for _ in range(3))
    return k, v, q, kn, vn


def prefix(cache, new, t):
    """rows 0 .. t the attention sees: the cache's below t, the new token's at t"""
    return np.concatenate([cache[:, :t], new], axis=1)


def reference64(q, k, v, heads, mask):
    """the float64 composite of the prefix: scores, key bias, softmax, context over keys 0 .. t; k, v (b, t + 1, width)"""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    b, n, width = k.shape
    d = width // heads
    scores = np.einsum("bhd,bjhd->bhj", q.reshape(b, heads, d), k.reshape(b, n, heads, d)) / math.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask[:, :n].astype(np.float64)) * -10000.0)[:, None, :]
    e = np.exp(scores - scores.max(axis=-1, keepdims=True))
    probs = e / e.sum(axis=-1, keepdims=True)
    return np.einsum("bhj,bjhd->bhd", probs, v.reshape(b, n, heads, d)).reshape(b, 1, width), probs[:, :, None, :]


def composite32(hip, q, k, v, heads, mask):
    """the same over the tensor API on the HIP backend in float32 (examples/bert.py, composite decode branch)"""
    b, n, width = k.shape
    d = width // heads
    tq, tk, tv = (hip.from_numpy(a, requires_grad=False) for a in (q, k, v))
    q4 = tq.reshape(b, 1, heads, d).transpose(0, 2, 1, 3)
    k4 = tk.reshape(b, n, heads, d).transpose(0, 2, 3, 1)
    v4 = tv.reshape(b, n, heads, d).transpose(0, 2, 1, 3)
    scores = (q4 @ k4) / math.sqrt(d)
    if mask is not None:
        m = hip.from_numpy(np.ascontiguousarray(mask[:, :n]), requires_grad=False)
        scores = scores + (1.0 - m.reshape(b, 1, 1, n)) * -10000.0
    probs = scores.softmax(axis=-1)
    return (probs @ v4).transpose(0, 2, 1, 3).reshape(b, 1, width).numpy(), probs.numpy()


def position(hip, t):
    return hip.from_numpy(np.array([t], np.int32), requires_grad=False)


def decode(hip, q, kn, vn, k_cache, v_cache, t, heads, mask=None, probs=True):
    """one launch through the op on fresh device copies of everything: (context, probs, k_cache after, v_cache after) as numpy"""
    d = q.shape[-1] // heads
    tk, tv = hip.from_numpy(k_cache, requires_grad=False), hip.from_numpy(v_cache, requires_grad=False)
    tm = None if mask is None else hip.from_numpy(mask, requires_grad=False)
    tq, tkn, tvn = (hip.from_numpy(a, requires_grad=False) for a in (q, kn, vn))
    assert tq.decode_attention_supported(heads, k_cache.shape[1])
    out = tq.decode_attention(tkn, tvn, tk, tv, position(hip, t), heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=probs)
    assert out.shape == q.shape and not out.requires_grad and out.ctx is None
    p = None
    if probs:
        assert out.attention_probs.shape == (q.shape[0], heads, 1, k_cache.shape[1]) and not out.attention_probs.requires_grad
        p = out.attention_probs.numpy()
    return out.numpy(), p, tk.numpy(), tv.numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = [(shape, capacity) for shape in SHAPES for capacity in CAPACITIES]


@pytest.mark.parametrize("shape,capacity", CASES, ids=["%dx%dx%d-cap%d" % (c[0] + (c[1],)) for c in CASES])
def test_sweep_against_the_float64_composite(hip, shape, capacity):
    b, heads, d = shape
    k, v, q, kn, vn = operands(b, capacity, heads, d)
    ts = sorted({t for t in T_VALUES + (capacity - 1,) if t < capacity})
    for t in ts:
        kp, vp = prefix(k, kn, t), prefix(v, vn, t)
        for masked in (False, True):
            mask = padding_mask(b, capacity) if masked else None
            ctx, probs, _, _ = decode(hip, q, kn, vn, k, v, t, heads, mask)
            want_ctx, want_probs = reference64(q, kp, vp, heads, mask)
            comp_ctx, comp_probs = composite32(hip, q, kp, vp, heads, mask)
            what = "%s cap %d t %d %s" % (shape, capacity, t, "mask" if masked else "nomask")
            assert np.isfinite(ctx).all() and np.isfinite(probs).all(), what
            np.testing.assert_allclose(probs.sum(axis=-1), 1.0, rtol=0, atol=1e-5, err_msg=what)
            assert (bits(probs[..., t + 1:]) == 0).all(), what                           # exact +0.0 beyond t
            for name, g, c, r in (("context", ctx, comp_ctx, want_ctx), ("probs", probs[..., :t + 1], comp_probs, want_probs)):
                e_fused, e_comp = rel_frobenius(g, r), rel_frobenius(c, r)
                print("%s %s: fused %.3e, fp32 composite %.3e" % (what, name, e_fused, e_comp))
                assert e_fused <= 1e-5, (what, name, e_fused, e_comp)
                assert e_fused <= 2 * e_comp + 2e-7, (what, name, e_fused, e_comp)
            if t == 0 and not masked:
                assert (probs[..., 0] == 1.0).all(), what
                np.testing.assert_array_equal(bits(ctx), bits(vn), err_msg=what)


@pytest.mark.parametrize("shape,capacity,t", [((2, 2, 32), 64, 0), ((2, 2, 32), 64, 33), ((3, 1, 64), 129, 17), ((2, 2, 64), 129, 128),
                                              ((2, 2, 64), 512, 300)])
def test_cache_discipline_bit_for_bit(hip, shape, capacity, t):
    """rows above t are neither read (NaN there changes nothing) nor written, rows below t stay, row t becomes k_new / v_new -
    compared as uint32 -, and mask entries beyond t do not matter"""
    b, heads, d = shape
    k, v, q, kn, vn = operands(b, capacity, heads, d, seed=11)
    mask = padding_mask(b, capacity)
    k0, v0 = k.copy(), v.copy()
    k0[:, t:], v0[:, t:] = 0, 0
    kn_, vn_ = k.copy(), v.copy()
    kn_[:, t:], vn_[:, t:] = np.nan, np.nan
    for m in (None, mask):
        ctx0, p0, k_after0, v_after0 = decode(hip, q, kn, vn, k0, v0, t, heads, m)
        ctx1, p1, k_after1, v_after1 = decode(hip, q, kn, vn, kn_, vn_, t, heads, m)
        assert np.isfinite(ctx1).all() and np.isfinite(p1).all()
        np.testing.assert_array_equal(bits(ctx1), bits(ctx0))
        np.testing.assert_array_equal(bits(p1), bits(p0))
        for before, after, new in ((k0, k_after0, kn), (v0, v_after0, vn), (kn_, k_after1, kn), (vn_, v_after1, vn)):
            np.testing.assert_array_equal(bits(after[:, :t]), bits(before[:, :t]))
            np.testing.assert_array_equal(bits(after[:, t:t + 1]), bits(new))
            np.testing.assert_array_equal(bits(after[:, t + 1:]), bits(before[:, t + 1:]))
    other = mask.copy()
    other[:, t + 1:] = np.nan
    ctx2, p2, _, _ = decode(hip, q, kn, vn, k0, v0, t, heads, other)
    ctx3, p3, _, _ = decode(hip, q, kn, vn, k0, v0, t, heads, mask)
    np.testing.assert_array_equal(bits(ctx2), bits(ctx3))
    np.testing.assert_array_equal(bits(p2), bits(p3))


def test_independence_determinism_and_operands_in_place(hip):
    b, heads, d, capacity, t = 3, 2, 64, 129, 70
    width = heads * d
    k, v, q, kn, vn = operands(b, capacity, heads, d, seed=13)
    mask = padding_mask(b, capacity)
    ctx, probs, k_after, _ = decode(hip, q, kn, vn, k, v, t, heads, mask)
    again = decode(hip, q, kn, vn, k, v, t, heads, mask)
    np.testing.assert_array_equal(bits(again[0]), bits(ctx))                             # two identical calls: identical bits
    np.testing.assert_array_equal(bits(again[1]), bits(probs))
    for i in range(b):                                                                   # an element of the batch alone
        one = decode(hip, q[i:i + 1], kn[i:i + 1], vn[i:i + 1], k[i:i + 1], v[i:i + 1], t, heads, mask[i:i + 1])
        np.testing.assert_array_equal(bits(one[0]), bits(ctx[i:i + 1]))
        np.testing.assert_array_equal(bits(one[1]), bits(probs[i:i + 1]))
    # q | k | v of one (b, 1, 3 * width) projection buffer, taken in place (no copy: the views' storage is the buffer's)
    qkv = hip.from_numpy(np.concatenate([q, kn, vn], axis=2), requires_grad=False)
    views = [type(qkv)(qkv.data, (b, 1, width), (3 * width, 3 * width, 1), i * width, qkv.dtype, requires_grad=False) for i in range(3)]
    from lightgrad_amd.autograd.hip import ops_attention
    assert all(ops_attention._token_row(view, "test")[0] is view for view in views)
    tk, tv, tm = (hip.from_numpy(a, requires_grad=False) for a in (k, v, mask))
    out = views[0].decode_attention(views[1], views[2], tk, tv, position(hip, t), heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=True)
    np.testing.assert_array_equal(bits(out.numpy()), bits(ctx))
    np.testing.assert_array_equal(bits(out.attention_probs.numpy()), bits(probs))
    np.testing.assert_array_equal(bits(tk.numpy()), bits(k_after))
    # (b, width) operands give (b, width)
    flat = [hip.from_numpy(a[:, 0], requires_grad=False) for a in (q, kn, vn)]
    tk2, tv2 = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
    out2 = flat[0].decode_attention(flat[1], flat[2], tk2, tv2, position(hip, t), heads=heads, scale=math.sqrt(d) ** -1, mask=tm)
    assert out2.shape == (b, width) and not hasattr(out2, "attention_probs")
    np.testing.assert_array_equal(bits(out2.numpy()), bits(ctx[:, 0]))


def test_the_ops_are_inference_ops(hip):
    """operands that ask for a gradient are refused while gradients are enabled, taken under no_grad; the result is no tape node"""
    import lightgrad_amd as light
    b, heads, d, capacity = 2, 2, 32, 8
    k, v, q, kn, vn = operands(b, capacity, heads, d)
    tk, tv = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
    tq, tkn, tvn = hip.from_numpy(q), hip.from_numpy(kn), hip.from_numpy(vn)
    assert tq.requires_grad
    with pytest.raises(AssertionError, match="inference op"):
        tq.decode_attention(tkn, tvn, tk, tv, position(hip, 3), heads=heads, scale=1.0)
    with light.no_grad():
        out = tq.decode_attention(tkn, tvn, tk, tv, position(hip, 3), heads=heads, scale=1.0)
    assert not out.requires_grad and out.ctx is None
    with pytest.raises(AssertionError, match="requires_grad"):
        with light.no_grad():
            tq.decode_attention(tkn, tvn, hip.from_numpy(k), tv, position(hip, 3), heads=heads, scale=1.0)
    assert not tq.decode_attention_supported(heads, 513) and not tq.decode_attention_supported(4, 8)


# ---- through the C ABI --------------------------------------------------------------------------------------------------------

SENTINEL = 3.0


class Call(object):
    """one (batch, capacity, heads * d) problem on the device and the entry's argument list, every argument replaceable"""
    def __init__(self, hip, b=2, heads=2, d=32, capacity=8, t=3):
        from lightgrad_amd.autograd.hip import lib as L
        self.lib = L.lib()
        width = heads * d
        k, v, q, kn, vn = operands(b, capacity, heads, d)
        self.k, self.v, self.q, self.kn, self.vn = (hip.from_numpy(a, requires_grad=False) for a in (k, v, q, kn, vn))
        self.o = hip.from_numpy(np.full((b, width), SENTINEL, np.float32), requires_grad=False)
        self.p = hip.from_numpy(np.full((b, heads, capacity), SENTINEL, np.float32), requires_grad=False)
        self.mask = hip.from_numpy(np.ones((b, capacity), np.float32), requires_grad=False)
        self.pos = position(hip, t)
        self.host = dict(k=k, v=v)
        self.args = dict(q=self.q.ptr, sbq=width, k_new=self.kn.ptr, sbk=width, v_new=self.vn.ptr, sbv=width, k_cache=self.k.ptr,
                         v_cache=self.v.ptr, ldc=width, sbc=capacity * width, pos=self.pos.ptr, o=self.o.ptr, sbo=width, p=self.p.ptr,
                         batch=b, heads=heads, capacity=capacity, D=d, scale=0.2, mask=None, sbm=0)

    def __call__(self, **override):
        return self.lib.lg_attention_decode_f32(*dict(self.args, **override).values())

    def untouched(self):
        return ((self.o.numpy() == SENTINEL).all() and (self.p.numpy() == SENTINEL).all()
                and (bits(self.k.numpy()) == bits(self.host["k"])).all() and (bits(self.v.numpy()) == bits(self.host["v"])).all())


@pytest.mark.parametrize("bad", ["capacity", "-1"])
def test_position_out_of_range_is_reported_not_a_fault(hip, bad):
    call = Call(hip)
    call.pos.upload_(np.array([call.args["capacity"] if bad == "capacity" else -1], np.int32))
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the word
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert call.untouched()                                               # caches and outputs hold their previous bits
    call.pos.upload_(np.array([3], np.int32))
    assert call() == 0                                                    # a following valid call works
    HipDevice.synchronize()
    got = call.o.numpy()
    assert np.isfinite(got).all() and not (got == SENTINEL).any()
    np.testing.assert_array_equal(bits(call.k.numpy()[:, 3]), bits(call.kn.numpy()[:, 0]))


REFUSALS = [("D", dict(D=48)), ("D16", dict(D=16)), ("capacity0", dict(capacity=0)), ("capacity513", dict(capacity=513)),
            ("pitch-q", dict(sbq=66)), ("pitch-cache-row", dict(ldc=66)), ("pitch-cache-batch", dict(sbc=8 * 64 + 2)), ("pitch-o", dict(sbo=65)),
            ("base-q", "q"), ("base-k_new", "k_new"), ("base-v_new", "v_new"), ("base-k_cache", "k_cache"), ("base-v_cache", "v_cache"),
            ("base-o", "o"), ("row-pitch-below-width", dict(ldc=32)), ("mask-pitch", dict(mask=True, sbm=7)), ("mask-pitch-1", dict(mask=True, sbm=1))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_launch_nothing(hip, name, change):
    call = Call(hip)
    if isinstance(change, str):
        change = {change: call.args[change] + 4}                          # a base that is not 16-byte aligned
    if change.get("mask") is True:
        change = dict(change, mask=call.mask.ptr)
    assert call(**change) == LG_EINVAL, name
    assert b"lg_attention_decode_f32" in call.lib.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched(), name


def test_first_refusal_wins_and_a_shared_mask_row_is_taken(hip):
    """the checks run in their fixed order: D / capacity before alignment before the row pitch before the mask; sbm = 0 (one mask
    row for the batch) and sbm >= capacity are fine"""
    call = Call(hip)
    assert call(D=48, q=call.args["q"] + 4, ldc=32, mask=call.mask.ptr, sbm=1) == LG_EINVAL and b"unsupported" in call.lib.lg_last_error()
    assert call(q=call.args["q"] + 4, ldc=32, mask=call.mask.ptr, sbm=1) == LG_EINVAL and b"aligned" in call.lib.lg_last_error()
    assert call(ldc=32, mask=call.mask.ptr, sbm=1) == LG_EINVAL and b"row pitch" in call.lib.lg_last_error()
    assert call(mask=call.mask.ptr, sbm=1) == LG_EINVAL and b"mask" in call.lib.lg_last_error()
    assert call.untouched()
    assert call(mask=call.mask.ptr, sbm=0) == 0 and call(mask=call.mask.ptr, sbm=8) == 0 and call(batch=0) == 0
    HipDevice.synchronize()


# ---- the model ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prompt-mask"])
def test_teacher_forced_logits_on_hip(hip, masked):
    """tests/test_decode_cpu.py's run on HipTensor, against the same float64 yardstick"""
    ref64, cpu32 = dc.teacher_reference(masked)
    got = dc.teacher_forced(hip, masked)
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="cached forward on HipTensor")


def test_generate_on_hip_equals_the_float64_tokens(hip):
    want = dc.assert_margins_rule_out_ties()
    np.testing.assert_array_equal(dc.greedy(hip), want)


def test_a_decode_step_takes_the_decode_launch_twice(hip, recorder):  # noqa: F811
    """a decode step of the 2-layer model: exactly 2 lg_attention_decode_f32 calls and no prefill attention call"""
    _, ids = dc.parameters()
    model = dc.make_model(hip)
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    model(hip.from_numpy(ids[:, :dc.S0], requires_grad=False), cache=cache)
    assert recorder.calls and "lg_attention_decode_f32" not in recorder.calls and len(recorder.calls) == dc.CFG["num_hidden_layers"]
    del recorder.calls[:]
    model(hip.from_numpy(ids[:, dc.S0:dc.S0 + 1], requires_grad=False), cache=cache)
    assert recorder.calls == ["lg_attention_decode_f32"] * 2


def test_a_captured_decode_step_replays_the_eager_tokens(hip):
    """one decode step captured after an eager prefill and replayed 7 times: with the prompt's own token, 8 new tokens per
    sequence, bit for bit those of the eager `generate`.  The position ends at s0 + 7: it is the position of the token the next
    step would FEED (the contract of lg_attention_decode_f32's `pos`) - the 8th new token sits in column s0 + 7 of the ids and
    has been fed to nobody - so the 7 advances of 7 steps, not 8"""
    _, ids = dc.parameters()
    model = dc.make_model(hip)
    eager = dc.greedy(hip, new=8, model=model)
    np.testing.assert_array_equal(eager, dc.assert_margins_rule_out_ties()[:, :8])
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    graph = HipGraph()
    replayed = dc.greedy(hip, new=8, model=model, cache=cache, graph=graph)
    print("kernels of one captured decode step: %d" % graph.kernel_count())
    np.testing.assert_array_equal(bits(replayed), bits(eager))
    assert int(cache.pos.numpy()[0]) == cache.length == dc.S0 + 7
    graph.destroy()
