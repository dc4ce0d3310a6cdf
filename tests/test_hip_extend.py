"""lg_attention_extend_f32 (csrc/extend.hip) and what stands on it: `extend_attention`, `self_attention_extend`, the append
forward of examples/bert.py on HipTensor (`model(ids, cache=cache, append=True)`), `generate(prefill_chunk=)`,
`generate(append=True)`, and a captured append step.

The error rule is the project's own (test_hip_decode.py): a result must be within 1e-5 (relative Frobenius) of the float64
composite and no further from it than twice the fp32 composite on the same backend plus 2e-7.

The kernel's partition (csrc/extend.hip): one workgroup per block of 32 query rows; the keys 0 .. t + m - 1 stream in chunks of
128, the cache's rows below t, the new tokens' from t on, up to Kend = round32(t + q0 + rows of the block); row i of the block
sees the columns [0, t + q0 + i].  The sweep takes t and m at, one below and one above a block edge (32) and a chunk edge
(128), so the cache / new-row seam falls on, before and behind both, with one and with several query blocks."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd.autograd.hip import HipDevice, HipGraph
from common import assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from test_hip_attention_masked import padding_mask
from test_hip_attention_dispatch import recorder  # noqa: F401  (fixture)
import decode_cases as dc
import extend_cases as ec

pytestmark = pytest.mark.gpu

LG_EINVAL = -1
T_VALUES = (0, 1, 31, 32, 33, 95, 96, 127, 128, 129, 255, 256, 383)
M_VALUES = (1, 2, 31, 32, 33, 64, 65, 127, 128, 129)
SHAPES = [(1, 1, 32), (2, 2, 32), (3, 1, 64), (2, 2, 64)]
CAPACITIES = [1, 5, 64, 129, 512]


def pairs(shape, capacity):
    """the (t, m) of one case.  The two shapes of a head size share the lists: each takes every second value of T_VALUES with
    an m that walks through M_VALUES, and every second value of M_VALUES with a t that walks through T_VALUES - at capacity 512
    every value of both lists occurs for each D; a smaller capacity takes what fits.  Always: t + m == capacity and (0, capacity)"""
    half = SHAPES.index(shape) % 2
    chosen = {(0, capacity), (capacity - min(capacity, 33), min(capacity, 33)), (capacity - 1, 1)}
    for i, t in enumerate(T_VALUES):
        if i % 2 == half:
            fits = [m for m in M_VALUES if t + m <= capacity]
            if fits:
                chosen.add((t, fits[(i // 2 + half) % len(fits)]))
    for j, m in enumerate(M_VALUES):
        if j % 2 == half:
            fits = [t for t in T_VALUES if t + m <= capacity]
            if fits:
                chosen.add((fits[(3 * j + 1 + half) % len(fits)], m))
    return sorted(chosen)


def test_the_sweep_holds_every_value_of_both_lists_for_each_head_size():
    for d in (32, 64):
        seen = [p for shape in SHAPES if shape[2] == d for p in pairs(shape, 512)]
        assert {t for t, _ in seen} >= set(T_VALUES) and {m for _, m in seen} >= set(M_VALUES)
    for shape in SHAPES:
        for capacity in CAPACITIES:
            ps = pairs(shape, capacity)
            assert (0, capacity) in ps and all(t >= 0 and m >= 1 and t + m <= capacity for t, m in ps) and len(ps) <= 16


def operands(b, capacity, m, heads, d, seed=7):
    """uniform(-1.5, 1.5) draws as test_hip_decode.operands: the cache's rows (b, capacity, width) twice, and the new tokens' q,
    k_new, v_new (b, m, width)"""
    rng = np.random.RandomState(seed)
    width = heads * d
    k, v = (rng.uniform(-1.5, 1.5, (b, capacity, width)).astype(np.float32) for _ in range(2))
    q, kn, vn = (rng.uniform(-1.5, 1.5, (b, m, width)).astype(np.float32) for _ in range(3))
    return k, v, q, kn, vn


def prefix(cache, new, t):
    """rows 0 .. t + m - 1 the attention sees: the cache's below t, the new tokens' from t on"""
    return np.concatenate([cache[:, :t], new], axis=1)


def reference64(q, k, v, t, heads, mask):
    """the float64 composite: row i over the keys 0 .. t + i of k, v (b, t + m, width) - scores, key bias, softmax over the keys
    the row sees, context.  Returns the context (b, m, width) and the probabilities (b, heads, m, t + m), 0 beyond t + i"""
    q, k, v = (a.astype(np.float64) for a in (q, k, v))
    b, n, width = k.shape
    m, d = q.shape[1], width // heads
    scores = np.einsum("bihd,bjhd->bhij", q.reshape(b, m, heads, d), k.reshape(b, n, heads, d)) / math.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask[:, :n].astype(np.float64)) * -10000.0)[:, None, None, :]
    seen = np.arange(n)[None, :] <= t + np.arange(m)[:, None]
    scores = np.where(seen, scores, -np.inf)
    e = np.exp(scores - scores.max(axis=-1, keepdims=True))
    probs = e / e.sum(axis=-1, keepdims=True)
    return np.einsum("bhij,bjhd->bihd", probs, v.reshape(b, n, heads, d)).reshape(b, m, width), probs


def composite32(hip, q, k, v, t, heads, mask):
    """the same over the tensor API on the HIP backend in float32 (examples/bert.py, composite append branch)"""
    b, n, width = k.shape
    m, d = q.shape[1], width // heads
    tq, tk, tv = (hip.from_numpy(a, requires_grad=False) for a in (q, k, v))
    q4 = tq.reshape(b, m, heads, d).transpose(0, 2, 1, 3)
    k4 = tk.reshape(b, n, heads, d).transpose(0, 2, 3, 1)
    v4 = tv.reshape(b, n, heads, d).transpose(0, 2, 1, 3)
    scores = (q4 @ k4) / math.sqrt(d)
    if mask is not None:
        km = hip.from_numpy(np.ascontiguousarray(mask[:, :n]), requires_grad=False)
        scores = scores + (1.0 - km.reshape(b, 1, 1, n)) * -10000.0
    tri = hip.from_numpy(np.tril(np.ones((1, 1, m, n), np.float32), k=t), requires_grad=False)
    scores = scores + (1.0 - tri) * -10000.0
    probs = scores.softmax(axis=-1)
    return (probs @ v4).transpose(0, 2, 1, 3).reshape(b, m, width).numpy(), probs.numpy()


def position(hip, t):
    return hip.from_numpy(np.array([t], np.int32), requires_grad=False)


def extend(hip, q, kn, vn, k_cache, v_cache, t, heads, mask=None, probs=True):
    """one launch through the op on fresh device copies of everything: (context, probs, k_cache after, v_cache after) as numpy"""
    d = q.shape[-1] // heads
    tk, tv = hip.from_numpy(k_cache, requires_grad=False), hip.from_numpy(v_cache, requires_grad=False)
    tm = None if mask is None else hip.from_numpy(mask, requires_grad=False)
    tq, tkn, tvn = (hip.from_numpy(a, requires_grad=False) for a in (q, kn, vn))
    assert tq.extend_attention_supported(heads, k_cache.shape[1])
    out = tq.extend_attention(tkn, tvn, tk, tv, position(hip, t), heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=probs)
    assert out.shape == q.shape and not out.requires_grad and out.ctx is None
    p = None
    if probs:
        assert out.attention_probs.shape == (q.shape[0], heads, q.shape[1], k_cache.shape[1]) and not out.attention_probs.requires_grad
        p = out.attention_probs.numpy()
    return out.numpy(), p, tk.numpy(), tv.numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = [(shape, capacity) for shape in SHAPES for capacity in CAPACITIES]


@pytest.mark.parametrize("shape,capacity", CASES, ids=["%dx%dx%d-cap%d" % (c[0] + (c[1],)) for c in CASES])
def test_sweep_against_the_float64_composite(hip, shape, capacity):
    b, heads, d = shape
    for t, m in pairs(shape, capacity):
        k, v, q, kn, vn = operands(b, capacity, m, heads, d)
        kp, vp = prefix(k, kn, t), prefix(v, vn, t)
        n = t + m
        beyond = np.arange(capacity)[None, :] > t + np.arange(m)[:, None]                 # (m, capacity): columns row i does not see
        for masked in (False, True):
            mask = padding_mask(b, capacity) if masked else None
            ctx, probs, _, _ = extend(hip, q, kn, vn, k, v, t, heads, mask)
            want_ctx, want_probs = reference64(q, kp, vp, t, heads, mask)
            comp_ctx, comp_probs = composite32(hip, q, kp, vp, t, heads, mask)
            what = "%s cap %d t %d m %d %s" % (shape, capacity, t, m, "mask" if masked else "nomask")
            assert np.isfinite(ctx).all() and np.isfinite(probs).all(), what
            np.testing.assert_allclose(probs.sum(axis=-1), 1.0, rtol=0, atol=1e-5, err_msg=what)
            assert (bits(probs)[:, :, beyond] == 0).all(), what                          # exact +0.0 beyond column t + i
            for name, g, c, r in (("context", ctx, comp_ctx, want_ctx), ("probs", probs[..., :n], comp_probs, want_probs)):
                e_fused, e_comp = rel_frobenius(g, r), rel_frobenius(c, r)
                print("%s %s: fused %.3e, fp32 composite %.3e" % (what, name, e_fused, e_comp))
                assert e_fused <= 1e-5, (what, name, e_fused, e_comp)
                assert e_fused <= 2 * e_comp + 2e-7, (what, name, e_fused, e_comp)
            if t == 0 and not masked:
                assert (probs[:, :, 0, 0] == 1.0).all(), what                            # row 0 of an empty cache sees itself only
                np.testing.assert_array_equal(bits(ctx[:, 0]), bits(vn[:, 0]), err_msg=what)


DISCIPLINE = [((2, 2, 32), 64, 0, 5), ((2, 2, 32), 64, 33, 31), ((3, 1, 64), 129, 17, 40), ((2, 2, 64), 129, 96, 33),
              ((1, 1, 32), 512, 127, 129), ((2, 2, 64), 512, 300, 130)]


@pytest.mark.parametrize("shape,capacity,t,m", DISCIPLINE)
def test_cache_discipline_bit_for_bit(hip, shape, capacity, t, m):
    """rows from t on may hold NaN before the launch: rows below t stay, rows t .. t + m - 1 become k_new / v_new, rows beyond
    keep their NaN bits - compared as uint32 -, the outputs are finite and those of a cache of zeros; mask entries beyond
    t + m do not matter; operands in place in one (b, m, 3 * width) buffer give the bits of contiguous copies"""
    b, heads, d = shape
    width = heads * d
    k, v, q, kn, vn = operands(b, capacity, m, heads, d, seed=11)
    mask = padding_mask(b, capacity)
    k0, v0 = k.copy(), v.copy()
    k0[:, t:], v0[:, t:] = 0, 0
    k1, v1 = k.copy(), v.copy()
    k1[:, t:], v1[:, t:] = np.nan, np.nan
    for km in (None, mask):
        ctx0, p0, k_after0, v_after0 = extend(hip, q, kn, vn, k0, v0, t, heads, km)
        ctx1, p1, k_after1, v_after1 = extend(hip, q, kn, vn, k1, v1, t, heads, km)
        assert np.isfinite(ctx1).all() and np.isfinite(p1).all()
        np.testing.assert_array_equal(bits(ctx1), bits(ctx0))
        np.testing.assert_array_equal(bits(p1), bits(p0))
        for before, after, new in ((k0, k_after0, kn), (v0, v_after0, vn), (k1, k_after1, kn), (v1, v_after1, vn)):
            np.testing.assert_array_equal(bits(after[:, :t]), bits(before[:, :t]))
            np.testing.assert_array_equal(bits(after[:, t:t + m]), bits(new))
            np.testing.assert_array_equal(bits(after[:, t + m:]), bits(before[:, t + m:]))
    other = mask.copy()
    other[:, t + m:] = np.nan
    ctx2, p2, _, _ = extend(hip, q, kn, vn, k0, v0, t, heads, other)
    ctx3, p3, k_after3, v_after3 = extend(hip, q, kn, vn, k0, v0, t, heads, mask)
    np.testing.assert_array_equal(bits(ctx2), bits(ctx3))
    np.testing.assert_array_equal(bits(p2), bits(p3))
    # q | k | v of one (b, m, 3 * width) projection buffer, taken in place (no copy: the views' storage is the buffer's)
    qkv = hip.from_numpy(np.concatenate([q, kn, vn], axis=2), requires_grad=False)
    views = [type(qkv)(qkv.data, (b, m, width), (m * 3 * width, 3 * width, 1), i * width, qkv.dtype, requires_grad=False) for i in range(3)]
    from lightgrad_amd.autograd.hip import ops_attention
    assert all(ops_attention._token_rows_in_place(view, "test")[0] is view for view in views)
    tk, tv, tm = (hip.from_numpy(a, requires_grad=False) for a in (k0, v0, mask))
    out = views[0].extend_attention(views[1], views[2], tk, tv, position(hip, t), heads=heads, scale=math.sqrt(d) ** -1, mask=tm, probs=True)
    np.testing.assert_array_equal(bits(out.numpy()), bits(ctx3))
    np.testing.assert_array_equal(bits(out.attention_probs.numpy()), bits(p3))
    np.testing.assert_array_equal(bits(tk.numpy()), bits(k_after3))
    np.testing.assert_array_equal(bits(tv.numpy()), bits(v_after3))


@pytest.mark.parametrize("capacity,t,m", [(129, 70, 40), (512, 120, 45)])
def test_determinism_and_independence(hip, capacity, t, m):
    b, heads, d = 3, 2, 64
    k, v, q, kn, vn = operands(b, capacity, m, heads, d, seed=13)
    mask = padding_mask(b, capacity)
    ctx, probs, k_after, _ = extend(hip, q, kn, vn, k, v, t, heads, mask)
    again = extend(hip, q, kn, vn, k, v, t, heads, mask)
    np.testing.assert_array_equal(bits(again[0]), bits(ctx))                             # two identical calls: identical bits
    np.testing.assert_array_equal(bits(again[1]), bits(probs))
    for i in range(b):                                                                   # an element of the batch alone
        one = extend(hip, q[i:i + 1], kn[i:i + 1], vn[i:i + 1], k[i:i + 1], v[i:i + 1], t, heads, mask[i:i + 1])
        np.testing.assert_array_equal(bits(one[0]), bits(ctx[i:i + 1]))
        np.testing.assert_array_equal(bits(one[1]), bits(probs[i:i + 1]))
    shared = extend(hip, q, kn, vn, k, v, t, heads, mask[1:2])                           # one (1, capacity) row for the batch
    repeated = extend(hip, q, kn, vn, k, v, t, heads, np.repeat(mask[1:2], b, axis=0))
    np.testing.assert_array_equal(bits(shared[0]), bits(repeated[0]))
    np.testing.assert_array_equal(bits(shared[1]), bits(repeated[1]))
    without = extend(hip, q, kn, vn, k, v, t, heads, mask, probs=False)                  # the context does not depend on `p`
    assert without[1] is None
    np.testing.assert_array_equal(bits(without[0]), bits(ctx))


def test_the_ops_are_inference_ops(hip):
    """operands that ask for a gradient are refused while gradients are enabled, taken under no_grad; the result is no tape node"""
    b, heads, d, capacity, m = 2, 2, 32, 8, 3
    k, v, q, kn, vn = operands(b, capacity, m, heads, d)
    tk, tv = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
    tq, tkn, tvn = hip.from_numpy(q), hip.from_numpy(kn), hip.from_numpy(vn)
    assert tq.requires_grad
    with pytest.raises(AssertionError, match="inference op"):
        tq.extend_attention(tkn, tvn, tk, tv, position(hip, 3), heads=heads, scale=1.0)
    with light.no_grad():
        out = tq.extend_attention(tkn, tvn, tk, tv, position(hip, 3), heads=heads, scale=1.0)
    assert not out.requires_grad and out.ctx is None and not hasattr(out, "attention_probs")
    with pytest.raises(AssertionError, match="requires_grad"):
        with light.no_grad():
            tq.extend_attention(tkn, tvn, hip.from_numpy(k), tv, position(hip, 3), heads=heads, scale=1.0)
    assert not tq.extend_attention_supported(heads, 513) and not tq.extend_attention_supported(4, 8) and not tq.extend_attention_supported(heads, 2)
    # the one-node form: the same refusals, and the bits of the three projections followed by `extend_attention`
    rng = np.random.RandomState(5)
    width = heads * d
    x = hip.from_numpy(rng.uniform(-1, 1, (b, m, width)).astype(np.float32))
    ws = [hip.from_numpy(rng.uniform(-0.2, 0.2, (width, width)).astype(np.float32)) for _ in range(3)]
    bs = [hip.from_numpy(rng.uniform(-0.2, 0.2, (width,)).astype(np.float32)) for _ in range(3)]
    params = [t for pair in zip(ws, bs) for t in pair]
    with pytest.raises(AssertionError, match="inference op"):
        x.self_attention_extend(*params, tk, tv, position(hip, 3), heads=heads, scale=0.2)
    assert x.self_attention_extend_supported(ws[0], heads, capacity) and not x.self_attention_extend_supported(ws[0], heads, 2)
    with light.no_grad():
        tk2, tv2 = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
        one = x.self_attention_extend(*params, tk2, tv2, position(hip, 3), heads=heads, scale=0.2, probs=True)
        x2 = x.reshape(b * m, width)
        qkv = [(x2 @ w.transpose(1, 0) + c).reshape(b, m, width) for w, c in zip(ws, bs)]
        tk3, tv3 = hip.from_numpy(k, requires_grad=False), hip.from_numpy(v, requires_grad=False)
        two = qkv[0].extend_attention(qkv[1], qkv[2], tk3, tv3, position(hip, 3), heads=heads, scale=0.2, probs=True)
    assert not one.requires_grad and one.ctx is None and one.attention_probs.shape == (b, heads, m, capacity)
    np.testing.assert_allclose(one.numpy(), two.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_allclose(tk2.numpy(), tk3.numpy(), rtol=0, atol=1e-5)
    np.testing.assert_array_equal(bits(tk2.numpy()[:, :3]), bits(k[:, :3]))


# ---- through the C ABI --------------------------------------------------------------------------------------------------------

SENTINEL = 3.0


class Call(object):
    """one (batch, capacity, heads * d) problem with m new tokens on the device and the entry's argument list, every argument
    replaceable"""
    def __init__(self, hip, b=2, heads=2, d=32, capacity=8, m=3, t=3):
        from lightgrad_amd.autograd.hip import lib as L
        self.lib = L.lib()
        width = heads * d
        k, v, q, kn, vn = operands(b, capacity, m, heads, d)
        self.k, self.v, self.q, self.kn, self.vn = (hip.from_numpy(a, requires_grad=False) for a in (k, v, q, kn, vn))
        self.o = hip.from_numpy(np.full((b, m, width), SENTINEL, np.float32), requires_grad=False)
        self.p = hip.from_numpy(np.full((b, heads, m, capacity), SENTINEL, np.float32), requires_grad=False)
        self.mask = hip.from_numpy(np.ones((b, capacity), np.float32), requires_grad=False)
        self.pos = position(hip, t)
        self.host = dict(k=k, v=v)
        self.args = dict(q=self.q.ptr, ldq=width, sbq=m * width, k_new=self.kn.ptr, ldk=width, sbk=m * width, v_new=self.vn.ptr, ldv=width,
                         sbv=m * width, k_cache=self.k.ptr, v_cache=self.v.ptr, ldc=width, sbc=capacity * width, pos=self.pos.ptr,
                         o=self.o.ptr, ldo=width, sbo=m * width, p=self.p.ptr, batch=b, heads=heads, m=m, capacity=capacity, D=d, scale=0.2,
                         mask=None, sbm=0)

    def __call__(self, **override):
        return self.lib.lg_attention_extend_f32(*dict(self.args, **override).values())

    def untouched(self):
        return ((self.o.numpy() == SENTINEL).all() and (self.p.numpy() == SENTINEL).all()
                and (bits(self.k.numpy()) == bits(self.host["k"])).all() and (bits(self.v.numpy()) == bits(self.host["v"])).all())


@pytest.mark.parametrize("bad", ["capacity - m + 1", "-1"])
def test_position_out_of_range_is_reported_not_a_fault(hip, bad):
    call = Call(hip)
    call.pos.upload_(np.array([call.args["capacity"] - call.args["m"] + 1 if bad != "-1" else -1], np.int32))
    assert call() == 0                                                    # the launch itself is fine: the kernel reads the word
    with pytest.raises(IndexError):
        HipDevice.synchronize()
    HipDevice.synchronize()                                               # reported once
    assert call.untouched()                                               # caches and outputs hold their previous bits
    call.pos.upload_(np.array([call.args["capacity"] - call.args["m"]], np.int32))
    assert call() == 0                                                    # a following valid call works: the last rows of the cache
    HipDevice.synchronize()
    got = call.o.numpy()
    assert np.isfinite(got).all() and not (got == SENTINEL).any()
    np.testing.assert_array_equal(bits(call.k.numpy()[:, 5:8]), bits(call.kn.numpy()))


REFUSALS = [("D", dict(D=48)), ("D16", dict(D=16)), ("capacity0", dict(capacity=0)), ("capacity513", dict(capacity=513)), ("m0", dict(m=0)),
            ("m-above-capacity", dict(m=9)), ("pitch-q", dict(ldq=66)), ("pitch-q-batch", dict(sbq=3 * 64 + 2)), ("pitch-k_new", dict(ldk=65)),
            ("pitch-v_new-negative", dict(ldv=-64)), ("pitch-cache-row", dict(ldc=66)), ("pitch-cache-batch", dict(sbc=8 * 64 + 2)),
            ("pitch-o", dict(ldo=65)), ("base-q", "q"), ("base-k_new", "k_new"), ("base-v_new", "v_new"), ("base-k_cache", "k_cache"),
            ("base-v_cache", "v_cache"), ("base-o", "o"), ("base-p", "p"), ("row-pitch-below-width", dict(ldc=32)),
            ("mask-pitch", dict(mask=True, sbm=7)), ("mask-pitch-1", dict(mask=True, sbm=1)), ("k_new-in-k_cache", dict(k_new="k_cache")),
            ("v_new-in-k_cache", dict(v_new="k_cache")), ("k_new-in-v_cache", dict(k_new="v_cache")), ("v_new-behind-row-0", dict(v_new="v_cache+"))]


@pytest.mark.parametrize("name,change", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_host_refusals_launch_nothing(hip, name, change):
    call = Call(hip)
    if isinstance(change, str):
        change = {change: call.args[change] + 4}                          # a base that is not 16-byte aligned
    if change.get("mask") is True:
        change = dict(change, mask=call.mask.ptr)
    for key, value in list(change.items()):
        if isinstance(value, str):                                        # new rows inside a cache: at its base, or from its row 2 on
            change[key] = call.args[value.rstrip("+")] + (2 * 64 * 4 if value.endswith("+") else 0)
    assert call(**change) == LG_EINVAL, name
    assert b"lg_attention_extend_f32" in call.lib.lg_last_error()
    HipDevice.synchronize()
    assert call.untouched(), name


def test_first_refusal_wins_and_a_shared_mask_row_is_taken(hip):
    """the checks run in their fixed order: D / m / capacity before alignment before the row pitch before the mask before the
    overlap; sbm = 0 (one mask row for the batch) and sbm >= capacity are fine, batch == 0 launches nothing"""
    call = Call(hip)
    wrong = dict(D=48, q=call.args["q"] + 4, ldc=32, mask=call.mask.ptr, sbm=1, k_new=call.args["k_cache"])
    order = [("D", b"unsupported"), ("q", b"aligned"), ("ldc", b"row pitch"), ("sbm", b"mask"), ("k_new", b"overlap")]
    for key, word in order:
        assert call(**wrong) == LG_EINVAL and word in call.lib.lg_last_error(), key
        wrong.pop(key)
        if key == "sbm":
            wrong["sbm"] = 0
    assert call.untouched()
    assert call(batch=0, D=48) == LG_EINVAL and call(batch=0, q=call.args["q"] + 4) == 0 and call.untouched()
    assert call(mask=call.mask.ptr, sbm=0) == 0 and call(mask=call.mask.ptr, sbm=8) == 0
    HipDevice.synchronize()


# ---- the model ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "prompt-mask"])
def test_appended_pieces_on_hip(hip, masked):
    """tests/test_extend_cpu.py's run on HipTensor, against the same float64 yardstick"""
    ref64, cpu32 = ec.append_reference(masked)
    got = ec.append_run(hip, masked)
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="append forward on HipTensor")


def test_two_turns_and_chunked_prefill_on_hip_equal_the_float64_tokens(hip):
    first, second = ec.assert_two_turn_margins_rule_out_ties()
    got1, got2 = ec.two_turns(hip)
    np.testing.assert_array_equal(got1, first)
    np.testing.assert_array_equal(got2, second)
    np.testing.assert_array_equal(dc.greedy(hip, prefill_chunk=3), dc.assert_margins_rule_out_ties())


def test_an_append_takes_the_extend_launch_once_per_layer(hip, recorder):  # noqa: F811
    """an append of 3 tokens to the 2-layer model's filled cache: exactly 2 lg_attention_extend_f32 calls, no decode call and no
    prefill attention call; a (b, 1) step without append= keeps the decode launch"""
    _, ids = dc.parameters()
    model = dc.make_model(hip)
    cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
    model(hip.from_numpy(ids[:, :dc.S0], requires_grad=False), cache=cache)
    del recorder.calls[:]
    model(hip.from_numpy(ids[:, dc.S0:dc.S0 + 3], requires_grad=False), cache=cache, append=True)
    cache.advance(3)
    assert recorder.calls == ["lg_attention_extend_f32"] * 2
    del recorder.calls[:]
    model(hip.from_numpy(ids[:, dc.S0 + 3:dc.S0 + 4], requires_grad=False), cache=cache)
    assert recorder.calls == ["lg_attention_decode_f32"] * 2


def test_a_captured_append_step_replays_the_eager_run(hip):
    """a step that appends 3 given tokens and moves the position on by 3, captured once behind an eager prefill and replayed
    twice with different tokens in its id buffer: logits and caches are those of two eager appends - the replay reads the
    position word, which the first replay moved"""
    _, ids = dc.parameters()
    model = dc.make_model(hip)
    m, s0 = 3, dc.S0
    pieces = [np.ascontiguousarray(ids[:, s0:s0 + m]), np.ascontiguousarray(ids[:, s0 + m:s0 + 2 * m])]

    def filled_cache():
        cache = nn.KVCache(dc.CFG["num_hidden_layers"], dc.B, dc.CAPACITY, dc.CFG["hidden_size"], like=model.cls.predictions.bias)
        model(hip.from_numpy(ids[:, :s0], requires_grad=False), cache=cache)
        return cache

    cache = filled_cache()
    tokens = hip.from_numpy(pieces[0].copy(), requires_grad=False)
    eager = []
    for piece in pieces:
        tokens.upload_(piece)
        eager.append(model(tokens, cache=cache, append=True).numpy().copy())
        cache.advance(m)
    assert cache.length == s0 + 2 * m == int(cache.pos.numpy()[0])

    replayed_cache = filled_cache()
    tokens.upload_(pieces[0])
    model(tokens, cache=replayed_cache, append=True)                   # once eagerly: kernels loaded, constants uploaded
    graph = HipGraph()
    with graph.capture():
        logits = model(tokens, cache=replayed_cache, append=True)       # recorded, not run: the host mirror moves on, the device position not
        replayed_cache.advance(m)
    for i, piece in enumerate(pieces):
        tokens.upload_(piece)
        graph.replay()
        if i:
            replayed_cache.replayed(m)
        np.testing.assert_array_equal(bits(logits.numpy()), bits(eager[i]))
    assert int(replayed_cache.pos.numpy()[0]) == replayed_cache.length == s0 + 2 * m
    for layer in range(dc.CFG["num_hidden_layers"]):
        for a, b_ in ((cache.k[layer], replayed_cache.k[layer]), (cache.v[layer], replayed_cache.v[layer])):
            np.testing.assert_array_equal(bits(a.numpy()[:, :s0 + 2 * m]), bits(b_.numpy()[:, :s0 + 2 * m]))
    print("kernels of one captured append step: %d" % graph.kernel_count())
    graph.destroy()
