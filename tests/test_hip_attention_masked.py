"""the masked / tail forms of the fused attention launches (csrc/attention.hip TAIL instantiations, ops `masked_attention` and
`self_attention(mask=)`): any length 1 .. 128 and a key-padding mask, against a float64 run of the model's own composite lines
(examples/bert.py: divide by sqrt(d), additive mask, softmax), against the unmasked kernels bit for bit where the two must agree,
and through the C ABI for what lies outside the sequence.

The error rule is the project's own (test_hip_bert.py::test_fused_attention): context, probabilities, dq, dk, dv each within 1e-5
(relative Frobenius) of the float64 composite, and no further from it than twice the fp32 composite on the same backend + 2e-7."""
import math
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
from common import float64_tape, rel_frobenius
from test_bert_cpu import bert

pytestmark = pytest.mark.gpu

NAMES = ("context", "probs", "dq", "dk", "dv")


def composite(q, k, v, heads, mask=None):
    """examples/bert.py BertSelfAttention.forward, composite branch"""
    b, s, width = q.shape
    d = width // heads
    q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
    k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
    v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
    scores = (q4 @ k4) / math.sqrt(d)
    if mask is not None:
        m = mask.reshape(mask.shape[0], 1, 1, mask.shape[1])
        scores = scores + ((1.0 - m) * -10000.0).detach()
    probs = scores.softmax(axis=-1)
    return (probs @ v4).transpose(0, 2, 1, 3).reshape(b, s, width), probs


def operands(b, s, heads, d, seed=7):
    rng = np.random.RandomState(seed)
    width = heads * d
    q, k, v = (rng.uniform(-1.5, 1.5, (b, s, width)).astype(np.float32) for _ in range(3))
    w = rng.uniform(-1, 1, (b, s, width)).astype(np.float32)
    return q, k, v, w


def padding_mask(b, s):
    """trailing padding of a different length per batch element, one hole in the middle, one value 0.5; key 0 stays at 1"""
    m = np.ones((b, s), np.float32)
    for i in range(b):
        m[i, max(1, s - (1 + i) * max(1, s // 5)):] = 0
    if s >= 5:
        m[0, s // 3] = 0
        m[b - 1, 1] = 0.5
    assert (m == 1).any(axis=1).all()
    return m


def run(T, f64, arrays, heads, mask, how):
    """[context, probs, dq, dk, dv] as numpy; how = "fused" (masked_attention), "plain" (attention) or "composite" """
    q, k, v, w = arrays
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    ts = [T.from_numpy(cast(x)) for x in (q, k, v)]
    tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
    scale = float(np.sqrt(q.shape[2] // heads)) ** -1
    if how == "fused":
        assert ts[0].masked_attention_supported(heads)
        out = ts[0].masked_attention(ts[1], ts[2], heads=heads, scale=scale, mask=tm)
        probs = out.attention_probs
        assert probs.shape == (q.shape[0], heads, q.shape[1], q.shape[1]) and not probs.requires_grad
    elif how == "plain":
        out = ts[0].attention(ts[1], ts[2], heads=heads, scale=scale)
        probs = out.attention_probs
    else:
        out, probs = composite(*ts, heads, tm)
    (out * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), probs.numpy()] + [t.grad.numpy() for t in ts]


def assert_close_to_float64(got, comp, want, what):
    for name, g, c, r in zip(NAMES, got, comp, want):
        e_fused, e_comp = rel_frobenius(g, r), rel_frobenius(c, r)
        print("%s %s: fused %.3e, fp32 composite %.3e" % (what, name, e_fused, e_comp))
        assert e_fused <= 1e-5, (what, name, e_fused, e_comp)
        assert e_fused <= 2 * e_comp + 2e-7, (what, name, e_fused, e_comp)


SHAPES = [(1, 1, 1, 32), (2, 5, 2, 32), (3, 33, 1, 64), (2, 48, 2, 32), (1, 100, 3, 32), (2, 127, 2, 64), (2, 64, 2, 64), (2, 128, 2, 64)]


# every shape with a mask; without one only where the length is no multiple of 32 (length alone, at a multiple of 32, is the
# unmasked kernels' ground: test_hip_bert.py)
CASES = [(shape, False) for shape in SHAPES if shape[1] % 32] + [(shape, True) for shape in SHAPES]


@pytest.mark.parametrize("shape,masked", CASES, ids=["%dx%dx%dx%d-%s" % (c[0] + ("mask" if c[1] else "length_only",)) for c in CASES])
def test_sweep_against_the_float64_composite(hip, shape, masked):
    b, s, heads, d = shape
    arrays = operands(b, s, heads, d)
    mask = padding_mask(b, s) if masked else None
    got = run(hip, False, arrays, heads, mask, "fused")
    comp = run(hip, False, arrays, heads, mask, "composite")
    with float64_tape():
        want = run(CpuTensor, True, arrays, heads, mask, "composite")
    assert all(np.isfinite(x).all() for x in got)
    probs = got[1]
    np.testing.assert_allclose(probs.sum(axis=-1), 1.0, rtol=0, atol=1e-5)
    if mask is not None:
        gone = np.broadcast_to((mask == 0)[:, None, None, :], probs.shape)
        assert (probs[gone] == 0).all()
    assert_close_to_float64(got, comp, want, str((b, s, heads, d, masked)))


def test_a_mask_of_ones_is_the_unmasked_kernel(hip):
    b, s, heads, d = 2, 64, 2, 32
    arrays = operands(b, s, heads, d, seed=8)
    plain = run(hip, False, arrays, heads, None, "plain")
    for mask in (np.ones((b, s), np.float32), np.ones((1, s), np.float32), None):
        for name, x, y in zip(NAMES, run(hip, False, arrays, heads, mask, "fused"), plain):
            np.testing.assert_array_equal(x, y, err_msg=name)
    # a (1, s) mask is its (b, s) tiling
    row = padding_mask(1, s)
    for name, x, y in zip(NAMES, run(hip, False, arrays, heads, row, "fused"), run(hip, False, arrays, heads, np.tile(row, (b, 1)), "fused")):
        np.testing.assert_array_equal(x, y, err_msg=name)
    # a mask that is not row-contiguous is copied once: same values
    wide = hip.from_numpy(np.repeat(np.tile(row, (b, 1)), 2, axis=1), requires_grad=False)
    strided = hip(wide.data, (b, s), (2 * s, 2), wide.offset, wide.dtype, requires_grad=False)
    ts = [hip.from_numpy(x) for x in arrays[:3]]
    out = ts[0].masked_attention(ts[1], ts[2], heads=heads, scale=float(np.sqrt(d)) ** -1, mask=strided)
    np.testing.assert_array_equal(out.numpy(), run(hip, False, arrays, heads, row, "fused")[0])


def self_attention_run(hip, x, params, w, heads, scale, mask):
    leaf = hip.from_numpy(x)
    tx = leaf * 1.0
    ps = [hip.from_numpy(p) for p in params]
    extra = {} if mask is None else {"mask": hip.from_numpy(mask, requires_grad=False)}
    out = tx.self_attention(*ps, heads=heads, scale=scale, **extra)
    (out * hip.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), out.attention_probs.numpy(), leaf.grad.numpy()] + [p.grad.numpy() for p in ps]


def test_self_attention_with_a_mask_of_ones_is_self_attention(hip):
    rng = np.random.RandomState(10)
    b, s, hidden, heads, d = 2, 64, 96, 2, 32
    width = heads * d
    x = rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32)
    params = []
    for _ in range(3):
        params += [rng.uniform(-0.2, 0.2, (width, hidden)).astype(np.float32), rng.uniform(-0.2, 0.2, (width,)).astype(np.float32)]
    w = rng.uniform(-1, 1, (b, s, width)).astype(np.float32)
    scale = float(np.sqrt(d)) ** -1
    plain = self_attention_run(hip, x, params, w, heads, scale, None)
    ones = self_attention_run(hip, x, params, w, heads, scale, np.ones((b, s), np.float32))
    for i, (p, o) in enumerate(zip(plain, ones)):
        np.testing.assert_array_equal(o, p, err_msg=str(i))
    # asked as before, the predicate answers as before; masked=True asks the new entry point
    t = hip.from_numpy(np.ascontiguousarray(x[:, :48]))
    wq = hip.from_numpy(params[0])
    assert not t.self_attention_supported(wq, heads) and t.self_attention_supported(wq, heads, masked=True)


def test_nothing_outside_the_sequence_is_read_or_written(hip):
    """through the C ABI at s = 45: operands are views of buffers with 19 more rows per batch element, all NaN; outputs have
    that batch pitch too and are prefilled - the results are the dense run's bits, every surplus row is as it was"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, s, heads, d, extra = 2, 45, 2, 32, 19
    w = heads * d
    rows = s + extra
    q, k, v, g = operands(b, s, heads, d, seed=11)
    mask = padding_mask(b, s)
    sentinel = np.float32(-777.25)

    def padded(x):
        buf = np.full((b, rows, w), np.nan, np.float32)
        buf[:, :s] = x
        return hip.from_numpy(buf, requires_grad=False)

    def fresh(shape):
        return hip.from_numpy(np.full(shape, sentinel, np.float32), requires_grad=False)

    def launch(ops, mask_t, sbm, pitch, outs, p):
        tq, tk, tv, tg = ops
        o, dq, dk, dv = outs
        L.check(lib.lg_attention_masked_fwd_f32(tq.ptr, w, pitch, tk.ptr, w, pitch, tv.ptr, w, pitch, o.ptr, w, pitch, p.ptr,
                                                b, heads, s, d, 0.2, mask_t.ptr, sbm))
        L.check(lib.lg_attention_masked_bwd_f32(tq.ptr, w, pitch, tk.ptr, w, pitch, tv.ptr, w, pitch, tg.ptr, w, pitch, p.ptr,
                                                dq.ptr, w, pitch, dk.ptr, w, pitch, dv.ptr, w, pitch, b, heads, s, d, 0.2))

    n_p = b * heads * s * s
    dense_ops = [hip.from_numpy(x, requires_grad=False) for x in (q, k, v, g)]
    dense_outs = [fresh((b, s, w)) for _ in range(4)]
    dense_p = fresh((n_p,))
    launch(dense_ops, hip.from_numpy(mask, requires_grad=False), s, s * w, dense_outs, dense_p)

    wide_ops = [padded(x) for x in (q, k, v, g)]
    wide_outs = [fresh((b, rows, w)) for _ in range(4)]
    wide_p = fresh((n_p + 64,))
    mbuf = np.full((b, rows), np.nan, np.float32)
    mbuf[:, :s] = mask
    launch(wide_ops, hip.from_numpy(mbuf, requires_grad=False), rows, rows * w, wide_outs, wide_p)

    assert np.isfinite(dense_p.numpy()).all()
    np.testing.assert_array_equal(wide_p.numpy()[:n_p], dense_p.numpy())
    assert (wide_p.numpy()[n_p:] == sentinel).all()
    for name, wide, dense in zip(("o", "dq", "dk", "dv"), wide_outs, dense_outs):
        wide, dense = wide.numpy(), dense.numpy()
        assert np.isfinite(dense).all() and (dense != sentinel).any(), name
        np.testing.assert_array_equal(wide[:, :s], dense, err_msg=name)
        assert (wide[:, s:] == sentinel).all(), name
    for name, t, x in zip("qkvg", wide_ops, (q, k, v, g)):
        after = t.numpy()
        np.testing.assert_array_equal(after[:, :s], x, err_msg=name)
        assert np.isnan(after[:, s:]).all(), name


def test_a_fully_masked_batch_element(hip):
    """every key of batch element 1 masked: -10000 on all of its scores - finite everywhere, its rows still sum to 1 (no closeness
    to float64 is asked of it: the add quantises fp32 scores to ~1e-3 on any implementation); element 0 is its run alone"""
    b, s, heads, d = 2, 48, 2, 32
    arrays = operands(b, s, heads, d, seed=12)
    mask = padding_mask(b, s)
    mask[1, :] = 0
    both = run(hip, False, arrays, heads, mask, "fused")
    alone = run(hip, False, [x[:1] for x in arrays], heads, mask[:1], "fused")
    for name, x, y in zip(NAMES, both, alone):
        assert np.isfinite(x).all(), name
        np.testing.assert_array_equal(x[:1], y, err_msg=name)
    np.testing.assert_allclose(both[1][1].sum(axis=-1), 1.0, rtol=0, atol=1e-5)


def test_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    assert lib.lg_attention_masked_supported(48, 32) == 1 and lib.lg_attention_masked_supported(129, 32) == 0
    assert lib.lg_attention_masked_supported(0, 32) == 0 and lib.lg_attention_masked_supported(64, 48) == 0
    assert lib.lg_attention_masked_supported(1, 64) == 1 and lib.lg_attention_masked_supported(128, 64) == 1
    b, s, heads, d = 2, 48, 2, 32
    w = heads * d
    q, k, v, o = (hip.from_numpy(np.zeros((b, s, w), np.float32), requires_grad=False) for _ in range(4))
    p = hip.from_numpy(np.zeros((b, heads, s, s), np.float32), requires_grad=False)
    m = hip.from_numpy(np.ones((b, s), np.float32), requires_grad=False)
    fwd = lambda **kw: lib.lg_attention_masked_fwd_f32(kw.get("q", q.ptr), kw.get("ld", w), s * w, k.ptr, w, s * w, v.ptr, w, s * w,     # noqa: E731
                                                       kw.get("o", o.ptr), w, s * w, kw.get("p", p.ptr), b, heads, kw.get("s", s), kw.get("d", d), 0.5,
                                                       kw.get("m", m.ptr), kw.get("sbm", s))
    assert fwd() == 0 and fwd(sbm=0) == 0 and fwd(m=None, sbm=7) == 0 and fwd(sbm=s + 5) == 0
    assert fwd(sbm=s - 1) == -1 and b"mask" in lib.lg_last_error()
    assert fwd(sbm=-s) == -1 and b"mask" in lib.lg_last_error()
    assert fwd(s=129) == -1 and b"unsupported" in lib.lg_last_error()
    assert fwd(s=0) == -1 and fwd(d=16) == -1
    assert fwd(q=q.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert fwd(ld=w - 4) == -1 and b"row pitch" in lib.lg_last_error()
    assert fwd(o=None) == -1 and b"aligned" in lib.lg_last_error()
    assert fwd(p=None) == -1
    bwd = lambda **kw: lib.lg_attention_masked_bwd_f32(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, kw.get("g", o.ptr), kw.get("ld", w), s * w,     # noqa: E731
                                                       p.ptr, q.ptr, w, s * w, k.ptr, w, s * w, kw.get("dv", v.ptr), w, s * w,
                                                       b, heads, kw.get("s", s), d, 0.5)
    assert bwd(dv=None) == -1 and b"aligned" in lib.lg_last_error()
    assert bwd(g=o.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert bwd(ld=w - 4) == -1 and b"row pitch" in lib.lg_last_error()
    assert bwd(s=130) == -1 and b"unsupported" in lib.lg_last_error()
    # the op: a mask of the wrong shape or dtype, and one that wants a gradient
    tq, tk, tv = (hip.from_numpy(np.zeros((b, s, w), np.float32)) for _ in range(3))
    for bad in (hip.from_numpy(np.ones((b, s + 1), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((b + 1, s), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((s,), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((b, s), np.int32), requires_grad=False)):
        with pytest.raises(AssertionError, match="mask"):
            tq.masked_attention(tk, tv, heads=heads, mask=bad)
    with pytest.raises(AssertionError, match="gradient"):
        tq.masked_attention(tk, tv, heads=heads, mask=hip.from_numpy(np.ones((b, s), np.float32), requires_grad=True))
    with pytest.raises(AssertionError, match="gradient"):
        tq.masked_attention(tk, tv, heads, 1.0, hip.from_numpy(np.ones((b, s), np.float32), requires_grad=True))
    with pytest.raises(AssertionError, match="unsupported"):
        big = hip.from_numpy(np.zeros((1, 129, w), np.float32))
        big.masked_attention(big, big, heads=heads)


def tape_nodes(t):
    seen, stack, names = set(), [t.ctx], []
    while stack:
        node = stack.pop()
        if node is None or id(node) in seen:
            continue
        seen.add(id(node))
        names.append(node.__class__.__name__)
        stack += [p.ctx for p in node.parent_tensors]
    return names


@pytest.mark.parametrize("s,with_mask", [(48, True), (37, False)])
def test_model_with_padding_masks_takes_the_node(hip, s, with_mask):
    """BertForMaskedLM, one layer, hidden 64 / 2 heads, batch 2 with padding masks of two lengths (and a length that is no multiple
    of 32 without a mask): a `self_attention` node on the tape, every parameter gradient of the weighted-logits objective
    within 1e-5 of a float64 run (test_hip_bert.py::test_forward_backward_matches_cpu_backend's rule and its key-bias exemption)"""
    cfg = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
               max_position_embeddings=48, type_vocab_size=2)
    rng = np.random.RandomState(13)
    ids = rng.randint(0, 60, (2, s)).astype(np.int32)
    w = rng.uniform(-1, 1, (2, s, 60)).astype(np.float32)
    mask = None
    if with_mask:
        mask = np.ones((2, s), np.float32)
        mask[0, 40:] = 0
        mask[1, 29:] = 0

    def build():
        np.random.seed(5)
        return bert.BertForMaskedLM(**cfg)

    def forward(model, T, f64):
        cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
        extra = {} if mask is None else {"attention_mask": T.from_numpy(cast(mask), requires_grad=False)}
        logits = model(T.from_numpy(ids, requires_grad=False), **extra)
        (logits * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
        return logits

    hip_model = build().map_parameters(lambda p: p.hip())
    values = {n: p.numpy().astype(np.float64) for n, p in build().named_parameters()}
    logits = forward(hip_model, hip, False)
    assert "self_attention" in tape_nodes(logits)
    with float64_tape():
        ref_model = build()
        ref_model.load_parameters(values)
        assert all(p.dtype == np.float64 for p in ref_model.parameters())
        ref_logits = forward(ref_model, CpuTensor, True)
    e = rel_frobenius(logits.numpy(), ref_logits.numpy())
    assert e <= 1e-5, ("logits", e)
    for (n, p), (_, r) in zip(hip_model.named_parameters(), ref_model.named_parameters()):
        got, ref = p.grad.numpy().astype(np.float64), r.grad.numpy()
        if ".key.bias" in n:
            # mathematically zero (softmax is invariant to a per-query constant): rounding noise
            assert np.abs(got).max() < 1e-6 and np.abs(ref).max() < 1e-12, (n, np.abs(got).max(), np.abs(ref).max())
            continue
        e = rel_frobenius(got, ref)
        print("%-60s %.3e" % (n, e))
        assert e <= 1e-5, (n, e)
