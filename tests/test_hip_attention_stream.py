"""streaming attention (csrc/attention_stream.hip; `stream_attention`, `self_attention(probs=False)`, examples/bert.py config key
`attention_probs=False`) against a float64 run of the model's composite lines: context, lse, dq, dk, dv each within 1e-5 (relative
Frobenius).  Lengths on both sides of the 32-key block, the 128-row chunk / workgroup, the old 512 limit, both parities of s % 4."""
import math
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
from common import float64_tape, rel_frobenius
from test_bert_cpu import bert
from test_hip_attention_masked import composite, operands, padding_mask, tape_nodes

pytestmark = pytest.mark.gpu

NAMES = ("context", "lse", "dq", "dk", "dv")


def reference(q, k, v, heads, mask, causal):
    """the composite lines of examples/bert.py; causal: their `(1 - tril) * -10000` behind the key-padding bias"""
    if not causal:
        return composite(q, k, v, heads, mask)[0]
    (b, s, width), d = q.shape, q.shape[2] // heads
    q4, k4, v4 = (t.reshape(b, s, heads, d).transpose(*axes) for t, axes in ((q, (0, 2, 1, 3)), (k, (0, 2, 3, 1)), (v, (0, 2, 1, 3))))
    scores = (q4 @ k4) / math.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, s)) * -10000.0).detach()
    tril = q.__class__.from_numpy(np.tril(np.ones((1, 1, s, s), dtype=q.dtype)), requires_grad=False)
    scores = scores + ((1.0 - tril) * -10000.0).detach()
    return (scores.softmax(axis=-1) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)


def lse_float64(arrays, heads, mask, causal):
    """log-sum-exp of the biased scores, in float64"""
    q, k = (x.astype(np.float64) for x in arrays[:2])
    (b, s, width), d = q.shape, q.shape[2] // heads
    scores = np.einsum("bihd,bjhd->bhij", q.reshape(b, s, heads, d), k.reshape(b, s, heads, d)) / math.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask.astype(np.float64)) * -10000.0)[:, None, None, :]
    if causal:
        scores = scores + (1.0 - np.tril(np.ones((s, s)))) * -10000.0
    top = scores.max(axis=-1)
    return top + np.log(np.exp(scores - top[..., None]).sum(axis=-1))


def run(T, f64, arrays, heads, mask, causal, fused):
    """[context, lse, dq, dk, dv] as numpy (lse: None for the composite)"""
    q, k, v, w = arrays
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    ts = [T.from_numpy(cast(x)) for x in (q, k, v)]
    tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
    if fused:
        assert ts[0].stream_attention_supported(heads)
        out = ts[0].stream_attention(ts[1], ts[2], heads=heads, scale=float(np.sqrt(q.shape[2] // heads)) ** -1, mask=tm, causal=causal)
        assert out.attention_probs is None and out.attention_lse.shape == (q.shape[0], heads, q.shape[1]) and not out.attention_lse.requires_grad
        lse = out.attention_lse.numpy()
    else:
        out, lse = reference(*ts, heads, tm, causal), None
    (out * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), lse] + [t.grad.numpy() for t in ts]


def check_against_float64(hip, arrays, heads, mask, causal, what):
    got = run(hip, False, arrays, heads, mask, causal, True)
    comp = run(hip, False, arrays, heads, mask, causal, False)
    with float64_tape():
        want = run(CpuTensor, True, arrays, heads, mask, causal, False)
    want[1] = lse_float64(arrays, heads, mask, causal)
    errors = [(name, rel_frobenius(g, r), float("nan") if c is None else rel_frobenius(c, r)) for name, g, c, r in zip(NAMES, got, comp, want)]
    for name, fused, fp32 in errors:
        print("%s %s: fused %.3e, fp32 composite %.3e" % (what, name, fused, fp32))
    assert all(np.isfinite(x).all() for x in got)
    for name, fused, _ in errors:
        assert fused <= 1e-5, (what, name, fused)
    return got


SHAPES = [(1, 1, 1, 32), (1, 31, 2, 32), (2, 33, 1, 64), (1, 127, 2, 64), (1, 129, 1, 32), (2, 160, 2, 32), (1, 257, 2, 64),
          (1, 300, 1, 32), (1, 513, 2, 64), (1, 640, 1, 32)]
CASES = [(shape, masked, causal) for shape in SHAPES for masked in (True, False) for causal in (False, True)]


@pytest.mark.parametrize("shape,masked,causal", CASES, ids=["%dx%dx%dx%d-%s-%s" % (c[0] + ("mask" if c[1] else "no_mask", "causal" if c[2] else "full"))
                                                            for c in CASES])
def test_sweep_against_the_float64_composite(hip, shape, masked, causal):
    b, s, heads, d = shape
    check_against_float64(hip, operands(b, s, heads, d), heads, padding_mask(b, s) if masked else None, causal, str(shape + (masked, causal)))


@pytest.mark.parametrize("which", ["first_chunk_padding", "last_two_chunks_padding"])
def test_the_maximum_arrives_late(hip, which):
    """s = 300 is three chunks of keys: keys 0 .. 139 masked leave the first chunk all -10000, so the running maximum jumps by 1e4
    in the second; keys 100.. masked leave the last two entirely padding"""
    mask = np.ones((1, 300), np.float32)
    mask[:, (slice(0, 140) if which == "first_chunk_padding" else slice(100, None))] = 0
    check_against_float64(hip, operands(1, 300, 2, 32, seed=21), 2, mask, False, which)


def test_a_fully_masked_batch_element(hip):
    """every key of element 1 masked: finite everywhere; element 0 is bit for bit its run alone"""
    arrays, mask = operands(2, 300, 1, 32, seed=22), padding_mask(2, 300)
    mask[1, :] = 0
    both = run(hip, False, arrays, 1, mask, False, True)
    alone = run(hip, False, [x[:1] for x in arrays], 1, mask[:1], False, True)
    for name, x, y in zip(NAMES, both, alone):
        assert np.isfinite(x).all(), name
        np.testing.assert_array_equal(x[:1], y, err_msg=name)


@pytest.mark.parametrize("causal", [False, True])
def test_two_runs_give_the_same_bits(hip, causal):
    b, s, heads, d = 2, 300, 2, 64
    arrays, row = operands(b, s, heads, d, seed=23), padding_mask(1, s)
    same = [(padding_mask(b, s), padding_mask(b, s)), (None, np.ones((b, s), np.float32)), (row, np.tile(row, (b, 1)))]
    for one, other in same:
        for name, x, y in zip(NAMES, run(hip, False, arrays, heads, one, causal, True), run(hip, False, arrays, heads, other, causal, True)):
            np.testing.assert_array_equal(x, y, err_msg=name)


def test_in_place_operands_and_nothing_outside_them_through_the_c_abi(hip):
    """q, k, v (and dq, dk, dv) as column blocks of one NaN-filled (b, s + 3, 3 w + 8) buffer, o and dO with a row pitch above w: the
    bits of the dense run; surplus rows, pitch gaps and the floats around lse and delta keep their NaN; operands unchanged"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, s, heads, d, extra, gap = 2, 131, 2, 32, 3, 8
    w, n = heads * d, b * heads * s
    rows, ld3, ldo = s + extra, 3 * w + gap, w + gap
    q, k, v, g = operands(b, s, heads, d, seed=24)
    tm = hip.from_numpy(padding_mask(b, s), requires_grad=False)
    nan = lambda shape: hip.from_numpy(np.full(shape, np.nan, np.float32), requires_grad=False)      # noqa: E731

    def launch(tq, tk, tv, tg, o, dq, dk, dv, ld_in, sb_in, ld_out, sb_out, lse, delta):
        ins = (tq, ld_in, sb_in, tk, ld_in, sb_in, tv, ld_in, sb_in, o, ld_out, sb_out)
        L.check(lib.lg_attention_stream_fwd_f32(*ins, lse, b, heads, s, d, 0.2, tm.ptr, s, 1))
        L.check(lib.lg_attention_stream_bwd_f32(*ins, tg, ld_out, sb_out, lse, delta, dq, ld_in, sb_in, dk, ld_in, sb_in, dv, ld_in, sb_in,
                                                b, heads, s, d, 0.2, tm.ptr, s, 1))

    dense = [hip.from_numpy(x, requires_grad=False) for x in (q, k, v, g)] + [nan((b, s, w)) for _ in range(4)]
    rows_d = [nan((n,)), nan((n,))]
    launch(*(t.ptr for t in dense), w, s * w, w, s * w, *(t.ptr for t in rows_d))
    want = [t.numpy() for t in dense[4:] + rows_d]
    assert all(np.isfinite(x).all() for x in want)

    qkv_host, g_host = np.full((b, rows, ld3), np.nan, np.float32), np.full((b, rows, ldo), np.nan, np.float32)
    for i, x in enumerate((q, k, v)):
        qkv_host[:, :s, i * w:(i + 1) * w] = x
    g_host[:, :s, :w] = g
    qkv, tg = hip.from_numpy(qkv_host, requires_grad=False), hip.from_numpy(g_host, requires_grad=False)
    o, dqkv, lse, delta = nan((b, rows, ldo)), nan((b, rows, ld3)), nan((n + 10,)), nan((n + 10,))
    launch(qkv.ptr, qkv.ptr + 4 * w, qkv.ptr + 8 * w, tg.ptr, o.ptr, dqkv.ptr, dqkv.ptr + 4 * w, dqkv.ptr + 8 * w,
           ld3, rows * ld3, ldo, rows * ldo, lse.ptr + 4 * 5, delta.ptr + 4 * 5)
    for name, t, ref in (("lse", lse, want[4]), ("delta", delta, want[5])):
        x = t.numpy()
        np.testing.assert_array_equal(x[5:5 + n], ref, err_msg=name)
        assert np.isnan(x[:5]).all() and np.isnan(x[5 + n:]).all(), name
    got_o, got_d = o.numpy(), dqkv.numpy()
    np.testing.assert_array_equal(got_o[:, :s, :w], want[0], err_msg="o")
    assert np.isnan(got_o[:, s:]).all() and np.isnan(got_o[:, :, w:]).all()
    for i, name in enumerate(("dq", "dk", "dv")):
        np.testing.assert_array_equal(got_d[:, :s, i * w:(i + 1) * w], want[1 + i], err_msg=name)
    assert np.isnan(got_d[:, s:]).all() and np.isnan(got_d[:, :, 3 * w:]).all()
    np.testing.assert_array_equal(qkv.numpy(), qkv_host)
    np.testing.assert_array_equal(tg.numpy(), g_host)


def test_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib, fits = L.lib(), L.lib().lg_attention_stream_supported
    assert fits(1, 32) == 1 and fits(513, 64) == 1 and fits(8192, 32) == 1 and fits(0, 32) == 0 and fits(64, 48) == 0
    assert lib.lg_attention_long_supported(513, 64) == 0
    b, s, heads, d, w = 2, 131, 2, 32, 64
    q, k, v, o = (hip.from_numpy(np.zeros((b, s, w), np.float32), requires_grad=False) for _ in range(4))
    lse, delta = (hip.from_numpy(np.zeros((b, heads, s), np.float32), requires_grad=False) for _ in range(2))
    m = hip.from_numpy(np.ones((b, s), np.float32), requires_grad=False)

    def fwd(**kw):
        return lib.lg_attention_stream_fwd_f32(kw.get("q", q.ptr), kw.get("ld", w), s * w, k.ptr, w, s * w, v.ptr, w, s * w, kw.get("o", o.ptr), w, s * w,
                                               kw.get("lse", lse.ptr), kw.get("b", b), heads, kw.get("s", s), kw.get("d", d), 0.5,
                                               kw.get("m", m.ptr), kw.get("sbm", s), 0)

    def bwd(**kw):
        return lib.lg_attention_stream_bwd_f32(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, o.ptr, w, s * w, kw.get("g", o.ptr), kw.get("ld", w), s * w,
                                               lse.ptr, kw.get("delta", delta.ptr), q.ptr, w, s * w, k.ptr, w, s * w, kw.get("dv", v.ptr), w, s * w,
                                               kw.get("b", b), heads, kw.get("s", s), kw.get("d", d), 0.5, m.ptr, kw.get("sbm", s), 0)

    assert fwd() == 0 and fwd(sbm=0) == 0 and fwd(m=None, sbm=7) == 0 and fwd(b=0, q=None) == 0 and bwd(b=0, dv=None) == 0
    for call in (fwd, bwd):
        assert call(sbm=s - 1) == -1 and b"mask" in lib.lg_last_error()
        assert call(s=0) == -1 and b"unsupported" in lib.lg_last_error()
        assert call(d=48) == -1 and b"unsupported" in lib.lg_last_error()
        assert call(ld=w - 4) == -1 and b"row pitch" in lib.lg_last_error()
    assert fwd(q=q.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert fwd(o=None) == -1 and b"aligned" in lib.lg_last_error() and fwd(lse=None) == -1
    assert bwd(g=o.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert bwd(dv=None) == -1 and b"aligned" in lib.lg_last_error() and bwd(delta=None) == -1
    x, wq = hip.from_numpy(np.zeros((b, 530, 64), np.float32)), hip.from_numpy(np.zeros((w, 64), np.float32))
    assert not x.self_attention_supported(wq, heads, long=True) and x.self_attention_supported(wq, heads, stream=True)
    with pytest.raises(AssertionError, match="dropout > 0 with probs=False"):
        x.self_attention(wq, hip.from_numpy(np.zeros(w, np.float32)), wq, hip.from_numpy(np.zeros(w, np.float32)), wq,
                         hip.from_numpy(np.zeros(w, np.float32)), heads=heads, dropout=0.1, probs=False)


MODEL_CFG = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
                 max_position_embeddings=544, type_vocab_size=2, attention_probs=False)


@pytest.mark.parametrize("causal", [False, True], ids=["padding_masks", "causal"])
def test_model_beyond_512_positions_takes_the_node(hip, causal):
    """BertForMaskedLM, one layer, hidden 64 / 2 heads, batch 2 at 530 positions with padding masks of two lengths, and causal
    without a mask: a `self_attention` node on the tape, no probabilities, logits and every parameter gradient within 1e-5 of a
    float64 run (test_hip_attention_long.py's rule and its key-bias exemption)"""
    rng, s = np.random.RandomState(25), 530
    ids, w = rng.randint(0, 60, (2, s)).astype(np.int32), rng.uniform(-1, 1, (2, s, 60)).astype(np.float32)
    mask = None if causal else np.ones((2, s), np.float32)
    if not causal:
        mask[0, 520:], mask[1, 97:] = 0, 0

    def build():
        np.random.seed(5)
        return bert.BertForMaskedLM(**dict(MODEL_CFG, causal=causal))

    def forward(model, T, f64):
        cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
        extra = {} if mask is None else {"attention_mask": T.from_numpy(cast(mask), requires_grad=False)}
        hidden = model.bert.embeddings(T.from_numpy(ids, requires_grad=False))
        assert model.bert.encoder.layer[0].attention.self(hidden, **extra)[1] is None
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
        ref_logits = forward(ref_model, CpuTensor, True)
    assert rel_frobenius(logits.numpy(), ref_logits.numpy()) <= 1e-5, "logits"
    for (n, p), (_, r) in zip(hip_model.named_parameters(), ref_model.named_parameters()):
        got, ref = p.grad.numpy().astype(np.float64), r.grad.numpy()
        if ".key.bias" in n:
            # mathematically zero (softmax is invariant to a per-query constant): rounding noise
            assert np.abs(got).max() < 1e-6 and np.abs(ref).max() < 1e-12, (n, np.abs(got).max(), np.abs(ref).max())
            continue
        print("%-60s %.3e" % (n, rel_frobenius(got, ref)))
        assert rel_frobenius(got, ref) <= 1e-5, n


def test_the_node_replayed_from_a_graph(hip):
    """forward and backward of `self_attention(probs=False)` at 530 positions with a mask, captured once: two replays give the eager bits"""
    from lightgrad_amd.autograd.hip import HipGraph
    rng, (b, s, hidden, heads, d) = np.random.RandomState(26), (2, 530, 64, 2, 32)
    width = heads * d
    x = hip.from_numpy(rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32))
    params = []
    for _ in range(3):
        params += [hip.from_numpy(rng.uniform(-0.2, 0.2, (width, hidden)).astype(np.float32)),
                   hip.from_numpy(rng.uniform(-0.2, 0.2, (width,)).astype(np.float32))]
    w = hip.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32), requires_grad=False)
    mask = hip.from_numpy(padding_mask(b, s), requires_grad=False)

    def step():
        for t in [x] + params:
            t.zero_grad()
        out = x.self_attention(*params, heads=heads, scale=float(np.sqrt(d)) ** -1, mask=mask, probs=False)
        (out * w).backward(allow_fill=True)
        return out

    def results(out):
        return [out.numpy(), out.attention_lse.numpy(), x.grad.numpy()] + [p.grad.numpy() for p in params]

    step()
    eager = results(step())
    graph = HipGraph()
    with graph.capture():
        out = step()
    for _ in range(2):
        graph.replay()
        for i, (got, want) in enumerate(zip(results(out), eager)):
            np.testing.assert_array_equal(got, want, err_msg=str(i))
    graph.destroy()
