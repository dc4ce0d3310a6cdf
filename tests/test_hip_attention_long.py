"""the long forms of the fused attention launches (csrc/attention_long.hip, ops `long_attention` and `self_attention` beyond 128
positions): any length 129 .. 512 with or without a key-padding mask, against a float64 run of the model's own composite lines
(examples/bert.py: divide by sqrt(d), additive mask, softmax), run against run bit for bit, and through the C ABI for what lies
outside the sequence.

The error rule is the project's own (test_hip_bert.py::test_fused_attention): context, probabilities, dq, dk, dv each within 1e-5
(relative Frobenius) of the float64 composite, and no further from it than twice the fp32 composite on the same backend + 2e-7.
The lengths sit on both sides of every chunk (128) and block (32) boundary of the kernels and on both parities of S % 4 (the
probabilities' row pitch is 16-byte aligned only when S % 4 == 0)."""
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
from common import float64_tape, rel_frobenius
from test_bert_cpu import bert
from test_hip_attention_masked import NAMES, composite, operands, padding_mask, assert_close_to_float64, tape_nodes

pytestmark = pytest.mark.gpu


def run(T, f64, arrays, heads, mask, how):
    """[context, probs, dq, dk, dv] as numpy; how = "fused" (long_attention) or "composite" """
    q, k, v, w = arrays
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    ts = [T.from_numpy(cast(x)) for x in (q, k, v)]
    tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
    scale = float(np.sqrt(q.shape[2] // heads)) ** -1
    if how == "fused":
        assert ts[0].long_attention_supported(heads)
        out = ts[0].long_attention(ts[1], ts[2], heads=heads, scale=scale, mask=tm)
        probs = out.attention_probs
        assert probs.shape == (q.shape[0], heads, q.shape[1], q.shape[1]) and not probs.requires_grad
    else:
        out, probs = composite(*ts, heads, tm)
    (out * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), probs.numpy()] + [t.grad.numpy() for t in ts]


SHAPES = [(1, 129, 1, 32), (2, 160, 2, 32), (1, 255, 1, 64), (2, 256, 1, 64), (1, 257, 2, 64), (1, 300, 1, 32), (1, 383, 2, 32),
          (2, 511, 1, 32), (1, 512, 2, 64)]
CASES = [(shape, masked) for shape in SHAPES for masked in (True, False)]


def check_against_float64(hip, arrays, heads, mask, what):
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
    assert_close_to_float64(got, comp, want, what)
    return got


@pytest.mark.parametrize("shape,masked", CASES, ids=["%dx%dx%dx%d-%s" % (c[0] + ("mask" if c[1] else "no_mask",)) for c in CASES])
def test_sweep_against_the_float64_composite(hip, shape, masked):
    b, s, heads, d = shape
    check_against_float64(hip, operands(b, s, heads, d), heads, padding_mask(b, s) if masked else None, str((b, s, heads, d, masked)))


@pytest.mark.parametrize("which", ["last_two_chunks_padding", "first_chunk_padding"])
def test_masks_that_empty_whole_chunks(hip, which):
    """s = 300 is three chunks of keys (128, 128, 44): keys 100.. masked leaves the last two entirely padding; keys 0 .. 139 masked
    makes the first one entirely padding, so the row maximum arrives late"""
    b, s, heads, d = 1, 300, 2, 32
    mask = np.ones((b, s), np.float32)
    if which == "last_two_chunks_padding":
        mask[:, 100:] = 0
    else:
        mask[:, :140] = 0
    check_against_float64(hip, operands(b, s, heads, d, seed=21), heads, mask, which)


def test_a_fully_masked_batch_element(hip):
    """every key of batch element 1 masked: -10000 on all of its scores - finite everywhere, its rows still sum to 1 (no closeness
    to float64 is asked of it: the add quantises fp32 scores to ~1e-3 on any implementation); element 0 is its run alone and,
    like it, close to the float64 composite"""
    b, s, heads, d = 2, 300, 1, 32
    arrays = operands(b, s, heads, d, seed=22)
    mask = padding_mask(b, s)
    mask[1, :] = 0
    both = run(hip, False, arrays, heads, mask, "fused")
    first = [x[:1] for x in arrays]
    alone = check_against_float64(hip, first, heads, mask[:1], "next to a fully masked element")
    for name, x, y in zip(NAMES, both, alone):
        assert np.isfinite(x).all(), name
        np.testing.assert_array_equal(x[:1], y, err_msg=name)
    np.testing.assert_allclose(both[1][1].sum(axis=-1), 1.0, rtol=0, atol=1e-5)


def test_two_runs_give_the_same_bits(hip):
    b, s, heads, d = 2, 300, 2, 64
    arrays = operands(b, s, heads, d, seed=23)
    mask = padding_mask(b, s)
    first = run(hip, False, arrays, heads, mask, "fused")
    for name, x, y in zip(NAMES, run(hip, False, arrays, heads, mask, "fused"), first):
        np.testing.assert_array_equal(x, y, err_msg=name)
    # a (1, s) mask is its (b, s) tiling
    row = padding_mask(1, s)
    for name, x, y in zip(NAMES, run(hip, False, arrays, heads, row, "fused"), run(hip, False, arrays, heads, np.tile(row, (b, 1)), "fused")):
        np.testing.assert_array_equal(x, y, err_msg=name)
    # no mask is a mask of ones
    for name, x, y in zip(NAMES, run(hip, False, arrays, heads, None, "fused"), run(hip, False, arrays, heads, np.ones((b, s), np.float32), "fused")):
        np.testing.assert_array_equal(x, y, err_msg=name)


@pytest.mark.parametrize("s", [131, 160])
def test_in_place_operands_and_nothing_outside_them_through_the_c_abi(hip, s):
    """q, k, v (and dq, dk, dv) as column blocks of one (b, s + extra, 3 * width + gap) buffer, o and dO with a row pitch above
    heads * d: the bits of the dense run; the surplus rows, the pitch gaps and the floats around p keep their NaN"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, heads, d, extra, gap = 2, 2, 32, 3, 8
    w = heads * d
    rows, ld3, ldo = s + extra, 3 * w + gap, w + gap
    q, k, v, g = operands(b, s, heads, d, seed=24)
    mask = padding_mask(b, s)
    n_p = b * heads * s * s
    tm = hip.from_numpy(mask, requires_grad=False)

    def nan(shape):
        return np.full(shape, np.nan, np.float32)

    def launch(ptrs, ld_in, sb_in, ld_out, sb_out, p):
        tq, tk, tv, tg, o, dq, dk, dv = ptrs
        L.check(lib.lg_attention_long_fwd_f32(tq, ld_in, sb_in, tk, ld_in, sb_in, tv, ld_in, sb_in, o, ld_out, sb_out, p,
                                              b, heads, s, d, 0.2, tm.ptr, s))
        L.check(lib.lg_attention_long_bwd_f32(tq, ld_in, sb_in, tk, ld_in, sb_in, tv, ld_in, sb_in, tg, ld_out, sb_out, p,
                                              dq, ld_in, sb_in, dk, ld_in, sb_in, dv, ld_in, sb_in, b, heads, s, d, 0.2))

    dense = [hip.from_numpy(x, requires_grad=False) for x in (q, k, v, g)] + [hip.from_numpy(nan((b, s, w)), requires_grad=False) for _ in range(4)]
    dense_p = hip.from_numpy(nan((n_p,)), requires_grad=False)
    launch([t.ptr for t in dense], w, s * w, w, s * w, dense_p.ptr)
    dense_out = [t.numpy() for t in dense[4:]]
    assert all(np.isfinite(x).all() for x in dense_out) and np.isfinite(dense_p.numpy()).all()

    qkv_host = nan((b, rows, ld3))
    for i, x in enumerate((q, k, v)):
        qkv_host[:, :s, i * w:(i + 1) * w] = x
    g_host = nan((b, rows, ldo))
    g_host[:, :s, :w] = g
    qkv, tg = hip.from_numpy(qkv_host, requires_grad=False), hip.from_numpy(g_host, requires_grad=False)
    o, dqkv = hip.from_numpy(nan((b, rows, ldo)), requires_grad=False), hip.from_numpy(nan((b, rows, ld3)), requires_grad=False)
    wide_p = hip.from_numpy(nan((n_p + 128,)), requires_grad=False)
    launch([qkv.ptr, qkv.ptr + 4 * w, qkv.ptr + 8 * w, tg.ptr, o.ptr, dqkv.ptr, dqkv.ptr + 4 * w, dqkv.ptr + 8 * w],
           ld3, rows * ld3, ldo, rows * ldo, wide_p.ptr + 4 * 64)

    got_p = wide_p.numpy()
    np.testing.assert_array_equal(got_p[64:64 + n_p], dense_p.numpy())
    assert np.isnan(got_p[:64]).all() and np.isnan(got_p[64 + n_p:]).all()
    got_o, got_d = o.numpy(), dqkv.numpy()
    np.testing.assert_array_equal(got_o[:, :s, :w], dense_out[0], err_msg="o")
    assert np.isnan(got_o[:, s:]).all() and np.isnan(got_o[:, :, w:]).all()
    for i, name in enumerate(("dq", "dk", "dv")):
        np.testing.assert_array_equal(got_d[:, :s, i * w:(i + 1) * w], dense_out[1 + i], err_msg=name)
    assert np.isnan(got_d[:, s:]).all() and np.isnan(got_d[:, :, 3 * w:]).all()
    # the operands are as they were
    np.testing.assert_array_equal(qkv.numpy(), qkv_host)
    np.testing.assert_array_equal(tg.numpy(), g_host)


def test_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    assert lib.lg_attention_long_supported(128, 32) == 0 and lib.lg_attention_long_supported(129, 32) == 1
    assert lib.lg_attention_long_supported(512, 64) == 1 and lib.lg_attention_long_supported(513, 64) == 0
    assert lib.lg_attention_long_supported(256, 48) == 0
    b, s, heads, d = 2, 160, 2, 32
    w = heads * d
    q, k, v, o = (hip.from_numpy(np.zeros((b, s, w), np.float32), requires_grad=False) for _ in range(4))
    p = hip.from_numpy(np.zeros((b, heads, s, s), np.float32), requires_grad=False)
    m = hip.from_numpy(np.ones((b, s), np.float32), requires_grad=False)
    fwd = lambda **kw: lib.lg_attention_long_fwd_f32(kw.get("q", q.ptr), kw.get("ld", w), s * w, k.ptr, w, s * w, v.ptr, w, s * w,     # noqa: E731
                                                     kw.get("o", o.ptr), w, s * w, kw.get("p", p.ptr), kw.get("b", b), kw.get("heads", heads),
                                                     kw.get("s", s), kw.get("d", d), 0.5, kw.get("m", m.ptr), kw.get("sbm", s))
    assert fwd() == 0 and fwd(sbm=0) == 0 and fwd(m=None, sbm=7) == 0 and fwd(sbm=s + 5) == 0
    assert fwd(b=0, q=None) == 0
    assert fwd(sbm=s - 1) == -1 and b"mask" in lib.lg_last_error()
    assert fwd(sbm=-s) == -1 and b"mask" in lib.lg_last_error()
    assert fwd(s=128) == -1 and b"unsupported" in lib.lg_last_error()
    assert fwd(s=513) == -1 and b"unsupported" in lib.lg_last_error()
    assert fwd(d=16) == -1 and b"unsupported" in lib.lg_last_error()
    assert fwd(q=q.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert fwd(ld=w - 4) == -1 and b"row pitch" in lib.lg_last_error()
    assert fwd(o=None) == -1 and b"aligned" in lib.lg_last_error()
    assert fwd(p=None) == -1
    bwd = lambda **kw: lib.lg_attention_long_bwd_f32(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, kw.get("g", o.ptr), kw.get("ld", w), s * w,     # noqa: E731
                                                     p.ptr, q.ptr, w, s * w, k.ptr, w, s * w, kw.get("dv", v.ptr), w, s * w,
                                                     kw.get("b", b), kw.get("heads", heads), kw.get("s", s), d, 0.5)
    assert bwd(b=0, dv=None) == 0
    assert bwd(dv=None) == -1 and b"aligned" in lib.lg_last_error()
    assert bwd(g=o.ptr + 4) == -1 and b"aligned" in lib.lg_last_error()
    assert bwd(ld=w - 4) == -1 and b"row pitch" in lib.lg_last_error()
    assert bwd(s=128) == -1 and b"unsupported" in lib.lg_last_error()
    assert bwd(s=513) == -1 and b"unsupported" in lib.lg_last_error()
    assert bwd(b=8193) == -1 and b"pairs" in lib.lg_last_error()          # more pairs than hand-off counters: refused before any launch
    # the op: lengths outside 129 .. 512, a mask of the wrong shape or dtype, and one that wants a gradient
    for bad_s in (128, 513):
        t = hip.from_numpy(np.zeros((1, bad_s, w), np.float32))
        assert not t.long_attention_supported(heads)
        with pytest.raises(AssertionError, match="unsupported"):
            t.long_attention(t, t, heads=heads)
    tq, tk, tv = (hip.from_numpy(np.zeros((b, s, w), np.float32)) for _ in range(3))
    for bad in (hip.from_numpy(np.ones((b, s + 1), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((b + 1, s), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((s,), np.float32), requires_grad=False),
                hip.from_numpy(np.ones((b, s), np.int32), requires_grad=False)):
        with pytest.raises(AssertionError, match="mask"):
            tq.long_attention(tk, tv, heads=heads, mask=bad)
    with pytest.raises(AssertionError, match="gradient"):
        tq.long_attention(tk, tv, heads=heads, mask=hip.from_numpy(np.ones((b, s), np.float32), requires_grad=True))
    # the node's predicate: asked as before it answers as before; long=True asks the long form's question
    x = hip.from_numpy(np.zeros((b, s, 64), np.float32))
    wq = hip.from_numpy(np.zeros((w, 64), np.float32))
    assert not x.self_attention_supported(wq, heads) and not x.self_attention_supported(wq, heads, masked=True)
    assert x.self_attention_supported(wq, heads, long=True)
    short = hip.from_numpy(np.zeros((b, 64, 64), np.float32))
    assert short.self_attention_supported(wq, heads) and not short.self_attention_supported(wq, heads, long=True)


MODEL_CFG = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
                 max_position_embeddings=160, type_vocab_size=2)


@pytest.mark.parametrize("s,with_mask", [(160, True), (131, False)])
def test_model_beyond_128_positions_takes_the_node(hip, s, with_mask):
    """BertForMaskedLM, one layer, hidden 64 / 2 heads, batch 2 at 160 positions with padding masks of two lengths, and at 131
    without a mask: a `self_attention` node on the tape, the logits and every parameter gradient of the weighted-logits objective
    within 1e-5 of a float64 run (test_hip_bert.py::test_forward_backward_matches_cpu_backend's rule and its key-bias exemption)"""
    rng = np.random.RandomState(25)
    ids = rng.randint(0, 60, (2, s)).astype(np.int32)
    w = rng.uniform(-1, 1, (2, s, 60)).astype(np.float32)
    mask = None
    if with_mask:
        mask = np.ones((2, s), np.float32)
        mask[0, 150:] = 0
        mask[1, 97:] = 0

    def build():
        np.random.seed(5)
        return bert.BertForMaskedLM(**MODEL_CFG)

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


def test_the_node_replayed_from_a_graph(hip):
    """forward and backward of `self_attention` at 160 positions with a mask, captured once: two replays give the eager bits"""
    from lightgrad_amd.autograd.hip import HipGraph
    rng = np.random.RandomState(26)
    b, s, hidden, heads, d = 2, 160, 64, 2, 32
    width = heads * d
    x = hip.from_numpy(rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32))
    params = []
    for _ in range(3):
        params += [hip.from_numpy(rng.uniform(-0.2, 0.2, (width, hidden)).astype(np.float32)),
                   hip.from_numpy(rng.uniform(-0.2, 0.2, (width,)).astype(np.float32))]
    w = hip.from_numpy(rng.uniform(-1, 1, (b, s, width)).astype(np.float32), requires_grad=False)
    mask = hip.from_numpy(padding_mask(b, s), requires_grad=False)
    scale = float(np.sqrt(d)) ** -1

    def step():
        for t in [x] + params:
            t.zero_grad()
        out = x.self_attention(*params, heads=heads, scale=scale, mask=mask)
        (out * w).backward(allow_fill=True)
        return out

    def results(out):
        return [out.numpy(), out.attention_probs.numpy(), x.grad.numpy()] + [p.grad.numpy() for p in params]

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
