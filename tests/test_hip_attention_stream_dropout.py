"""attention dropout inside the streaming launches (csrc/attention_stream.hip, DROP; `stream_attention(dropout=p)`, `self_attention(probs=False,
dropout=p, stream_dropout=True)`): shapes (b, heads, S, D) on both sides of the 32-key block, the 128-row chunk and 512, every S % 4;
bounds are the 1e-5 relative Frobenius contract of test_hip_attention_stream.py."""
import contextlib
import math
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, rel_frobenius
from test_bert_cpu import bert
from test_hip_dropout import SEEDS, LG_EINVAL
from test_hip_attention_masked import padding_mask, tape_nodes
from test_hip_attention_dropout import operands, burn
from test_hip_attention_stream import lse_float64, MODEL_CFG, NAMES

pytestmark = pytest.mark.gpu

SHAPES = [(2, 1, 5, 32), (1, 2, 33, 64), (1, 1, 130, 32), (2, 2, 160, 32), (1, 1, 515, 64)]
CASES = [(shape, masked, causal) for shape in SHAPES for masked in (False, True) for causal in (False, True)
         if not masked or shape in (SHAPES[1], SHAPES[3])]
IDS = ["%dx%dx%dx%d-%s-%s" % (c[0] + ("mask" if c[1] else "no_mask", "causal" if c[2] else "full")) for c in CASES]
PROBS, SEED, DRAW = (0.1, 0.5), SEEDS[1], 3


def composite(q, k, v, heads, mask, causal, p):
    """the composite lines of examples/bert.py with `probs.dropout(p)`"""
    (b, s, width), d = q.shape, q.shape[2] // heads
    q4, k4, v4 = (t.reshape(b, s, heads, d).transpose(*axes) for t, axes in ((q, (0, 2, 1, 3)), (k, (0, 2, 3, 1)), (v, (0, 2, 1, 3))))
    scores = (q4 @ k4) / math.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask.reshape(mask.shape[0], 1, 1, s)) * -10000.0).detach()
    if causal:
        tril = q.__class__.from_numpy(np.tril(np.ones((1, 1, s, s), dtype=q.dtype)), requires_grad=False)
        scores = scores + ((1.0 - tril) * -10000.0).detach()
    return (scores.softmax(axis=-1).dropout(p) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)


def run(T, f64, arrays, heads, mask, causal, fused, **dropout):
    """[context, lse, dq, dk, dv] as numpy (lse: None for the composite)"""
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    ts = [T.from_numpy(cast(x)) for x in arrays[:3]]
    tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
    out = ts[0].stream_attention(ts[1], ts[2], heads=heads, scale=math.sqrt(arrays[0].shape[2] // heads) ** -1, mask=tm, causal=causal,
                                 **dropout) if fused else composite(*ts, heads, tm, causal, dropout["dropout"])
    lse = out.attention_lse.numpy() if fused else None
    (out * T.from_numpy(cast(arrays[3]), requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), lse] + [t.grad.numpy() for t in ts]


@pytest.mark.parametrize("shape,masked,causal", CASES, ids=IDS)
def test_the_mask_lands_where_the_stream_puts_it(hip, shape, masked, causal):
    """V[j] = e_(j - w D) in window w: the context is columns [w D, w D + D) of Pd = D o P, one term per sum.  Visible (i, j): key j
    has mask 1 (padding_mask's 0.5 is a bias of -5000: padded) and j <= i when causal; |score| <= 18, so a kept visible entry is not 0"""
    (b, heads, s, d), (q, k, _, _) = shape, operands(shape)
    mask = padding_mask(b, s) if masked else None
    visible = np.ones((b, 1, s, s), bool) if mask is None else np.broadcast_to((mask == 1)[:, None, None, :], (b, 1, s, s))
    visible = np.broadcast_to(visible & (np.tril(np.ones((s, s), bool)) if causal else True), (b, heads, s, s))
    x = np.einsum("bihd,bjhd->bhij", *(t.astype(np.float64).reshape(b, s, heads, d) for t in (q, k))) / math.sqrt(d)
    x = x + (0 if mask is None else ((1.0 - mask.astype(np.float64)) * -10000.0)[:, None, None, :]) + (1.0 - np.tril(np.ones((s, s)))) * (-10000.0 * causal)
    probs64 = np.exp(x - lse_float64((q, k), heads, mask, causal)[..., None])
    tm = None if mask is None else hip.from_numpy(mask, requires_grad=False)
    for p in PROBS:
        pd = np.zeros((b, heads, s, s), np.float32)
        for w in range((s + d - 1) // d):
            v, cols = np.zeros((b, s, heads, d), np.float32), min(s, w * d + d) - w * d
            v[:, np.arange(w * d, w * d + cols), :, np.arange(cols)] = 1
            light.manual_seed(SEED)
            burn(hip, DRAW)
            with light.no_grad():
                out = hip.from_numpy(q).stream_attention(hip.from_numpy(k), hip.from_numpy(v.reshape(b, s, heads * d)), heads=heads,
                                                         scale=math.sqrt(d) ** -1, mask=tm, causal=causal, dropout=p)
            assert lrandom.get_state("hip") == (SEED, DRAW + 1)
            pd[..., w * d:w * d + cols] = out.numpy().reshape(b, s, heads, d).transpose(0, 2, 1, 3)[..., :cols]
        keep = lrandom.keep_mask(SEED, DRAW, b * heads * s * s, p).reshape(b, heads, s, s)
        assert ((pd != 0) == keep)[visible].all() and not np.signbit(pd[visible & ~keep]).any()
        assert rel_frobenius(pd[visible & keep], (probs64 * lrandom.scale(p))[visible & keep]) <= 1e-5


@pytest.mark.parametrize("shape,masked,causal", CASES, ids=IDS)
def test_against_the_float64_composite(hip, shape, masked, causal):
    (b, heads, s, d), arrays = shape, operands(shape, seed=9)
    mask = padding_mask(b, s) if masked else None
    for p in PROBS:
        results = []
        for T, f64, fused in ((hip, False, True), (hip, False, False), (CpuTensor, True, False)):
            light.manual_seed(SEED)
            with float64_tape() if f64 else contextlib.nullcontext():
                results.append(run(T, f64, arrays, heads, mask, causal, fused, dropout=p))
            assert lrandom.get_state("cpu" if f64 else "hip") == (SEED, 1)           # one call forward, none backward
        got, comp, want = results
        want[1] = lse_float64(arrays, heads, mask, causal)                          # dropout does not change it
        errors = [(name, rel_frobenius(g, r), float("nan") if c is None else rel_frobenius(c, r)) for name, g, c, r in zip(NAMES, got, comp, want)]
        print("\n".join("%s p=%.1f %s: fused %.3e, fp32 composite %.3e" % ((shape, p) + e) for e in errors))
        assert all(np.isfinite(g).all() for g in got) and all(e[1] <= 1e-5 for e in errors), errors


@pytest.mark.parametrize("shape", [SHAPES[2], SHAPES[3]], ids=["per_element", "aligned_and_quad"])
def test_bookkeeping_and_graph_replay(hip, shape):
    """dropout=0.0 is the call without the keyword; one (seed, draw) is one set of bits; replay k of a captured step is the eager run at draw k"""
    from lightgrad_amd.autograd.hip import HipGraph
    (b, heads, s, d), arrays, mask = shape, operands(shape, seed=31), padding_mask(shape[0], shape[2])
    for x, y in zip(run(hip, False, arrays, heads, mask, True, True, dropout=0.0), run(hip, False, arrays, heads, mask, True, True)):
        np.testing.assert_array_equal(x, y)
    q, k, v = (hip.from_numpy(x) for x in arrays[:3])
    w, tm = hip.from_numpy(arrays[3], requires_grad=False), hip.from_numpy(mask, requires_grad=False)

    def step():
        for t in (q, k, v):
            t.zero_grad()
        out = q.stream_attention(k, v, heads=heads, scale=math.sqrt(d) ** -1, mask=tm, causal=True, dropout=0.5)
        (out * w).backward(allow_fill=True)
        return out, out.attention_lse, q.grad, k.grad, v.grad

    eager = []
    for draw in (0, 1, 1):
        light.manual_seed(SEED)
        burn(hip, draw)
        eager.append([t.numpy().copy() for t in step()])
        assert lrandom.get_state("hip") == (SEED, draw + 1)
    assert all(np.array_equal(x, y) for x, y in zip(eager[1], eager[2])) and not np.array_equal(eager[0][0], eager[1][0])
    graph = HipGraph()
    with graph.capture():
        captured = step()
    light.manual_seed(SEED)
    for draw in (0, 1):
        graph.replay()
        for name, got, want in zip(NAMES, captured, eager[draw]):
            np.testing.assert_array_equal(got.numpy(), want, err_msg="replay %d %s" % (draw, name))
    graph.destroy()


def test_the_node_and_the_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    rng, (b, s, hidden, heads, d, p) = np.random.RandomState(26), (2, 530, 64, 2, 32, 0.1)
    width, scale = heads * d, math.sqrt(d) ** -1
    x = hip.from_numpy(rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32))
    params = [hip.from_numpy(rng.uniform(-0.2, 0.2, sh).astype(np.float32)) for _ in range(3) for sh in ((width, hidden), (width,))]
    mask = hip.from_numpy(padding_mask(b, s), requires_grad=False)
    outs = []
    for node in (True, False):
        light.manual_seed(SEED)
        burn(hip, DRAW)
        with light.no_grad():
            if node:
                out = x.self_attention(*params, heads=heads, scale=scale, mask=mask, probs=False, dropout=p, stream_dropout=True)
                q, k, v = (out.attention_qkv[:, :, i * width:(i + 1) * width] for i in range(3))
            else:
                out = q.stream_attention(k, v, heads=heads, scale=scale, mask=mask, dropout=p)
        assert out.attention_probs is None and lrandom.get_state("hip") == (SEED, DRAW + 1)
        outs.append((out.numpy(), out.attention_lse.numpy()))
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])
    with pytest.raises(AssertionError, match="stream_dropout=True with probs=True"):
        x.self_attention(*params, heads=heads, scale=scale, dropout=p, stream_dropout=True)
    lib, n, w = L.lib(), b * s * width, width
    o, lse, base = (hip.from_numpy(np.zeros(m, t), requires_grad=False) for m, t in ((n, np.float32), (b * heads * s, np.float32), (1, np.uint64)))
    rows = lambda *ts: sum(((t.ptr, w, s * w) for t in ts), ())      # noqa: E731
    tail = (b, heads, s, d, scale, None, 0, 0)
    calls = ((lib.lg_attention_stream_dropout_fwd_f32, rows(o, o, o, o) + (lse.ptr,) + tail),
             (lib.lg_attention_stream_dropout_bwd_f32, rows(o, o, o, o, o) + (lse.ptr, lse.ptr) + rows(o, o, o) + tail))
    for entry, args in calls:
        for bad, word in (((1.0, base.ptr), b"p ="), ((-0.1, base.ptr), b"p ="), ((0.5, None), b"base")):
            assert entry(*args, *bad) == LG_EINVAL and word in lib.lg_last_error(), (bad, lib.lg_last_error())
    assert lrandom.get_state("hip") == (SEED, DRAW + 1)


def test_the_model_takes_the_node_in_training_mode(hip):
    """530 positions: a `self_attention` node, one call of the stream (no hidden dropout), the kernel count of the model with p = 0"""
    from lightgrad_amd.autograd.hip import HipGraph
    rng, s, counts = np.random.RandomState(27), 530, {}
    ids = hip.from_numpy(rng.randint(0, 60, (2, s)).astype(np.int32), requires_grad=False)
    labels = hip.from_numpy(rng.randint(0, 60, (2 * s,)).astype(np.int64), requires_grad=False)
    for p in (0.1, 0.0):
        np.random.seed(5)
        model = bert.BertForMaskedLM(**dict(MODEL_CFG, attention_probs_dropout_prob=p)).map_parameters(lambda t: t.hip())

        def step():
            loss = light.loss.cross_entropy(model(ids).reshape(-1, 60), labels)
            for t in model.parameters():
                t.zero_grad()
            loss.backward()
            return loss
        light.manual_seed(SEED)
        assert "self_attention" in tape_nodes(step()) and lrandom.get_state("hip") == (SEED, int(p > 0))
        graph = HipGraph()
        with graph.capture():
            step()
        counts[p] = graph.kernel_count()
        graph.destroy()
    assert counts[0.1] == counts[0.0] > 0, counts
