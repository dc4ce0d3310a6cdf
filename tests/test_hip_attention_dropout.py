"""dropout of the attention probabilities inside the fused attention launches (DROP instantiations of csrc/attention.hip and
csrc/attention_long.hip; ops `attention`, `masked_attention`, `long_attention`, `self_attention` with dropout=p): where the mask
lands, bit for bit; the float64 composite with the same mask; the stream's bookkeeping, back to back and under graph replay;
what lies outside the operands through the C ABI; argument checks; and the BERT example in training mode.

Shapes are (b, heads, S, D): plain (no mask, S a multiple of 32 up to 128), tail (any S up to 128, mask or none) and long (129 .. 512)."""
import itertools
import math
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from test_hip_dropout import SEEDS, LG_EINVAL
from test_hip_attention_masked import padding_mask
from test_bert_cpu import bert

pytestmark = pytest.mark.gpu

PLAIN = [(2, 2, 32, 32), (1, 2, 128, 64)]
TAIL = [(2, 1, 1, 32), (1, 2, 5, 32), (1, 1, 33, 64), (2, 2, 127, 32)]
LONG = [(1, 1, 129, 32), (1, 2, 131, 64), (1, 1, 257, 32), (1, 1, 512, 64)]
# (shape, with a padding mask): the plain kernels take no mask; a mask at a multiple of 32 is the tail kernels' ground
PLACEMENT = [(s, False) for s in PLAIN + TAIL + LONG] + [(s, True) for s in TAIL]
AGAINST64 = PLACEMENT + [((1, 1, 96, 32), False), ((1, 1, 96, 32), True), ((1, 1, 160, 64), False), ((1, 1, 160, 64), True)]
PROBS = (0.1, 0.5)


def ident(case):
    return "%dx%dx%dx%d-%s" % (case[0] + ("mask" if case[1] else "nomask",))


def operands(shape, seed=7):
    b, heads, s, d = shape
    rng = np.random.RandomState(seed)
    q, k, v = (rng.uniform(-1.5, 1.5, (b, s, heads * d)).astype(np.float32) for _ in range(3))
    w = rng.uniform(-1, 1, (b, s, heads * d)).astype(np.float32)
    return q, k, v, w


def fused(q, k, v, heads, mask, p):
    """the form the model would take for this length and mask"""
    s = q.shape[1]
    scale = math.sqrt(q.shape[2] // heads) ** -1
    if s > 128:
        return q.long_attention(k, v, heads=heads, scale=scale, mask=mask, dropout=p)
    if mask is not None or s % 32:
        return q.masked_attention(k, v, heads=heads, scale=scale, mask=mask, dropout=p)
    return q.attention(k, v, heads=heads, scale=scale, dropout=p)


def composite(q, k, v, heads, mask, p):
    """examples/bert.py BertSelfAttention.forward, composite branch, with the dropout of the probabilities"""
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
    return (probs.dropout(p) @ v4).transpose(0, 2, 1, 3).reshape(b, s, width)


def burn(hip, n):
    """n plain dropout calls: the next call of the stream has base = n"""
    x = hip.from_numpy(np.ones(4, np.float32), requires_grad=False)
    with light.no_grad():
        for _ in range(n):
            x.dropout(0.5)


def run_fused(hip, arrays, heads, mask, p):
    """context, probabilities, dq, dk, dv of one fused forward and backward, as numpy"""
    q, k, v, w = arrays
    ts = [hip.from_numpy(x) for x in (q, k, v)]
    tm = None if mask is None else hip.from_numpy(mask, requires_grad=False)
    out = fused(*ts, heads, tm, p)
    probs = out.attention_probs
    (out * hip.from_numpy(w, requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), probs.numpy()] + [t.grad.numpy() for t in ts]


@pytest.mark.parametrize("case", PLACEMENT, ids=ident)
def test_the_mask_lands_where_the_stream_puts_it(hip, case):
    """V rows are unit vectors, V[j] = e_(j - w D) for j in window w and 0 elsewhere: the context is columns [w D, w D + D) of Pd,
    one non-zero term per sum - exact.  Over the windows Pd is assembled and must be where(keep, probs * s, +0) bit for bit."""
    (b, heads, s, d), masked = case
    q, k, _, _ = operands(case[0])
    mask = padding_mask(b, s) if masked else None
    n = b * heads * s * s
    for p, seed in itertools.product(PROBS, SEEDS):
        pd = np.zeros((b, heads, s, s), np.float32)
        probs = None
        for w in range((s + d - 1) // d):
            v = np.zeros((b, s, heads, d), np.float32)
            for j in range(w * d, min(s, w * d + d)):
                v[:, j, :, j - w * d] = 1
            light.manual_seed(seed)
            burn(hip, 3)
            with light.no_grad():
                tm = None if mask is None else hip.from_numpy(mask, requires_grad=False)
                out = fused(hip.from_numpy(q), hip.from_numpy(k), hip.from_numpy(v.reshape(b, s, heads * d)), heads, tm, p)
            assert lrandom.get_state("hip") == (seed, 4)
            context = out.numpy().reshape(b, s, heads, d).transpose(0, 2, 1, 3)
            cols = min(s, w * d + d) - w * d
            pd[:, :, :, w * d:w * d + cols] = context[:, :, :, :cols]
            assert not context[:, :, :, cols:].any()
            if probs is None:
                probs = out.attention_probs.numpy()
            else:
                np.testing.assert_array_equal(out.attention_probs.numpy(), probs)
        keep = lrandom.keep_mask(seed, 3, n, p).reshape(b, heads, s, s)
        assert 0 < keep.sum() < n or n < 8
        np.testing.assert_array_equal(pd, np.where(keep, probs * lrandom.scale(p), np.float32(0)))
        assert not np.signbit(pd[~keep]).any()


@pytest.mark.parametrize("case", AGAINST64, ids=ident)
def test_against_the_float64_composite(hip, case):
    (b, heads, s, d), masked = case
    arrays = operands(case[0], seed=9)
    mask = padding_mask(b, s) if masked else None
    names = ("context", "dq", "dk", "dv")
    undropped = run_fused(hip, arrays, heads, mask, 0.0)[1]
    for p, seed in itertools.product(PROBS, SEEDS):
        def comp(f64):
            cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
            ts = [CpuTensor.from_numpy(cast(x)) for x in arrays[:3]]
            tm = None if mask is None else CpuTensor.from_numpy(cast(mask), requires_grad=False)
            out = composite(*ts, heads, tm, p)
            (out * CpuTensor.from_numpy(cast(arrays[3]), requires_grad=False)).backward(allow_fill=True)
            return dict(zip(names, [out.numpy()] + [t.grad.numpy() for t in ts]))
        light.manual_seed(seed)
        cpu32 = comp(False)
        got = run_fused(hip, arrays, heads, mask, p)
        assert lrandom.get_state("hip") == lrandom.get_state("cpu") == (seed, 1)
        light.manual_seed(seed)
        with float64_tape():
            ref64 = comp(True)
        np.testing.assert_array_equal(got[1], undropped)                # .attention_probs stays the undropped probabilities
        got = dict(zip(names, [got[0]] + got[2:]))
        for n in names:
            print("%s p=%.1f %s: fused %.3e, fp32 cpu composite %.3e" % (ident(case), p, n, rel_frobenius(got[n], ref64[n]),
                                                                         rel_frobenius(cpu32[n], ref64[n])))
        assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, ref64, floor=1e-5, what="%s p=%.1f" % (ident(case), p))


def test_bookkeeping(hip):
    seed = SEEDS[1]
    arrays = operands((1, 2, 5, 32))
    light.manual_seed(seed)
    q, k, v = (hip.from_numpy(x) for x in arrays[:3])
    out = fused(q, k, v, 2, None, 0.0)
    assert lrandom.get_state("hip") == (seed, 0)                       # dropout=0.0: the launches without it, nothing drawn
    out = fused(q, k, v, 2, None, 0.5)
    assert lrandom.get_state("hip") == (seed, 1)
    out.sum().backward()
    assert lrandom.get_state("hip") == (seed, 1)                       # the backward draws nothing

    # twelve calls enqueued without a synchronisation: eight fused forwards of the three families and four plain dropouts
    shapes = [(2, 2, 32, 32), (1, 2, 5, 32), (1, 1, 129, 32), None, (1, 2, 64, 64), (2, 2, 127, 32), None, (1, 2, 131, 64), (1, 1, 33, 64),
              None, (1, 1, 257, 32), None]
    assert len([s for s in shapes if s is not None]) == 8
    xa = np.random.RandomState(3).standard_normal(5000).astype(np.float32)
    inputs = [None if s is None else [hip.from_numpy(x) for x in operands(s, seed=20 + i)[:3]] for i, s in enumerate(shapes)]
    x = hip.from_numpy(xa)

    def queue():
        light.manual_seed(seed)
        lrandom.get_state("hip")                                        # the seed is on the device before the first call
        with light.no_grad():
            outs = [x.dropout(0.5) if s is None else fused(*inputs[i], s[1], None, 0.5) for i, s in enumerate(shapes)]
        return [o.numpy() for o in outs]

    first, second = queue(), queue()
    assert lrandom.get_state("hip") == (seed, len(shapes))
    for i, (a, b) in enumerate(zip(first, second)):
        np.testing.assert_array_equal(a, b, err_msg="call %d: two runs from one seed" % i)
    for i, s in enumerate(shapes):
        light.manual_seed(seed)
        burn(hip, i)
        with light.no_grad():
            alone = x.dropout(0.5) if s is None else fused(*inputs[i], s[1], None, 0.5)
        np.testing.assert_array_equal(first[i], alone.numpy(), err_msg="call %d against its eager run at base %d" % (i, i))
        if s is None:
            np.testing.assert_array_equal(first[i] != 0, lrandom.keep_mask(seed, i, len(xa), 0.5) & (xa != 0))


@pytest.mark.parametrize("shape", [(1, 2, 5, 32), (1, 1, 131, 32)], ids=["tail", "long"])
def test_graph_replay_draws_a_fresh_mask(hip, shape):
    from lightgrad_amd.autograd.hip import GraphedStep
    seed, p = SEEDS[1], 0.5
    qa, ka, va, wa = operands(shape, seed=31)
    q, k, v = (hip.from_numpy(x) for x in (qa, ka, va))
    w = hip.from_numpy(wa, requires_grad=False)

    def once():
        out = fused(q, k, v, shape[1], None, p)
        for t in (q, k, v):
            t.zero_grad()
        (out * w).backward(allow_fill=True)
        return out, q.grad, k.grad, v.grad

    expected = []
    for draw in range(3):
        light.manual_seed(seed)
        burn(hip, draw)
        expected.append([t.numpy().copy() for t in once()])
    step = GraphedStep(once, warmup=1)
    step()
    light.manual_seed(seed)
    for draw in range(3):
        got = [t.numpy() for t in step()]
        assert lrandom.get_state("hip") == (seed, draw + 1)
        for name, g, e in zip(("context", "dq", "dk", "dv"), got, expected[draw]):
            np.testing.assert_array_equal(g, e, err_msg="replay %d %s" % (draw, name))
    assert step._graph is not None and step._graph.kernel_count() > 0
    assert not np.array_equal(expected[0][0], expected[1][0])
    step.destroy()


@pytest.mark.parametrize("shape", [(1, 2, 5, 32), (1, 1, 131, 32)], ids=["tail", "long"])
def test_nothing_outside_the_operands_is_read_or_written(hip, shape):
    """through the C ABI: q, k, v, g, the probabilities the backward reads and the mask lie between bands of NaN, the outputs between
    bands of a marker; the results are the bits of the run on exact buffers and every band is as it was"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, heads, s, d = shape
    w, band, marker, seed, p = heads * d, 7, np.float32(-777.25), SEEDS[1], 0.5
    q, k, v, g = operands(shape, seed=11)
    mask = padding_mask(b, s)
    n_p = b * heads * s * s
    bands = {"rows": band * w, "p": 64, "mask": 5}                       # floats on either side (16-byte steps where the ABI asks for them)

    def launch(wide):
        lead = {kind: (n if wide else 0) for kind, n in bands.items()}

        def banded(x, fill, kind):
            side = np.full(lead[kind], fill, np.float32)
            return hip.from_numpy(np.concatenate([side, np.asarray(x, np.float32).reshape(-1), side]), requires_grad=False)

        def parts(t, kind, n):
            a = t.numpy()
            return a[:lead[kind]], a[lead[kind]:lead[kind] + n], a[lead[kind] + n:]

        def at(t, kind):
            return t.ptr + 4 * lead[kind]

        tq, tk, tv, tg = ins = [banded(x, np.nan, "rows") for x in (q, k, v, g)]
        tm = banded(mask, np.nan, "mask")
        o, dq, dk, dv = outs = [banded(np.full((b, s, w), marker), marker, "rows") for _ in range(4)]
        pout = banded(np.full(n_p, marker), marker, "p")
        base = hip.from_numpy(np.full(3, 99, np.uint64))
        light.manual_seed(seed)
        burn(hip, 2)
        L.check(lib.lg_attention_dropout_fwd_f32(at(tq, "rows"), w, s * w, at(tk, "rows"), w, s * w, at(tv, "rows"), w, s * w,
                                                 at(o, "rows"), w, s * w, at(pout, "p"), b, heads, s, d, 0.2, at(tm, "mask"), s, p,
                                                 base.ptr + 8))
        pin = banded(parts(pout, "p", n_p)[1], np.nan, "p")
        L.check(lib.lg_attention_dropout_bwd_f32(at(tq, "rows"), w, s * w, at(tk, "rows"), w, s * w, at(tv, "rows"), w, s * w,
                                                 at(tg, "rows"), w, s * w, at(pin, "p"), at(dq, "rows"), w, s * w, at(dk, "rows"), w, s * w,
                                                 at(dv, "rows"), w, s * w, b, heads, s, d, 0.2, p, base.ptr + 8))
        assert lrandom.get_state("hip") == (seed, 3)
        np.testing.assert_array_equal(base.numpy(), [99, 2, 99])
        results = []
        for t, kind, n in [(x, "rows", b * s * w) for x in outs] + [(pout, "p", n_p)]:
            before, body, after = parts(t, kind, n)
            assert (before == marker).all() and (after == marker).all()
            results.append(body.copy())
        for t, x in zip(ins, (q, k, v, g)):
            before, body, after = parts(t, "rows", b * s * w)
            assert np.isnan(before).all() and np.isnan(after).all()
            np.testing.assert_array_equal(body, x.reshape(-1))
        return results

    dense, wide = launch(False), launch(True)
    for name, a, c in zip(("o", "dq", "dk", "dv", "p"), wide, dense):
        assert np.isfinite(a).all() and (a != marker).any(), name
        np.testing.assert_array_equal(a, c, err_msg=name)


def test_argument_checks(hip):
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, heads, s, d = 1, 2, 5, 32
    w = heads * d
    q, k, v, g = (hip.from_numpy(x) for x in operands((b, heads, s, d)))
    for bad in (-0.1, 1.0, float("nan")):
        for call in (lambda: q.attention(k, v, heads=heads, dropout=bad), lambda: q.masked_attention(k, v, heads=heads, dropout=bad),
                     lambda: q.long_attention(k, v, heads=heads, dropout=bad)):
            with pytest.raises(ValueError):
                call()
    light.manual_seed(4)
    before = lrandom.get_state("hip")
    o, dq, dk, dv = (hip.from_numpy(np.full((b, s, w), 3.0, np.float32)) for _ in range(4))
    pr = hip.from_numpy(np.full(b * heads * s * s, 3.0, np.float32))
    base = hip.from_numpy(np.zeros(1, np.uint64))

    def fwd(p=0.5, base_ptr=base.ptr, S=s, D=d):
        return lib.lg_attention_dropout_fwd_f32(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, o.ptr, w, s * w, pr.ptr, b, heads, S, D, 0.2,
                                                None, 0, p, base_ptr)

    def bwd(p=0.5, base_ptr=base.ptr, S=s, D=d):
        return lib.lg_attention_dropout_bwd_f32(q.ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, g.ptr, w, s * w, pr.ptr, dq.ptr, w, s * w,
                                                dk.ptr, w, s * w, dv.ptr, w, s * w, b, heads, S, D, 0.2, p, base_ptr)

    for call, name in ((fwd, b"lg_attention_dropout_fwd_f32"), (bwd, b"lg_attention_dropout_bwd_f32")):
        for kwargs, word in (({"p": -0.1}, b"p ="), ({"p": 1.0}, b"p ="), ({"p": float("nan")}, b"p ="), ({"base_ptr": None}, b"base"),
                             ({"D": 48}, b"D = 48"), ({"S": 513}, b"S = 513")):
            assert call(**kwargs) == LG_EINVAL, (name, kwargs)
            message = lib.lg_last_error()
            assert name in message and word in message, message
    assert lrandom.get_state("hip") == before
    for t in (o, dq, dk, dv, pr):
        assert (t.numpy() == 3.0).all()                                  # the refused calls wrote nothing


def _tape_nodes(t):
    seen, stack, out = set(), [t], []
    while stack:
        x = stack.pop()
        ctx = getattr(x, "ctx", None)
        if ctx is None or id(ctx) in seen:
            continue
        seen.add(id(ctx))
        out.append(ctx)
        stack.extend(p for p in ctx._parents if p is not None)
    return out


def _bert(positions, attention_p):
    np.random.seed(6)
    return bert.BertForMaskedLM(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=50,
                                max_position_embeddings=positions, type_vocab_size=2, hidden_dropout_prob=0.1,
                                attention_probs_dropout_prob=attention_p)


@pytest.mark.parametrize("s,masked", [(32, False), (20, True), (160, False)], ids=["s32", "s20-mask", "s160"])
def test_the_model_takes_the_fused_node_in_training_mode(hip, s, masked):
    from lightgrad_amd.autograd.hip import HipGraph
    b, heads, seed = 2, 2, SEEDS[1]
    rng = np.random.RandomState(s)
    ids = rng.randint(0, 50, (b, s)).astype(np.int32)
    labels = rng.randint(0, 50, (b * s,)).astype(np.int64)
    mask = None
    if masked:
        mask = np.ones((b, s), np.float32)
        mask[0, 15:] = 0
        mask[1, 9:] = 0

    def loss_of(model, T, cast=lambda a: a):
        tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
        logits = model(T.from_numpy(ids, requires_grad=False), attention_mask=tm)
        return light.loss.cross_entropy(logits.reshape(-1, 50), T.from_numpy(labels, requires_grad=False))

    def loss_and_grads(model, T, cast=lambda a: a):
        loss = loss_of(model, T, cast)
        for p in model.parameters():
            p.zero_grad()
        loss.backward()
        out = {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}
        out["loss"] = np.asarray(loss.item(), np.float64)
        return out

    cpu_model = _bert(s, 0.1)
    values = {n: p.numpy() for n, p in cpu_model.named_parameters()}
    hip_model = _bert(s, 0.1).map_parameters(lambda p: p.hip())

    light.manual_seed(seed)
    loss = loss_of(hip_model, hip)
    nodes = _tape_nodes(loss)
    names = [type(c).__name__ for c in nodes]
    assert "self_attention" in names, sorted(set(names))
    for c in nodes:
        if type(c).__name__ == "dropout":
            assert tuple(c._parents[0].shape) != (b, heads, s, s)

    light.manual_seed(seed)
    cpu32 = loss_and_grads(cpu_model, CpuTensor)
    got = loss_and_grads(hip_model, hip)
    assert lrandom.get_state("cpu") == lrandom.get_state("hip") == (seed, 4)
    light.manual_seed(seed)
    with float64_tape():
        ref_model = _bert(s, 0.1)
        ref_model.load_parameters({n: a.astype(np.float64) for n, a in values.items()})
        ref64 = loss_and_grads(ref_model, CpuTensor, cast=lambda a: a.astype(np.float64))
    noise = [n for n in ref64 if n.endswith(".key.bias")]
    for n in noise:
        assert np.abs(got[n]).max() < 1e-6 and np.abs(cpu32[n]).max() < 1e-6 and np.abs(ref64[n]).max() < 1e-12
    for n in ref64:
        print("%-60s hip %.2e  cpu32 %.2e" % (n, rel_frobenius(got[n], ref64[n]), rel_frobenius(cpu32[n], ref64[n])))
    rest = {n: a for n, a in ref64.items() if n not in noise}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, rest, what="tiny-BERT, attention dropout fused, s = %d" % s)

    # the captured step reads tensors that are on the device before the capture begins
    ids_t, labels_t = hip.from_numpy(ids, requires_grad=False), hip.from_numpy(labels, requires_grad=False)
    mask_t = None if mask is None else hip.from_numpy(mask, requires_grad=False)
    counts = {}
    for attention_p in (0.1, 0.0):
        model = _bert(s, attention_p).map_parameters(lambda p: p.hip())

        def step():
            loss = light.loss.cross_entropy(model(ids_t, attention_mask=mask_t).reshape(-1, 50), labels_t)
            for p in model.parameters():
                p.zero_grad()
            loss.backward()
        step()
        graph = HipGraph()
        with graph.capture():
            step()
        counts[attention_p] = graph.kernel_count()
        graph.destroy()
    assert counts[0.1] == counts[0.0] > 0, counts
