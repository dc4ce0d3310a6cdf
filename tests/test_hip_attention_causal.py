"""causal attention inside the fused forward launches (CAUSAL instantiations of csrc/attention.hip and csrc/attention_long.hip, entry
lg_attention_causal_fwd_f32; ops `attention`, `masked_attention`, `long_attention`, `self_attention` with causal=True) and the
causal-LM objective of examples/bert.py: against a float64 run of the model's own composite lines with one more additive constant
(`scores + (1 - tril) * -10000` behind the key-padding bias), the exact properties of a causal softmax, what a position may depend
on bit for bit, dropout from the same stream, which entries are called, and the model.

The error rule is the project's own (test_hip_attention_masked.py): each result within 1e-5 (relative Frobenius) of the float64
composite, and no further from it than twice the fp32 composite on the same backend + 2e-7.  A gradient that is mathematically
zero - the key bias: a softmax does not move when every score of a row moves by the same amount - is rounding noise on every path
and has no relative error: it is held to the magnitude test_hip_bert.py::test_self_attention_node holds it to."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, rel_frobenius, assert_as_close_to_float64_as_the_cpu_backend
from test_hip_dropout import LG_EINVAL
from test_hip_attention_masked import operands, padding_mask, assert_close_to_float64
from test_hip_attention_dispatch import recorder, PLAIN, MASKED, LONG, DROPOUT        # noqa: F401 (recorder is a fixture)
from test_bert_cpu import bert

pytestmark = pytest.mark.gpu

CAUSAL = "lg_attention_causal_fwd_f32"


def causal_lines(scores, mask, s):
    """the composite's additive constants: the key-padding bias, then the causal one"""
    if mask is not None:
        m = mask.reshape(mask.shape[0], 1, 1, mask.shape[1])
        scores = scores + ((1.0 - m) * -10000.0).detach()
    tril = scores.__class__.from_numpy(np.tril(np.ones((1, 1, s, s), dtype=scores.dtype)), requires_grad=False)
    return scores + ((1.0 - tril) * -10000.0).detach()


def composite(q, k, v, heads, mask=None, dropout=0.0):
    """examples/bert.py BertSelfAttention.forward, composite branch, causal=True"""
    b, s, width = q.shape
    d = width // heads
    q4 = q.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
    k4 = k.reshape(b, s, heads, d).transpose(0, 2, 3, 1)
    v4 = v.reshape(b, s, heads, d).transpose(0, 2, 1, 3)
    probs = causal_lines((q4 @ k4) / math.sqrt(d), mask, s).softmax(axis=-1)
    dropped = probs.dropout(dropout) if dropout > 0 else probs
    return (dropped @ v4).transpose(0, 2, 1, 3).reshape(b, s, width), probs


def fused(q, k, v, heads, mask=None, dropout=0.0):
    """the form the model takes for this length and mask, causal=True"""
    s = q.shape[1]
    scale = float(np.sqrt(q.shape[2] // heads)) ** -1
    if s > 128:
        assert q.long_attention_supported(heads, causal=True)
        return q.long_attention(k, v, heads=heads, scale=scale, mask=mask, dropout=dropout, causal=True)
    if mask is not None or s % 32:
        assert q.masked_attention_supported(heads, causal=True)
        return q.masked_attention(k, v, heads=heads, scale=scale, mask=mask, dropout=dropout, causal=True)
    assert q.attention_supported(heads, causal=True)
    return q.attention(k, v, heads=heads, scale=scale, dropout=dropout, causal=True)


def run(T, f64, arrays, heads, mask, how, dropout=0.0):
    """[context, probs, dq, dk, dv] as numpy; how = "fused" or "composite" """
    q, k, v, w = arrays
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    ts = [T.from_numpy(cast(x)) for x in (q, k, v)]
    tm = None if mask is None else T.from_numpy(cast(mask), requires_grad=False)
    if how == "fused":
        out = fused(*ts, heads, tm, dropout)
        probs = out.attention_probs
        assert probs.shape == (q.shape[0], heads, q.shape[1], q.shape[1]) and not probs.requires_grad
    else:
        out, probs = composite(*ts, heads, tm, dropout)
    (out * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
    return [out.numpy(), probs.numpy()] + [t.grad.numpy() for t in ts]


def future(s):
    return np.triu(np.ones((s, s), bool), 1)


# both the first and the last block of queries of every form; a last chunk of keys that is partial (129, 160, 383), cut by the
# diagonal (every block of 257, 383, 512 but the last) or left out (the first blocks beyond 128)
SHAPES = [(1, 1, 1, 32), (2, 5, 2, 32), (3, 33, 1, 64), (2, 64, 2, 64), (2, 127, 2, 64), (2, 128, 2, 64), (1, 129, 1, 32), (2, 160, 2, 64),
          (1, 257, 2, 32), (1, 383, 1, 64), (1, 512, 1, 64)]
CASES = [(shape, masked) for shape in SHAPES for masked in (False, True)]


@pytest.mark.parametrize("shape,masked", CASES, ids=["%dx%dx%dx%d-%s" % (c[0] + ("mask" if c[1] else "nomask",)) for c in CASES])
def test_sweep_against_the_float64_causal_composite(hip, shape, masked):
    b, s, heads, d = shape
    arrays = operands(b, s, heads, d)
    mask = padding_mask(b, s) if masked else None
    got = run(hip, False, arrays, heads, mask, "fused")
    comp = run(hip, False, arrays, heads, mask, "composite")
    with float64_tape():
        want = run(CpuTensor, True, arrays, heads, mask, "composite")
    assert all(np.isfinite(x).all() for x in got)
    context, probs = got[:2]
    above = probs[:, :, future(s)]
    assert (above == 0).all() and not np.signbit(above).any()
    np.testing.assert_allclose(probs.sum(axis=-1), 1.0, rtol=0, atol=1e-5)
    if mask is None:
        assert (probs[:, :, 0, 0] == 1.0).all()
        np.testing.assert_array_equal(context[:, 0], arrays[2][:, 0])         # row 0 sees key 0 alone: its context is v row 0
    else:
        gone = np.broadcast_to((mask == 0)[:, None, None, :], probs.shape)
        assert (probs[gone] == 0).all()
    assert_close_to_float64(got, comp, want, str((b, s, heads, d, masked)))


@pytest.mark.parametrize("shape,t", [((2, 100, 2, 32), 37), ((1, 300, 1, 64), 150)], ids=["100-t37", "300-t150"])
def test_nothing_from_the_future(hip, shape, t):
    """q, k, v and the output gradient replaced at positions >= t: context, probabilities and dq before t keep every bit"""
    b, s, heads, d = shape
    arrays = operands(b, s, heads, d, seed=21)
    first = run(hip, False, arrays, heads, None, "fused")
    other = operands(b, s, heads, d, seed=22)
    replaced = [x.copy() for x in arrays]
    for x, y in zip(replaced, other):
        x[:, t:] = 3 * y[:, t:]
    second = run(hip, False, replaced, heads, None, "fused")
    np.testing.assert_array_equal(second[0][:, :t], first[0][:, :t], err_msg="context")
    np.testing.assert_array_equal(second[1][:, :, :t, :], first[1][:, :, :t, :], err_msg="probs")
    np.testing.assert_array_equal(second[2][:, :t], first[2][:, :t], err_msg="dq")
    assert (second[0][:, t:] != first[0][:, t:]).any() and (second[2][:, t:] != first[2][:, t:]).any()


@pytest.mark.parametrize("shape", [(2, 5, 2, 32), (1, 64, 1, 32), (1, 160, 1, 32)], ids=["5", "64", "160"])
def test_dropout_against_the_float64_composite(hip, shape):
    """p = 0.5: the float64 composite draws the same mask (`probs.dropout(p)` behind the causal softmax, the same seed)"""
    b, s, heads, d = shape
    p, seed = 0.5, 1234
    arrays = operands(b, s, heads, d, seed=9)
    undropped = run(hip, False, arrays, heads, None, "fused")[1]
    light.manual_seed(seed)
    got = run(hip, False, arrays, heads, None, "fused", p)
    assert lrandom.get_state("hip") == (seed, 1)                          # one call of the stream, forward and backward
    light.manual_seed(seed)
    comp = run(hip, False, arrays, heads, None, "composite", p)
    assert lrandom.get_state("hip") == (seed, 1)
    light.manual_seed(seed)
    with float64_tape():
        want = run(CpuTensor, True, arrays, heads, None, "composite", p)
    assert lrandom.get_state("cpu") == (seed, 1)
    np.testing.assert_array_equal(got[1], undropped)                      # .attention_probs stays the undropped probabilities
    assert (got[1][:, :, future(s)] == 0).all()
    assert (got[0] != run(hip, False, arrays, heads, None, "fused")[0]).any()
    assert_close_to_float64(got, comp, want, "dropout %s" % (shape,))


@pytest.mark.parametrize("s", [20, 32, 160])
def test_self_attention_causal_node(hip, s):
    """projections + causal attention as one node against three nn.Linear and the causal composite lines"""
    b, hidden, heads = 2, 64, 2
    rng = np.random.RandomState(10 + s)
    x = rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32)
    params = []
    for _ in range(3):
        params += [rng.uniform(-0.2, 0.2, (hidden, hidden)).astype(np.float32), rng.uniform(-0.2, 0.2, (hidden,)).astype(np.float32)]
    w = rng.uniform(-1, 1, (b, s, hidden)).astype(np.float32)
    scale = float(np.sqrt(hidden // heads)) ** -1

    def go(T, f64, node):
        cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
        leaf = T.from_numpy(cast(x))
        tx = leaf * 1.0
        ps = [T.from_numpy(cast(p)) for p in params]
        if node:
            assert tx.self_attention_supported(ps[0], heads, masked=s % 32 != 0, long=s > 128, causal=True)
            out = tx.self_attention(*ps, heads=heads, scale=scale, causal=True)
            probs = out.attention_probs
        else:
            layers = []
            for i in range(3):
                layer = nn.Linear(hidden, hidden)
                layer.weight, layer.bias = ps[2 * i], ps[2 * i + 1]
                layers.append(layer)
            out, probs = composite(*(layer(tx) for layer in layers), heads)
        (out * T.from_numpy(cast(w), requires_grad=False)).backward(allow_fill=True)
        return [out.numpy(), probs.numpy(), leaf.grad.numpy()] + [t.grad.numpy() for t in ps]

    got, comp = go(hip, False, True), go(hip, False, False)
    with float64_tape():
        want = go(CpuTensor, True, False)
    assert (got[1][:, :, future(s)] == 0).all()
    names = ["context", "probs", "dx", "dwq", "dbq", "dwk", "dbk", "dwv", "dbv"]
    for name, g, c, r in zip(names, got, comp, want):
        if name == "dbk":                                          # mathematically zero: rounding noise on every path
            assert np.abs(g).max() < 1e-4 * np.abs(want[4]).max() + 1e-6
            continue
        e_fused, e_comp = rel_frobenius(g, r), rel_frobenius(c, r)
        print("s = %d %s: fused %.3e, fp32 composite %.3e" % (s, name, e_fused, e_comp))
        assert e_fused <= 1e-5, (name, e_fused, e_comp)
        assert e_fused <= 2 * e_comp + 2e-7, (name, e_fused, e_comp)


def tensors(hip, *shapes, seed=3):
    rng = np.random.RandomState(seed)
    return [hip.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)) for shape in shapes]


OPS = [("attention", 32, 0.0, PLAIN), ("attention", 64, 0.5, DROPOUT), ("masked_attention", 5, 0.0, MASKED), ("masked_attention", 5, 0.5, DROPOUT),
       ("long_attention", 131, 0.0, LONG), ("long_attention", 131, 0.5, DROPOUT)]


@pytest.mark.parametrize("op,s,dropout,family", OPS, ids=["%s-%d-p%g" % c[:3] for c in OPS])
def test_entries_of_the_ops(hip, recorder, op, s, dropout, family):            # noqa: F811
    """causal=True: the causal forward entry, then the backward entry the form has without it; causal=False: the entries of before"""
    light.manual_seed(1)
    q, k, v = tensors(hip, *[(1, s, 32)] * 3)
    out = getattr(q, op)(k, v, heads=1, scale=32 ** -0.5, dropout=dropout, causal=True)
    out.backward(allow_fill=True)
    assert recorder.calls == [CAUSAL, family[1]]
    assert all(np.isfinite(t.grad.numpy()).all() for t in (q, k, v))
    del recorder.calls[:]
    out = getattr(q, op)(k, v, heads=1, scale=32 ** -0.5, dropout=dropout, causal=False)
    out.backward(allow_fill=True)
    assert recorder.calls == list(family)


@pytest.mark.parametrize("s,family", [(32, PLAIN), (20, MASKED), (160, LONG)], ids=["32", "20", "160"])
def test_entries_of_self_attention(hip, recorder, s, family):                  # noqa: F811
    hidden, heads = 64, 2
    x, wq, bq, wk, bk, wv, bv = tensors(hip, (1, s, hidden), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,), (hidden, hidden), (hidden,))
    out = x.self_attention(wq, bq, wk, bk, wv, bv, heads=heads, scale=(hidden // heads) ** -0.5, causal=True)
    out.backward(allow_fill=True)
    assert recorder.calls == [CAUSAL, family[1]]
    assert all(np.isfinite(t.grad.numpy()).all() for t in (x, wq, bq, wk, bk, wv, bv))


SENTINEL = 3.0


def raw_call(hip, s, d=32, heads=1):
    """the causal entry over operands of ONE batch element - `batch` is what the caller says - and the tensors it would write"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    w = heads * d
    q, k, v = tensors(hip, *[(1, s, w)] * 3)
    o = hip.from_numpy(np.full((1, s, w), SENTINEL, np.float32))
    pr = hip.from_numpy(np.full((1, heads, s, s), SENTINEL, np.float32))
    base = hip.from_numpy(np.zeros(1, np.uint64))

    def forward(batch=1, S=s, q_ptr=None, prob=0.0, base_ptr=None):
        return lib.lg_attention_causal_fwd_f32(q.ptr if q_ptr is None else q_ptr, w, s * w, k.ptr, w, s * w, v.ptr, w, s * w, o.ptr, w, s * w,
                                               pr.ptr, batch, heads, S, d, 0.2, None, 0, prob, base_ptr)
    return lib, forward, (o, pr), (q, k, v, base)


def test_the_entry_through_the_c_abi(hip):
    lib, forward, written, keep = raw_call(hip, 32)
    assert lib.lg_attention_causal_supported(1, 32) == 1 and lib.lg_attention_causal_supported(512, 64) == 1
    assert lib.lg_attention_causal_supported(0, 32) == 0 and lib.lg_attention_causal_supported(513, 32) == 0
    assert lib.lg_attention_causal_supported(64, 48) == 0
    light.manual_seed(4)
    before = lrandom.get_state("hip")
    assert forward(batch=0) == 0                                          # an empty batch: nothing to do, nothing drawn
    # an unsupported length AND a misaligned q: the length is what the message names
    assert forward(S=513, q_ptr=keep[0].ptr + 4) == LG_EINVAL
    message = lib.lg_last_error()
    assert b"unsupported" in message and CAUSAL.encode() + b":" in message and b"513" in message, message
    # dropout needs the word the launch writes the call's number to
    assert forward(prob=0.5) == LG_EINVAL
    message = lib.lg_last_error()
    assert CAUSAL.encode() + b":" in message and b"base_out" in message, message
    # with one, the dropout entry's rules: a probability in [0, 1), a batch that is not empty
    assert forward(prob=1.0, base_ptr=keep[3].ptr) == LG_EINVAL and b"outside" in lib.lg_last_error()
    assert forward(batch=0, prob=0.5, base_ptr=keep[3].ptr) == LG_EINVAL and b"batch" in lib.lg_last_error()
    assert forward(q_ptr=keep[0].ptr + 4) == LG_EINVAL and b"aligned" in lib.lg_last_error()
    assert lrandom.get_state("hip") == before
    for t in written:
        assert (t.numpy() == SENTINEL).all()
    assert forward() == 0
    assert lrandom.get_state("hip") == before
    assert (written[0].numpy() != SENTINEL).any() and (written[1].numpy()[0, 0][future(32)] == 0).all()


@pytest.mark.parametrize("s", [5, 131])
def test_nothing_outside_the_operands_is_read_or_written(hip, s):
    """operands between bands of NaN, outputs between bands of a marker: the dense run's bits, every band as it was"""
    from lightgrad_amd.autograd.hip import lib as L
    lib = L.lib()
    b, heads, d, band = 2, 2, 32, 8
    w = heads * d
    q, k, v, _ = operands(b, s, heads, d, seed=11)
    mask = padding_mask(b, s)
    marker = np.float32(-777.25)

    def banded(x, fill):
        flat = np.full(band * w + x.size + band * w, fill, np.float32)
        flat[band * w:band * w + x.size] = x.reshape(-1)
        return hip.from_numpy(flat, requires_grad=False)

    n_o, n_p = b * s * w, b * heads * s * s
    ins = [banded(x, np.nan) for x in (q, k, v)]
    tm = banded(mask, np.nan)
    o, p = banded(np.full(n_o, marker, np.float32), marker), banded(np.full(n_p, marker, np.float32), marker)
    first = band * w * 4                                                  # bytes in front of every payload: a multiple of 16
    L.check(lib.lg_attention_causal_fwd_f32(ins[0].ptr + first, w, s * w, ins[1].ptr + first, w, s * w, ins[2].ptr + first, w, s * w,
                                            o.ptr + first, w, s * w, p.ptr + first, b, heads, s, d, float(np.sqrt(d)) ** -1,
                                            tm.ptr + first, s, 0.0, None))
    ts = [hip.from_numpy(x) for x in (q, k, v)]
    with light.no_grad():
        dense = fused(*ts, heads, hip.from_numpy(mask, requires_grad=False))
    for name, t, n, want in (("o", o, n_o, dense.numpy()), ("p", p, n_p, dense.attention_probs.numpy())):
        flat = t.numpy()
        assert (flat[:band * w] == marker).all() and (flat[band * w + n:] == marker).all(), name
        np.testing.assert_array_equal(flat[band * w:band * w + n], want.reshape(-1), err_msg=name)
        assert np.isfinite(want).all()
    for name, t, x in zip(("q", "k", "v", "mask"), ins + [tm], (q, k, v, mask)):
        flat = t.numpy()
        assert np.isnan(flat[:band * w]).all() and np.isnan(flat[band * w + x.size:]).all(), name
        np.testing.assert_array_equal(flat[band * w:band * w + x.size], x.reshape(-1), err_msg=name)


def _model(positions, causal):
    np.random.seed(6)
    return bert.BertForMaskedLM(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=50,
                                max_position_embeddings=positions, type_vocab_size=2, causal=causal)


def _tape_names(t):
    seen, stack, names = set(), [t], []
    while stack:
        ctx = getattr(stack.pop(), "ctx", None)
        if ctx is None or id(ctx) in seen:
            continue
        seen.add(id(ctx))
        names.append(type(ctx).__name__)
        stack.extend(p for p in ctx._parents if p is not None)
    return names


@pytest.mark.parametrize("s", [20, 160])
def test_the_causal_lm_step_of_the_model(hip, s):
    """one `clm_forward_backward` of a one-layer model with causal=True: every parameter gradient as close to a float64 run as the
    numpy backend's; the captured step has the launches of the same model with causal=False; two replays give the same loss"""
    from lightgrad_amd.autograd.hip import HipGraph
    ids = np.random.RandomState(s).randint(0, 50, (2, s)).astype(np.int32)

    def loss_and_grads(model, T):
        loss = bert.clm_forward_backward(model, T.from_numpy(ids, requires_grad=False))
        out = {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}
        out["loss"] = np.asarray(loss.item(), np.float64)
        return out, loss

    cpu_model = _model(s, True)
    values = {n: p.numpy() for n, p in cpu_model.named_parameters()}
    cpu32, _ = loss_and_grads(cpu_model, CpuTensor)
    got, loss = loss_and_grads(_model(s, True).map_parameters(lambda p: p.hip()), hip)
    assert "self_attention" in _tape_names(loss)
    with float64_tape():
        ref_model = _model(s, True)
        ref_model.load_parameters({n: a.astype(np.float64) for n, a in values.items()})
        ref64, _ = loss_and_grads(ref_model, CpuTensor)
    noise = [n for n in ref64 if n.endswith(".key.bias")]              # mathematically zero: rounding noise on every path
    for n in noise:
        assert np.abs(got[n]).max() < 1e-6 and np.abs(cpu32[n]).max() < 1e-6 and np.abs(ref64[n]).max() < 1e-12
    for n in ref64:
        print("%-60s hip %.2e  cpu32 %.2e" % (n, rel_frobenius(got[n], ref64[n]), rel_frobenius(cpu32[n], ref64[n])))
    rest = {n: a for n, a in ref64.items() if n not in noise}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, rest, what="causal LM, s = %d" % s)

    ids_t = hip.from_numpy(ids, requires_grad=False)
    counts = {}
    for causal in (True, False):
        model = _model(s, causal).map_parameters(lambda p: p.hip())
        bert.clm_forward_backward(model, ids_t)                           # eager once: pool, kernels, the model's constants
        graph = HipGraph()
        with graph.capture():
            step_loss = bert.clm_forward_backward(model, ids_t)
        counts[causal] = graph.kernel_count()
        if causal:
            graph.replay()
            one = np.float32(step_loss.item())
            graph.replay()
            two = np.float32(step_loss.item())
            assert one.tobytes() == two.tobytes() and abs(float(one) - float(ref64["loss"])) <= 1e-5 * abs(float(ref64["loss"]))
        graph.destroy()
    assert counts[True] == counts[False] > 0, counts


def test_next_token_labels_on_the_device(hip):
    for dtype in (np.int32, np.int64):
        ids = np.random.RandomState(2).randint(0, 1000, (3, 7)).astype(dtype)
        t = hip.from_numpy(ids, requires_grad=False)
        labels = light.data.next_token_labels(t)
        assert isinstance(labels, hip) and labels.dtype == np.dtype(dtype) and labels.shape == (3, 7) and not labels.requires_grad
        want = light.data.next_token_labels(CpuTensor.from_numpy(ids, requires_grad=False)).numpy()
        np.testing.assert_array_equal(labels.numpy(), want)
        # a strided view of ids, and one column
        wide = hip.from_numpy(np.repeat(ids, 2, axis=1), requires_grad=False)
        view = hip(wide.data, (3, 7), (14, 2), wide.offset, wide.dtype, requires_grad=False)
        np.testing.assert_array_equal(light.data.next_token_labels(view, ignore_index=-1).numpy(), np.where(want == -100, -1, want))
        assert (light.data.next_token_labels(hip.from_numpy(ids[:, :1], requires_grad=False)).numpy() == -100).all()
