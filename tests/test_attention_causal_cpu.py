"""causal attention and the next-token labels on the numpy backend, which defines their values: the composite causal branch of
examples/bert.py (`scores + (1 - tril) * -10000` behind the key-padding bias) against a direct float64 formula - a softmax over
the keys j <= i only -, `light.data.next_token_labels`, and what `causal=False` leaves as it was.

The error rule is the float64 tape's (tests/common.py): a float32 result lies within 1e-5 (relative Frobenius) of the float64 one."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from common import float64_tape, rel_frobenius
from test_bert_cpu import bert

SHAPES = [(1, 1, 1, 32), (2, 5, 2, 32), (3, 33, 1, 64), (2, 128, 2, 64)]          # (b, s, heads, d)


def padding_mask(b, s):
    """trailing padding of a different length per batch element and one hole; key 0 stays at 1"""
    m = np.ones((b, s), np.float32)
    for i in range(b):
        m[i, max(1, s - (1 + i) * max(1, s // 5)):] = 0
    if s >= 5:
        m[0, s // 3] = 0
    return m


def direct(x, params, heads, mask):
    """float64: context and probabilities of causal self-attention, the softmax taken over the keys j <= i alone"""
    x = x.astype(np.float64)
    wq, bq, wk, bk, wv, bv = (p.astype(np.float64) for p in params)
    b, s, _ = x.shape
    d = wq.shape[0] // heads
    q, k, v = ((x @ w.T + c).reshape(b, s, heads, d).transpose(0, 2, 1, 3) for w, c in ((wq, bq), (wk, bk), (wv, bv)))
    scores = q @ k.transpose(0, 1, 3, 2) / np.sqrt(d)
    if mask is not None:
        scores = scores + ((1.0 - mask.astype(np.float64)) * -10000.0)[:, None, None, :]
    probs = np.zeros_like(scores)
    for i in range(s):
        row = scores[:, :, i, :i + 1]
        e = np.exp(row - row.max(axis=-1, keepdims=True))
        probs[:, :, i, :i + 1] = e / e.sum(axis=-1, keepdims=True)
    return (probs @ v).transpose(0, 2, 1, 3).reshape(b, s, heads * d), probs


def module_run(x, params, heads, mask, f64, causal=True):
    """context, probabilities and input gradient of BertSelfAttention(causal=) on CpuTensor, float32 or on the float64 tape"""
    cast = (lambda a: a.astype(np.float64)) if f64 else (lambda a: a)
    hidden = x.shape[2]
    np.random.seed(0)
    m = bert.BertSelfAttention(hidden, heads, causal=causal)
    m.load_parameters({n: cast(p) for n, p in zip(("query.weight", "query.bias", "key.weight", "key.bias", "value.weight", "value.bias"), params)})
    tx = CpuTensor.from_numpy(cast(x))
    tm = None if mask is None else CpuTensor.from_numpy(cast(mask), requires_grad=False)
    context, probs = m(tx, attention_mask=tm)
    w = np.random.RandomState(5).uniform(-1, 1, context.shape)
    (context * CpuTensor.from_numpy(cast(w.astype(np.float32)), requires_grad=False)).backward(allow_fill=True)
    with light.no_grad():
        values = m.value(tx).numpy()                # the module's own value projection of the same input: the same bits
    return context.numpy(), probs.numpy(), tx.grad.numpy(), values


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%dx%dx%d" % s for s in SHAPES])
def test_composite_causal_branch_against_the_direct_formula(shape, masked):
    b, s, heads, d = shape
    width = heads * d
    rng = np.random.RandomState(s)
    x = rng.uniform(-1, 1, (b, s, width)).astype(np.float32)
    params = []
    for _ in range(3):
        params += [rng.uniform(-0.3, 0.3, (width, width)).astype(np.float32), rng.uniform(-0.3, 0.3, (width,)).astype(np.float32)]
    mask = padding_mask(b, s) if masked else None
    want_context, want_probs = direct(x, params, heads, mask)
    got32 = module_run(x, params, heads, mask, False)
    with float64_tape():
        got64 = module_run(x, params, heads, mask, True)
    assert got32[0].dtype == np.float32 and got64[0].dtype == np.float64
    future = np.triu(np.ones((s, s), bool), 1)
    for name, got, tol in (("float32", got32, 1e-5), ("float64", got64, 1e-12)):
        context, probs = got[:2]
        assert (probs[:, :, future] == 0).all(), name                       # exp underflows to exactly 0 behind the -10000
        assert not np.signbit(probs[:, :, future]).any(), name
        np.testing.assert_allclose(probs.sum(axis=-1), 1.0, rtol=0, atol=1e-5)
        if mask is None:
            assert (probs[:, :, 0, 0] == 1.0).all(), name
        e_context, e_probs = rel_frobenius(context, want_context), rel_frobenius(probs, want_probs)
        print("%s %s: context %.3e probs %.3e" % (shape, name, e_context, e_probs))
        assert e_context <= tol and e_probs <= tol, (name, e_context, e_probs)
    e_dx = rel_frobenius(got32[2], got64[2])
    assert e_dx <= 1e-5, e_dx
    if mask is None:
        # row 0 sees key 0 alone: its context is the value row itself, bit for bit
        np.testing.assert_array_equal(got32[0][:, 0], got32[3][:, 0])


def test_nothing_from_the_future_reaches_an_earlier_position():
    b, s, heads, d, t = 2, 40, 2, 32, 17
    width = heads * d
    rng = np.random.RandomState(1)
    x = rng.uniform(-1, 1, (b, s, width)).astype(np.float32)
    params = []
    for _ in range(3):
        params += [rng.uniform(-0.3, 0.3, (width, width)).astype(np.float32), rng.uniform(-0.3, 0.3, (width,)).astype(np.float32)]
    first = module_run(x, params, heads, None, False)
    x2 = x.copy()
    x2[:, t:] = rng.uniform(-1, 1, (b, s - t, width)).astype(np.float32)
    second = module_run(x2, params, heads, None, False)
    np.testing.assert_array_equal(second[0][:, :t], first[0][:, :t])
    np.testing.assert_array_equal(second[1][:, :, :t], first[1][:, :, :t])
    assert (second[0][:, t:] != first[0][:, t:]).any()
    # and without the flag the module is what it was: the future is seen
    plain = module_run(x, params, heads, None, False, causal=False)
    plain2 = module_run(x2, params, heads, None, False, causal=False)
    assert (plain[1][:, :, :t, t:] > 0).all() and (plain2[0][:, :t] != plain[0][:, :t]).any()


@pytest.mark.parametrize("dtype", [np.int32, np.int64])
def test_next_token_labels(dtype):
    ids = np.random.RandomState(2).randint(0, 1000, (3, 7)).astype(dtype)
    labels = light.data.next_token_labels(CpuTensor.from_numpy(ids, requires_grad=False))
    assert isinstance(labels, CpuTensor) and labels.dtype == np.dtype(dtype) and labels.shape == (3, 7) and not labels.requires_grad
    got = labels.numpy()
    np.testing.assert_array_equal(got[:, :-1], ids[:, 1:])
    assert (got[:, -1] == -100).all()
    other = light.data.next_token_labels(CpuTensor.from_numpy(ids, requires_grad=False), ignore_index=-1).numpy()
    assert (other[:, -1] == -1).all() and (other[:, :-1] == ids[:, 1:]).all()
    one = light.data.next_token_labels(CpuTensor.from_numpy(ids[:, :1], requires_grad=False)).numpy()
    assert one.shape == (3, 1) and (one == -100).all()
    with pytest.raises(TypeError):
        light.data.next_token_labels(ids)
    with pytest.raises(AssertionError):
        light.data.next_token_labels(CpuTensor.from_numpy(ids.astype(np.float32), requires_grad=False))


def test_the_causal_lm_step_on_the_numpy_backend():
    """`clm_forward_backward`: the loss of the next-token labels, the last position left out; every parameter takes a gradient"""
    cfg = dict(hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, vocab_size=13,
               max_position_embeddings=9, type_vocab_size=2)
    ids = np.random.RandomState(4).randint(0, 13, (2, 9)).astype(np.int32)
    np.random.seed(8)
    model = bert.BertForMaskedLM(**cfg, causal=True)
    loss = bert.clm_forward_backward(model, CpuTensor.from_numpy(ids, requires_grad=False))
    with light.no_grad():
        logits32 = model(CpuTensor.from_numpy(ids, requires_grad=False)).numpy()
    logits = logits32.astype(np.float64)
    logp = logits - np.log(np.exp(logits - logits.max(-1, keepdims=True)).sum(-1, keepdims=True)) - logits.max(-1, keepdims=True)
    want = -np.mean([logp[b, i, ids[b, i + 1]] for b in range(2) for i in range(8)])
    assert abs(loss.item() - want) <= 1e-5 * abs(want)
    assert all(p.grad is not None and np.isfinite(p.grad.numpy()).all() for p in model.parameters())
    # logits of position i do not move when the tokens behind it change
    ids2 = ids.copy()
    ids2[:, 5:] = (ids2[:, 5:] + 3) % 13
    with light.no_grad():
        moved = model(CpuTensor.from_numpy(ids2, requires_grad=False)).numpy()
    np.testing.assert_array_equal(moved[:, :5], logits32[:, :5])


def test_causal_false_is_the_model_of_before():
    """the default and an explicit causal=False build the same model with the same bits (tests/golden holds them:
    test_bert_cpu.py::test_forward_matches_reference_fixture runs the default)"""
    cfg = dict(hidden_size=16, intermediate_size=32, num_hidden_layers=1, num_attention_heads=2, vocab_size=13,
               max_position_embeddings=9, type_vocab_size=2)
    ids = CpuTensor.from_numpy(np.random.RandomState(4).randint(0, 13, (2, 9)).astype(np.int32), requires_grad=False)
    outs = []
    for extra in ({}, {"causal": False}, {"causal": True}):
        np.random.seed(8)
        model = bert.BertForMaskedLM(**cfg, **extra)
        with light.no_grad():
            outs.append(model(ids).numpy())
    np.testing.assert_array_equal(outs[0], outs[1])
    assert (outs[0] != outs[2]).any()
