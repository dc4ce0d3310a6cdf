"""Grouped-query attention in examples/bert.py (num_key_value_heads) on the CPU backend: the folded composite against the
repeat-heads definition in float64, its gradients, the model that has as many K/V heads as heads, and the refusals by name."""
import math
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor
from lightgrad_amd.autograd.utils.gradcheck import assert_gradcheck
from common import float64_tape
import decode_cases as dc

H, KVH, D, HIDDEN = 4, 2, 8, 32
CFG = dict(dc.CFG, num_attention_heads=4)


def attention(**options):
    np.random.seed(4)
    module = dc.bert.BertSelfAttention(HIDDEN, H, num_key_value_heads=KVH, **options)
    module.map_parameters(lambda p: CpuTensor.from_numpy(p.numpy() * (8.0 if p.numpy().ndim == 2 else 1.0)))
    return module


def repeat_heads_definition(module, x, mask):
    """softmax(q_h k_{h // R}^T / sqrt(d) + biases) v_{h // R} in numpy float64, heads repeated"""
    b, s, _ = x.shape
    q, k, v = (x @ lin.weight.numpy().T + lin.bias.numpy() for lin in (module.query, module.key, module.value))
    k, v = (np.repeat(a.reshape(b, s, KVH, D), H // KVH, axis=2) for a in (k, v))
    scores = np.einsum("bihd,bjhd->bhij", q.reshape(b, s, H, D), k) / math.sqrt(D)
    scores = scores + ((1.0 - mask) * -10000.0)[:, None, None, :] + ((1.0 - np.tril(np.ones((s, s)))) * -10000.0)
    e = np.exp(scores - scores.max(-1, keepdims=True))
    probs = e / e.sum(-1, keepdims=True)
    return np.einsum("bhij,bjhd->bihd", probs, v).reshape(b, s, H * D), probs


def test_the_folded_composite_is_the_repeat_heads_definition():
    with float64_tape():
        module = attention(causal=True)
        x = np.random.RandomState(1).uniform(-1, 1, (2, 5, HIDDEN))
        mask = np.array([[1, 1, 0, 1, 1], [1, 0, 1, 1, 0]], np.float64)
        context, probs = module(CpuTensor.from_numpy(x), CpuTensor.from_numpy(mask, requires_grad=False))
        want, want_probs = repeat_heads_definition(module, x, mask)
    np.testing.assert_allclose(context.numpy(), want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(probs.numpy(), want_probs, rtol=0, atol=1e-13)


def test_gradients_of_the_key_weight():
    with float64_tape():
        module = attention(causal=True)
        x = CpuTensor.from_numpy(np.random.RandomState(2).uniform(-1, 1, (1, 5, HIDDEN)), requires_grad=False)

        def f(w):
            module.key.weight = w
            return module(x)[0]
        assert_gradcheck(f, module.key.weight, eps=1e-6, atol=1e-7, rtol=1e-6)


def test_cached_steps_are_the_full_forwards_last_rows():
    """prefill and `_grouped_decode` over the tensor API: the cache holds the unexpanded rows"""
    with float64_tape():
        np.random.seed(dc.SEED)
        model = dc.bert.BertForMaskedLM(**dict(CFG, num_key_value_heads=2)).eval()
        model.map_parameters(lambda p: CpuTensor.from_numpy(p.numpy() * (dc.GAIN if p.numpy().ndim == 2 else 1.0)))
        ids = np.random.randint(0, CFG["vocab_size"], (2, 9)).astype(np.int32)
        out = dc.bert.generate(model, CpuTensor.from_numpy(ids[:, :5], requires_grad=False), 4).numpy()
        seq = ids[:, :5]
        for _ in range(4):
            seq = np.concatenate([seq, dc.full_logits(model, seq)[:, -1].argmax(-1).astype(np.int32)[:, None]], axis=1)
    np.testing.assert_array_equal(out, seq)


def test_as_many_kv_heads_as_heads_is_the_old_model():
    _, ids = dc.parameters()
    models = []
    for extra in ({}, {"num_key_value_heads": CFG["num_attention_heads"]}):
        np.random.seed(1)
        models.append(dc.bert.BertForMaskedLM(**dict(CFG, **extra)).eval())
    old, new = ({n: p.numpy() for n, p in m.named_parameters()} for m in models)
    assert list(old) == list(new) and all(old[n].shape == new[n].shape for n in old)
    np.testing.assert_array_equal(dc.full_logits(models[0], ids), dc.full_logits(models[1], ids))


ROUTES = [("num_beams", dict(num_beams=2)), ("speculate", dict(speculate=2)), ("lengths", dict(lengths=[5, 4])),
          ("prefill_chunk", dict(prefill_chunk=2)), ("serve", None), ("_extend", "append")]


@pytest.mark.parametrize("name,options", ROUTES, ids=[r[0] for r in ROUTES])
def test_the_other_routes_refuse_the_model_by_name(name, options):
    np.random.seed(1)
    model = dc.bert.BertForMaskedLM(**dict(CFG, num_key_value_heads=1)).eval()
    ids = CpuTensor.from_numpy(dc.parameters()[1][:, :5], requires_grad=False)
    with pytest.raises(AssertionError, match="%s.* num_key_value_heads = 1 below its 4 heads" % name):
        if options is None:
            dc.bert.serve(model, [[1, 2, 3]], 2)
        elif options == "append":
            cache = dc.nn.KVCache(CFG["num_hidden_layers"], 2, 16, 16, like=model.cls.predictions.bias)
            with light.no_grad():
                model(ids, cache=cache, append=True)
        else:
            dc.bert.generate(model, ids, 2, **options)
