"""examples/bert.py config key `attention_probs=False` on the CpuTensor backend: the composite lines run as they did, the probabilities
are computed and dropped - (context, None), the context bits of the default model - also beyond 512 positions"""
import numpy as np
import pytest
from lightgrad_amd import CpuTensor
from test_bert_cpu import bert

CFG = dict(hidden_size=64, intermediate_size=128, num_hidden_layers=1, num_attention_heads=2, vocab_size=60,
           max_position_embeddings=544, type_vocab_size=2)


@pytest.mark.parametrize("causal", [False, True])
def test_no_probabilities_and_the_default_context(causal):
    rng = np.random.RandomState(3)
    ids = CpuTensor.from_numpy(rng.randint(0, 60, (2, 530)).astype(np.int32), requires_grad=False)
    mask = np.ones((2, 530), np.float32)
    mask[1, 400:] = 0
    results = []
    for extra in ({}, {"attention_probs": False}):
        np.random.seed(5)
        model = bert.BertForMaskedLM(**dict(CFG, causal=causal, **extra))
        attention = model.bert.encoder.layer[0].attention.self
        assert attention.attention_probs == (not extra)
        results.append(attention(model.bert.embeddings(ids), attention_mask=CpuTensor.from_numpy(mask, requires_grad=False)))
    (context, probs), (streamed, none) = results
    assert probs.shape == (2, 2, 530, 530) and none is None
    np.testing.assert_array_equal(streamed.numpy(), context.numpy())
