"""examples/bert.py in training mode with hidden dropout on the HIP backend: every hidden dropout sits next to a LayerNorm and
is one node with it (`layer_norm_dropout` behind the embeddings, `dropout_add_layer_norm` behind the attention output and the
feed-forward block, which stays the one-node `feed_forward`), so the captured step launches what the model without hidden
dropout launches; loss and gradients against the float64 run of the same tape."""
import numpy as np
import pytest
import lightgrad_amd as light
from lightgrad_amd import CpuTensor, random as lrandom
from common import float64_tape, assert_as_close_to_float64_as_the_cpu_backend, rel_frobenius
from test_hip_dropout import SEEDS
from test_hip_attention_dropout import _tape_nodes
from test_bert_cpu import bert

pytestmark = pytest.mark.gpu

B, S, VOCAB, LAYERS = 2, 32, 50, 1
IDS = np.random.RandomState(S).randint(0, VOCAB, (B, S)).astype(np.int32)
LABELS = np.random.RandomState(S + 1).randint(0, VOCAB, (B * S,)).astype(np.int64)


def _bert(hidden_p, attention_p=0.0):
    np.random.seed(6)
    return bert.BertForMaskedLM(hidden_size=64, intermediate_size=128, num_hidden_layers=LAYERS, num_attention_heads=2, vocab_size=VOCAB,
                                max_position_embeddings=S, type_vocab_size=2, hidden_dropout_prob=hidden_p,
                                attention_probs_dropout_prob=attention_p)


def _loss(model, T):
    logits = model(T.from_numpy(IDS, requires_grad=False))
    return light.loss.cross_entropy(logits.reshape(-1, VOCAB), T.from_numpy(LABELS, requires_grad=False))


def _names(loss):
    return [type(c).__name__ for c in _tape_nodes(loss)]


def test_tape_structure(hip):
    light.manual_seed(3)
    model = _bert(0.1).map_parameters(lambda p: p.hip())
    plain = _bert(0.0).map_parameters(lambda p: p.hip())
    names = _names(_loss(model, hip))
    assert names.count("feed_forward") == LAYERS and names.count("dropout_add_layer_norm") == 2 * LAYERS, sorted(names)
    assert names.count("layer_norm_dropout") == 1 and "dropout" not in names, sorted(names)
    assert lrandom.get_state("hip") == (3, 1 + 2 * LAYERS)                # attention dropout is off in this model
    plain_names = _names(_loss(plain, hip))
    assert "dropout_add_layer_norm" not in plain_names and "layer_norm_dropout" not in plain_names
    model.eval()
    assert _names(_loss(model, hip)) == plain_names                       # eval(): node for node the model without dropout
    assert lrandom.get_state("hip") == (3, 1 + 2 * LAYERS)                # ... and nothing drawn


@pytest.mark.parametrize("attention_p", [0.1, 0.0], ids=["attention-dropout", "no-attention-dropout"])
def test_the_captured_step_launches_what_the_model_without_hidden_dropout_launches(hip, attention_p):
    from lightgrad_amd.autograd.hip import HipGraph
    ids, labels = hip.from_numpy(IDS, requires_grad=False), hip.from_numpy(LABELS, requires_grad=False)
    counts = {}
    for hidden_p in (0.1, 0.0):
        model = _bert(hidden_p, attention_p).map_parameters(lambda p: p.hip())

        def step():
            loss = light.loss.cross_entropy(model(ids).reshape(-1, VOCAB), labels)
            for p in model.parameters():
                p.zero_grad()
            loss.backward()
        step()
        graph = HipGraph()
        with graph.capture():
            step()
        counts[hidden_p] = graph.kernel_count()
        graph.destroy()
    assert counts[0.1] == counts[0.0] > 0, counts


def test_values_against_the_float64_tape(hip):
    """loss and every parameter gradient: within 1e-5 (relative Frobenius) of the float64 run of the same tape on the CPU backend,
    or no further from it than twice the float32 CPU composite under the same seed.  The key projection's bias has a gradient
    of exactly zero in exact arithmetic and is bounded as rounding noise, like tests/test_hip_bert.py does."""
    seed = SEEDS[1]

    def loss_and_grads(model, T):
        loss = _loss(model, T)
        for p in model.parameters():
            p.zero_grad()
        loss.backward()
        out = {n: p.grad.numpy().astype(np.float64) for n, p in model.named_parameters()}
        out["loss"] = np.asarray(loss.item(), np.float64)
        return out

    cpu_model = _bert(0.1, 0.1)
    values = {n: p.numpy() for n, p in cpu_model.named_parameters()}
    hip_model = _bert(0.1, 0.1).map_parameters(lambda p: p.hip())
    light.manual_seed(seed)
    cpu32 = loss_and_grads(cpu_model, CpuTensor)
    got = loss_and_grads(hip_model, hip)
    assert lrandom.get_state("cpu") == lrandom.get_state("hip") == (seed, 4)
    light.manual_seed(seed)
    with float64_tape():
        ref_model = _bert(0.1, 0.1)
        ref_model.load_parameters({n: a.astype(np.float64) for n, a in values.items()})
        assert all(p.dtype == np.float64 for p in ref_model.parameters())
        ref64 = loss_and_grads(ref_model, CpuTensor)
    noise = [n for n in ref64 if n.endswith(".key.bias")]
    for n in noise:
        assert np.abs(got[n]).max() < 1e-6 and np.abs(cpu32[n]).max() < 1e-6 and np.abs(ref64[n]).max() < 1e-12
    for n in ref64:
        print("%-60s hip %.2e  cpu32 %.2e" % (n, rel_frobenius(got[n], ref64[n]), rel_frobenius(cpu32[n], ref64[n])))
    rest = {n: a for n, a in ref64.items() if n not in noise}
    assert_as_close_to_float64_as_the_cpu_backend(got, cpu32, rest, what="tiny-BERT, hidden dropout inside the LayerNorm launches")
