"""Dropout on the CPU backend: the Philox4x32-10 stream of lightgrad_amd/random.py (known answers), the keep rule, the
bookkeeping of `draws`, the backward that regenerates the mask, Module.train / eval, nn.Dropout and the BERT example's wiring."""
import numpy as np
import pytest
import lightgrad_amd as light
import lightgrad_amd.nn as nn
from lightgrad_amd import CpuTensor, random as lrandom
from test_bert_cpu import bert

KNOWN_ANSWERS = [
    ((0x00000000,) * 4, (0x00000000, 0x00000000), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff, 0xffffffff), (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def f32(a):
    return CpuTensor.from_numpy(np.asarray(a, dtype=np.float32))


@pytest.mark.parametrize("counter,key,expected", KNOWN_ANSWERS)
def test_philox_known_answers(counter, key, expected):
    got = lrandom.philox4x32_10(counter, key)
    assert got.dtype == np.uint32 and tuple(int(w) for w in got) == expected


def test_philox_vectorised_and_high_index_word():
    """the function the backend calls (`words`) for a group index 2**32 + 5: counter word 1 carries the high half"""
    seed, draw = (0x299f31d0 << 32) | 0xa4093822, (3 << 32) | 9
    got = lrandom.words(seed, draw, 8, first_group=2**32 + 5)
    for j in range(2):
        one = lrandom.philox4x32_10((5 + j, 1, 9, 3), (0xa4093822, 0x299f31d0))
        np.testing.assert_array_equal(got[4 * j:4 * j + 4], one)
    low = lrandom.philox4x32_10((5, 0, 9, 3), (0xa4093822, 0x299f31d0))
    assert not np.array_equal(got[:4], low)
    # all three known answers again, as rows of one vectorised call with a shared key
    c = np.array([k[0] for k in KNOWN_ANSWERS[:1] * 3], dtype=np.uint64).T
    np.testing.assert_array_equal(lrandom.philox4x32_10(tuple(c), (0, 0)), [KNOWN_ANSWERS[0][2]] * 3)


def test_threshold_and_scale():
    assert lrandom.threshold(0.0) == 0 and lrandom.threshold(0.5) == 2**31
    assert lrandom.threshold(np.nextafter(1.0, 0.0)) == 2**32 - 1               # floor(2**32 - 2**-21)
    assert lrandom.threshold(0.1) == int(np.floor(0.1 * 2.0**32))
    assert lrandom.scale(0.5) == np.float32(2.0) and lrandom.scale(0.1).dtype == np.float32
    assert lrandom.scale(0.1) == np.float32(1.0 / 0.9)


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_rule(p):
    n = 2**20
    rng = np.random.RandomState(3)
    x = rng.standard_normal(n).astype(np.float32)
    light.manual_seed(1234)
    lrandom._CpuGenerator.draws = 7
    y = f32(x).dropout(p).numpy()
    keep = lrandom.words(1234, 7, n) >= np.uint32(lrandom.threshold(p))
    np.testing.assert_array_equal(y != 0, keep & (x != 0))
    sd = np.sqrt(p * (1 - p) / n)
    deviation = (keep.mean() - (1 - p)) / sd
    print("p = %.1f: kept fraction %.6f, %.2f standard deviations from 1 - p" % (p, keep.mean(), deviation))
    assert abs(deviation) <= 5
    np.testing.assert_array_equal(y, np.where(keep, x * lrandom.scale(p), np.float32(0)))
    if p == 0.5:
        assert np.all((y == 0) | (y == 2 * x))
        assert not np.signbit(y[~keep]).any()


def test_dropped_nan_and_infinity_become_plus_zero():
    light.manual_seed(5)
    keep = lrandom.keep_mask(5, 0, 64, 0.5)
    x = np.full(64, np.nan, np.float32)
    x[::2] = -np.inf
    y = f32(x).dropout(0.5).numpy()
    assert np.all(y[~keep] == 0) and not np.signbit(y[~keep]).any()
    odd = np.arange(64) % 2 == 1
    assert np.isnan(y[keep & odd]).all() and np.all(y[keep & ~odd] == -np.inf) and (keep & odd).any() and (~keep & odd).any()


def test_draws_advance_by_one_per_call():
    light.manual_seed(11)
    assert lrandom.get_state("cpu") == (11, 0)
    x = f32(np.ones((3, 5)))
    x.dropout(0.3)
    assert lrandom.get_state("cpu") == (11, 1)
    f32(np.ones((0,))).dropout(0.3)                          # n == 0
    assert lrandom.get_state("cpu") == (11, 2)
    with light.no_grad():
        y = x.dropout(0.3)
    assert y.ctx is None and lrandom.get_state("cpu") == (11, 3)
    assert x.dropout(0.0) is x                               # p == 0: nothing drawn, nothing launched
    r = f32(np.full((3, 5), 2.0))
    np.testing.assert_array_equal(x.dropout(0.0, residual=r).numpy(), np.full((3, 5), 3.0, np.float32))
    assert lrandom.get_state("cpu") == (11, 3)
    with pytest.raises(ValueError):
        lrandom.get_state("opencl")


def test_manual_seed_repeats_the_stream():
    x = f32(np.random.RandomState(0).standard_normal((7, 9)))
    light.manual_seed((1 << 40) + 3)
    first = [x.dropout(0.4).numpy() for _ in range(3)]
    light.manual_seed((1 << 40) + 3)
    again = [x.dropout(0.4).numpy() for _ in range(3)]
    for a, b in zip(first, again):
        np.testing.assert_array_equal(a, b)
    assert not np.array_equal(first[0], first[1])
    light.manual_seed(3)                                      # the high word of the seed matters
    assert not np.array_equal(x.dropout(0.4).numpy(), first[0])


def test_backward_regenerates_the_mask():
    rng = np.random.RandomState(1)
    x, r = f32(rng.standard_normal((6, 10))), f32(rng.standard_normal((6, 10)))
    g = rng.standard_normal((6, 10)).astype(np.float32)
    light.manual_seed(77)
    y_of_ones = f32(np.ones((6, 10))).dropout(0.25).numpy()
    light.manual_seed(77)
    y = x.dropout(0.25)
    x.dropout(0.25)                                           # a later call in between must not disturb the first one's backward
    (y * CpuTensor.from_numpy(g, requires_grad=False)).backward(allow_fill=True)
    np.testing.assert_array_equal(x.grad.numpy(), g * y_of_ones)
    # with a residual: y = dropout(x) + r in two roundings; the residual's gradient is the output gradient itself
    x2 = f32(x.numpy())
    light.manual_seed(77)
    y2 = x2.dropout(0.25, residual=r)
    np.testing.assert_array_equal(y2.numpy(), y.numpy() + r.numpy())
    out_grad = CpuTensor.from_numpy(g, requires_grad=False)
    grads = y2.ctx.backward(out_grad)
    assert grads[1].data is out_grad.data                     # no copy
    np.testing.assert_array_equal(grads[0].numpy(), g * y_of_ones)
    y2.backward(allow_fill=True)
    np.testing.assert_array_equal(r.grad.numpy(), np.ones((6, 10), np.float32))
    np.testing.assert_array_equal(x2.grad.numpy(), y_of_ones)


def test_non_dense_input_is_indexed_as_its_dense_result():
    a = np.random.RandomState(2).standard_normal((5, 8)).astype(np.float32)
    light.manual_seed(9)
    y = f32(a).transpose(1, 0).dropout(0.5).numpy()
    light.manual_seed(9)
    np.testing.assert_array_equal(y, f32(np.ascontiguousarray(a.T)).dropout(0.5).numpy())


def test_argument_checks():
    x = f32(np.ones(4))
    for bad in (1.0, -0.1, 1.5, float("nan")):
        with pytest.raises(ValueError):
            x.dropout(bad)
    with pytest.raises(ValueError):
        nn.Dropout(1.0)
    for dtype in (np.int32, np.float64):
        with pytest.raises(TypeError):
            CpuTensor.from_numpy(np.ones(4, dtype=dtype)).dropout(0.5)
    with pytest.raises(TypeError):
        x.dropout(0.5, residual=CpuTensor.from_numpy(np.ones(4, dtype=np.float64)))
    with pytest.raises(ValueError):
        x.dropout(0.5, residual=f32(np.ones(5)))
    before = lrandom.get_state("cpu")
    with pytest.raises(TypeError):
        CpuTensor.from_numpy(np.ones(4, dtype=np.int32)).dropout(0.0)      # p == 0 does not excuse a wrong dtype
    assert lrandom.get_state("cpu") == before


def test_module_train_eval_and_dropout_layer():
    class Net(nn.Module):
        def __init__(self):
            nn.Module.__init__(self)
            self.a = nn.Linear(3, 3)
            self.blocks = nn.ModuleList(nn.Linear(3, 3), nn.Dropout(0.5))
            self.inner = nn.Module()
            self.inner.drop = nn.Dropout(0.2)
    net = Net()
    modules = [net, net.a, net.blocks, net.blocks[0], net.blocks[1], net.inner, net.inner.drop]
    assert all(m.training for m in modules)
    names = [n for n, _ in net.named_parameters()]
    assert net.eval() is net and not any(m.training for m in modules)
    assert net.train() is net and all(m.training for m in modules)
    assert net.train(False) is net and not any(m.training for m in modules)
    assert [n for n, _ in net.named_parameters()] == names and not any("training" in n for n in names)
    assert len(list(net.parameters())) == 4
    net.load_parameters({n: p.numpy() for n, p in net.named_parameters()})      # no entry for `training` is asked for

    drop, x, r = nn.Dropout(0.5), f32(np.ones((4, 4))), f32(np.ones((4, 4)))
    light.manual_seed(1)
    y = drop(x)
    assert y is not x and set(np.unique(y.numpy())) <= {0.0, 2.0} and lrandom.get_state("cpu")[1] == 1
    drop.eval()
    assert drop(x) is x and lrandom.get_state("cpu")[1] == 1
    np.testing.assert_array_equal(drop(x, residual=r).numpy(), np.full((4, 4), 2.0, np.float32))
    assert nn.Dropout(0.0)(x) is x


BERT_CFG = dict(hidden_size=32, intermediate_size=64, num_hidden_layers=1, num_attention_heads=2, vocab_size=50,
                max_position_embeddings=8, type_vocab_size=2)
BERT_IDS = np.random.RandomState(4).randint(0, 50, (2, 8)).astype(np.int32)


def build_bert(seed=6, **dropout):
    np.random.seed(seed)
    return bert.BertForMaskedLM(**BERT_CFG, **dropout)


def test_bert_with_dropout():
    ids = CpuTensor.from_numpy(BERT_IDS, requires_grad=False)
    plain = build_bert()
    model = build_bert(hidden_dropout_prob=0.1, attention_probs_dropout_prob=0.1)
    assert [n for n, _ in model.named_parameters()] == [n for n, _ in plain.named_parameters()]
    for (_, p), (_, q) in zip(model.named_parameters(), plain.named_parameters()):
        np.testing.assert_array_equal(p.numpy(), q.numpy())
    expected = plain(ids).numpy()
    light.manual_seed(8)
    model.eval()
    np.testing.assert_array_equal(model(ids).numpy(), expected)          # bit for bit, and nothing drawn
    assert lrandom.get_state("cpu") == (8, 0)
    model.train()
    first, second = model(ids).numpy(), model(ids).numpy()
    # 3 hidden sites + 1 attention site per forward
    assert lrandom.get_state("cpu") == (8, 8)
    assert not np.array_equal(first, second) and not np.array_equal(first, expected)
    light.manual_seed(8)
    np.testing.assert_array_equal(model(ids).numpy(), first)
    np.testing.assert_array_equal(model(ids).numpy(), second)
    # the tape runs backward through all four sites
    loss = light.loss.cross_entropy(model(ids).reshape(-1, 50), CpuTensor.from_numpy(np.arange(16) % 50, requires_grad=False))
    for p in model.parameters():
        p.zero_grad()
    loss.backward()
    assert all(np.isfinite(p.grad.numpy()).all() for p in model.parameters())
    assert np.abs(model.bert.embeddings.word_embeddings.weight.grad.numpy()).max() > 0
